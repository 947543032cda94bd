"""fmgpu_chains_align (include/fmgpu.h) on the host: the symbol and the two structs, every argument check that comes before the first use of the device, the empty call,
and the plain-Python model of tests/align_model.py held against two statements that share nothing with it: a replay of every line over the read and the window, and
an unbanded Levenshtein distance for every gap."""
import ctypes as C
import os
import re

import numpy as np

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests import align_cases as cases
from tests import align_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def last_error():
    return capi.lib().fmgpu_last_error()


def test_the_symbol_exists_and_the_abi_version_stays():
    L = capi.lib()
    assert "fmgpu_chains_align" in capi.EXPORTS and hasattr(L, "fmgpu_chains_align")
    assert re.search(r"\bint\s+fmgpu_chains_align\s*\(", header())
    assert L.fmgpu_abi_version() == 6 and re.search(r"#define FMGPU_ABI_VERSION 6\b", header())
    assert "align_chains" in fm.__all__ and "ChainAlignments" in fm.__all__
    assert len(capi.OPTIONS) == 13                                      # the option count stays


def fields_of(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            names += [re.sub(r"\[\d+\]", "", first.split()[-1]).lstrip("*")] + [re.sub(r"\[\d+\]", "", m.strip()).lstrip("*") for m in more]
    return names


def test_the_structs_mirror_the_header():
    A, dt = capi.ChainAlignment, capi.CHAIN_ALIGNMENT_DTYPE
    names = ["first_op", "n_ops", "status", "n_match", "n_mismatch", "n_ins", "n_del"]
    assert C.sizeof(A) == 32 == dt.itemsize
    assert [f[0] for f in A._fields_] == fields_of("fmgpu_chain_alignment") == list(dt.names) == names
    assert [getattr(A, f[0]).offset for f in A._fields_] == [dt.fields[k][1] for k in names] == [0, 8, 12, 16, 20, 24, 28]
    S = capi.AlignSpec
    assert C.sizeof(S) == 32
    assert [f[0] for f in S._fields_] == fields_of("fmgpu_align_spec") == ["nq", "max_cells", "band", "max_gap_len", "reserved"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 20, 24]
    assert (capi.OP_I, capi.OP_D, capi.OP_S, capi.OP_EQ, capi.OP_X) == (1, 2, 4, 7, 8) == (model.I, model.D, model.S, model.EQ, model.X)
    for name, value in (("I", 1), ("D", 2), ("S", 4), ("EQ", 7), ("X", 8)):
        assert re.search(r"#define FMGPU_OP_%s\s+%du" % (name, value), header())


GARBAGE = C.c_void_p(0x10)                                               # never read through: the checks come first


def spec(nq=2, max_cells=1 << 24, band=64, max_gap_len=5000, reserved=(0,) * 8):
    return capi.AlignSpec(nq, max_cells, band, max_gap_len, (C.c_uint8 * 8)(*reserved))


ARRAYS = ("chains", "anchors", "positions", "spans", "qbuf", "qoff", "tbuf", "toff", "out")


def test_argument_checks_come_before_the_device():
    L = capi.lib()
    total = C.c_uint64(7)
    g = GARBAGE

    def call(s, n_chains=2, n_anchor=2, count=2, n_spans=2, ops=g, capacity=4, out_count=C.byref(total), **null):
        p = {name: (None if name in null else g) for name in ARRAYS}
        return L.fmgpu_chains_align(p["chains"], n_chains, p["anchors"], n_anchor, p["positions"], count, p["spans"], n_spans, p["qbuf"], p["qoff"], p["tbuf"], p["toff"],
                                    None if s is None else C.byref(s), p["out"], ops, capacity, out_count, None)

    checks = [
        (lambda: call(None), b"spec is null"),
        (lambda: call(spec(), out_count=None), b"out_ops_count is null"),
        (lambda: call(spec(band=65536)), b"band must lie in 0 .. 65535"),
        (lambda: call(spec(band=0xffffffff)), b"band must lie in 0 .. 65535"),
        (lambda: call(spec(max_gap_len=65536)), b"max_gap_len must lie in 0 .. 65535"),
        (lambda: call(spec(max_cells=0)), b"max_cells must lie in 1 .. 2^30"),
        (lambda: call(spec(max_cells=(1 << 30) + 1)), b"max_cells must lie in 1 .. 2^30"),
        (lambda: call(spec(reserved=(0, 0, 0, 0, 0, 0, 0, 1))), b"reserved must be 0"),
        (lambda: call(spec(reserved=(9,) + (0,) * 7)), b"reserved must be 0"),
        (lambda: call(spec(), ops=None), b"out_ops is null while ops_capacity > 0"),
    ] + [(lambda name=name: call(spec(), **{name: True}), b"%s is null while n_chains > 0" % name.encode()) for name in ARRAYS]
    messages = set()
    for run, word in checks:
        total.value = 7
        assert run() == capi.FMGPU_ERR_INVALID and word in last_error(), (word, last_error())
        messages.add(last_error())
    assert len(messages) == 7 + len(ARRAYS)                               # each check has a message of its own
    # the limits: refused before anything is staged
    for k in range(4):
        counts = [2, 2, 2, 2]
        counts[k] = (1 << 32) - 256
        total.value = 7
        assert call(spec(), *counts, ops=None, capacity=0) == capi.FMGPU_ERR_UNSUPPORTED and b"2^32 - 256" in last_error() and total.value == 0
    # the accepted ends of every range get past the checks: without a chain there is nothing to do
    for s in (spec(nq=0, max_cells=1, band=0, max_gap_len=0), spec(max_cells=1 << 30, band=65535, max_gap_len=65535)):
        total.value = 7
        assert call(s, n_chains=0, ops=None, capacity=0) == 0 and total.value == 0
    total.value = 7
    assert L.fmgpu_chains_align(None, 0, None, 0, None, 0, None, 0, None, None, None, None, C.byref(spec()), None, None, 0, C.byref(total), None) == 0 and total.value == 0
    # and the checks still come first without a chain
    assert call(spec(band=65536), n_chains=0) == capi.FMGPU_ERR_INVALID
    res = fm.align_chains(None, (np.zeros(0, dtype=capi.CHAIN_DTYPE), np.zeros(0, dtype=np.uint32)), np.zeros(0, dtype=capi.POSITION_DTYPE),
                          np.zeros(0, dtype=capi.SEED_SPAN_DTYPE), [[1, 2]], text=(np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64)))
    assert len(res) == 0 and res.alignments.dtype == capi.CHAIN_ALIGNMENT_DTYPE and res.ops.dtype == np.uint32 and res.ops.size == 0


def test_cigar_strings_of_the_python_layer():
    rec = np.zeros(3, dtype=capi.CHAIN_ALIGNMENT_DTYPE)
    ops = np.array([n << 4 | c for n, c in ((3, 4), (10, 7), (1, 8), (2, 7), (4, 1), (5, 7), (7, 2), (6, 7), (2, 4), (9, 7))], dtype=np.uint32)
    rec[0]["n_ops"], rec[1]["first_op"], rec[1]["status"], rec[2]["first_op"], rec[2]["n_ops"] = 9, 9, 1, 9, 1
    res = fm.ChainAlignments(rec, ops)
    assert res.cigar(0) == "3S10=1X2=4I5=7D6=2S" and res.cigar(0, extended=False) == "3S13M4I5M7D6M2S"
    assert res.cigar(1) == "*" and res.ops_of(1) == [] and res.cigar(2, extended=False) == "9M" and res.ops_of(2) == [(9, 7)]
    assert model.cigar(ops[:9]) == res.cigar(0)


def test_the_model_on_cases_written_by_hand():
    # Q = ACGT, T = ACT with w = 0: the band holds the diagonals -1 and 0; the first that applies at every cell
    assert model.gap_ops([1, 2, 3, 4], [1, 2, 4], 0) == (1, [(2, model.EQ), (1, model.I), (1, model.EQ)])
    assert model.gap_ops([1, 2, 4], [1, 2, 3, 4], 0) == (1, [(2, model.EQ), (1, model.D), (1, model.EQ)])
    # a tie between X and I + D goes to the diagonal
    assert model.gap_ops([1], [2], 5) == (1, [(1, model.X)])
    # TTTTA against ATTTT: two substitutions, or D, four matches, I: the diagonal goes first
    assert model.gap_ops([4, 4, 4, 4, 1], [1, 4, 4, 4, 4], 1)[0] == 2 and model.gap_ops([4, 4, 4, 4, 1], [1, 4, 4, 4, 4], 0) == (2, [(1, model.X), (3, model.EQ), (1, model.X)])
    assert model.cells(3, 5, 2) == 4 * 7 and model.band_of(5, 3, 1) == (-3, 1)
    # a whole line: clips, a merged run of two adjacent pieces, a pure insertion and a pure deletion from overlapping anchors
    rng = np.random.default_rng(1)
    case = cases.build(rng, [cases.chain_spec([5, 6, 4, 3], [(0, 0), (3, 0), (0, 2)], head=2, tail=1, extra={1: 2, 2: 1})], shuffle=False, empty_reads=())
    records, ops = model.align(*cases.model_args(case))
    assert model.cigar(ops) == "2S11=3I4=2D3=1S" and records == [(0, 7, 0, 18, 0, 3, 2)]


def test_the_model_against_a_replay_and_against_levenshtein():
    rng = np.random.default_rng(5)
    gaps_seen = chains_seen = left_out = 0
    kinds = set()
    for trial in range(12):
        case = cases.build(rng, cases.random_specs(rng, 25), sigma=int(rng.choice([2, 4])))
        args = cases.model_args(case)
        # statement 2: with w >= max(gq, gt) the band holds the whole matrix and every gap costs its Levenshtein distance
        gaps = []
        records, ops = model.align(*args, band=12, max_gap_len=12, want_gaps=gaps)
        for c, k, Q, T, cost in gaps:
            assert cost == model.levenshtein(Q, T)
        gaps_seen += len(gaps)
        # statement 1: every line replays over its read and its window, at every band width and with chains left out
        for band, max_gap_len, max_cells in ((12, 12, 1 << 24), (0, 12, 1 << 24), (1, 8, 1 << 24), (3, 12, 60)):
            records, ops = model.align(*args, band=band, max_gap_len=max_gap_len, max_cells=max_cells)
            at = 0
            for c, (first, n, status, nm, nx, ni, nd) in enumerate(records):
                assert first == at
                at += n
                ch = case["chains"][c]
                if status:
                    assert (n, nm, nx, ni, nd) == (0, 0, 0, 0, 0)
                    left_out += 1
                    continue
                Q = case["qbuf"][int(case["qoff"][ch["qidx"]]): int(case["qoff"][int(ch["qidx"]) + 1])]
                T = case["tbuf"][int(case["toff"][c]): int(case["toff"][c + 1])]
                a, b, count = model.replay(ops[first: first + n], Q, T)
                assert (a, b) == (len(Q), int(ch["tend"] - ch["tbeg"])) == (len(Q), len(T))
                assert (count[model.EQ], count[model.X], count[model.I], count[model.D]) == (nm, nx, ni, nd)
                assert count[model.S] == int(ch["qbeg"]) + len(Q) - int(ch["qend"])
                kinds |= {int(w) & 15 for w in ops[first: first + n]}
                chains_seen += 1
            assert at == len(ops)
    print("gaps", gaps_seen, "chains", chains_seen, "left out", left_out)
    assert gaps_seen >= 100 and chains_seen + left_out == 12 * 25 * 4 and chains_seen >= 900 and left_out >= 20 and kinds == {1, 2, 4, 7, 8}
