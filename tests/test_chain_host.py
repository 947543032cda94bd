"""fmgpu_seeds_chain (include/fmgpu.h) on the host: the symbol and the two structs, every argument check that comes before the first use of the device, the call without
anchors, and the plain-Python model of tests/chain_model.py: hand-written cases, and its two statements of chain extraction against each other."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import CHAIN_DTYPE, POSITION_DTYPE, SEED_SPAN_DTYPE
from tests import chain_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def last_error():
    return capi.lib().fmgpu_last_error()


def test_the_symbol_exists_and_the_abi_version_stays():
    L = capi.lib()
    assert "fmgpu_seeds_chain" in capi.EXPORTS and hasattr(L, "fmgpu_seeds_chain")
    assert re.search(r"\bint\s+fmgpu_seeds_chain\s*\(", header())
    assert L.fmgpu_abi_version() == 6 and re.search(r"#define FMGPU_ABI_VERSION 6\b", header())
    assert "chain_seeds" in fm.__all__ and "SeedChains" in fm.__all__


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
    K = capi.Chain
    names = ["qidx", "seq_id", "tbeg", "tend", "qbeg", "qend", "score", "n_anchors", "first", "flags"]
    assert C.sizeof(K) == 56 == CHAIN_DTYPE.itemsize
    assert [f[0] for f in K._fields_] == fields_of("fmgpu_chain") == list(CHAIN_DTYPE.names) == names
    assert [getattr(K, f[0]).offset for f in K._fields_] == [CHAIN_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    S = capi.ChainSpec
    assert C.sizeof(S) == 48
    assert [f[0] for f in S._fields_] == fields_of("fmgpu_chain_spec") == ["nq", "max_gap", "max_skew", "gap_cost_q8", "max_lookback", "min_score", "min_anchors",
                                                                          "max_chains", "max_anchors", "reserved"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40]


GARBAGE = C.c_void_p(0x10)                                               # never read through: the checks come first


def spec(nq=2, max_gap=5000, max_skew=500, gap_cost_q8=128, max_lookback=64, min_score=0, min_anchors=1, max_chains=0, max_anchors=0, reserved=(0,) * 8):
    return capi.ChainSpec(nq, max_gap, max_skew, gap_cost_q8, max_lookback, min_score, min_anchors, max_chains, max_anchors, (C.c_uint8 * 8)(*reserved))


def test_argument_checks_come_before_the_device():
    L = capi.lib()
    out = np.full(4, 0xAA, dtype=np.uint8).repeat(56).view(CHAIN_DTYPE)
    total = C.c_uint64(7)
    g = GARBAGE

    def call(s, pos=g, count=2, spans=g, n_spans=2, out_=capi.ptr(out), capacity=4, out_count=C.byref(total), anchors=g, off=g, cls=g):
        return L.fmgpu_seeds_chain(pos, count, spans, n_spans, None if s is None else C.byref(s), out_, capacity, out_count, anchors, off, cls, None)

    cases = [
        (lambda: call(None), b"spec is null"),
        (lambda: call(spec(), out_count=None), b"out_count is null"),
        (lambda: call(spec(max_gap=0)), b"max_gap must lie in"),
        (lambda: call(spec(max_gap=1 << 31)), b"max_gap must lie in"),
        (lambda: call(spec(max_skew=0)), b"max_skew must lie in"),
        (lambda: call(spec(max_skew=0xffffffff)), b"max_skew must lie in"),
        (lambda: call(spec(gap_cost_q8=65537)), b"gap_cost_q8 must lie in"),
        (lambda: call(spec(max_lookback=0)), b"max_lookback must lie in"),
        (lambda: call(spec(max_lookback=257)), b"max_lookback must lie in"),
        (lambda: call(spec(reserved=(0, 0, 0, 0, 0, 0, 0, 1))), b"reserved must be 0"),
        (lambda: call(spec(reserved=(9,) + (0,) * 7)), b"reserved must be 0"),
        (lambda: call(spec(), pos=None), b"positions is null while count > 0"),
        (lambda: call(spec(), spans=None), b"spans is null while count > 0"),
        (lambda: call(spec(), out_=None), b"out is null while capacity > 0"),
    ]
    messages = set()
    for run, word in cases:
        total.value = 7
        assert run() == capi.FMGPU_ERR_INVALID and word in last_error(), (word, last_error())
        messages.add(last_error())
    assert len(messages) == 10                                           # each check has a message of its own
    assert (out.view(np.uint8) == 0xAA).all()
    # the limits: refused before anything is staged
    for count, n_spans in (((1 << 32) - 256, 2), (2, (1 << 32) - 256), (1 << 40, 2)):
        total.value = 7
        assert call(spec(), count=count, n_spans=n_spans, out_=None, capacity=0) == capi.FMGPU_ERR_UNSUPPORTED and b"2^32 - 256" in last_error() and total.value == 0
    # the accepted ends of every range get past the checks: without a query there is nothing to do
    assert call(spec(nq=0, max_gap=(1 << 31) - 1, max_skew=1, gap_cost_q8=65536, max_lookback=256), out_=None, capacity=0, anchors=None, off=None, cls=None) == 0
    assert call(spec(nq=0, max_gap=1, max_skew=(1 << 31) - 1, gap_cost_q8=0, max_lookback=1), out_=None, capacity=0, anchors=None, off=None, cls=None) == 0
    with pytest.raises(ValueError):
        fm.chain_seeds(np.zeros(0, dtype=POSITION_DTYPE), np.zeros(0, dtype=SEED_SPAN_DTYPE), 1, gap_cost=-1.0)


def test_no_query_or_no_anchor_returns_empty_outputs():
    L = capi.lib()
    total = C.c_uint64(7)
    off, cls = np.full(4, 9, dtype=np.uint64), np.full(4, 9, dtype=np.uint8)
    s = spec(nq=3)
    assert L.fmgpu_seeds_chain(None, 0, None, 0, C.byref(s), None, 0, C.byref(total), None, capi.ptr(off), capi.ptr(cls), None) == 0
    assert total.value == 0 and off.tolist() == [0, 0, 0, 0] and cls.tolist() == [0, 0, 0, 9]
    total.value = 7
    off[:] = 9
    s = spec(nq=0)
    assert L.fmgpu_seeds_chain(GARBAGE, 5, GARBAGE, 5, C.byref(s), None, 0, C.byref(total), None, capi.ptr(off), None, None) == 0
    assert total.value == 0 and off.tolist() == [0, 9, 9, 9]
    res = fm.chain_seeds(np.zeros(0, dtype=POSITION_DTYPE), np.zeros(0, dtype=SEED_SPAN_DTYPE), 2)
    assert len(res) == 0 and res.chains.dtype == CHAIN_DTYPE and res.off.tolist() == [0, 0, 0] and res.cls.tolist() == [0, 0] and res.anchors.size == 0
    assert model.chain([], [], 2) == ([], [0, 0, 0], [0, 0], [])


def anchors(rows):
    """(qidx, seq_id, t, q, l) -> (positions, spans): anchor i has hit i"""
    return [(q, s, t, 0, i) for i, (q, s, t, _, _) in enumerate(rows)], [(qb, l) for _, _, _, qb, l in rows]


def one(rows, **kw):
    """the chains of ONE query as (tbeg, tend, qbeg, qend, score, n_anchors, flags, [anchors])"""
    pos, spans = anchors([(0, 0) + r for r in rows])
    chains, off, cls, idx = model.chain(pos, spans, 1, **kw)
    assert off == [0, len(chains)] and cls == [1 if chains else 2]
    return [c[2:8] + (c[9], idx[c[8]: c[8] + c[7]]) for c in chains]


def test_the_model_holds_against_cases_written_by_hand():
    # two collinear anchors link: gain = min(l, dq, dt) = 20, f = 20 + 20
    assert one([(1000, 0, 20), (1030, 30, 20)]) == [(1000, 1050, 0, 50, 40, 2, 0, [0, 1])]
    # a skew of max_skew + 1 does not link; max_skew itself does (cost (128 * 5) >> 8 = 2)
    assert one([(1000, 0, 20), (1036, 30, 20)], max_skew=5) == [(1000, 1020, 0, 20, 20, 1, 0, [0]), (1036, 1056, 30, 50, 20, 1, 0, [1])]
    assert one([(1000, 0, 20), (1035, 30, 20)], max_skew=5) == [(1000, 1055, 0, 50, 38, 2, 0, [0, 1])]
    # max_gap, on dt and on dq alike
    assert len(one([(1000, 0, 20), (1031, 31, 20)], max_gap=30)) == 2 and len(one([(1000, 0, 20), (1030, 30, 20)], max_gap=30)) == 1
    # a penalty that eats the gain does not link: skew 40 at 0.5 per base costs 20 = the gain; skew 38 leaves 1
    assert len(one([(1000, 0, 20), (1070, 30, 20)])) == 2
    assert one([(1000, 0, 20), (1068, 30, 20)]) == [(1000, 1088, 0, 50, 21, 2, 0, [0, 1])]
    assert len(one([(1000, 0, 20), (1068, 30, 20)], gap_cost_q8=65536)) == 2 and one([(1000, 0, 20), (1068, 30, 20)], gap_cost_q8=0)[0][4] == 40
    # an overlap in the read links with gain dq
    assert one([(1000, 0, 20), (1012, 12, 20)]) == [(1000, 1032, 0, 32, 32, 2, 0, [0, 1])]
    # the same t, or the same q, is no predecessor
    assert len(one([(1000, 0, 20), (1000, 30, 20)])) == 2 and len(one([(1000, 0, 20), (1030, 0, 20)])) == 2
    # a fork: anchors 1 and 2 both hang off anchor 0; the better leaf takes the main chain, the other is a branch with the differential score
    fork = [(1000, 0, 20), (1030, 30, 25), (1032, 30, 20)]
    assert one(fork) == [(1000, 1055, 0, 55, 45, 2, 0, [0, 1]), (1032, 1052, 30, 50, 19, 1, 1, [2])]
    # a value equal to l_i does not link: f(0) = 3, gain 2 by the overlap dq = 2, value 5 = l_1
    assert one([(1000, 0, 3), (1002, 2, 5)]) == [(1002, 1007, 2, 7, 5, 1, 0, [1]), (1000, 1003, 0, 3, 3, 1, 0, [0])]
    assert one([(1000, 0, 4), (1002, 2, 5)]) == [(1000, 1007, 0, 7, 6, 2, 0, [0, 1])]
    # the nearest candidate wins among equal values: anchors 0 and 1 both give anchor 2 the value 40
    tie = [(1000, 0, 20), (1000, 5, 20), (1050, 50, 20)]
    assert one(tie, gap_cost_q8=0) == [(1000, 1070, 5, 70, 40, 2, 0, [1, 2]), (1000, 1020, 0, 20, 20, 1, 0, [0])]
    # the earliest child is the heir among equal t: both children of anchor 0 reach 40
    heirs = [(1000, 0, 20), (1030, 30, 20), (1030, 31, 20)]
    assert one(heirs, gap_cost_q8=0) == [(1000, 1050, 0, 50, 40, 2, 0, [0, 1]), (1030, 1050, 31, 51, 20, 1, 1, [2])]
    # max_lookback: the third anchor no longer sees the first
    far = [(1000, 0, 20), (1005, 300, 20), (1030, 30, 20)]
    assert len(one(far, max_lookback=2)) == 2 and len(one(far, max_lookback=1)) == 3
    # filters, then the max_chains cut in output order
    assert one(fork, min_score=20) == [(1000, 1055, 0, 55, 45, 2, 0, [0, 1])] and one(fork, min_anchors=2) == [(1000, 1055, 0, 55, 45, 2, 0, [0, 1])]
    assert one(fork, max_chains=1) == [(1000, 1055, 0, 55, 45, 2, 0, [0, 1])] and one(fork, min_score=46) == []
    # two sequences and three queries: chains never cross either; class 3 for max_anchors, class 2 behind the filters, class 0 without anchors
    rows = [(0, 7, 1000, 0, 20), (0, 8, 1030, 30, 20), (2, 7, 1030, 30, 20), (2, 7, 1000, 0, 20), (2, 7, 5000, 60, 20), (3, 1, 5, 5, 9)]
    pos, spans = anchors(rows)
    chains, off, cls, idx = model.chain(pos, spans, 5, min_score=10)
    assert cls == [1, 0, 1, 2, 0] and off == [0, 2, 2, 4, 4, 4]
    assert chains == [(0, 7, 1000, 1020, 0, 20, 20, 1, 0, 0), (0, 8, 1030, 1050, 30, 50, 20, 1, 1, 0), (2, 7, 1000, 1050, 0, 50, 40, 2, 2, 0), (2, 7, 5000, 5020, 60, 80, 20, 1, 4, 0)]
    assert idx == [0, 1, 3, 2, 4]
    assert model.chain(pos, spans, 5, max_anchors=2)[1:3] == ([0, 2, 2, 2, 3, 3], [1, 0, 3, 1, 0])
    # what the device refuses: the kinds in the header's order, the lowest offender
    for rows_, spans_, nq, index, what in (([(0, 0, 5, 0, 0), (9, 0, 5, 0, 0), (1, 0, 5, 0, 7)], [(0, 5)], 2, 1, "range"),
                                           ([(1, 0, 5, 0, 0), (0, 0, 1 << 62, 0, 0)], [(0, 5)], 2, 1, "order"),
                                           ([(0, 0, 1 << 62, 0, 0), (1, 0, 5, 0, 1)], [(0, 5)], 2, 1, "hit"),
                                           ([(0, 0, 5, 0, 1), (1, 0, 1 << 62, 0, 0)], [(0, 5), (0, 0)], 2, 1, "pos"),
                                           ([(0, 0, 5, 0, 0), (1, 0, 5, 0, 1), (1, 0, 5, 0, 2)], [(0, 5), (0, 0), ((1 << 31) - 5, 5)], 2, 1, "span")):
        with pytest.raises(model.ChainError) as e:
            model.chain(rows_, spans_, nq)
        assert (e.value.code, e.value.index, e.value.what) == (model.INVALID, index, what)
    assert model.chain([(0, 0, 5, 0, 0)], [((1 << 31) - 6, 5)], 1)[0][0][5] == (1 << 31) - 1


def test_the_two_statements_of_chain_extraction_agree_without_ties():
    """heirs (the header's rule) against minimap2's backtracking from the best ends: random forests, anchor lengths that make every f distinct"""
    rng = np.random.default_rng(11)
    compared = branches = 0
    for trial in range(400):
        n = int(rng.integers(2, 60))
        diag = rng.integers(0, 3, n) * 40
        q = np.sort(rng.choice(2000, n, replace=False))
        rows = [(int(diag[k] + q[k] + rng.integers(0, 6)), int(q[k]), int(rng.integers(5, 40))) for k in range(n)]
        kw = dict(max_gap=5000, max_skew=500, gap_cost_q8=int(rng.choice([0, 128, 300])), max_lookback=int(rng.choice([1, 3, 64])))
        run = sorted((t, qb, l, i) for i, (t, qb, l) in enumerate(rows))
        f, p = model.links(run, **kw)
        if len(set(f)) != len(f):
            continue
        a, b = model.heir_chains(f, p), model.backtrack_chains(f, p)
        assert a == b
        compared += 1
        branches += sum(1 for c in a if c[2])
        pos, spans = anchors([(0, 0) + r for r in rows])
        assert model.chain(pos, spans, 1, **kw) == model.chain(pos, spans, 1, extract=model.backtrack_chains, **kw)
    print("compared", compared, "branches", branches)
    assert compared >= 50 and branches >= 50


def test_the_end_to_end_inputs_map_every_read_on_the_cpu():
    """the reads of the end-to-end GPU test (tests/test_gpu_chain.py) through brute-force seeds, a brute-force locate and the model: with the seed fixed in
    tests/chain_cases.py every read's top chain on its true strand lies at its true place, without exception"""
    from tests import chain_cases as cases
    from tests import smem_brute as sb
    seqs, reads, truth = cases.end_to_end()
    qbuf, qoff = fm.both_strands(reads)
    doubled = [qbuf[int(qoff[i]): int(qoff[i + 1])] for i in range(2 * len(reads))]
    texts = [bytes(s) for s in seqs]
    rows, spans = [], []
    for q, b, ln, _, _ in sb.Batch(seqs, doubled, 5).seeds(min_len=15):
        pattern = bytes(doubled[q][b: b + ln])
        for s, text in enumerate(texts):
            at = text.find(pattern)
            while at >= 0:
                rows.append((q, s, at, 0, len(spans)))
                at = text.find(pattern, at + 1)
        spans.append((b, ln))
    chains, off, cls, _ = model.chain(rows, spans, 2 * len(reads))
    cases.check_top_chains(chains, off, truth)
    assert all(cls[2 * r + (1 if rev else 0)] == 1 for r, (_, _, rev) in enumerate(truth))
