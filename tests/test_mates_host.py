"""fmgpu_positions_mates (include/fmgpu.h) on the host: the symbol and the two structs, every argument check that comes before the first use of the device, the call
without a fragment, and the plain-Python model of tests/mates_model.py against hand-written cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import MATE_PAIR_DTYPE, POSITION_DTYPE
from tests import mates_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def last_error():
    return capi.lib().fmgpu_last_error()


def test_the_symbol_exists_and_the_abi_version_stays():
    L = capi.lib()
    assert "fmgpu_positions_mates" in capi.EXPORTS and hasattr(L, "fmgpu_positions_mates")
    assert re.search(r"\bint\s+fmgpu_positions_mates\s*\(", header())
    assert L.fmgpu_abi_version() == 6 and re.search(r"#define FMGPU_ABI_VERSION 6\b", header())
    assert (capi.MATES_FR, capi.MATES_ANY) == tuple(int(re.search(r"#define %s\s+(\d+)" % name, header()).group(1)) for name in ("FMGPU_MATES_FR", "FMGPU_MATES_ANY"))
    assert "join_mates" in fm.__all__


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
    P = capi.MatePair
    assert C.sizeof(P) == 32 == MATE_PAIR_DTYPE.itemsize
    assert [f[0] for f in P._fields_] == fields_of("fmgpu_mate_pair") == list(MATE_PAIR_DTYPE.names) == ["fragment", "tlen", "a", "b", "errors", "flags"]
    assert [getattr(P, f[0]).offset for f in P._fields_] == [MATE_PAIR_DTYPE.fields[k][1] for k in MATE_PAIR_DTYPE.names] == [0, 8, 16, 20, 24, 28]
    S = capi.MatesSpec
    assert C.sizeof(S) == 56
    assert [f[0] for f in S._fields_] == fields_of("fmgpu_mates_spec") == ["qoff_a", "qoff_b", "n_fragments", "min_tlen", "max_tlen", "max_records", "strand_shift",
                                                                           "interleaved", "orientation", "best", "reserved"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 49, 50, 51, 52]


QOFF = np.array([0, 4, 8], dtype=np.uint64)
GARBAGE = C.c_void_p(0x10)                                               # never read through: the checks come first


def spec(qoff_a=QOFF, qoff_b=QOFF, n=2, min_tlen=0, max_tlen=1000, max_records=0, strand_shift=1, interleaved=0, orientation=0, best=0, reserved=(0, 0, 0, 0)):
    p = lambda a: a if a is None or isinstance(a, C.c_void_p) else capi.ptr(a)          # noqa: E731
    return capi.MatesSpec(p(qoff_a), p(qoff_b), n, min_tlen, max_tlen, max_records, strand_shift, interleaved, orientation, best, (C.c_uint8 * 4)(*reserved))


def test_argument_checks_come_before_the_device():
    L = capi.lib()
    out = np.full(4, 0xAA, dtype=np.uint8).repeat(32).view(MATE_PAIR_DTYPE)
    total = C.c_uint64(7)
    g = GARBAGE

    def call(s, pa=g, ca=2, pb=g, cb=2, out_=capi.ptr(out), capacity=4, out_count=C.byref(total), off=g, cls=g):
        return L.fmgpu_positions_mates(pa, ca, pb, cb, None if s is None else C.byref(s), out_, capacity, out_count, off, cls, None)

    bad = dict(qoff_a=g, qoff_b=g)                                       # garbage pointers behind a bad argument are never looked at
    cases = [
        (lambda: call(None), b"spec is null"),
        (lambda: call(spec(**bad), out_count=None), b"out_count is null"),
        (lambda: call(spec(qoff_a=None, qoff_b=g)), b"qoff_a is null"),
        (lambda: call(spec(strand_shift=2, **bad)), b"strand_shift must be 0 or 1"),
        (lambda: call(spec(interleaved=2, **bad)), b"interleaved must be 0 or 1"),
        (lambda: call(spec(orientation=2, **bad)), b"orientation must be"),
        (lambda: call(spec(best=255, **bad)), b"best must be 0 or 1"),
        (lambda: call(spec(reserved=(0, 0, 0, 1), **bad)), b"reserved must be 0"),
        (lambda: call(spec(reserved=(3, 0, 0, 0), **bad)), b"reserved must be 0"),
        (lambda: call(spec(min_tlen=11, max_tlen=10, **bad)), b"min_tlen lies above max_tlen"),
        (lambda: call(spec(interleaved=1, **bad)), b"qoff_b must be null in interleaved mode"),
        (lambda: call(spec(interleaved=1, qoff_a=g, qoff_b=None)), b"positions_b must be null with count_b = 0 in interleaved mode"),
        (lambda: call(spec(interleaved=1, qoff_a=g, qoff_b=None), pb=None), b"positions_b must be null with count_b = 0 in interleaved mode"),
        (lambda: call(spec(interleaved=1, qoff_a=g, qoff_b=None), cb=0), b"positions_b must be null with count_b = 0 in interleaved mode"),
        (lambda: call(spec(qoff_a=g, qoff_b=None)), b"qoff_b is null in separate mode"),
        (lambda: call(spec(**bad), pb=None), b"positions_b is null while count_b > 0"),
        (lambda: call(spec(**bad), pa=None), b"positions_a is null while count_a > 0"),
        (lambda: call(spec(**bad), out_=None), b"out is null while capacity > 0"),
    ]
    messages = set()
    for run, word in cases:
        total.value = 7
        assert run() == capi.FMGPU_ERR_INVALID and word in last_error(), (word, last_error())
        messages.add(last_error())
    assert len(messages) >= 15                                           # each check has a message of its own
    assert (out.view(np.uint8) == 0xAA).all()
    # the limits: refused before anything is staged
    for ca, cb, n, word in (((1 << 32) - 256, 2, 2, b"2^32 - 256"), (2, (1 << 32) - 256, 2, b"2^32 - 256"), (2, 2, (1 << 31) - 1, b"2^31 - 1")):
        assert call(spec(n=n, **bad), ca=ca, cb=cb, out_=None, capacity=0) == capi.FMGPU_ERR_UNSUPPORTED and word in last_error()
    assert call(spec(interleaved=1, qoff_a=g, qoff_b=None, n=(1 << 31) - 1), pb=None, cb=0, out_=None, capacity=0) == capi.FMGPU_ERR_UNSUPPORTED
    # the Python layer refuses what does not fit the mode before it calls
    rec = np.zeros(0, dtype=POSITION_DTYPE)
    for kwargs in (dict(positions_b=rec, qoff_b=QOFF, interleaved=True), dict(), dict(positions_b=rec, qoff_b=QOFF[:2]), dict(positions_b=rec, qoff_b=QOFF, orientation="rf")):
        with pytest.raises(ValueError):
            fm.join_mates(rec, QOFF, **kwargs)
    with pytest.raises(ValueError):
        fm.join_mates(rec, QOFF[:2], interleaved=True)                   # one read is no fragment


def test_no_fragment_returns_zero_before_anything_else_is_looked_at():
    L = capi.lib()
    total = C.c_uint64(7)
    off = np.full(3, 9, dtype=np.uint64)
    none = spec(qoff_a=GARBAGE, qoff_b=GARBAGE, n=0, strand_shift=9, reserved=(1, 1, 1, 1), min_tlen=5, max_tlen=1)
    assert L.fmgpu_positions_mates(GARBAGE, 5, GARBAGE, 5, C.byref(none), GARBAGE, 5, C.byref(total), capi.ptr(off), GARBAGE, None) == 0
    assert total.value == 0 and off.tolist() == [0, 9, 9]
    total.value = 7
    assert L.fmgpu_positions_mates(None, 0, None, 0, C.byref(none), None, 0, C.byref(total), None, None, None) == 0 and total.value == 0
    # the Python layer: no fragment, no pair
    res = fm.join_mates(np.zeros(0, dtype=POSITION_DTYPE), [0], np.zeros(0, dtype=POSITION_DTYPE), [0])
    assert len(res) == 0 and res.pairs.dtype == MATE_PAIR_DTYPE and res.off.tolist() == [0] and res.cls.size == 0
    res = fm.join_mates(np.zeros(0, dtype=POSITION_DTYPE), [7], interleaved=True)
    assert len(res) == 0 and res.off.tolist() == [0] and res.cls.size == 0


def records(rows):
    """(qidx, seq_id, pos, errors)"""
    return np.array([(q, s, p, e, 0) for q, s, p, e in rows], dtype=POSITION_DTYPE)


def one(a, b, ma=50, mb=50, **kw):
    """the pairs of ONE fragment whose mates have the records a and b (read 0 of each batch)"""
    return model.join(records(a), [0, ma], records(b), [100, 100 + mb], **kw)


def test_the_model_holds_against_cases_written_by_hand():
    # A forward at 1000, B reverse at 1250, both 50 long: tlen = 1300 - 1000 = 300.  Exactly at min_tlen, at max_tlen, and one off each
    a, b = [(0, 3, 1000, 1)], [(1, 3, 1250, 2)]
    want = [(0, 300, 0, 0, 3, 1)]
    assert one(a, b, min_tlen=300, max_tlen=300) == (want, [0, 1], [4])
    assert one(a, b, min_tlen=301, max_tlen=400) == ([], [0, 0], [3])
    assert one(a, b, min_tlen=0, max_tlen=299) == ([], [0, 0], [3])
    assert one(a, b, min_tlen=0, max_tlen=300)[0] == want and one(a, b, min_tlen=300, max_tlen=1000)[0] == want
    # mate A on the reverse strand downstream of a forward mate B: the same fragment seen from the other side; bit 0 of flags is clear
    assert one([(1, 3, 1250, 0)], [(0, 3, 1000, 0)])[0] == [(0, 300, 0, 0, 0, 0)]
    # the read lengths enter: a longer mate B moves the right end (tlen = 1250 + 80 - 1000)
    assert one(a, b, mb=80)[0] == [(0, 330, 0, 0, 3, 1)]
    # dovetail: the reverse mate starts upstream of the forward mate; and the forward mate reaching past the reverse mate's end
    assert one([(0, 3, 1000, 0)], [(1, 3, 990, 0)]) == ([], [0, 0], [3])
    assert one([(0, 3, 1000, 0)], [(1, 3, 1010, 0)], ma=80, mb=50) == ([], [0, 0], [3])
    assert one([(0, 3, 1000, 0)], [(1, 3, 1010, 0)], ma=80, mb=50, orientation=model.ANY)[0] == [(0, 80, 0, 0, 0, 1)]
    assert one([(0, 3, 1000, 0)], [(1, 3, 1000, 0)])[0] == [(0, 50, 0, 0, 0, 1)]                  # both mates on the same 50 symbols: equal ends are no dovetail
    # the same pos on different sequences
    assert one([(0, 3, 1000, 0)], [(1, 4, 1250, 0)], orientation=model.ANY) == ([], [0, 0], [3])
    # equal strands under FR and under ANY; without strands (strand_shift = 0) FR finds nothing
    assert one([(0, 3, 1000, 0)], [(0, 3, 1250, 0)]) == ([], [0, 0], [3]) and one([(1, 3, 1000, 0)], [(1, 3, 1250, 0)]) == ([], [0, 0], [3])
    assert one([(0, 3, 1000, 0)], [(0, 3, 1250, 0)], orientation=model.ANY)[0] == [(0, 300, 0, 0, 0, 1)]
    assert model.join(records([(0, 3, 1000, 0)]), [0, 50], records([(0, 3, 1250, 0)]), [0, 50], strand_shift=0) == ([], [0, 0], [3])
    assert model.join(records([(0, 3, 1000, 0)]), [0, 50], records([(0, 3, 1250, 0)]), [0, 50], strand_shift=0, orientation=model.ANY)[0] == [(0, 300, 0, 0, 0, 1)]
    # order inside a fragment: a ascending, then (p(b), b); best keeps the ties at the minimal error sum
    a = [(0, 3, 1000, 1), (0, 3, 1007, 0)]
    b = [(1, 3, 1300, 0), (1, 3, 1250, 1), (1, 3, 1250, 0), (1, 9, 1250, 0)]
    every = [(0, 300, 0, 1, 2, 1), (0, 300, 0, 2, 1, 1), (0, 350, 0, 0, 1, 1), (0, 293, 1, 1, 1, 1), (0, 293, 1, 2, 0, 1), (0, 343, 1, 0, 0, 1)]
    assert one(a, b) == (every, [0, 6], [4])
    assert one(a, b, best=True) == ([every[4], every[5]], [0, 2], [4])
    assert one(a, b, best=True, max_tlen=300) == ([every[4]], [0, 1], [4])
    # the class table, separate mode: fragments 0 .. 5 = none, only A, only B, discordant, paired, skipped (max_records = 2)
    qa = [0, 50, 100, 150, 200, 250, 300]
    ra = records([(2, 0, 10, 0), (6, 0, 10, 0), (8, 0, 10, 0), (10, 0, 10, 0), (10, 0, 20, 0), (10, 0, 30, 0)])
    rb = records([(5, 0, 10, 0), (7, 0, 5000, 0), (9, 0, 100, 0), (11, 0, 100, 0)])
    pairs, off, cls = model.join(ra, qa, rb, qa, max_records=2)
    assert cls == [0, 1, 2, 3, 4, 5] and off == [0, 0, 0, 0, 0, 1, 1] and pairs == [(4, 140, 2, 2, 0, 1)]
    assert model.join(ra, qa, rb, qa)[2] == [0, 1, 2, 3, 4, 4] and len(model.join(ra, qa, rb, qa)[0]) == 4
    # interleaved: the same fragments as one batch, reads 2f and 2f + 1; both indices count in the one array
    qi = [50 * k for k in range(13)]
    both = records([(4 * 1 + 0, 0, 10, 0), (4 * 2 + 3, 0, 10, 0), (4 * 3 + 0, 0, 10, 0), (4 * 3 + 3, 0, 5000, 0), (4 * 4 + 0, 0, 10, 0), (4 * 4 + 3, 0, 100, 0)])
    assert model.join(both, qi, interleaved=True) == ([(4, 140, 4, 5, 0, 1)], [0, 0, 0, 0, 0, 1, 1], [0, 1, 2, 3, 4, 0])
    # what the device refuses: kinds in the header's order, array A before array B, the lowest offender
    for ra_, rb_, array, index, what in ((records([(0, 0, 0, 0), (12, 0, 0, 0)]), rb, "positions_a", 1, "range"),
                                         (ra, records([(4, 0, 0, 0), (2, 0, 0, 0), (0, 0, 0, 0)]), "positions_b", 1, "order"),
                                         (records([(2, 0, 1 << 62, 0)]), records([(4, 0, 0, 0), (2, 0, 0, 0)]), "positions_b", 1, "order"),
                                         (records([(2, 0, 1 << 62, 0)]), records([(0, 0, 1 << 63, 0)]), "positions_a", 0, "pos")):
        with pytest.raises(model.MatesError) as e:
            model.join(ra_, qa, rb_, qa)
        assert (e.value.code, e.value.array, e.value.index, e.value.what) == (model.INVALID, array, index, what)
    with pytest.raises(model.MatesError) as e:
        model.join(ra, qa, rb, [0, 50, 100, 99, 200, 199, 300])
    assert (e.value.array, e.value.index, e.value.what) == ("qoff_b", 2, "qoff")


def test_the_numpy_row_of_the_model_equals_its_plain_loop():
    """mates with many records are compared a row at a time (model.VECTOR_FROM): the same pairs as the plain double loop"""
    rng = np.random.default_rng(5)
    na, nb = 40, 300
    ra = records([(int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 2000)), int(rng.integers(0, 3))) for _ in range(na)])
    rb = records([(int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 2000)), int(rng.integers(0, 3))) for _ in range(nb)])
    assert nb >= model.VECTOR_FROM
    for kw in (dict(), dict(orientation=model.ANY, min_tlen=100, max_tlen=400), dict(best=True), dict(orientation=model.ANY, max_tlen=77)):
        fast = model.join(ra, [0, 50], rb, [0, 60], **kw)
        keep, model.VECTOR_FROM = model.VECTOR_FROM, 1 << 40
        try:
            plain = model.join(ra, [0, 50], rb, [0, 60], **kw)
        finally:
            model.VECTOR_FROM = keep
        assert fast == plain and len(fast[0]) > 0
