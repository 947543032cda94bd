"""The both-strand calls (include/fmgpu.h: fmgpu_queries_strands, fmgpu_search_best_pairs / _ng21_pairs, fmgpu_map_strands, fmgpu_feed_map_strands,
fmgpu_feed_map_text_strands) on the host: the symbols and the struct, what the calls decide before a handle or a device is looked at, the NumPy restatement
both_strands against a plain double loop and against the example's rule, and the pair-ladder model of tests/strands_model.py on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE
from tests import strands_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("fmgpu_queries_strands", "fmgpu_search_best_pairs", "fmgpu_search_best_ng21_pairs", "fmgpu_map_strands", "fmgpu_feed_map_strands", "fmgpu_feed_map_text_strands")
DNA5 = np.array([0, 4, 3, 2, 1], dtype=np.uint8)


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def last_error():
    return capi.lib().fmgpu_last_error()


def test_the_six_symbols_exist_and_abi_version_and_option_count_stay():
    L = capi.lib()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header()), name
    assert L.fmgpu_abi_version() == 6 and re.search(r"#define FMGPU_ABI_VERSION 6\b", header())
    assert re.search(r"FMGPU_OPT_COUNT_ = 13\b", header()) and len(capi.OPTIONS) == 13
    assert C.sizeof(capi.MapQuery) == 40


def test_strands_struct():
    assert [f[0] for f in capi.Strands._fields_] == ["complement", "n", "pair"]
    assert C.sizeof(capi.Strands) == 16
    assert (capi.Strands.complement.offset, capi.Strands.n.offset, capi.Strands.pair.offset) == (0, 8, 12)
    body = re.search(r"typedef struct fmgpu_strands \{(.*?)\} fmgpu_strands;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.split()[-1] for d in body.split(";") if d.strip()] == ["complement", "n", "pair"]


def strands(n=5, pair=0, comp=DNA5):
    return capi.Strands(None if comp is None else comp.ctypes.data_as(capi.u8p), n, pair)


def map_calls():
    """(name, call(what, strands, nq, cnt)) for the three calls that take a flat batch or a text, with a null handle / feed"""
    L = capi.lib()
    one = np.zeros(8, dtype=np.uint64)
    text = np.frombuffer(b"ACGT\n", dtype=np.uint8)
    table = np.zeros(256, dtype=np.uint8)
    res = capi.ParseResult()

    def flat(call, tail):
        return lambda what, st, nq, cnt: call(None, capi.ptr(one), capi.ptr(one), nq, what, st, None, 0, cnt, None, 0, None, None, None, None, *tail)
    return [("fmgpu_map_strands", flat(L.fmgpu_map_strands, (None,))), ("fmgpu_feed_map_strands", flat(L.fmgpu_feed_map_strands, ())),
            ("fmgpu_feed_map_text_strands", lambda what, st, nq, cnt: L.fmgpu_feed_map_text_strands(None, capi.ptr(text), text.size if nq else 0, capi.TEXT_LINES, 1, capi.ptr(table), 0,
                                                                                                    what, st, None, 0, cnt, None, 0, None, None, None, None, None, 0,
                                                                                                    C.byref(res), None, None))]


def test_the_strands_argument_is_checked_behind_what_and_before_the_handle():
    good = capi.MapQuery(capi.MAP_EXACT, 0, None, 1, 0, 0, 0)
    bad_what = capi.MapQuery(capi.MAP_EXACT, 0, None, 1, 0, 7, 0)
    for name, call in map_calls():
        for nq in (0, 1):
            cnt = C.c_uint64(7)
            for st, word in ((None, b"strands is null"), (strands(comp=None), b"complement is null"), (strands(n=0), b"n must be in [1, 256]"),
                             (strands(n=257), b"n must be in [1, 256]"), (strands(n=-1), b"n must be in [1, 256]"), (strands(pair=2), b"pair must be 0 or 1"),
                             (strands(pair=-1), b"pair must be 0 or 1")):
                rc = call(C.byref(good), None if st is None else C.byref(st), nq, C.byref(cnt))
                assert rc == capi.FMGPU_ERR_INVALID and word in last_error(), (name, nq, word, last_error())
                assert cnt.value == 0
            # a bad `what` is refused first, whatever `strands` is
            for st in (None, strands(n=0), strands()):
                rc = call(C.byref(bad_what), None if st is None else C.byref(st), nq, C.byref(cnt))
                assert rc == capi.FMGPU_ERR_INVALID and b"reserved" in last_error(), (name, nq, last_error())
        # good arguments and no read: 0 before the handle (or, for text, no byte: the null feed is named as fmgpu_feed_map_text names it)
        cnt = C.c_uint64(7)
        for n, pair in ((1, 0), (5, 1), (256, 1)):
            st = strands(n=n, pair=pair, comp=np.arange(256, dtype=np.uint8))
            rc = call(C.byref(good), C.byref(st), 0, C.byref(cnt))
            if "text" in name:
                assert rc == capi.FMGPU_ERR_INVALID and b"feed" in last_error()
            else:
                assert rc == 0 and cnt.value == 0, (name, last_error())
        # good arguments and a read: the null handle / feed is what is refused
        st = strands()
        assert call(C.byref(good), C.byref(st), 1, C.byref(cnt)) == capi.FMGPU_ERR_INVALID, name
        assert (b"feed" if "feed" in name else b"handle") in last_error(), (name, last_error())


def test_two_to_the_thirty_reads_are_refused_without_a_device():
    L = capi.lib()
    one = np.zeros(8, dtype=np.uint64)
    byte = np.zeros(8, dtype=np.uint8)
    good = capi.MapQuery(capi.MAP_EXACT, 0, None, 1, 0, 0, 0)
    st = strands()
    cnt = C.c_uint64(7)
    assert L.fmgpu_queries_strands(capi.ptr(byte), capi.ptr(one), 1 << 30, capi.ptr(DNA5), 5, capi.ptr(byte), capi.ptr(one), None) == capi.FMGPU_ERR_UNSUPPORTED
    assert b"2^30 - 1" in last_error()
    assert L.fmgpu_map_strands(None, capi.ptr(byte), capi.ptr(one), 1 << 30, C.byref(good), C.byref(st), None, 0, C.byref(cnt), None, 0, None, None, None, None,
                               None) == capi.FMGPU_ERR_UNSUPPORTED and b"2^30 - 1" in last_error()
    assert L.fmgpu_feed_map_strands(None, capi.ptr(byte), capi.ptr(one), 1 << 30, C.byref(good), C.byref(st), None, 0, C.byref(cnt), None, 0, None, None, None,
                                    None) == capi.FMGPU_ERR_UNSUPPORTED and b"2^30 - 1" in last_error()


def test_queries_strands_argument_errors_come_before_the_device():
    L = capi.lib()
    one = np.zeros(8, dtype=np.uint64)
    byte = np.zeros(8, dtype=np.uint8)
    for n in (0, 257, -3):
        for nq in (0, 1):
            assert L.fmgpu_queries_strands(capi.ptr(byte), capi.ptr(one), nq, capi.ptr(DNA5), n, capi.ptr(byte), capi.ptr(one), None) == capi.FMGPU_ERR_INVALID
            assert b"n must be in [1, 256]" in last_error()
    # no read: 0, and out_qoff[0] = 0 where out_qoff is given
    off = np.full(3, 9, dtype=np.uint64)
    assert L.fmgpu_queries_strands(None, None, 0, None, 5, None, capi.ptr(off), None) == 0 and off.tolist() == [0, 9, 9]
    assert L.fmgpu_queries_strands(None, None, 0, None, 5, None, None, None) == 0
    # a null pointer while there are reads
    args = [capi.ptr(byte), capi.ptr(one), 1, capi.ptr(DNA5), 5, capi.ptr(byte), capi.ptr(one), None]
    for k in (0, 1, 3, 5, 6):
        a = list(args)
        a[k] = None
        assert L.fmgpu_queries_strands(*a) == capi.FMGPU_ERR_INVALID and b"is null" in last_error(), k


def test_the_pair_ladder_refuses_an_odd_batch_without_a_device():
    L = capi.lib()
    one = np.zeros(8, dtype=np.uint64)
    byte = np.zeros(8, dtype=np.uint8)
    hits = np.zeros(4, dtype=HIT_DTYPE)
    cnt = C.c_uint64(7)
    sch, ex = (capi.Scheme * 1)(), (capi.ExpandedScheme * 1)()
    for call, arr in ((L.fmgpu_search_best_pairs, sch), (L.fmgpu_search_best_ng21_pairs, ex)):
        for nq in (1, 3, 7):
            for n_schemes in (0, 1):
                assert call(None, capi.ptr(byte), capi.ptr(one), nq, arr, n_schemes, 1, capi.ptr(hits), 4, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID
                assert b"even number of reads" in last_error()
        assert call(None, capi.ptr(byte), capi.ptr(one), 2, arr, 255, 1, capi.ptr(hits), 4, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID
        assert b"n_schemes" in last_error()
        # no read, or no scheme and no out_stratum: 0, as fmgpu_search_best
        assert call(None, None, None, 0, arr, 1, 1, None, 0, C.byref(cnt), None, None, None) == 0 and cnt.value == 0
        assert call(None, capi.ptr(byte), capi.ptr(one), 2, arr, 0, 1, None, 0, C.byref(cnt), None, None, None) == 0


# ---- both_strands
def ragged(seed, lens, lo=0, hi=7):
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi, size=m, dtype=np.uint8) for m in lens]


def test_both_strands_equals_the_double_loop():
    reads = ragged(1, [0, 0, 1, 2, 3, 7, 15, 16, 17, 31, 32, 33, 0, 70, 5])
    reads[5][:3] = (0, 5, 255)
    reads[13][10:13] = (255, 5, 0)
    for comp in (DNA5, np.array([3], dtype=np.uint8), np.array([0, 4, 3, 2, 1, 5], dtype=np.uint8), (255 - np.arange(256)).astype(np.uint8)):
        q, o = fm.both_strands(reads, comp)
        wq, wo = model.both_strands_loops(reads, comp)
        assert np.array_equal(q, wq) and np.array_equal(o, wo) and o.dtype == np.uint64 and q.dtype == np.uint8
    q, o = fm.both_strands(reads, "dna5")
    assert np.array_equal(q, model.both_strands_loops(reads, DNA5)[0])
    # bytes 0, 5 and 255 with n = 5: 0 -> complement[0] = 0, 5 and 255 stay
    q, o = fm.both_strands([np.array([0, 5, 255, 1, 2], dtype=np.uint8)], DNA5)
    assert q.tolist() == [0, 5, 255, 1, 2, 3, 4, 255, 5, 0] and o.tolist() == [0, 5, 10]
    # only empty reads, and no read
    q, o = fm.both_strands([np.zeros(0, dtype=np.uint8)] * 3, DNA5)
    assert q.size == 0 and o.tolist() == [0] * 7
    q, o = fm.both_strands((np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)), DNA5)
    assert q.size == 0 and o.tolist() == [0]
    with pytest.raises(ValueError):
        fm.both_strands(reads, np.zeros(0, dtype=np.uint8))


def test_both_strands_with_an_offset_batch_and_the_examples_rule():
    reads = ragged(2, [4, 0, 9, 33, 1], lo=0, hi=6)                      # ranks $ A C G T N
    qbuf, qoff = fm.flatten(reads)
    want = model.both_strands_loops(reads, DNA5)
    for shift in (0, 3, 16):
        q, o = fm.both_strands((np.concatenate([np.full(shift, 7, dtype=np.uint8), qbuf]), qoff + np.uint64(shift)), DNA5)
        assert np.array_equal(q, want[0]) and np.array_equal(o, want[1]) and o[0] == 0
    q, o = want
    for i, r in enumerate(reads):
        assert q[int(o[2 * i]): int(o[2 * i + 1])].tolist() == list(r)
        assert q[int(o[2 * i + 1]): int(o[2 * i + 2])].tolist() == model.example_reverse_complement(r)


def test_packing_both_strands_equals_the_packers_own_second_strand():
    reads = ragged(3, [0, 1, 2, 5, 16, 17, 40, 0, 3], lo=0, hi=5)         # no byte >= 5: the two rules agree there
    a = fm.pack_queries(fm.both_strands(reads, DNA5), 5)
    b = fm.pack_queries(reads, 5, complement=[0, 4, 3, 2, 1])
    assert np.array_equal(a.packed, b.packed) and np.array_equal(a.qoff, b.qoff) and a.nq == b.nq == 2 * len(reads)


# ---- the pair ladder model on hand-made cases: four pairs, three strata
def hand_made():
    """pair 0: strand 0 found at stratum 0.  pair 1: strand 0 found at stratum 2, strand 1 at stratum 0.  pair 2: both strands at stratum 1.  pair 3: nothing.
    Every stratum also reports what a lower stratum would have found (a scheme with k errors finds the hits with fewer), and a record without rows for read 6."""
    s0 = {0: [(10, 2, 0)], 3: [(30, 1, 0)]}
    s1 = {0: [(10, 2, 0), (12, 1, 1)], 3: [(30, 1, 0)], 4: [(40, 1, 1)], 5: [(50, 3, 1), (55, 1, 1)], 6: [(60, 0, 1)]}
    s2 = {**s1, 2: [(20, 1, 2)], 6: [(60, 0, 1)]}
    return [s0, s1, s2]


def test_pair_ladder_model_on_hand_made_cases():
    rec, stratum, searched = model.pair_ladder(8, 3, model.table_search(hand_made()))
    assert stratum.tolist() == [0, 0, 0, 0, 1, 1, 255, 255]
    assert searched == [8, 4, 2]
    got = model.callback_order(rec)
    assert [(int(r["qidx"]), int(r["lb"]), int(r["len"]), int(r["errors"]), int(r["seq"])) for r in got] == \
        [(0, 10, 2, 0, 0), (3, 30, 1, 0, 0), (4, 40, 1, 1, 0), (5, 50, 3, 1, 0), (5, 55, 1, 1, 1), (6, 60, 0, 1, 0), (6, 60, 0, 1, 0)]
    # the independent ladder on the same tables: read 2 goes on to stratum 2 and is found there; the pair ladder's records are a sub-multiset, and fewer
    irec, istratum, isearched = model.independent_ladder(8, 3, model.table_search(hand_made()))
    assert istratum.tolist() == [0, 255, 2, 0, 1, 1, 255, 255] and isearched == [8, 6, 4]
    mine, theirs = sorted(map(tuple, got.tolist())), sorted(map(tuple, model.callback_order(irec).tolist()))
    assert len(mine) < len(theirs) and all(mine.count(x) <= theirs.count(x) for x in mine)
    assert (2, 20, 0, 1, 2, 0) in theirs and (2, 20, 0, 1, 2, 0) not in mine


def test_pair_ladder_model_corner_cases():
    none = model.pair_ladder(4, 2, model.table_search([{}, {}]))
    assert len(none[0]) == 0 and none[1].tolist() == [255] * 4 and none[2] == [4, 4]
    # everything found at once: the later strata are not run
    allf = model.pair_ladder(4, 3, model.table_search([{1: [(1, 1, 0)], 2: [(2, 1, 0)]}, {}, {}]))
    assert allf[1].tolist() == [0, 0, 0, 0] and allf[2] == [4] and len(allf[0]) == 2
    # a record without rows does not find its pair
    empty = model.pair_ladder(2, 2, model.table_search([{0: [(5, 0, 0)]}, {1: [(6, 2, 1)]}]))
    assert empty[1].tolist() == [1, 1] and empty[2] == [2, 2] and len(empty[0]) == 2
    assert model.pair_ladder(0, 3, model.table_search([{}, {}, {}]))[2] == []


def test_python_facades_refuse_what_is_not_built():
    with pytest.raises(ValueError):
        fm._strands(None, True)
    st, keep = fm._strands("dna5", True)
    assert (st.n, st.pair) == (5, 1) and keep.tolist() == [0, 4, 3, 2, 1]
    assert fm._strands(None, False) == (None, None)
