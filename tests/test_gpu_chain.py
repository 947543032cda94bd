"""fmgpu_seeds_chain / fm.chain_seeds on the device against the plain-Python model of tests/chain_model.py: chains, off, cls and anchors byte for byte, on the smallest
shapes that can break the kernels (runs around the wave width, the short-run bound of 32 and the LDS ring of 256), every filter, every memory space, the counting call,
every device-side error, and one end-to-end test from reads to chains."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import CHAIN_DTYPE, POSITION_DTYPE, SEED_SPAN_DTYPE
from tests import chain_cases as cases
from tests import chain_model as model

pytestmark = pytest.mark.gpu

RUNS = (1, 2, 63, 64, 65, 257, 258, 1000, 31, 32, 33, 34, 3, 5)      # one query each; 32 | 33 is the short-run / wave-run bound


@functools.lru_cache(maxsize=None)
def base_case():
    """queries without anchors at the front (0), in the middle (5, 9) and at the end (the last two); one run per query, then two queries with several sequences, the
    second one with positions above 2^32"""
    rng = np.random.default_rng(3)
    rows, q = [], 1
    for n in RUNS:
        rows += cases.run_anchors(rng, n, q, int(rng.integers(0, 5)))
        q += 2 if q in (4, 8) else 1
    for seq, n in ((4, 40), (2, 7), (9, 1), (3, 70)):
        rows += cases.run_anchors(rng, n, q, seq)
    q += 1
    for seq, n in (((1 << 40) + 1, 50), (1 << 40, 33), (0, 2)):
        rows += cases.run_anchors(rng, n, q, seq, base=(1 << 61) - 5000 if seq else (1 << 32) - 100)
    nq = q + 3
    pos, spans = cases.pack(rows, rng)
    return pos, spans, nq


def agree(pos, spans, nq, **kw):
    """the device against the model, byte for byte"""
    q8 = kw.pop("gap_cost_q8", 128)
    want = model.chain(pos, spans, nq, gap_cost_q8=q8, **kw)
    res = fm.chain_seeds(pos, spans, nq, gap_cost=q8 / 256, **kw)
    chains = np.array(want[0], dtype=CHAIN_DTYPE) if want[0] else np.zeros(0, dtype=CHAIN_DTYPE)
    assert res.chains.tobytes() == chains.tobytes()
    assert res.off.tobytes() == np.array(want[1], dtype=np.uint64).tobytes() and res.cls.tobytes() == np.array(want[2], dtype=np.uint8).tobytes()
    assert res.anchors.tobytes() == np.array(want[3], dtype=np.uint32).tobytes()
    for k in range(0, len(res), max(len(res) // 7, 1)):
        assert res.anchors_of(k).tolist() == want[3][want[0][k][8]: want[0][k][8] + want[0][k][7]]
    return res


@pytest.mark.parametrize("max_lookback", [1, 3, 64, 65, 256])
def test_run_lengths_and_lookbacks(max_lookback):
    pos, spans, nq = base_case()
    res = agree(pos, spans, nq, max_lookback=max_lookback)
    assert res.cls[0] == 0 and res.cls[5] == 0 and res.cls[9] == 0 and res.cls[-1] == 0 and res.cls[-2] == 0 and (res.cls[1:5] == 1).all()
    assert (res.chains["flags"] & 1).any() or max_lookback == 1
    assert (res.chains["n_anchors"] > 256).any() or max_lookback < 64


@pytest.mark.parametrize("gap_cost_q8", [0, 128, 65536])
def test_gap_costs(gap_cost_q8):
    pos, spans, nq = base_case()
    agree(pos, spans, nq, gap_cost_q8=gap_cost_q8, max_skew=9)


def test_filters_and_cuts():
    pos, spans, nq = base_case()
    every = agree(pos, spans, nq)
    for kw in (dict(min_score=60), dict(min_anchors=3), dict(max_chains=1), dict(max_chains=2, min_anchors=2), dict(max_anchors=64), dict(max_anchors=33, max_chains=3),
               dict(max_gap=40), dict(max_skew=1), dict(min_score=1 << 31)):
        res = agree(pos, spans, nq, **kw)
        assert len(res) != len(every)
    assert (agree(pos, spans, nq, max_anchors=64).cls == 3).sum() >= 5 and (agree(pos, spans, nq, min_score=1 << 31).cls == 2).sum() >= len(RUNS)
    # 257 queries: the highest query number is 2^8, one key bit more in the last sort than 256 queries take; anchors in the first query and in the last two
    rng = np.random.default_rng(9)
    pos, spans = cases.pack(cases.run_anchors(rng, 5, 0, 1) + cases.run_anchors(rng, 40, 255, 2) + cases.run_anchors(rng, 3, 256, 0), rng)
    assert agree(pos, spans, 257).cls[[0, 1, 255, 256]].tolist() == [1, 0, 1, 1]


def exact_lookback_rows(lookback, further):
    """a run whose only good link lies exactly `lookback` places back (further: one more): fillers in between that nothing links to or from"""
    rows = [(0, 0, 1000, 0, 30)]
    rows += [(0, 0, 1001 + k, 100000 + 40 * k, 5) for k in range(lookback - 1 + (1 if further else 0))]
    return rows + [(0, 0, 1000 + 2 * lookback + 40, 2 * lookback + 40, 30)]


@pytest.mark.parametrize("lookback", [3, 64, 65, 256])
def test_the_link_exactly_max_lookback_back(lookback):
    for further in (False, True):
        pos, spans = cases.pack(exact_lookback_rows(lookback, further), np.random.default_rng(lookback))
        res = agree(pos, spans, 1, max_lookback=lookback, max_gap=100000)
        assert (int(res.chains["n_anchors"].max()) == 2) == (not further)


def test_a_tandem_repeat_with_ties_everywhere():
    rows = cases.tandem_anchors(1, 6)
    assert len(rows) == 20000
    pos, spans = cases.pack(rows + cases.run_anchors(np.random.default_rng(1), 9, 2, 6), np.random.default_rng(2))
    res = agree(pos, spans, 3)
    assert res.cls.tolist() == [0, 1, 1] and int(res.chains["n_anchors"].max()) == 20
    assert agree(pos, spans, 3, max_anchors=20000).cls.tolist() == [0, 1, 1]
    cut = agree(pos, spans, 3, max_anchors=19999)
    assert cut.cls.tolist() == [0, 3, 1] and cut.off.tolist()[:3] == [0, 0, 0]


def raw_call(pos, count, spans, n_spans, nq, out, capacity, anchors, off, cls, **kw):
    s = capi.ChainSpec(nq, kw.get("max_gap", 5000), kw.get("max_skew", 500), 128, kw.get("max_lookback", 64), 0, 1, kw.get("max_chains", 0), 0, (C.c_uint8 * 8)())
    total = C.c_uint64(77)
    p = lambda a: None if a is None else capi.ptr(a)                 # noqa: E731
    rc = capi.lib().fmgpu_seeds_chain(p(pos), count, p(spans), n_spans, C.byref(s), p(out), capacity, C.byref(total), p(anchors), p(off), p(cls), None)
    return rc, total.value


def test_host_and_device_memory_for_each_array():
    pos, spans, nq = base_case()
    want = fm.chain_seeds(pos, spans, nq)
    n, count = len(want), len(pos)
    for device in range(1 << 6):
        if device not in (0, 63) and bin(device).count("1") not in (1, 5):
            continue                                                 # all host, all device, each array alone on either side
        bufs = []

        def place(k, array):
            if not device >> k & 1:
                return array
            bufs.append(fm.DeviceBuffer.from_array(array))
            return bufs[-1]
        out, anchors = np.zeros(n, dtype=CHAIN_DTYPE), np.zeros(count, dtype=np.uint32)
        off, cls = np.zeros(nq + 1, dtype=np.uint64), np.zeros(nq, dtype=np.uint8)
        args = [place(0, pos), count, place(1, spans), len(spans), nq, place(2, out), n, place(3, anchors), place(4, off), place(5, cls)]
        assert raw_call(*args) == (0, n)
        back = lambda a, dtype, m: a.to_array(dtype, m) if isinstance(a, fm.DeviceBuffer) else a      # noqa: E731
        assert back(args[5], CHAIN_DTYPE, n).tobytes() == want.chains.tobytes() and back(args[7], np.uint32, count)[: want.anchors.size].tobytes() == want.anchors.tobytes()
        assert back(args[8], np.uint64, nq + 1).tobytes() == want.off.tobytes() and back(args[9], np.uint8, nq).tobytes() == want.cls.tobytes()
        for b in bufs:
            b.free()
    # device-resident input through the Python layer
    dp, ds = fm.DeviceBuffer.from_array(pos), fm.DeviceBuffer.from_array(spans)
    res = fm.chain_seeds(dp, ds, nq, want_anchors=False)
    assert res.chains.tobytes() == want.chains.tobytes() and res.anchors is None
    dp.free()
    ds.free()


def test_the_counting_call_and_capacity():
    pos, spans, nq = base_case()
    want = fm.chain_seeds(pos, spans, nq)
    n = len(want)
    off, cls = np.zeros(nq + 1, dtype=np.uint64), np.zeros(nq, dtype=np.uint8)
    assert raw_call(pos, len(pos), spans, len(spans), nq, None, 0, None, off, cls) == (0, n)
    assert off.tobytes() == want.off.tobytes() and cls.tobytes() == want.cls.tobytes()
    out, anchors = np.full(n, 0xAA, dtype=np.uint8).repeat(56).view(CHAIN_DTYPE), np.full(len(pos), 0xAAAAAAAA, dtype=np.uint32)
    off[:], cls[:] = 0, 0
    assert raw_call(pos, len(pos), spans, len(spans), nq, out, n - 1, anchors, off, cls) == (capi.FMGPU_ERR_CAPACITY, n)
    assert (out.view(np.uint8) == 0xAA).all() and (anchors == 0xAAAAAAAA).all() and off.tobytes() == want.off.tobytes() and cls.tobytes() == want.cls.tobytes()
    assert raw_call(pos, len(pos), spans, len(spans), nq, out, n, None, None, None) == (0, n) and out.tobytes() == want.chains.tobytes()
    cut = fm.chain_seeds(pos, spans, nq, max_chains=1)
    assert raw_call(pos, len(pos), spans, len(spans), nq, None, 0, None, None, None, max_chains=1) == (0, len(cut)) and len(cut) == int((want.cls == 1).sum())


def test_every_device_side_error_names_the_lowest_offender():
    pos, spans, nq = base_case()
    count = len(pos)
    out, off = np.full(4, 0xAA, dtype=np.uint8).repeat(56).view(CHAIN_DTYPE), np.full(nq + 1, 9, dtype=np.uint64)

    def refused(p, s, what, n=nq):
        with pytest.raises(model.ChainError) as e:
            model.chain(p, s, n)
        assert e.value.what == what
        rc, total = raw_call(p, len(p), s, len(s), n, out, 4, None, off, None)
        assert rc == capi.FMGPU_ERR_INVALID and total == 0 and (out.view(np.uint8) == 0xAA).all() and (off == 9).all()
        return e.value.index, capi.lib().fmgpu_last_error()

    a, b = count // 3, count // 2
    bad = pos.copy()
    bad["qidx"][b:] = nq
    assert refused(bad, spans, "range") == (b, b"fmgpu_seeds_chain: record %d names a query beyond nq" % b)
    bad["pos"][a] = 1 << 62                                           # range goes first, whichever record is lower
    assert refused(bad, spans, "range")[0] == b
    bad = pos.copy()
    bad["qidx"][a], bad["qidx"][b] = bad["qidx"][a] + 2, 0
    lowest = a + 1 if pos["qidx"][a + 1] < bad["qidx"][a] else b
    assert refused(bad, spans, "order") == (lowest, b"fmgpu_seeds_chain: record %d names a query below its predecessor's" % lowest)
    bad = pos.copy()
    bad["hit"][[a, b]] = len(spans), 0xffffffff
    bad["pos"][0] = 1 << 63
    assert refused(bad, spans, "hit") == (a, b"fmgpu_seeds_chain: record %d has a hit beyond the spans" % a)
    bad = pos.copy()
    bad["pos"][[a, b]] = 1 << 62, 1 << 63
    short = spans.copy()
    short["qlen"][pos["hit"][0]] = 0
    assert refused(bad, short, "pos") == (a, b"fmgpu_seeds_chain: record %d has a pos of 2^62 or more" % a)
    assert refused(pos, short, "span") == (0, b"fmgpu_seeds_chain: record 0 has a span with qlen == 0 or qbeg + qlen of 2^31 or more")
    long_ = spans.copy()
    long_[pos["hit"][b]] = ((1 << 31) - 5, 5)
    assert refused(pos, long_, "span")[0] == b
    long_[pos["hit"][b]] = ((1 << 31) - 6, 5)                          # qbeg + qlen = 2^31 - 1 is the last one accepted
    agree(pos, long_, nq)


def test_reads_to_chains_end_to_end():
    """three sequences, 200 reads with three substitutions and a two-base deletion each, half of them reverse-complemented: search_smems -> locate_hits -> chain_seeds.
    The device equals the model on the same anchors, and EVERY read's top chain on its true strand lies at its true place (tests/test_chain_host.py confirms on the
    CPU that these inputs allow it)"""
    seqs, reads, truth = cases.end_to_end()
    gx = fm.BiFMIndex.from_sequences(seqs, 5, "IB16", 4)
    doubled = fm.both_strands(reads)
    hits, spans = fm.search_smems(gx, doubled, min_len=15)
    pos = gx.locate_hits(hits)
    nq = 2 * len(reads)
    assert len(pos) >= 4 * len(reads)
    res = agree(pos, spans, nq)
    cases.check_top_chains(res.chains, res.off, truth)
