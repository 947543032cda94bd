"""fmgpu_chains_align / fm.align_chains on the device against the plain-Python model of tests/align_model.py: records and operations byte for byte, on the smallest
shapes that can break the kernels (gaps on both sides of the lane bound of 15 x 15, of the 16 KiB of the LDS tier and of the 512 KiB of a slice; band widths around
the wave width), every kind of gap, the guards, every memory space, the counting call, every device-side error, and one end-to-end test from reads to CIGAR lines."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import CHAIN_ALIGNMENT_DTYPE
from tests import align_cases as cases
from tests import align_model as model
from tests import chain_cases

pytestmark = pytest.mark.gpu

NAMES = ("chains", "anchors", "positions", "spans", "qbuf", "qoff", "tbuf", "toff")


def device(case, **kw):
    return fm.align_chains(None, (case["chains"], case["anchors"]), case["positions"], case["spans"], (case["qbuf"], case["qoff"]), text=(case["tbuf"], case["toff"]), **kw)


def agree(case, **kw):
    """the device against the model, byte for byte"""
    records, ops = model.align(*cases.model_args(case), **kw)
    res = device(case, **kw)
    assert res.alignments.tobytes() == np.array(records, dtype=CHAIN_ALIGNMENT_DTYPE).tobytes()
    assert res.ops.tobytes() == np.array(ops, dtype=np.uint32).tobytes()
    return res


def test_chain_shapes():
    """one anchor; adjacent anchors (one merged `=`); overlapping anchors (pure I, pure D); gaps of 1 x 1; every clip present and absent"""
    rng = np.random.default_rng(2)
    specs = [cases.chain_spec([7], []), cases.chain_spec([7], [], head=3), cases.chain_spec([7], [], tail=4), cases.chain_spec([1], [], head=1, tail=1),
             cases.chain_spec([5, 6, 7], [(0, 0), (0, 0)], head=2),
             cases.chain_spec([5, 6, 7], [(4, 0), (0, 9)], extra={0: 3, 1: 5}, tail=2),
             cases.chain_spec([5, 6, 7, 8], [(1, 1), (1, 1), (1, 1)], noise=1.0),
             cases.chain_spec([5, 6, 7, 8], [(1, 1), (0, 0), (1, 1)], noise=0.0, head=1, tail=1),
             cases.chain_spec([3, 1, 1, 4], [(2, 2), (0, 0), (3, 0)], noise=0.0)]
    case = cases.build(rng, specs, empty_reads=(0, 3))
    res = agree(case, band=2)
    assert res.cigar(4) == "2S18=" and res.cigar(0) == "7=" and res.cigar(1) == "3S7=" and res.cigar(2) == "7=4S"
    assert res.cigar(5) == "5=4I6=9D7=2S"
    for band in (0, 1, 64):
        agree(case, band=band)
    for seed in range(3):
        agree(cases.build(np.random.default_rng(seed), cases.random_specs(np.random.default_rng(10 + seed), 60)), band=seed)


LANE = [(15, 15), (15, 16), (16, 15), (16, 16), (1, 16), (16, 1), (15, 1), (1, 15), (14, 3), (2, 2), (17, 17)]


@pytest.mark.parametrize("band", [0, 1, 64])
def test_gaps_on_both_sides_of_the_lane_bound(band):
    rng = np.random.default_rng(band)
    specs = [cases.chain_spec([6, 6], [g], noise=n) for g in LANE for n in (0.0, 0.3)]
    specs.append(cases.chain_spec([4] * (len(LANE) + 1), LANE, head=1, tail=1))
    agree(cases.build(rng, specs, sigma=2), band=band)


@functools.lru_cache(maxsize=None)
def band_case():
    """gaps of the LDS tier (several chunks per row with the wider bands) and of the slice tier (more than 16 KiB of directions)"""
    rng = np.random.default_rng(4)
    gaps = [(100, 100), (70, 130), (130, 70), (40, 200), (200, 40), (150, 200), (64, 64), (63, 65), (400, 400), (400, 380), (20, 300)]
    specs = [cases.chain_spec([9, 9], [g], noise=0.15) for g in gaps]
    specs.append(cases.chain_spec([5, 5, 5, 5], [(100, 90), (3, 3), (30, 300)], noise=0.3, head=2))
    return cases.build(rng, specs)


@pytest.mark.parametrize("band", [0, 1, 63, 64, 65, 129])
def test_band_widths(band):
    res = agree(band_case(), band=band)
    assert (res.alignments["status"] == 0).all() and (res.alignments["n_ins"] > 0).any() and (res.alignments["n_del"] > 0).any()


def test_a_gap_beyond_a_slice_goes_through_the_last_list():
    """3400 x 3500 with w = 250: ten chunks per row, 544 KiB of directions: more than a slice of 512 KiB holds"""
    rng = np.random.default_rng(6)
    case = cases.build(rng, [cases.chain_spec([8, 8], [(20, 20)]), cases.chain_spec([8, 8, 8], [(3400, 3500), (5, 5)], noise=0.1), cases.chain_spec([8, 8], [(300, 310)])])
    res = agree(case, band=250)
    assert (res.alignments["status"] == 0).all()


def test_the_two_guards_and_both_skews():
    rng = np.random.default_rng(7)
    specs = [cases.chain_spec([6, 6], [(20, 20)]), cases.chain_spec([6, 6, 6], [(3, 3), (20, 21)]), cases.chain_spec([6, 6], [(5, 5)]),
             cases.chain_spec([6, 6], [(10, 60)]), cases.chain_spec([6, 6], [(60, 10)]), cases.chain_spec([6, 6, 6], [(30, 0), (0, 30)], extra={0: 2})]
    case = cases.build(rng, specs)
    # max_gap_len: 20 aligns the first chain and leaves the second out (21 text symbols); trivial gaps of 30 are never left out
    res = agree(case, band=3, max_gap_len=20)
    assert res.alignments["status"].tolist() == [0, 1, 0, 1, 1, 0]
    assert res.alignments["first_op"][2] == res.alignments["first_op"][1] and res.alignments["n_ops"][1] == 0       # the running sequence goes on behind a chain left out
    assert agree(case, band=3, max_gap_len=21).alignments["status"].tolist() == [0, 0, 0, 1, 1, 0]
    assert agree(case, band=3, max_gap_len=19).alignments["status"].tolist() == [1, 1, 0, 1, 1, 0]
    assert agree(case, band=3, max_gap_len=0).alignments["status"].tolist() == [1, 1, 1, 1, 1, 0]
    # max_cells: (20 + 1) x (2 x 3 + 1) = 147 cells for the first chain, (20 + 1) x (1 + 2 x 3 + 1) = 168 for the second
    assert model.cells(20, 20, 3) == 147 and model.cells(20, 21, 3) == 168
    assert agree(case, band=3, max_cells=147).alignments["status"].tolist() == [0, 1, 0, 1, 1, 0]
    assert agree(case, band=3, max_cells=146).alignments["status"].tolist() == [1, 1, 0, 1, 1, 0]
    assert agree(case, band=3, max_cells=168).alignments["status"].tolist() == [0, 0, 0, 1, 1, 0]
    # gt - gq = +50 and -50, the skew a chain call with max_skew = 50 lets through
    res = agree(case, band=0, max_gap_len=60)
    assert res.alignments["status"].tolist() == [0] * 6 and res.alignments["n_del"][3] >= 50 and res.alignments["n_ins"][4] >= 50
    agree(case, band=64)


def test_a_chain_of_1000_anchors_and_enough_chains_to_cross_every_scan_block():
    rng = np.random.default_rng(8)
    kinds = [(0, 0), (2, 0), (0, 3), (1, 1), (4, 6), (7, 2), (16, 18)]
    long_ = cases.chain_spec([int(v) for v in rng.integers(1, 9, 1000)], [kinds[int(v)] for v in rng.integers(0, len(kinds), 999)], head=5, tail=5, noise=0.3)
    case = cases.build(rng, cases.random_specs(rng, 1500, max_piece=9, max_gap=8) + [long_] + cases.random_specs(rng, 1500, max_piece=9, max_gap=8), sigma=2)
    assert len(case["anchors"]) > 8192 and len(case["chains"]) > 2048
    res = agree(case, band=2, max_gap_len=17)
    assert len(res.ops) > 8192 and res.alignments["status"][1500] == 1 and (res.alignments["status"] == 1).sum() == 1
    res = agree(case, band=2)
    assert res.alignments["n_ops"][1500] > 1000


def raw_call(arrays, n, nq, out, ops, capacity, **kw):
    """arrays: the eight inputs as numpy arrays or DeviceBuffers, n: their four counts"""
    s = capi.AlignSpec(nq, kw.get("max_cells", 1 << 24), kw.get("band", 2), kw.get("max_gap_len", 5000), (C.c_uint8 * 8)())
    total = C.c_uint64(77)
    p = lambda a: None if a is None else capi.ptr(a)                 # noqa: E731
    a = arrays
    rc = capi.lib().fmgpu_chains_align(p(a[0]), n[0], p(a[1]), n[1], p(a[2]), n[2], p(a[3]), n[3], p(a[4]), p(a[5]), p(a[6]), p(a[7]), C.byref(s), p(out), p(ops), capacity,
                                       C.byref(total), None)
    return rc, total.value


@functools.lru_cache(maxsize=None)
def small_case():
    rng = np.random.default_rng(9)
    specs = cases.random_specs(rng, 40) + [cases.chain_spec([6, 6], [(30, 40)]), cases.chain_spec([6, 6], [(16, 16)])]
    case = cases.build(rng, specs)
    return case, [case[k] for k in NAMES], [len(case["chains"]), len(case["anchors"]), len(case["positions"]), len(case["spans"])]


def test_host_and_device_memory_for_each_array():
    case, arrays, n = small_case()
    want = device(case, band=2)
    nc, total = n[0], len(want.ops)
    for where in range(1 << 10):
        if where not in (0, 1023) and bin(where).count("1") not in (1, 9):
            continue                                                 # all host, all device, each array alone on either side
        bufs = []

        def place(k, array):
            if not where >> k & 1:
                return array
            bufs.append(fm.DeviceBuffer.from_array(array))
            return bufs[-1]
        out, ops = np.zeros(nc, dtype=CHAIN_ALIGNMENT_DTYPE), np.zeros(total, dtype=np.uint32)
        placed = [place(k, a) for k, a in enumerate(arrays)]
        o, p = place(8, out), place(9, ops)
        assert raw_call(placed, n, case["nq"], o, p, total) == (0, total), (where, capi.lib().fmgpu_last_error())
        back = lambda a, dtype, m: a.to_array(dtype, m) if isinstance(a, fm.DeviceBuffer) else a      # noqa: E731
        assert back(o, CHAIN_ALIGNMENT_DTYPE, nc).tobytes() == want.alignments.tobytes() and back(p, np.uint32, total).tobytes() == want.ops.tobytes()
        for b in bufs:
            b.free()
    # device-resident input through the Python layer
    bufs = {k: fm.DeviceBuffer.from_array(case[k]) for k in NAMES}
    res = fm.align_chains(None, (bufs["chains"], bufs["anchors"]), bufs["positions"], bufs["spans"], (bufs["qbuf"], bufs["qoff"]), text=(bufs["tbuf"], bufs["toff"]), band=2)
    assert res.alignments.tobytes() == want.alignments.tobytes() and res.ops.tobytes() == want.ops.tobytes()
    for b in bufs.values():
        b.free()


def test_the_counting_call_and_capacity():
    case, arrays, n = small_case()
    want = device(case, band=2)
    nc, total = n[0], len(want.ops)
    out = np.zeros(nc, dtype=CHAIN_ALIGNMENT_DTYPE)
    assert raw_call(arrays, n, case["nq"], out, None, 0) == (0, total) and out.tobytes() == want.alignments.tobytes()
    out[:] = 0
    ops = np.full(total, 0xAAAAAAAA, dtype=np.uint32)
    assert raw_call(arrays, n, case["nq"], out, ops, total - 1) == (capi.FMGPU_ERR_CAPACITY, total)
    assert (ops == 0xAAAAAAAA).all() and out.tobytes() == want.alignments.tobytes()
    assert raw_call(arrays, n, case["nq"], out, ops, total) == (0, total) and ops.tobytes() == want.ops.tobytes()
    # every chain left out: no operation at all
    out[:] = 0
    rc, none = raw_call(arrays, n, case["nq"], out, ops, total, max_gap_len=0)
    assert (rc, none) == (0, int(model.align(*cases.model_args(case), band=2, max_gap_len=0)[0][-1][0])) and out["status"][-1] == 1


def test_every_device_side_error_names_the_lowest_offender():
    case, arrays, n = small_case()
    nq = case["nq"]
    nc = n[0]
    out, ops = np.full(nc, 0xAA, dtype=np.uint8).repeat(32).view(CHAIN_ALIGNMENT_DTYPE), np.full(4096, 0xAAAAAAAA, dtype=np.uint32)
    chains = case["chains"]
    a, b = nc // 3, nc // 2
    first = lambda c, k=0: int(case["anchors"][int(chains["first"][c]) + k])                            # noqa: E731: the record of anchor k of chain c

    def refused(what, chain, message, anchor=None, code=capi.FMGPU_ERR_INVALID, **changed):
        bad = dict(case)
        bad.update(changed)
        with pytest.raises(model.AlignError) as e:
            model.align(*cases.model_args(bad), band=2)
        assert (e.value.what, e.value.chain, e.value.anchor, e.value.code) == (what, chain, anchor, code)
        counts = [len(bad["chains"]), len(bad["anchors"]), len(bad["positions"]), len(bad["spans"])]
        rc, total = raw_call([bad[k] for k in NAMES], counts, len(bad["qoff"]) - 1, out, ops, 4096)
        assert rc == code and total == 0 and (out.view(np.uint8) == 0xAA).all() and (ops == 0xAAAAAAAA).all()
        assert capi.lib().fmgpu_last_error() == b"fmgpu_chains_align: chain %d" % chain + message, capi.lib().fmgpu_last_error()

    def edit(name, field, where, value):
        x = case[name].copy()
        if field is None:
            x[where] = value
        else:
            x[field][where] = value
        return x

    # (1) no anchors; anchors beyond n_anchor; more anchors than n_anchor all together.  Other kinds behind it do not matter, whichever chain is lower
    bad = edit("chains", "n_anchors", [a, b], 0)
    bad["qidx"][0] = nq
    refused("anchors", a, b" has no anchors, or anchors beyond n_anchor", chains=bad)
    refused("anchors", b, b" has no anchors, or anchors beyond n_anchor", chains=edit("chains", "first", b, n[1]))
    refused("anchors", nc - 1, b" has no anchors, or anchors beyond n_anchor", chains=edit("chains", "n_anchors", 0, int(chains["n_anchors"][0]) + 1))
    # (2) an anchor index beyond count
    refused("index", a, b" has an anchor index beyond count", anchors=edit("anchors", None, [int(chains["first"][a]), int(chains["first"][b])], [n[2], 0xffffffff]))
    # (3) a hit beyond the spans, a span without symbols
    refused("hit", a, b" has an anchor with a hit beyond the spans or a span with qlen == 0", positions=edit("positions", "hit", [first(a), first(b)], n[3]))
    refused("hit", b, b" has an anchor with a hit beyond the spans or a span with qlen == 0", spans=edit("spans", "qlen", int(case["positions"]["hit"][first(b)]), 0))
    # (4) a query beyond nq; an anchor of another query; of another sequence
    what = b" names a query beyond nq, or has an anchor of another query or sequence"
    refused("query", b, what, chains=edit("chains", "qidx", b, nq))
    refused("query", a, what, positions=edit("positions", "qidx", [first(a), first(b)], 0))
    refused("query", b, what, positions=edit("positions", "seq_id", first(b), 99))
    # (5) two anchors at the same q; at the same t
    two = next(c for c in range(nc) if chains["n_anchors"][c] >= 2)
    what = b" has two consecutive anchors that do not ascend in both q and t"
    refused("order", two, what, positions=edit("positions", "pos", first(two, 1), int(case["positions"]["pos"][first(two)])))
    hit0, hit1 = (int(case["positions"]["hit"][first(two, k)]) for k in (0, 1))
    refused("order", two, what, spans=edit("spans", "qbeg", hit1, int(case["spans"]["qbeg"][hit0])))
    # (6) each of the four ends
    for field in ("tbeg", "tend", "qbeg", "qend"):
        bad = edit("chains", field, a, int(chains[field][a]) + 1)
        if field == "qend":
            bad = edit("chains", field, a, int(chains[field][a]) - 1)
        refused("ends", a, b" has tbeg, tend, qbeg or qend that its first and last anchor do not give", chains=bad)
    # (7) qend beyond the read: the read loses its last symbols (its chain has no tail clip)
    tight = next(c for c in range(nc) if int(chains["qend"][c]) == int(case["qoff"][int(chains["qidx"][c]) + 1] - case["qoff"][int(chains["qidx"][c])]))
    qoff = case["qoff"].copy()
    qoff[int(chains["qidx"][tight]) + 1:] -= 1
    refused("qend", tight, b" has a qend beyond its read", qoff=qoff)
    # (8) a window of another length
    toff = case["toff"].copy()
    toff[b + 1:] += 1
    refused("window", b, b" has a window whose length is not tend - tbeg", toff=toff, tbuf=np.concatenate([case["tbuf"], np.zeros(4, dtype=np.uint8)]))
    # (9) a piece that differs from the read: the lowest chain, then the lowest anchor
    tbuf = case["tbuf"].copy()
    for c in (two, a if a != two else b):
        tbuf[int(case["toff"][c + 1]) - 1] ^= 7                         # the last symbol of the window: the last piece
        tbuf[int(case["toff"][c])] ^= 7                                 # and the first
    low = min(two, a if a != two else b)
    refused("piece", low, b", anchor 0: the text differs from the read", anchor=0, tbuf=tbuf)
    tbuf = case["tbuf"].copy()
    tbuf[int(case["toff"][two + 1]) - 1] ^= 7
    last = int(chains["n_anchors"][two]) - 1
    refused("piece", two, b", anchor %d: the text differs from the read" % last, anchor=last, tbuf=tbuf)
    # and the call still works
    agree(case, band=2)


def test_reads_to_cigars_end_to_end():
    """the reads of the chain tests (three substitutions and a two-base deletion each, half of them reverse-complemented) through search_smems -> locate_hits ->
    chain_seeds -> align_chains with the text read from the index: the device equals the model, and every line replays over the read and the text"""
    seqs, reads, truth = chain_cases.end_to_end()
    gx = fm.BiFMIndex.from_sequences(seqs, 5, "IB16", 4)
    doubled = fm.both_strands(reads)
    hits, spans = fm.search_smems(gx, doubled, min_len=15)
    pos = gx.locate_hits(hits)
    chained = fm.chain_seeds(pos, spans, 2 * len(reads))
    res = fm.align_chains(gx, chained, pos, spans, doubled)
    assert not gx.formats & capi.FMT_EXTRACT                            # the table built for the call is dropped again
    gx.accelerate_extract()
    ch = chained.chains
    tbuf, toff = gx.extract(ch["seq_id"], ch["tbeg"], ch["tend"] - ch["tbeg"])
    qbuf, qoff = doubled
    records, ops = model.align(ch, chained.anchors, pos, spans, qbuf, qoff, tbuf, toff)
    assert res.alignments.tobytes() == np.array(records, dtype=CHAIN_ALIGNMENT_DTYPE).tobytes() and res.ops.tobytes() == np.array(ops, dtype=np.uint32).tobytes()
    assert len(res) == len(ch) >= len(reads) and (res.alignments["status"] == 0).all()
    for k in range(len(res)):
        c, r = ch[k], res.alignments[k]
        Q = qbuf[int(qoff[c["qidx"]]): int(qoff[int(c["qidx"]) + 1])]
        T = tbuf[int(toff[k]): int(toff[k + 1])]
        a, b, count = model.replay(res.ops[int(r["first_op"]): int(r["first_op"]) + int(r["n_ops"])], Q, T)
        assert (a, b) == (len(Q), len(T)) and (count[model.EQ], count[model.X], count[model.I], count[model.D]) == tuple(int(r[f]) for f in ("n_match", "n_mismatch", "n_ins", "n_del"))
    assert (res.alignments["n_del"] > 0).any() and (res.alignments["n_mismatch"] > 0).any()
    # the same with the text handed in and with the index keeping its table
    again = fm.align_chains(None, chained, pos, spans, doubled, text=(tbuf, toff))
    assert again.ops.tobytes() == res.ops.tobytes() and fm.align_chains(gx, chained, pos, spans, doubled).ops.tobytes() == res.ops.tobytes()
    assert gx.formats & capi.FMT_EXTRACT
