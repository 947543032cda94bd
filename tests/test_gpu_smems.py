"""fmgpu_search_smems / fm.search_smems: match lengths, seeds, their intervals and located positions against the brute-force restatement of tests/smem_brute.py
and against the exact search of the same handle.  Every check is exact.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, SEED_SPAN_DTYPE
from tests import smem_brute as sb
from tests.util import oracle_arrays

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ texts, reads and their brute-force results (made once)
def sequences(sigma, big):
    rng = np.random.default_rng(100 + sigma + big)
    if big:                                                         # one long sequence: intervals of the first steps span many blocks of the table
        return [rng.integers(1, sigma, size=70_000, dtype=np.uint8)]
    unit = rng.integers(1, sigma, size=7, dtype=np.uint8)
    seqs = [rng.integers(1, sigma, size=l, dtype=np.uint8) for l in (400, 0, 137, 1, 333)]
    seqs.insert(3, np.tile(unit, 38)[:260])                         # a tandem repeat: intervals of many rows
    return seqs


def reads_for(seqs, sigma, big):
    rng = np.random.default_rng(7 + sigma + big)
    long = max(range(len(seqs)), key=lambda i: len(seqs[i]))
    src = seqs[long]

    def window(length, subs=0, seq=None):
        s = src if seq is None else seqs[seq]
        at = int(rng.integers(0, len(s) - length + 1))
        r = s[at: at + length].copy()
        for _ in range(subs):
            p = int(rng.integers(0, length))
            r[p] = (int(r[p]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1
        return r

    reads = [window(l, subs) for l, subs in ((1, 0), (63, 1), (64, 0), (65, 2), (128, 3), (129, 1), (300, 3), (300, 0), (40, 0), (101, 2))]
    reads.append(np.zeros(0, dtype=np.uint8))                       # an empty read
    if not big:
        reads += [window(90, 1, seq=3), window(30, 0, seq=3), seqs[2].copy(), seqs[4][:1].copy()]     # inside the tandem repeat; a whole sequence; one symbol
    reads.append(np.concatenate([window(50), window(45)]))          # chimeras of two windows
    reads.append(np.concatenate([window(33, 1), window(70, 1)]))
    for foreign in ((0,), (sigma,), (255,), (0, sigma, 255, 0)):    # delimiters and bytes outside the alphabet: breaks
        r = window(80)
        for k, c in enumerate(foreign):
            r[(11 + 19 * k) % 80] = c
        reads.append(r)
    reads.append(np.array([255, 0, sigma], dtype=np.uint8))         # nothing but breaks
    reads.append(np.zeros(0, dtype=np.uint8))
    reads.append(window(64))
    return reads


@functools.lru_cache(maxsize=None)
def case(sigma, big):
    """(sequences, reads, their brute-force Batch): computed once, shared by every test, never modified"""
    seqs = sequences(sigma, big)
    reads = reads_for(seqs, sigma, big)
    return seqs, reads, sb.Batch(seqs, reads, sigma)


@functools.lru_cache(maxsize=None)
def tiny_batches(sigma):
    """batches of 1, 63, 64, 65 and 257 symbols: the wave and block boundaries of a one-lane-per-symbol grid"""
    seqs = sequences(sigma, False)
    out = []
    for total, cut in ((1, (1,)), (63, (20, 43)), (64, (64,)), (65, (64, 1)), (257, (128, 0, 129))):
        reads, at = [], 5
        for l in cut:
            reads.append(seqs[0][at: at + l].copy())
            at += l + 3
        assert sum(len(r) for r in reads) == total
        out.append((reads, sb.Batch(seqs, reads, sigma)))
    return seqs, out


def flat(reads, qoff0=0):
    """(qbuf, qoff) with qoff[0] = qoff0: bytes in front of the batch that no read owns"""
    qbuf, qoff = fm.flatten(reads)
    if qoff0:
        qbuf = np.concatenate([np.full(qoff0, 3, dtype=np.uint8), qbuf])
        qoff = qoff + np.uint64(qoff0)
    return qbuf, qoff


def records(hits, spans):
    return [(int(h["qidx"]), int(s["qbeg"]), int(s["qlen"]), int(h["seq"]), int(h["len"])) for h, s in zip(hits, spans)]


# ------------------------------------------------------------------------------------------------ the checks of one handle
def check_batch(gx, seqs, reads, brute, qoff0=0, locate=True):
    queries = flat(reads, qoff0)
    hits, spans, lengths, st = fm.search_smems(gx, queries, want_lengths=True, want_stats=True)
    assert lengths.tolist() == brute.lengths
    want = brute.seeds()
    assert records(hits, spans) == want                              # (qidx, qbeg, qlen, seq) in order, len = the brute occurrence count
    assert not hits["lb_rev"].any() and not hits["errors"].any()
    assert st.lf_steps == brute.steps and st.hits == len(want)
    if want:                                                        # every interval is the exact search's, on the same handle
        lb, ln = fm.search_no_errors.search(gx, [reads[q][b: b + l] for q, b, l, _, _ in want])
        assert np.array_equal(hits["lb"], lb) and np.array_equal(hits["len"], ln)
    if locate and want:
        pos = gx.locate_hits(hits)
        assert pos.size == int(hits["len"].sum())
        for p in pos:
            q, b, l, _, _ = want[int(p["hit"])]
            assert int(p["qidx"]) == q == int(hits["qidx"][int(p["hit"])])
            at = int(p["pos"])
            assert seqs[int(p["seq_id"])][at: at + l].tobytes() == reads[q][b: b + l].tobytes() and l == int(spans[int(p["hit"])]["qlen"])
    return hits, spans, lengths, st


def check_handle(gx, sigma, big=False):
    seqs, reads, brute = case(sigma, big)
    hits, spans, lengths, _ = check_batch(gx, seqs, reads, brute)
    count = len(hits)
    assert count > len(reads) // 2
    # qoff[0] != 0
    h2, s2, l2, _ = check_batch(gx, seqs, reads, brute, qoff0=13, locate=False)
    assert h2.tobytes() == hits.tobytes() and s2.tobytes() == spans.tobytes()
    # the filters
    for min_len in (1, 4, 12):
        for max_rows in (0, 1, 5):
            fh, fs = fm.search_smems(gx, reads, min_len=min_len, max_rows=max_rows)
            assert records(fh, fs) == brute.seeds(min_len, max_rows), (min_len, max_rows)
    assert len(brute.seeds(12, 0)) < count and len(brute.seeds(1, 1)) < count and brute.seeds(1, 5) != brute.seeds(1, 1)
    # capacity = count - 1: the count, untouched outputs, and the match lengths all the same
    qbuf, qoff = flat(reads)
    L = capi.lib()
    out = np.full((count + 2) * HIT_DTYPE.itemsize, 0xA5, dtype=np.uint8).view(HIT_DTYPE)
    span = np.full((count + 2) * SEED_SPAN_DTYPE.itemsize, 0x5A, dtype=np.uint8).view(SEED_SPAN_DTYPE)
    ml, cnt = np.full(len(brute.lengths), 0xFFFFFFFF, dtype=np.uint32), C.c_uint64()
    rc = L.fmgpu_search_smems(gx._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), 1, 0, capi.ptr(out), capi.ptr(span), count - 1, C.byref(cnt), capi.ptr(ml), None, None)
    assert rc == capi.FMGPU_ERR_CAPACITY and cnt.value == count
    assert (out.view(np.uint8) == 0xA5).all() and (span.view(np.uint8) == 0x5A).all()
    assert ml.tolist() == brute.lengths
    rc = L.fmgpu_search_smems(gx._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), 1, 0, capi.ptr(out), capi.ptr(span), count, C.byref(cnt), None, None, None)
    assert rc == 0 and cnt.value == count and out[:count].tobytes() == hits.tobytes() and span[:count].tobytes() == spans.tobytes()
    assert (out[count:].view(np.uint8) == 0xA5).all() and (span[count:].view(np.uint8) == 0x5A).all()
    # the 4-bit packed form: the byte call on the unpacked batch (a byte >= sigma comes back as 255: a break either way)
    if sigma <= 15:
        for packed in (fm.pack_queries(reads, sigma), fm.pack_queries_device(flat(reads, 13), sigma)):
            ph, ps, pl, pst = fm.search_smems(gx, packed, want_lengths=True, want_stats=True)
            assert ph.tobytes() == hits.tobytes() and ps.tobytes() == spans.tobytes() and pl.tolist() == brute.lengths and pst.lf_steps == brute.steps
    else:
        p4 = np.zeros(8, dtype=np.uint8)
        rc = L.fmgpu_search_smems_q4(gx._h, capi.ptr(p4), capi.ptr(np.array([0, 4], dtype=np.uint64)), 1, 1, 0, capi.ptr(out), capi.ptr(span), count, C.byref(cnt), None, None, None)
        assert rc == capi.FMGPU_ERR_UNSUPPORTED
    # batches that end on a wave or block boundary
    if not big:
        tseqs, tiny = tiny_batches(sigma)
        for treads, tbrute in tiny:
            check_batch(gx, tseqs, treads, tbrute, locate=False)
    return hits, spans


# ------------------------------------------------------------------------------------------------ the handles
@pytest.mark.parametrize("bidir", [False, True])
@pytest.mark.parametrize("wide", [0, 1])
def test_built_index(bidir, wide):
    seqs, _, _ = case(5, False)
    with fm.options(force_wide=wide):
        gx = (fm.BiFMIndex if bidir else fm.FMIndex).from_sequences(seqs, 5, "IB16", 4)
    assert gx.row_bits == (64 if wide else 32)
    check_handle(gx, 5)


LAYOUTS = [("IB16", 5, {}), ("EPR16", 5, {"expand_dna": 0}), ("EPR16", 5, {"expand_dna": 1}), ("FBV_512_64K", 5, {}),
           ("WAVELET", 21, {"symbol_planes": 0}), ("WAVELET", 21, {"symbol_planes": 1})]


@pytest.mark.parametrize("layout,sigma,opts", LAYOUTS)
@pytest.mark.parametrize("wide", [0, 1])
def test_reference_layouts(layout, sigma, opts, wide):
    seqs, _, _ = case(sigma, False)
    bidir = layout in ("IB16", "WAVELET")
    ox = fo.OraIndex.build(layout, sigma, seqs, 3, bidir)
    with fm.options(force_wide=wide, **opts):
        gx = (fm.BiFMIndex if bidir else fm.FMIndex).from_reference_arrays(**oracle_arrays(ox))
    assert gx.row_bits == (64 if wide else 32)
    check_handle(gx, sigma)


def test_long_sequence():
    seqs, _, _ = case(5, True)
    gx = fm.FMIndex.from_sequences(seqs, 5, "IB16", 16)
    check_handle(gx, 5, big=True)


# ------------------------------------------------------------------------------------------------ memory spaces, errors
def test_device_buffers_on_a_caller_stream():
    import torch
    seqs, reads, brute = case(5, False)
    gx = fm.BiFMIndex.from_sequences(seqs, 5, "IB16", 4)
    hits, spans, lengths = fm.search_smems(gx, reads, want_lengths=True)
    count, total = len(hits), len(brute.lengths)
    qbuf, qoff = flat(reads, 5)
    stream = torch.cuda.Stream()
    L = capi.lib()
    dq, do = fm.DeviceBuffer.from_array(qbuf), fm.DeviceBuffer.from_array(qoff)
    dh, ds, dl = fm.DeviceBuffer((count + 1) * HIT_DTYPE.itemsize), fm.DeviceBuffer((count + 1) * 8), fm.DeviceBuffer(total * 4)
    cnt = C.c_uint64()
    rc = L.fmgpu_search_smems(gx._h, capi.ptr(dq), capi.ptr(do), len(reads), 1, 0, capi.ptr(dh), capi.ptr(ds), count + 1, C.byref(cnt), capi.ptr(dl), None,
                              C.c_void_p(stream.cuda_stream))
    capi.check(rc)
    assert cnt.value == count                                        # (the call returns after completion)
    assert dh.to_array(HIT_DTYPE, count).tobytes() == hits.tobytes() and ds.to_array(SEED_SPAN_DTYPE, count).tobytes() == spans.tobytes()
    assert dl.to_array(np.uint32, total).tolist() == brute.lengths == lengths.tolist()
    # the records go into fmgpu_locate_hits where they are
    pos = gx.locate_hits(dh.to_array(HIT_DTYPE, count))
    dpos = fm.DeviceBuffer(max(pos.size, 1) * capi.POSITION_DTYPE.itemsize)
    rc = L.fmgpu_locate_hits(gx._h, capi.ptr(dh), count, capi.ptr(dpos), pos.size, C.byref(cnt), None, C.c_void_p(stream.cuda_stream))
    capi.check(rc)
    assert cnt.value == pos.size and dpos.to_array(capi.POSITION_DTYPE, pos.size).tobytes() == pos.tobytes()
    # packed queries in device memory
    pq = fm.pack_queries_device((dq, do), 5)
    ph, ps = fm.search_smems(gx, pq)
    assert ph.tobytes() == hits.tobytes() and ps.tobytes() == spans.tobytes()
    for b in (dq, do, dh, ds, dl, dpos, pq.packed, pq.qoff):
        b.free()


def test_argument_errors_and_empty_batches():
    seqs, reads, brute = case(5, False)
    gx = fm.FMIndex.from_sequences(seqs, 5, "IB16", 4)
    L = capi.lib()
    qbuf, qoff = flat(reads)
    nq = len(reads)
    out, span, cnt = np.zeros(4, dtype=HIT_DTYPE), np.zeros(4, dtype=SEED_SPAN_DTYPE), C.c_uint64(7)
    for call in (L.fmgpu_search_smems, L.fmgpu_search_smems_q4):
        for args in ((None, capi.ptr(qoff), nq, 1, 0, capi.ptr(out), capi.ptr(span), 4, C.byref(cnt)),
                     (capi.ptr(qbuf), None, nq, 1, 0, capi.ptr(out), capi.ptr(span), 4, C.byref(cnt)),
                     (capi.ptr(qbuf), capi.ptr(qoff), nq, 1, 0, capi.ptr(out), capi.ptr(span), 4, None),
                     (capi.ptr(qbuf), capi.ptr(qoff), nq, 1, 0, None, capi.ptr(span), 4, C.byref(cnt)),
                     (capi.ptr(qbuf), capi.ptr(qoff), nq, 1, 0, capi.ptr(out), None, 4, C.byref(cnt))):
            assert call(gx._h, *args, None, None, None) == capi.FMGPU_ERR_INVALID
        assert call(gx._h, None, None, 0, 1, 0, None, None, 0, C.byref(cnt), None, None, None) == 0 and cnt.value == 0
    # capacity 0 with null outputs: the count alone
    assert L.fmgpu_search_smems(gx._h, capi.ptr(qbuf), capi.ptr(qoff), nq, 1, 0, None, None, 0, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_CAPACITY
    assert cnt.value == len(brute.seeds())
    # reads without a symbol, and a batch without a match
    hits, spans, lengths = fm.search_smems(gx, [np.zeros(0, dtype=np.uint8)] * 3, want_lengths=True)
    assert len(hits) == 0 and len(spans) == 0 and lengths.size == 0
    hits, spans, lengths, st = fm.search_smems(gx, [np.array([0, 255, 5], dtype=np.uint8)], want_lengths=True, want_stats=True)
    assert len(hits) == 0 and lengths.tolist() == [0, 0, 0] and st.lf_steps == 0 and st.hits == 0
    # the retry of the host layer: a capacity that is too small is grown to the count the call reported
    small, _ = fm.search_smems(gx, reads, capacity=1)
    assert records(small, fm.search_smems(gx, reads)[1]) == brute.seeds()
