"""fmgpu_map / _q4, fmgpu_hits_from_intervals and fmgpu_feed_map / _v on the device (include/fmgpu.h).  Expected values come only from the calls the chain is made
of — fmgpu_search_best[_ng21] -> fmgpu_hits_sort -> fmgpu_locate_hits, and for exact search fmgpu_search_exact plus a NumPy restatement of the hits_from_intervals rule;
the Hamming ladders are additionally held against a brute-force scan of the sequences.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, POSITION_DTYPE
from tests.util import make_text

pytestmark = pytest.mark.gpu
UNLIMITED = fm.UINT64_MAX
BLOCK_LEN = 30                                                       # the equal-length block: what the ng21 ladder is expanded for
LENGTHS = [0, 0, 1, 2, 3, 7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 55, 60, 63, 64, 65, 66, 67, 68, 69, 70, 70, 70, 5, 9, 11, 13, 21, 27, 39, 43, 58, 40, 36, 24]


@functools.lru_cache(maxsize=None)
def sequences(sigma):
    """sigma = 5: three sequences, about 6 000 symbols, with 12 copies of one 40-symbol block planted in the second one"""
    if sigma != 5:
        return [make_text(4000, sigma, seed=32)]
    t = make_text(6000, 5, seed=41)
    block = make_text(40, 5, seed=42)
    mid = t[2500:4500].copy()
    for k in range(12):
        mid[100 + 150 * k: 140 + 150 * k] = block
    return [t[:2500].copy(), mid, t[4500:].copy()]


@functools.lru_cache(maxsize=None)
def batch(sigma):
    """60 reads (sigma = 5) of lengths 0 .. 70 — cut from the text with 0, 1 or 2 substitutions, or random; bytes 0, sigma and 255 inside a few; two from the repeat; and
    the equal-length block: 20 reads of 30 symbols"""
    rng = np.random.default_rng(5)
    seqs = sequences(sigma)
    reads = []

    def cut(m, subs):
        s = seqs[int(rng.integers(0, len(seqs)))]
        at = int(rng.integers(0, len(s) - m + 1))
        r = s[at: at + m].copy()
        for p in rng.choice(m, size=min(subs, m), replace=False) if m else []:
            r[p] = (int(r[p]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1
        return r

    for i, m in enumerate(LENGTHS):
        r = cut(m, (i // 4) % 3) if i % 4 != 3 else rng.integers(1, sigma, size=m, dtype=np.uint8)
        if m >= 40 and i % 5 == 0:
            r[m // 2] = (0, sigma, 255)[(i // 5) % 3]
        reads.append(r)
    if sigma == 5:
        rep = seqs[1]
        reads += [rep[100:140].copy(), rep[255:285].copy()]               # the whole planted block (12 rows), and 30 symbols inside a copy
        for i in range(20):
            reads.append(cut(BLOCK_LEN, i % 3) if i % 4 != 3 else rng.integers(1, sigma, size=BLOCK_LEN, dtype=np.uint8))
    qbuf, qoff = fm.flatten(reads)
    return reads, qbuf, qoff


@functools.lru_cache(maxsize=None)
def index(kind):
    if kind == "wavelet":
        return fm.FMIndex.from_sequences(sequences(28), 28, "WAVELET", 4)
    cls = fm.BiFMIndex if kind.startswith("bi") else fm.FMIndex
    with fm.options(force_wide=1 if kind.endswith("_wide") else 0):
        gx = cls.from_sequences(sequences(5), 5, "IB16", 4)
    assert gx.row_bits == (64 if kind.endswith("_wide") else 32)
    return gx


def sigma_of(ix):
    return 28 if ix == "wavelet" else 5


def ladder_of(mode):
    if mode == "ng21":
        return [fm.search_scheme.expand(fm.search_scheme.pigeon_opt(k, k), BLOCK_LEN) for k in range(3)]
    return [fm.search_scheme.h2(k + 2, 0, k) for k in range(3)]


def map_query(mode, n=UNLIMITED, locate=True, first=0, ladder=None):
    """(capi.MapQuery, keep-alive) for mode exact / hamming / edit / ng21"""
    if mode == "exact":
        return fm._map_query(0, None, False, True, n, locate, first)
    return fm._map_query(None, ladder_of(mode) if ladder is None else ladder, mode == "ng21", mode == "edit", n, locate, first)


@functools.lru_cache(maxsize=None)
def expected(ix, mode, n=UNLIMITED, nladder=3):
    """(H, P, stratum) composed from the calls the chain is made of"""
    gx = index(ix)
    reads, qbuf, qoff = batch(sigma_of(ix))
    nq = len(reads)
    if mode == "exact":
        lb, ln = fm.search_no_errors.search(gx, (qbuf, qoff))
        keep = np.nonzero((ln > 0) & (np.diff(qoff.astype(np.int64)) > 0) & (n > 0))[0]
        hits = np.zeros(keep.size, dtype=HIT_DTYPE)
        hits["qidx"], hits["lb"], hits["len"] = keep, lb[keep], np.minimum(ln[keep], np.uint64(n))
        stratum = np.full(nq, 255, dtype=np.uint8)
        stratum[keep] = 0
    elif mode == "ng21":
        hits, stratum = fm.search_ng21.search_best(gx, (qbuf, qoff), ladder_of(mode)[:nladder], n, want_stratum=True)
    else:
        hits, stratum = fm.search_best(gx, (qbuf, qoff), None, n, edit=(mode == "edit"), schemes=[(s, None) for s in ladder_of(mode)[:nladder]], want_stratum=True)
    pos = gx.locate_hits(hits) if len(hits) else np.zeros(0, dtype=POSITION_DTYPE)
    return np.ascontiguousarray(hits), np.ascontiguousarray(pos), np.ascontiguousarray(stratum)


def raw(target, a, b, nq, what, cap, hcap, pos=None, hits=None, stratum=None, name="fmgpu_map", stats=False):
    """the C call -> (rc, P buffer, P count, H buffer, H count, stratum buffer[, search stats, locate stats]); hits=False: out_hits = NULL"""
    call = getattr(capi.lib(), name)
    pos = np.zeros(max(cap, 1), dtype=POSITION_DTYPE) if pos is None else pos
    if hits is None:
        hits = np.zeros(max(hcap, 1), dtype=HIT_DTYPE)
    if stratum is None:
        stratum = np.full(max(nq, 1), 77, dtype=np.uint8)
    cnt, hcnt = C.c_uint64(12345), C.c_uint64(12345)
    sstats, lstats = (capi.Stats * max(1, what.n_schemes))(), capi.Stats()
    args = [target, capi.ptr(a), capi.ptr(b), nq, C.byref(what), capi.ptr(pos), cap, C.byref(cnt), None if hits is False else capi.ptr(hits), hcap, C.byref(hcnt),
            capi.ptr(stratum), sstats if stats else None, C.byref(lstats) if stats else None]
    rc = call(*(args + ([] if "feed" in name else [None])))
    res = (rc, pos, int(cnt.value), hits, int(hcnt.value), stratum)
    return res + ([sstats[i] for i in range(max(1, what.n_schemes))], lstats) if stats else res


def agrees(got, want, nq, located=True):
    rc, pos, cnt, hits, hcnt, stratum = got[:6]
    H, P, S = want
    assert rc == 0, capi.lib().fmgpu_last_error()
    assert hcnt == len(H) and hits[:hcnt].tobytes() == H.tobytes()
    assert cnt == (len(P) if located else 0) and (not located or pos[:cnt].tobytes() == P.tobytes())
    assert np.array_equal(stratum[:nq], S)
    return True


def test_the_fixture_is_a_test_of_the_ladder():
    H, P, S = expected("bi", "hamming")
    assert all(int((S == k).sum()) >= 5 for k in range(3)) and int((S == 255).sum()) >= 5, np.bincount(S)
    assert int(H["len"].max()) >= 12
    assert len(P) == int(H["len"].sum()) and np.array_equal(P["hit"], np.repeat(np.arange(len(H), dtype=np.uint32), H["len"].astype(np.int64)))


def brute_force(reads, seqs, sigma, kmax):
    """per read the best stratum k <= kmax with any occurrence (stratum k searches h2(k + 2, 0, k): reads shorter than k + 2 parts are skipped), and all its occurrences"""
    out = set()
    for q, r in enumerate(reads):
        m = len(r)
        r = np.asarray(r).astype(np.int64)
        r[(r < 1) | (r >= sigma)] = -1                               # never equal to a text symbol: always a mismatch
        for k in range(kmax + 1):
            if m < k + 2:
                continue
            occ = []
            for sid, s in enumerate(seqs):
                if len(s) < m:
                    continue
                win = np.lib.stride_tricks.sliding_window_view(s.astype(np.int64), m)
                d = (win != r[None, :]).sum(axis=1)
                occ += [(q, sid, int(p), int(d[p])) for p in np.nonzero(d <= k)[0]]
            if occ:
                out.update(occ)
                break
    return out


@pytest.mark.parametrize("ix", ["bi", "bi_wide"])
def test_hamming_ladder_against_a_brute_force_scan(ix):
    reads, qbuf, qoff = batch(5)
    pos = fm.map_reads(index(ix), (qbuf, qoff), errors=2, edit=False)
    got = set(zip(pos["qidx"].tolist(), pos["seq_id"].tolist(), pos["pos"].tolist(), pos["errors"].tolist()))
    assert len(got) == len(pos)                                      # a Hamming occurrence is reported once
    assert got == brute_force(reads, sequences(5), 5, 2)


@pytest.mark.parametrize("ix,mode", [("bi", "hamming"), ("bi", "edit"), ("bi", "ng21"), ("bi_wide", "hamming"), ("bi_wide", "edit"), ("bi_wide", "ng21"),
                                     ("bi", "exact"), ("fm", "exact"), ("bi_wide", "exact"), ("wavelet", "exact")])
def test_map_equals_the_composition(ix, mode):
    gx = index(ix)
    reads, qbuf, qoff = batch(sigma_of(ix))
    nq = len(reads)
    for n in (UNLIMITED, 3, 0):
        want = expected(ix, mode, n)
        H, P, S = want
        what, keep = map_query(mode, n)
        got = raw(gx._h, qbuf, qoff, nq, what, len(P), len(H), stats=True)
        assert agrees(got, want, nq), (n,)
        sstats, lstats = got[6], got[7]
        assert sum(s.hits for s in sstats) == len(H) if mode != "exact" else sstats[0].lf_steps > 0
        assert lstats.hits == len(P)
        if n == 0:
            assert len(P) == 0 and (S == 255).all() and (len(H) == 0 or mode == "ng21")      # (search_ng21 with n = 0 reports its cursors clipped to no row)
        # locate = 0 stops after H
        what0, keep0 = map_query(mode, n, locate=False)
        assert agrees(raw(gx._h, qbuf, qoff, nq, what0, 0, len(H), pos=None), want, nq, located=False)
    # first_records = 1: both scratches grow, the results are identical
    want = expected(ix, mode)
    H, P, S = want
    assert len(H) > 6 and len(P) > 8
    what, keep = map_query(mode, first=1)
    assert agrees(raw(gx._h, qbuf, qoff, nq, what, len(P) + 5, len(H) + 5), want, nq)
    # single-scheme ladders (n_schemes = 1)
    if mode in ("hamming", "ng21"):
        what1, keep1 = map_query(mode, ladder=ladder_of(mode)[:1])
        w1 = expected(ix, mode, UNLIMITED, 1)
        assert agrees(raw(gx._h, qbuf, qoff, nq, what1, len(w1[1]), len(w1[0])), w1, nq)


@pytest.mark.parametrize("ix,mode", [("bi", "hamming"), ("bi_wide", "ng21"), ("fm", "exact")])
def test_capacities_counts_device_pointers_and_packed_batches(ix, mode):
    gx = index(ix)
    reads, qbuf, qoff = batch(5)
    nq = len(reads)
    want = expected(ix, mode)
    H, P, S = want
    what, keep = map_query(mode)
    for cap in (len(P), len(P) - 1, 0):
        for hcap in (len(H), len(H) - 1, 0):
            rc, pos, cnt, hits, hcnt, stratum = raw(gx._h, qbuf, qoff, nq, what, cap, hcap)
            assert (cnt, hcnt) == (len(P), len(H)), (cap, hcap)      # exact totals, whatever the capacities
            assert rc == (0 if cap == len(P) and hcap == len(H) else capi.FMGPU_ERR_CAPACITY), (cap, hcap)
            if rc == 0:
                assert agrees((rc, pos, cnt, hits, hcnt, stratum), want, nq)
    # out_hits = NULL: only the positions count
    rc, pos, cnt, _, hcnt, stratum = raw(gx._h, qbuf, qoff, nq, what, len(P), 0, hits=False)
    assert rc == 0 and hcnt == len(H) and pos[:cnt].tobytes() == P.tobytes() and np.array_equal(stratum[:nq], S)
    # every buffer in device memory
    dq, do = capi.DeviceBuffer.from_array(qbuf), capi.DeviceBuffer.from_array(qoff)
    dpos, dhits, dstr = capi.DeviceBuffer(max(len(P), 1) * 32), capi.DeviceBuffer(max(len(H), 1) * 40), capi.DeviceBuffer(nq)
    rc, _, cnt, _, hcnt, _ = raw(gx._h, dq, do, nq, what, len(P), len(H), pos=dpos, hits=dhits, stratum=dstr)
    assert rc == 0 and (cnt, hcnt) == (len(P), len(H))
    assert dpos.to_array(POSITION_DTYPE, cnt).tobytes() == P.tobytes() and dhits.to_array(HIT_DTYPE, hcnt).tobytes() == H.tobytes()
    assert np.array_equal(dstr.to_array(np.uint8, nq), S)
    # the packed form gives what the byte call gives
    pq = fm.pack_queries(list(reads), 5)
    assert agrees(raw(gx._h, pq.packed, pq.qoff, nq, what, len(P), len(H), name="fmgpu_map_q4"), want, nq)
    # and the Python face
    pos, hits, stratum = fm.map_reads(gx, pq if mode != "exact" else (qbuf, qoff), want_hits=True, want_stratum=True,
                                      **(dict(errors=0) if mode == "exact" else dict(schemes=ladder_of(mode), ng21=mode == "ng21", edit=False)))
    assert pos.tobytes() == P.tobytes() and hits.tobytes() == H.tobytes() and np.array_equal(stratum, S)


def test_map_errors_are_those_of_the_pieces():
    L = capi.lib()
    reads, qbuf, qoff = batch(5)
    nq = len(reads)
    what, keep = map_query("hamming")
    assert raw(index("fm")._h, qbuf, qoff, nq, what, 10, 10)[0] == capi.FMGPU_ERR_INVALID              # a unidirectional handle
    wreads, wq, wo = batch(28)
    whatx, _ = map_query("exact")
    assert raw(index("wavelet")._h, wq, wo, len(wreads), whatx, 10, 10, name="fmgpu_map_q4")[0] == capi.FMGPU_ERR_UNSUPPORTED      # sigma > 15
    bad = [np.asarray(x).copy() for x in ladder_of("hamming")[1]]
    bad[0][0, 0] = 99                                                                                  # not a permutation
    whatb, keepb = map_query("hamming", ladder=[ladder_of("hamming")[0], tuple(bad)])
    rc = raw(index("bi")._h, qbuf, qoff, nq, whatb, 10, 10)[0]
    arr, keep2 = fm._map_query(None, [tuple(bad)], False, False, UNLIMITED, True, 0)
    one = np.zeros(4, dtype=HIT_DTYPE)
    cnt = C.c_uint64()
    assert rc != 0 and rc == L.fmgpu_search_scheme(index("bi")._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.cast(C.c_void_p(arr.schemes), C.POINTER(capi.Scheme)), UNLIMITED, capi.ptr(one), 4,
                                                   C.byref(cnt), None, None)
    assert raw(index("bi")._h, None, qoff, nq, what, 10, 10)[0] == capi.FMGPU_ERR_INVALID


@pytest.mark.parametrize("nq", [1, 256, 257, 5000])
def test_hits_from_intervals(nq):
    L = capi.lib()
    rng = np.random.default_rng(nq)
    ln = np.where(np.arange(nq) % 3 == 0, rng.integers(1, 50, size=nq), 0).astype(np.uint64)          # every third read found
    lb = rng.integers(0, 1 << 20, size=nq).astype(np.uint64) + (np.uint64(1) << np.uint64(33)) * (np.arange(nq, dtype=np.uint64) % np.uint64(5))   # some above 2^32
    lens = rng.integers(1, 9, size=nq)
    lens[::6] = 0                                                      # every second found read is empty
    qoff = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.uint64)
    for off in (None, qoff):
        for base, rows in ((0, UNLIMITED), (1000, 7), (5, 0)):
            yes = (ln > 0) & (rows > 0) & ((lens > 0) if off is not None else True)
            keep = np.nonzero(yes)[0]
            want = np.zeros(keep.size, dtype=HIT_DTYPE)
            want["qidx"], want["lb"], want["len"] = keep + base, lb[keep], np.minimum(ln[keep], np.uint64(rows))
            wstr = np.where(yes, 0, 255).astype(np.uint8)
            for device in (False, True):
                out, strat, cnt = np.full(keep.size + 2, 0x5a, dtype=np.uint8).repeat(40).view(HIT_DTYPE), np.full(nq, 77, dtype=np.uint8), C.c_uint64(99)
                a, b, c = (capi.DeviceBuffer.from_array(x) if device and x is not None else x for x in (lb, ln, off))
                o, s = (capi.DeviceBuffer.from_array(out), capi.DeviceBuffer.from_array(strat)) if device else (out, strat)
                assert L.fmgpu_hits_from_intervals(capi.ptr(a), capi.ptr(b), capi.ptr(c), nq, base, rows, capi.ptr(o), keep.size, C.byref(cnt), capi.ptr(s), None) == 0
                if device:
                    out, strat = o.to_array(HIT_DTYPE, keep.size + 2), s.to_array(np.uint8, nq)
                assert cnt.value == keep.size and out[: keep.size].tobytes() == want.tobytes() and np.array_equal(strat, wstr), (off is None, base, rows, device)
                assert out[keep.size:].tobytes() == bytes([0x5a]) * 80                                     # nothing behind the records
            if keep.size:                                              # one record short: the count, and nothing written
                out, cnt = np.full((keep.size - 1 + 1) * 40, 0x5a, dtype=np.uint8), C.c_uint64(99)
                assert L.fmgpu_hits_from_intervals(capi.ptr(lb), capi.ptr(ln), capi.ptr(off), nq, base, rows, capi.ptr(out), keep.size - 1, C.byref(cnt), None, None) == capi.FMGPU_ERR_CAPACITY
                assert cnt.value == keep.size and (out == 0x5a).all()


FEED_CONFIGS = (dict(chunk_reads=1), dict(chunk_reads=5), dict(chunk_reads=62), dict(chunk_reads=1000), dict(chunk_reads=5, slots=3), dict(chunk_reads=5, slots=4),
                dict(chunk_symbols=100))


def plan_chunks(qoff, cfg):
    nq = len(qoff) - 1
    n = C.c_uint64()
    out = np.zeros(nq + 2, dtype=np.uint64)
    capi.check(capi.lib().fmgpu_feed_plan(capi.ptr(qoff), nq, cfg.get("chunk_reads", 1 << 20), cfg.get("chunk_symbols", 128 << 20), capi.ptr(out), nq + 1, C.byref(n)))
    return int(n.value)


@pytest.mark.parametrize("ix,mode", [("bi", "hamming"), ("bi_wide", "edit"), ("bi", "ng21"), ("fm", "exact"), ("wavelet", "exact")])
def test_feed_map_equals_map_for_every_chunking(ix, mode):
    gx = index(ix)
    reads, qbuf, qoff = batch(sigma_of(ix))
    nq = len(reads)
    assert nq == 62 or ix == "wavelet"
    want = expected(ix, mode)
    H, P, S = want
    what, keep = map_query(mode)
    ptrs = np.fromiter((r.ctypes.data for r in reads), dtype=np.uint64, count=nq)
    lens = np.fromiter((r.size for r in reads), dtype=np.uint64, count=nq)
    for cfg in FEED_CONFIGS:
        with fm.Feed(gx, **cfg) as f:
            got = raw(f._f, qbuf, qoff, nq, what, len(P), len(H), name="fmgpu_feed_map", stats=True)
            assert agrees(got, want, nq), cfg
            assert f.info()["chunks"] == plan_chunks(qoff, cfg), cfg
            assert got[7].hits == len(P) and (mode == "exact" or sum(s.hits for s in got[6]) == len(H)), cfg      # stats are sums over the chunks
            assert agrees(raw(f._f, ptrs, lens, nq, what, len(P), len(H), name="fmgpu_feed_map_v"), want, nq), cfg
    # first_records = 1 per chunk, and the slots' buffers only grow
    what1, keep1 = map_query(mode, first=1)
    with fm.Feed(gx, chunk_reads=20) as f:
        assert agrees(raw(f._f, qbuf, qoff, nq, what1, len(P), len(H), name="fmgpu_feed_map"), want, nq)
        before = f.info()
        assert agrees(raw(f._f, qbuf, qoff, nq, what1, len(P), len(H), name="fmgpu_feed_map"), want, nq)
        assert f.info()["device_bytes"] >= before["device_bytes"] and f.info()["pinned_bytes"] >= before["pinned_bytes"]
    # pinned inputs and outputs: read and written in place
    pin = [capi.PinnedBuffer.from_array(x) for x in (qbuf, qoff)] + [capi.PinnedBuffer(max(len(P), 1) * 32), capi.PinnedBuffer(max(len(H), 1) * 40), capi.PinnedBuffer(nq)]
    pq, po = pin[0].array(np.uint8, qbuf.size), pin[1].array(np.uint64, qoff.size)
    ppos, phits, pstr = pin[2].array(POSITION_DTYPE, max(len(P), 1)), pin[3].array(HIT_DTYPE, max(len(H), 1)), pin[4].array(np.uint8, nq)
    with fm.Feed(gx, chunk_reads=7, slots=3) as f:
        assert agrees(raw(f._f, pq, po, nq, what, len(P), len(H), pos=ppos, hits=phits, stratum=pstr, name="fmgpu_feed_map"), want, nq)
        assert f.info()["staged_bytes"] == 0                          # nothing crossed a pinned slot
        # one record short: every chunk still runs, the totals are exact
        for cap, hcap in ((len(P) - 1, len(H)), (len(P), len(H) - 1), (0, 0)):
            rc, _, cnt, _, hcnt, _ = raw(f._f, qbuf, qoff, nq, what, cap, hcap, name="fmgpu_feed_map")
            assert rc == capi.FMGPU_ERR_CAPACITY and (cnt, hcnt) == (len(P), len(H)) and f.info()["chunks"] == plan_chunks(qoff, dict(chunk_reads=7))
        # the Python face
        pos, hits, stratum = f.map((qbuf, qoff), want_hits=True, want_stratum=True,
                                   **(dict(errors=0) if mode == "exact" else dict(schemes=ladder_of(mode), ng21=mode == "ng21", edit=mode == "edit")))
        assert pos.tobytes() == P.tobytes() and hits.tobytes() == H.tobytes() and np.array_equal(stratum, S)
        if mode != "ng21":
            pos = f.map(list(reads), **(dict(errors=0) if mode == "exact" else dict(errors=2, edit=mode == "edit")))
            assert pos.tobytes() == P.tobytes()
    # a feed takes host memory only
    with fm.Feed(gx) as f:
        d = capi.DeviceBuffer.from_array(qbuf)
        assert raw(f._f, d, qoff, nq, what, len(P), len(H), name="fmgpu_feed_map")[0] == capi.FMGPU_ERR_INVALID


def test_two_feeds_on_two_threads_on_one_handle():
    gx = index("bi")
    reads, qbuf, qoff = batch(5)
    nq = len(reads)
    results = {}

    def work(mode, cfg):
        want = expected("bi", mode)
        what, keep = map_query(mode)
        with fm.Feed(gx, **cfg) as f:
            for _ in range(3):
                got = raw(f._f, qbuf, qoff, nq, what, len(want[1]), len(want[0]), name="fmgpu_feed_map")
                results.setdefault(mode, []).append(got)

    expected("bi", "hamming"), expected("bi", "exact")                # (computed before the threads start)
    threads = [threading.Thread(target=work, args=a) for a in (("hamming", dict(chunk_reads=9)), ("exact", dict(chunk_reads=4, slots=3)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for mode in ("hamming", "exact"):
        assert len(results[mode]) == 3 and all(agrees(got, expected("bi", mode), nq) for got in results[mode])
