"""Feeds (include/fmgpu.h: fmgpu_feed_*) on the host: the planner against a restatement of its rule, its error codes, the symbols and the ABI version they leave
alone, and what the feed calls answer without a device."""
import ctypes as C

import numpy as np
import pytest

from fmindex_collection_amd import capi

CALLS = ("fmgpu_feed_create", "fmgpu_feed_destroy", "fmgpu_feed_plan", "fmgpu_feed_search_exact", "fmgpu_feed_search_exact_q4", "fmgpu_feed_search_exact_v",
         "fmgpu_feed_search_scheme", "fmgpu_feed_search_scheme_v", "fmgpu_feed_info", "fmgpu_malloc_host", "fmgpu_free_host")


def plan_by_the_rule(qoff, chunk_reads, chunk_symbols):
    """a chunk = the longest run of consecutive reads with at most chunk_reads reads and chunk_symbols symbols, never less than one read"""
    nq = len(qoff) - 1
    first, at = [], 0
    while at < nq:
        first.append(at)
        end = at + 1
        while end < nq and end - at < chunk_reads and int(qoff[end + 1]) - int(qoff[at]) <= chunk_symbols:
            end += 1
        at = end
    return first + [nq]


def feed_plan(qoff, chunk_reads, chunk_symbols, capacity=None):
    nq = len(qoff) - 1
    capacity = nq + 1 if capacity is None else capacity
    out = np.full(capacity + 1, 2 ** 64 - 1, dtype=np.uint64)
    chunks = C.c_uint64(12345)
    rc = capi.lib().fmgpu_feed_plan(capi.ptr(qoff), nq, chunk_reads, chunk_symbols, capi.ptr(out), capacity, C.byref(chunks))
    return rc, int(chunks.value), out


def test_symbols_exist_and_the_abi_version_stays():
    L = capi.lib()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert L.fmgpu_abi_version() == 6
    assert C.sizeof(capi.FeedConfig) == 32


@pytest.mark.parametrize("seed", range(6))
def test_plan_equals_the_rule_on_ragged_batches(seed):
    rng = np.random.default_rng(seed)
    nq = int(rng.integers(1, 300))
    lens = rng.integers(0, 60, size=nq)
    lens[rng.random(nq) < 0.2] = 0                                     # empty reads
    lens[nq // 2] = 500                                                # one read longer than most symbol limits below
    qoff = np.concatenate([[int(rng.integers(0, 9))], lens]).cumsum().astype(np.uint64)
    for chunk_reads in (1, 3, 37, nq, 10 * nq + 1):
        for chunk_symbols in (1, 64, 499, 500, 10 ** 9):               # 10^9 and 10 nq + 1: limits larger than the batch
            rc, chunks, out = feed_plan(qoff, chunk_reads, chunk_symbols)
            want = plan_by_the_rule(qoff, chunk_reads, chunk_symbols)
            assert rc == 0 and chunks == len(want) - 1, (chunk_reads, chunk_symbols)
            assert out[: chunks + 1].tolist() == want, (chunk_reads, chunk_symbols)
    rc, chunks, out = feed_plan(qoff, 10 * nq + 1, 10 ** 12)
    assert rc == 0 and chunks == 1 and out[:2].tolist() == [0, nq]
    rc, chunks, out = feed_plan(qoff, 1, 10 ** 9)
    assert rc == 0 and chunks == nq and out[: nq + 1].tolist() == list(range(nq + 1))


def test_plan_error_codes():
    L = capi.lib()
    qoff = np.array([2, 5, 5, 9, 30], dtype=np.uint64)
    assert feed_plan(qoff, 0, 10)[0] == capi.FMGPU_ERR_INVALID and b"at least 1" in L.fmgpu_last_error()
    assert feed_plan(qoff, 10, 0)[0] == capi.FMGPU_ERR_INVALID
    bad = np.array([2, 5, 4, 9, 30], dtype=np.uint64)
    assert feed_plan(bad, 10, 10)[0] == capi.FMGPU_ERR_INVALID and b"non-decreasing" in L.fmgpu_last_error()
    rc, chunks, out = feed_plan(qoff, 1, 100, capacity=2)                                    # four chunks, room for two
    assert rc == capi.FMGPU_ERR_CAPACITY and chunks == 4
    chunks = C.c_uint64(0)
    assert L.fmgpu_feed_plan(capi.ptr(qoff), 4, 1, 100, None, 0, C.byref(chunks)) == capi.FMGPU_ERR_CAPACITY and chunks.value == 4      # counting alone
    assert L.fmgpu_feed_plan(capi.ptr(qoff), 4, 1, 100, None, 0, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_feed_plan(None, 4, 1, 100, None, 0, C.byref(chunks)) == capi.FMGPU_ERR_INVALID
    one = np.zeros(1, dtype=np.uint64)
    chunks.value = 9
    assert L.fmgpu_feed_plan(None, 0, 1, 1, capi.ptr(one), 0, C.byref(chunks)) == 0 and chunks.value == 0


def test_argument_errors_without_a_gpu():
    L = capi.lib()
    one = np.zeros(8, dtype=np.uint64)
    rec = np.zeros(40, dtype=np.uint8)
    h = C.c_void_p(5)
    # no feed on a null handle
    assert L.fmgpu_feed_create(None, None, C.byref(h)) == capi.FMGPU_ERR_INVALID and h.value is None
    assert b"index handle is null" in L.fmgpu_last_error()
    assert L.fmgpu_feed_create(None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_feed_destroy(None) == 0
    assert L.fmgpu_feed_info(None, None, None, None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_free_host(None) == 0 and L.fmgpu_malloc_host(None, 8) == capi.FMGPU_ERR_INVALID
    # a null feed; nq == 0 returns 0 whatever else is passed, and resets what it reports
    for name in ("fmgpu_feed_search_exact", "fmgpu_feed_search_exact_q4", "fmgpu_feed_search_exact_v"):
        call = getattr(L, name)
        assert call(None, capi.ptr(one), capi.ptr(one), 1, capi.ptr(one), capi.ptr(one), None) == capi.FMGPU_ERR_INVALID, name
        assert b"feed is null" in L.fmgpu_last_error(), name
        st = capi.Stats()
        st.hits = 3
        assert call(None, None, None, 0, None, None, C.byref(st)) == 0 and st.hits == 0, name
    sc = capi.Scheme()
    for name in ("fmgpu_feed_search_scheme", "fmgpu_feed_search_scheme_v"):
        call = getattr(L, name)
        cnt = C.c_uint64(7)
        assert call(None, capi.ptr(one), capi.ptr(one), 1, C.byref(sc), 1, capi.ptr(rec), 1, C.byref(cnt), None) == capi.FMGPU_ERR_INVALID, name
        assert b"feed is null" in L.fmgpu_last_error(), name
        cnt.value = 7
        assert call(None, None, None, 0, C.byref(sc), 1, None, 0, C.byref(cnt), None) == 0 and cnt.value == 0, name
