"""What the launchers of the depth-first searches do around their kernels, through the C ABI: fmgpu_search_scheme (Hamming and edit distance), fmgpu_search_ng21 and
fmgpu_search_backtracking with host buffers and with qbuf / qoff / out in device memory, on 32- and 64-bit rows.  A capacity that is too small returns the total and
leaves the caller's buffer beyond `capacity` records alone; at full capacity the records are the oracle's, the two buffer forms agree record for record and step for
step, and the statistics a kernel does not produce stay zero.  Every check is exact.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, UINT64_MAX
from tests.util import oracle_arrays

pytestmark = pytest.mark.gpu

K = 1
HIT_KEYS = ("qidx", "lb", "lb_rev", "len", "errors")
# (call, batch): the scheme calls also take the ragged batch (one launch per read length, or the general kernels)
CASES = [("hamming", "equal"), ("hamming", "ragged"), ("edit", "equal"), ("edit", "ragged"), ("ng21", "equal"), ("backtracking", "equal")]


# ------------------------------------------------------------------------------------------------ text, index, batches, oracle records (made once, never modified)
@functools.lru_cache(maxsize=None)
def text():
    rng = np.random.default_rng(4242)
    base = rng.integers(1, 5, size=1400, dtype=np.uint8)
    return np.concatenate([base, base[300:700], rng.integers(1, 5, size=200, dtype=np.uint8)])      # 2000 symbols, base[300:700] twice


@functools.lru_cache(maxsize=None)
def oracle():
    return fo.OraIndex.build("IB16", 5, [text()], 2, True)


@functools.lru_cache(maxsize=None)
def handle(wide):
    with fm.options(force_wide=wide):
        gx = fm.BiFMIndex.from_reference_arrays(**oracle_arrays(oracle()))
    assert gx.row_bits == (64 if wide else 32)
    return gx


@functools.lru_cache(maxsize=None)
def batch(kind):
    """48 reads of 24 symbols (18 .. 30 in the ragged batch), every second one with a substitution; a third of them from the repeated stretch"""
    rng = np.random.default_rng(7 if kind == "equal" else 8)
    t = text()
    reads = []
    for k in range(48):
        m = 24 if kind == "equal" else 18 + k % 13
        at = int(rng.integers(300, 700 - m)) if k % 3 == 0 else int(rng.integers(0, len(t) - m + 1))
        r = t[at: at + m].copy()
        if k % 2:
            p = int(rng.integers(0, m))
            r[p] = int(r[p]) % 4 + 1
        reads.append(r)
    return fm.flatten(reads)


def scheme():
    return fo.scheme_pigeon_opt(0, K)


@functools.lru_cache(maxsize=None)
def want(call, kind):
    """the oracle's records in callback order"""
    qbuf, qoff = batch(kind)
    ox = oracle()
    if call == "hamming":
        return ox.search_ng26(qbuf, qoff, scheme())[0]
    if call == "edit":
        return ox.search_ng26(qbuf, qoff, scheme(), edit=True)[0]
    if call == "ng21":
        return ox.search_ng21(qbuf, qoff, fo.scheme_expand(scheme(), 24))[0]
    return ox.search_backtracking(qbuf, qoff, K)[0]


def same_hits(g, o):
    return len(g) == len(o) and all(np.array_equal(g[k].astype(np.uint64), o[k].astype(np.uint64)) for k in HIT_KEYS)


def search(call, gx, q, o, nq, out, cap, cnt, st):
    """one C-ABI call; q / o / out: numpy arrays, DeviceBuffers or None"""
    L = capi.lib()
    tail = (capi.ptr(out), cap, C.byref(cnt), C.byref(st) if st is not None else None, None)
    if call == "backtracking":
        return L.fmgpu_search_backtracking(gx._h, capi.ptr(q), capi.ptr(o), nq, K, *tail)
    pi, l, u = (np.ascontiguousarray(x, dtype=np.uint64) for x in (fo.scheme_expand(scheme(), 24) if call == "ng21" else scheme()))
    if call == "ng21":
        sc = capi.ExpandedScheme()
        sc.n_searches, sc.length = pi.shape
    else:
        sc = capi.Scheme()
        sc.n_searches, sc.n_parts = pi.shape
        sc.edit = 1 if call == "edit" else 0
    sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    fn = L.fmgpu_search_ng21 if call == "ng21" else L.fmgpu_search_scheme
    return fn(gx._h, capi.ptr(q), capi.ptr(o), nq, C.byref(sc), UINT64_MAX, *tail)


def run_form(call, gx, kind, device):
    """the capacity ladder and the full run in one buffer form; returns (sorted records, stats)"""
    qbuf, qoff = batch(kind)
    nq = len(qoff) - 1
    count = len(want(call, kind))
    assert count >= 48 and int(want(call, kind)["len"].max()) >= 2    # (an empty oracle result cannot pass; the repeated stretch gives cursors of two rows)
    fill = np.full((count + 2) * HIT_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    if device:
        q, o = fm.DeviceBuffer.from_array(qbuf), fm.DeviceBuffer.from_array(qoff)
        out = fm.DeviceBuffer.from_array(fill)
        read_out = lambda: out.to_array(HIT_DTYPE, count + 2)
    else:
        q, o, out = qbuf, qoff, fill.view(HIT_DTYPE)
        read_out = lambda: out
    cnt = C.c_uint64()
    for cap in (0, 1, count - 1):
        rc = search(call, gx, q, o, nq, None if cap == 0 else out, cap, cnt, None)
        assert rc == capi.FMGPU_ERR_CAPACITY and cnt.value == count, (cap, rc, cnt.value)
        assert (read_out()[cap:].view(np.uint8) == 0xA5).all(), cap
    st = capi.Stats()
    rc = search(call, gx, q, o, nq, out, count, cnt, st)
    assert rc == 0 and cnt.value == count and (read_out()[count:].view(np.uint8) == 0xA5).all()
    capi.check(capi.lib().fmgpu_hits_sort(capi.ptr(out), count, None))
    hits = np.ascontiguousarray(read_out()[:count])
    if device:
        for b in (q, o, out):
            b.free()
    return hits, st


@pytest.mark.parametrize("call,kind", CASES)
@pytest.mark.parametrize("wide", [0, 1])
def test_capacity_records_and_stats(call, kind, wide):
    gx = handle(wide)
    host, hst = run_form(call, gx, kind, False)
    dev, dst = run_form(call, gx, kind, True)
    assert same_hits(host, want(call, kind))
    assert host.tobytes() == dev.tobytes()
    for st in (hst, dst):
        assert st.hits == len(host) and st.lf_steps == hst.lf_steps > 0
        assert st.prepass_ms == 0                                   # (48 reads: no hand-out order pass)
        if call in ("ng21", "backtracking"):
            assert st.table_bytes == st.table_accesses == st.table_steps == 0
