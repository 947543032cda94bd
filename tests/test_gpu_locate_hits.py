"""fmgpu_locate_hits / Index.locate_hits / search_locate: every row of every hit record located in one call, against the per-cursor
LocateLinear path (order included), the oracle, the reference's own expectations and the text itself.  Run with -m gpu on an MI355X."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, POSITION_DTYPE
from tests.util import oracle_arrays

pytestmark = pytest.mark.gpu
REF = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_tests.json")))


def gpu_index(ox, **drop):
    arrays = oracle_arrays(ox)
    for k in drop:
        arrays.pop(k)
    return (fm.BiFMIndex if ox.bidirectional else fm.FMIndex).from_reference_arrays(**arrays)


def old_path(gx, hits):
    """what the per-cursor LocateLinear loop reports, as POSITION_DTYPE records"""
    ll = fm.LocateLinear(gx, hits["lb"], hits["len"])
    owner, seq, pos, steps = ll()
    want = np.zeros(owner.size, dtype=POSITION_DTYPE)
    o = owner.astype(np.int64)
    want["qidx"], want["seq_id"], want["pos"] = hits["qidx"][o], seq, pos + steps
    want["errors"], want["hit"] = hits["errors"][o] & 0xff, owner
    return want, ll.rows


def same(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def text_with_repeats(sigma, seed, n=24_000):
    rng = np.random.default_rng(seed)
    hi = min(sigma, 8)
    base = rng.integers(1, hi, size=n // 3, dtype=np.uint8)
    rep = np.concatenate([base[: n // 12]] * 6)                              # a six-copy repeat: cursors of several rows
    return [np.concatenate([base, rep, rng.integers(1, hi, size=n // 4, dtype=np.uint8)]), base[::-1].copy()]


def reads_from(seqs, count, length, subs, seed, sigma):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        s = seqs[int(rng.integers(0, len(seqs)))]
        p = int(rng.integers(0, len(s) - length))
        q = s[p: p + length].copy()
        for _ in range(int(rng.integers(0, subs + 1))):
            q[int(rng.integers(0, length))] = rng.integers(1, min(sigma, 8))
        out.append(q)
    return out


# ------------------------------------------------------------------------------------------------ 1. the reference's expectations
def test_reference_expectations():
    """search/checkSearches.cpp's located multisets (tests/golden/reference_tests.json, also checked through the old path in
    test_edit_distance_reference_vectors): search -> locate_hits, and search_locate for the fmc::search facade"""
    g = REF["searches_edit"]
    ox = fo.OraIndex.build("IB16", g["sigma"], g["input"], g["sampling_rate"], True)
    gx = gpu_index(ox)
    for key in ("ng26_pigeon_opt_CD_DB", "ng26_pigeon_opt_n3"):
        c = g[key]
        hits = fm.search_ng26.search(gx, c["queries"], fm.search_scheme.pigeon_opt(0, 1), n=c.get("n", fm.UINT64_MAX), edit=True)
        p = gx.locate_hits(hits)
        assert sorted([int(a), int(b), int(d)] for a, b, d in zip(p["qidx"], p["seq_id"], p["pos"])) == c["expected"], key
    for key in ("facade_k1", "facade_k1_n3"):
        c = g[key]
        hits = fm.search(gx, c["queries"], 1, n=c.get("n", fm.UINT64_MAX), edit=True)
        p = gx.locate_hits(hits)
        assert sorted([int(a), int(b), int(d)] for a, b, d in zip(p["qidx"], p["seq_id"], p["pos"])) == c["expected"], key
        s = fm.search_locate(gx, c["queries"], 1, n=c.get("n", fm.UINT64_MAX), edit=True)
        assert sorted([int(a), int(b), int(d)] for a, b, d in zip(s["qidx"], s["seq_id"], s["pos"])) == c["expected"], key


# ------------------------------------------------------------------------------------------------ 2. identical to the old path, every locate kernel
CONFIGS = [
    ("IB16", 5, "coop"), ("EPR16", 6, "general"), ("WAVELET", 28, "general"), ("IB16", 5, "per_lane"), ("IB16", 5, "answer_table"),
    ("EPR16", 6, "no_lf_table"), ("IB16", 5, "wide"), ("EPR16", 6, "wide"),
]


@pytest.mark.parametrize("layout,sigma,mode", CONFIGS)
def test_identical_to_locate_linear(layout, sigma, mode):
    seqs = text_with_repeats(sigma, seed=sigma * 7 + len(mode))
    ox = fo.OraIndex.build(layout, sigma, seqs, 4, True)
    with fm.options(force_wide=1 if mode == "wide" else 0):
        gx = gpu_index(ox)
    assert gx.row_bits == (64 if mode == "wide" else 32)
    if mode == "answer_table":
        gx.accelerate_locate()
    if mode == "no_lf_table":
        gx.accelerate_lf(False)
    reads = reads_from(seqs, 300, 24, 2, seed=sigma, sigma=sigma)
    sets = {"exact": fm.search(gx, reads, 0),
            "hamming2": fm.search_ng26.search(gx, reads, fm.search_scheme.h2(4, 0, 2), edit=False),
            "edit2": fm.search_ng26.search(gx, reads, fm.search_scheme.h2(4, 0, 2), edit=True)}
    sel = capi.SEL_LOCATE_PER_LANE if mode == "per_lane" else 0
    with fm.options(kernel_select=sel):
        for name, hits in sets.items():
            want, rows = old_path(gx, hits)
            got, st = gx.locate_hits(hits, want_stats=True)
            assert want.size > len(hits) > 0, name                              # cursors of several rows are part of the batch
            assert same(got, want), (mode, name)
            assert st.hits == want.size
            for i in np.random.default_rng(1).choice(want.size, size=min(200, want.size), replace=False):
                s, p, k = ox.locate(int(rows[i]))
                assert (int(got["seq_id"][i]), int(got["pos"][i])) == (s, p + k), (mode, name, i)
        allhits = np.concatenate(list(sets.values()))                           # one ragged call over all three sets
        assert same(gx.locate_hits(allhits), old_path(gx, allhits)[0])


# ------------------------------------------------------------------------------------------------ 3. shapes that cross workgroup boundaries
@pytest.fixture(scope="module")
def satellite():
    rng = np.random.default_rng(5)
    text = np.concatenate([rng.integers(1, 5, size=40_000, dtype=np.uint8), np.tile(np.array([1, 3], dtype=np.uint8), 250_000),
                           rng.integers(1, 5, size=40_000, dtype=np.uint8)])
    return text, fm.BiFMIndex.from_sequences([text], 5, "IB16", 16)


def synthetic(n, lens, seed):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.uint64)
    h = np.zeros(lens.size, dtype=HIT_DTYPE)
    h["qidx"] = np.arange(lens.size) // 3
    h["len"] = lens
    h["lb"] = rng.integers(0, n - lens.astype(np.int64) + 1, dtype=np.int64).astype(np.uint64)
    h["errors"] = rng.integers(0, 1 << 20, size=lens.size).astype(np.uint32)           # upper bits set: the records carry errors & 0xff
    h["seq"] = np.arange(lens.size)
    return h


def test_one_hit_over_many_workgroups(satellite):
    text, gx = satellite
    reads = [text[p: p + 30] for p in range(0, 20_000, 997)] + [np.tile(np.array([1, 3], dtype=np.uint8), 12)] + [text[p: p + 30] for p in range(20_000, 40_000, 997)]
    hits = fm.search(gx, reads, 0)
    assert int(hits["len"].max()) >= 200_000
    want = old_path(gx, hits)[0]
    assert same(gx.locate_hits(hits), want)
    with fm.options(kernel_select=capi.SEL_LOCATE_PER_LANE):
        assert same(gx.locate_hits(hits), want)


def test_empty_hits_and_workgroup_edges(satellite):
    _, gx = satellite
    n = gx.n
    cases = {
        "zero_one": [0, 1] * 3000 + [0] * 5000 + [1, 0] * 3000,                      # a workgroup's rows spread over more than 2048 hits
        "aligned": [2048, 3, 0, 0, 2045, 1, 2047, 6144, 0, 2048, 5, 4096 + 17],    # hits that begin at multiples of 2048 output rows
        "mixed": list(np.random.default_rng(3).choice([0, 0, 1, 2, 7, 300, 2500], size=4000)),
    }
    for name, lens in cases.items():
        hits = synthetic(n, lens, seed=len(name))
        want = old_path(gx, hits)[0]
        assert want.size == int(hits["len"].sum())
        assert same(gx.locate_hits(hits), want), name
    starts = np.cumsum([0] + cases["aligned"][:-1])
    assert sum(1 for s, l in zip(starts, cases["aligned"]) if l and s % 2048 == 0 and s) >= 3
    assert gx.locate_hits(np.zeros(0, dtype=HIT_DTYPE)).size == 0
    empty = synthetic(n, [0] * 100, seed=9)
    cnt = C.c_uint64(123)
    out = np.zeros(4, dtype=POSITION_DTYPE)
    capi.check(capi.lib().fmgpu_locate_hits(gx._h, capi.ptr(empty), 100, capi.ptr(out), 4, C.byref(cnt), None, None))
    assert cnt.value == 0
    capi.check(capi.lib().fmgpu_locate_hits(gx._h, None, 0, None, 0, C.byref(cnt), None, None))
    assert cnt.value == 0


# ------------------------------------------------------------------------------------------------ 4. host and device memory
def test_host_and_device_memory(satellite):
    torch = pytest.importorskip("torch")
    _, gx = satellite
    hits = synthetic(gx.n, list(np.random.default_rng(4).choice([0, 1, 3, 40, 3000], size=3000)), seed=4)
    total = int(hits["len"].sum())
    want = gx.locate_hits(hits).tobytes()
    dev = torch.device("cuda", 0)
    dhits = torch.from_numpy(hits.view(np.uint8).copy()).to(dev)
    stream = torch.cuda.Stream(device=dev)
    for hin in ("host", "device"):
        for hout in ("host", "device"):
            src = hits if hin == "host" else dhits
            with torch.cuda.stream(stream):
                if hout == "host":
                    got = gx.locate_hits(src, stream=stream).tobytes()
                else:
                    out = torch.full((total * 32 + 64,), 0xAB, dtype=torch.uint8, device=dev)
                    assert gx.locate_hits(src, out=out, stream=stream) == total
                    stream.synchronize()
                    tail = out[total * 32:].cpu().numpy()
                    assert (tail == 0xAB).all()                                         # nothing written past the records
                    got = out[: total * 32].cpu().numpy().tobytes()
            assert got == want, (hin, hout)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors(satellite):
    _, gx = satellite
    hits = synthetic(gx.n, [5, 0, 17, 2], seed=2)
    total = 24
    L = capi.lib()
    cnt = C.c_uint64()
    buf = np.zeros(total, dtype=POSITION_DTYPE)
    buf.view(np.uint8)[:] = 0x5A
    rc = L.fmgpu_locate_hits(gx._h, capi.ptr(hits), len(hits), capi.ptr(buf), total - 1, C.byref(cnt), None, None)
    assert rc == capi.FMGPU_ERR_CAPACITY and cnt.value == total
    assert (buf.view(np.uint8) == 0x5A).all()                                           # the output is untouched
    assert L.fmgpu_locate_hits(gx._h, capi.ptr(hits), len(hits), capi.ptr(buf), total, C.byref(cnt), None, None) == 0 and cnt.value == total
    bad = hits.copy()
    bad["lb"][2], bad["len"][2] = gx.n - 16, 17                                        # lb + len = n + 1
    assert L.fmgpu_locate_hits(gx._h, capi.ptr(bad), len(bad), capi.ptr(buf), total, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    bad["len"][2] = 16                                                                  # lb + len = n: the last row, valid
    assert L.fmgpu_locate_hits(gx._h, capi.ptr(bad), len(bad), capi.ptr(buf), total, C.byref(cnt), None, None) == 0
    with pytest.raises(fm.FmgpuError) as e:
        gx.locate_hits(np.array([(0, gx.n, 0, 1, 0, 0)], dtype=HIT_DTYPE))               # lb = n
    assert e.value.code == capi.FMGPU_ERR_INVALID
    ox = fo.OraIndex.build("IB16", 5, text_with_repeats(5, 1), 4, True)
    nosa = gpu_index(ox, sparse=True)
    with pytest.raises(fm.FmgpuError) as e:
        nosa.locate_hits(hits)
    assert e.value.code == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_locate_hits(gx._h, None, 3, capi.ptr(buf), total, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_locate_hits(gx._h, capi.ptr(hits), 3, None, total, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 6. full size
def test_genome_like_index_search_locate():
    """a >= 50 Mbp genome-like BiFMIndex, 20 000 reads at k = 2 (Hamming): search_locate equals search + LocateLinear record for record, and on
    2 000 reads every located position spells a text window within Hamming distance 2 of its read"""
    torch = pytest.importorskip("torch")
    import bench
    from fmindex_collection_amd import datasets
    dev = torch.device("cuda", 0)
    scale = 52e6 / sum(bench.GRCH38_LENGTHS)
    lengths = [max(1000, int(l * scale)) for l in bench.GRCH38_LENGTHS]
    text, _ = datasets.genome_like_text(lengths, seed=17, device=dev)
    seq_off = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])

    class V:
        def __init__(self, t):
            self.t, self.ptr, self.nbytes = t, t.data_ptr(), t.numel() * t.element_size()
    dseq_off = torch.from_numpy(seq_off).to(dev)
    gx = fm.BiFMIndex.from_sequences((V(text), V(dseq_off)), 5, "IB16", 16)
    assert gx.n >= 50_000_000
    host = text.cpu().numpy()
    del text
    rng = np.random.default_rng(21)
    L, reads = 101, []
    while len(reads) < 20_000:                                                          # reads of satellites with > 1 000 copies are left out (size of the comparison)
        starts = rng.integers(0, host.size - L, size=4000)
        cand = [host[s: s + L].copy() for s in starts]
        lb, ln = fm.search_no_errors.search(gx, cand)
        for q, k in zip(cand, ln):
            if 0 < k <= 1000 and len(reads) < 20_000:
                for _ in range(int(rng.integers(0, 3))):
                    q[int(rng.integers(0, L))] = rng.integers(1, 5)
                reads.append(q)
    got = fm.search_locate(gx, reads, 2, edit=False)
    hits = fm.search(gx, reads, 2, edit=False)
    want, _ = old_path(gx, hits)
    assert got.size == want.size > 20_000
    for k in ("qidx", "seq_id", "pos", "errors"):
        assert np.array_equal(got[k], want[k]), k
    sub = np.nonzero(got["qidx"] < 2000)[0]
    seq = got["seq_id"][sub].astype(np.int64)
    start = seq_off[seq] + got["pos"][sub].astype(np.int64)
    assert (got["pos"][sub].astype(np.int64) + L <= seq_off[seq + 1] - seq_off[seq]).all()
    windows = host[start[:, None] + np.arange(L)[None, :]]
    rd = np.stack([reads[int(q)] for q in got["qidx"][sub]])
    assert ((windows != rd).sum(axis=1) <= 2).all()
