"""fmgpu_extract / FMIndex.extract / fm.reconstruct_text: the text read back from the index on the device, against the sequences it was built from, against
restatements of the reference's reconstructText (utils.h:672-703) and against the reference's own fixtures.  Run with -m gpu on an MI355X."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import TEXT_RANGE_DTYPE
from tests.util import oracle_arrays

pytestmark = pytest.mark.gpu
REF = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_tests.json")))


def sequences(rate, sigma, seed, count=300, long=3000):
    """lengths 0, 1, rate - 1, rate, rate + 1 and a few thousand, then several hundred short and medium ones"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, max(rate - 1, 0), rate, rate + 1, long] + list(rng.integers(0, 160, size=count - 6))
    rng.shuffle(lens)
    return [rng.integers(1, sigma, size=int(l), dtype=np.uint8) for l in lens]


def as_bytes(texts):
    return [bytes(np.asarray(t, dtype=np.uint8)) for t in texts]


def via_oracle(layout, sigma, seqs, rate, bidir):
    ox = fo.OraIndex.build(layout, sigma, seqs, rate, bidir)
    return (fm.BiFMIndex if bidir else fm.FMIndex).from_reference_arrays(**oracle_arrays(ox))


def whole_sequences(gx):
    ids, lens = gx.sequence_lengths()
    return gx.extract(ids, np.zeros_like(ids), lens)


# ------------------------------------------------------------------------------------------------ 1. full reconstruction
BUILT = [(bidir, rate, wide, lf, fused) for bidir in (False, True) for rate in (1, 3, 16, 64) for wide in (0, 1) for lf, fused in ((1, 1), (0, 0))]


@pytest.mark.parametrize("bidir,rate,wide,lf,fused", BUILT)
def test_reconstruct_built_index(bidir, rate, wide, lf, fused):
    seqs = sequences(rate, 5, seed=rate * 7 + wide + 2 * lf)
    with fm.options(force_wide=wide, lf_table=lf, fused_locate=fused):
        gx = (fm.BiFMIndex if bidir else fm.FMIndex).from_sequences(seqs, 5, "IB16", rate)
    assert gx.row_bits == (64 if wide else 32)
    assert bool(gx.formats & capi.FMT_LF) == bool(lf)
    assert as_bytes(fm.reconstruct_text(gx)) == as_bytes(seqs)
    assert not gx.formats & capi.FMT_EXTRACT                     # (built for the call, dropped again)
    gx.accelerate_extract()
    ids, lens = gx.sequence_lengths()
    assert ids.tolist() == list(range(len(seqs))) and lens.tolist() == [len(s) for s in seqs]
    sym, off = whole_sequences(gx)
    assert sym.tobytes() == b"".join(as_bytes(seqs)) and off[-1] == sum(len(s) for s in seqs)


LAYOUTS = [("IB16", 5, {}), ("EPR16", 5, {"expand_dna": 0}), ("EPR16", 5, {"expand_dna": 1}), ("EPRV2_16", 5, {"expand_dna": 0}), ("EPRV2_16", 5, {"expand_dna": 1}),
           ("FBV_512_64K", 5, {}), ("WAVELET", 5, {"expand_dna": 0}), ("WAVELET", 21, {"symbol_planes": 0}), ("WAVELET", 21, {"symbol_planes": 1})]


@pytest.mark.parametrize("layout,sigma,opts", LAYOUTS)
@pytest.mark.parametrize("bidir", [False, True])
def test_reconstruct_reference_layouts(layout, sigma, opts, bidir):
    """the in-place EPR blocks, the multi-ary tree, the symbol planes and the flattened bitvectors are only reached through reference-held arrays"""
    rate = 3 if bidir else 16
    seqs = sequences(rate, sigma, seed=len(layout) + sigma + bidir, count=120, long=2000)
    for wide, lf in ((0, 0), (1, 1)):
        with fm.options(force_wide=wide, lf_table=lf, **opts):
            gx = via_oracle(layout, sigma, seqs, rate, bidir)
        assert gx.row_bits == (64 if wide else 32)
        assert as_bytes(fm.reconstruct_text(gx)) == as_bytes(seqs), (layout, opts, wide)


def per_row_restatement(gx):
    """utils.h:672-685 for every sentinel row at once, over the index's own symbol / rank (fmgpu_string_query)"""
    n = gx.n
    C_ = np.array([int(gx.prefix_rank(np.array([n], dtype=np.uint64), c)[0]) for c in range(gx.Sigma)], dtype=np.uint64)
    nsent = int(gx.rank(np.array([n], dtype=np.uint64), 0)[0])
    idx = np.arange(nsent, dtype=np.uint64)
    out = [[] for _ in range(nsent)]
    live = np.ones(nsent, dtype=bool)
    while live.any():
        rows = idx[live]
        c = gx.symbol(rows)
        nxt = gx.rank(rows, c.astype(np.uint8)) + C_[c.astype(np.int64)]
        for k, i in enumerate(np.nonzero(live)[0]):
            if c[k] != 0:
                out[i].append(int(c[k]))
        live_idx = np.nonzero(live)[0]
        idx[live_idx] = nxt
        live[live_idx[c == 0]] = False
    return [bytes(reversed(t)) for t in out]


def test_reconstruct_every_sentinel_row():
    seqs = sequences(5, 5, seed=3, count=40, long=400)
    for wide in (0, 1):
        with fm.options(force_wide=wide):
            gx = fm.FMIndex.from_sequences(seqs, 5, "IB16", 5)
        gx.accelerate_extract()
        want = per_row_restatement(gx)
        for r in range(len(want)):
            assert bytes(fm.reconstruct_text(gx, r)) == want[r], (wide, r)
        assert gx.formats & capi.FMT_EXTRACT                    # (a table the caller built stays)
        with pytest.raises(ValueError):
            fm.reconstruct_text(gx, len(want))


# ------------------------------------------------------------------------------------------------ 2. irregular sampling
def irregular_index(layout, sigma, seqs, wide, seed):
    """every sampled row of a hand-picked presence set: gaps that differ per sequence plus random extra rows, always pos 0"""
    full = via_oracle(layout, sigma, seqs, 1, False)
    n = full.n
    rows = np.arange(n, dtype=np.uint64)
    bwt = full.symbol(rows).astype(np.uint8)
    seq, pos, steps = full.locate(rows)
    pos = pos + steps
    rng = np.random.default_rng(seed)
    s64, p64 = seq.astype(np.int64), pos.astype(np.int64)
    gap = (s64 % 7 + 2) * (1 + (s64 % 3 == 0) * 9)                            # 2 .. 8, 20 .. 80
    has = (p64 % gap == 0) | (rng.random(n) < 0.03)
    with fm.options(force_wide=wide):
        gx = fm.FMIndex.from_reference_arrays(**oracle_arrays(fo.OraIndex.from_bwt(layout, sigma, bwt, None, has.astype(np.uint8), seq, pos)))
    samples = {}
    for s, p in zip(seq[has], pos[has]):
        samples.setdefault(int(s), []).append(int(p))
    return gx, {k: np.sort(v) for k, v in samples.items()}


@pytest.mark.parametrize("layout,sigma", [("IB16", 5), ("EPRV2_16", 5), ("WAVELET", 21)])
def test_irregular_sampling(layout, sigma):
    seqs = sequences(6, sigma, seed=11, count=150, long=2500)
    for wide in (0, 1):
        gx, _ = irregular_index(layout, sigma, seqs, wide, seed=5)
        assert as_bytes(fm.reconstruct_text(gx)) == as_bytes(seqs), (layout, wide)


# ------------------------------------------------------------------------------------------------ 3. the reference's fixtures
def fixture_restatement(bwt):
    """utils.h:688-703 over a literal BWT: one text per sentinel row, walked with the BWT's own LF; seqIds all 0 -> row order"""
    n = bwt.size
    C_ = np.concatenate([[0], np.cumsum(np.bincount(bwt, minlength=int(bwt.max()) + 1))])
    occ = np.array([np.count_nonzero(bwt[:i] == bwt[i]) for i in range(n)])
    texts = []
    for r in range(int(np.count_nonzero(bwt == 0))):
        t, i = [], r
        while True:
            c = int(bwt[i])
            i = int(C_[c] + occ[i])
            if c == 0:
                break
            t.append(c)
        texts.append(bytes(reversed(t)))
    return texts


@pytest.mark.parametrize("fixture,bidir", [("fmindex_hallo", False), ("bifmindex_hallo", True), ("bifmindex_long", True)])
def test_reference_fixtures(fixture, bidir):
    """fmindex/checkFMIndex.cpp:15-110, fmindex/checkBiFMIndex.cpp:13-105, :136-222: literal BWT / SA (all rows, and every second text position)"""
    g = REF[fixture]
    bwt, sa = np.array(g["bwt"], dtype=np.uint8), np.array(g["sa"], dtype=np.uint64)
    rev = np.array(g["bwtRev"], dtype=np.uint8) if bidir else None
    n = sa.size
    text = np.zeros(n, dtype=np.uint8)
    text[(sa.astype(np.int64) - 1) % n] = bwt                                  # T[(sa[i] - 1) mod n] = bwt[i]
    want = fixture_restatement(bwt)
    if fixture == "fmindex_hallo":
        assert want == [b"Hallo Welt", b""] or want == [b"", b"Hallo Welt"]
    for rule in (lambda s: True, lambda s: s % 2 == 0):
        has = np.array([rule(int(s)) for s in sa], dtype=np.uint8)
        for layout in ("IB16", "EPRV2_16", "WAVELET"):
            ox = fo.OraIndex.from_bwt(layout, g["sigma"], bwt, rev, has, np.zeros(n, dtype=np.uint64), sa)
            gx = (fm.BiFMIndex if bidir else fm.FMIndex).from_reference_arrays(**oracle_arrays(ox))
            got = as_bytes(fm.reconstruct_text(gx))
            assert got == want, (fixture, layout)
            gx.accelerate_extract()
            ids, lens = gx.sequence_lengths()
            assert ids.tolist() == [0] and int(lens[0]) == n - 1                # the last delimiter at pos n - 1
            sym, _ = whole_sequences(gx)
            assert sym.tobytes() == text[: n - 1].tobytes(), (fixture, layout)    # an interior delimiter included
    if fixture == "fmindex_hallo":
        assert [t.decode() for t in got] == ["Hallo Welt", ""]


# ------------------------------------------------------------------------------------------------ 4. ranges
def random_ranges(lens, samples, rng, count=4000):
    """random ranges, empty ones, whole sequences, ranges ending at a sequence end and ranges inside one piece"""
    nseq = len(lens)
    s = rng.integers(0, nseq, size=count)
    L = np.asarray(lens, dtype=np.int64)[s]
    a = (rng.random(count) * (L + 1)).astype(np.int64)
    b = (rng.random(count) * (L + 1)).astype(np.int64)
    p, e = np.minimum(a, b), np.maximum(a, b)
    kind = rng.integers(0, 5, size=count)
    p[kind == 1], e[kind == 1] = 0, L[kind == 1]                                 # whole sequences
    e[kind == 2] = L[kind == 2]                                                  # ending at the sequence end
    e[kind == 3] = p[kind == 3]                                                  # empty
    for i in np.nonzero(kind == 4)[0]:                                           # inside one piece: between two neighbouring samples
        sp = samples[int(s[i])]
        j = int(rng.integers(0, len(sp)))
        lo, hi = int(sp[j]), int(sp[j + 1]) if j + 1 < len(sp) else int(L[i])
        hi = min(hi, int(L[i]))
        if hi > lo + 1:
            p[i] = int(rng.integers(lo + 1, hi))
            e[i] = int(rng.integers(p[i], hi + 1))
    r = np.zeros(count, dtype=TEXT_RANGE_DTYPE)
    r["seq_id"], r["pos"], r["len"] = s, p, e - p
    return r


def predicted_steps(ranges, lens, samples):
    """every piece walks from its key down to its lower end: per range, from the first sample at or after its end (or the sequence end) down to its start"""
    total = 0
    for s, p, l in zip(ranges["seq_id"], ranges["pos"], ranges["len"]):
        if l == 0:
            continue
        sp = samples[int(s)]
        k = np.searchsorted(sp, int(p + l))
        key = int(sp[k]) if k < len(sp) and sp[k] <= lens[int(s)] else lens[int(s)]
        total += key - int(p)
    return total


def check_ranges(gx, seqs, samples, seed):
    rng = np.random.default_rng(seed)
    lens = [len(x) for x in seqs]
    r = random_ranges(lens, samples, rng)
    sym, off, st = gx.extract(r, want_stats=True)
    assert off[-1] == r["len"].sum() and sym.size == off[-1]
    for i in range(r.size):
        s, p, l = (int(r[k][i]) for k in ("seq_id", "pos", "len"))
        assert sym[int(off[i]): int(off[i + 1])].tobytes() == seqs[s][p: p + l].tobytes(), (i, s, p, l)
    assert st.lf_steps == predicted_steps(r, lens, samples)
    assert st.hits == off[-1] and st.kernel_ms > 0
    s2, o2 = gx.extract(r["seq_id"], r["pos"], r["len"])                         # the three-array form
    assert s2.tobytes() == sym.tobytes() and np.array_equal(o2, off)
    return r, sym


def test_ranges_regular_and_irregular():
    seqs = sequences(16, 5, seed=21, count=200, long=5000)
    for wide in (0, 1):
        with fm.options(force_wide=wide):
            gx = fm.BiFMIndex.from_sequences(seqs, 5, "IB16", 16)
        gx.accelerate_extract()
        samples = {i: np.arange(0, len(x) + 1, 16) for i, x in enumerate(seqs)}
        check_ranges(gx, seqs, samples, seed=wide)
        ix, isamp = irregular_index("IB16", 5, seqs, wide, seed=9)
        ix.accelerate_extract()
        check_ranges(ix, seqs, isamp, seed=7 + wide)


def test_host_and_device_memory():
    torch = pytest.importorskip("torch")
    seqs = sequences(16, 5, seed=4, count=100, long=4000)
    gx = fm.FMIndex.from_sequences(seqs, 5, "IB16", 16).accelerate_extract()
    samples = {i: np.arange(0, len(x) + 1, 16) for i, x in enumerate(seqs)}
    r = random_ranges([len(x) for x in seqs], samples, np.random.default_rng(8))
    want, off = gx.extract(r)
    total = int(off[-1])
    dev = torch.device("cuda", 0)
    dr = torch.from_numpy(r.view(np.uint8).copy()).to(dev)
    for rin in ("host", "device"):
        for rout in ("host", "device"):
            src = r if rin == "host" else dr
            if rout == "host":
                got, o = gx.extract(src)
                got = got.tobytes()
            else:
                out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device=dev)
                cnt, o = gx.extract(src, out=out)
                assert cnt == total
                host = out.cpu().numpy()
                assert (host[total:] == 0xAB).all()                               # nothing written past the symbols
                got = host[:total].tobytes()
            assert got == want.tobytes() and np.array_equal(o, off), (rin, rout)
    buf = fm.DeviceBuffer.from_array(r)
    got, o = gx.extract(buf)
    assert got.tobytes() == want.tobytes()
    buf.free()


# ------------------------------------------------------------------------------------------------ 5. errors and bookkeeping
def test_errors_and_bookkeeping():
    seqs = sequences(16, 5, seed=6, count=50, long=500)
    gx = fm.FMIndex.from_sequences(seqs, 5, "IB16", 16)
    L = capi.lib()
    r = np.zeros(3, dtype=TEXT_RANGE_DTYPE)
    r["seq_id"], r["pos"], r["len"] = [5, 0, 7], [0, 0, 1], [len(seqs[5]), 0, len(seqs[7]) - 1]
    total = int(r["len"].sum())
    out = np.full(total + 8, 0x5A, dtype=np.uint8)
    cnt = C.c_uint64()
    assert L.fmgpu_extract(gx._h, capi.ptr(r), 3, capi.ptr(out), total, C.byref(cnt), None, None) == capi.FMGPU_ERR_UNSUPPORTED
    assert L.fmgpu_sequence_lengths(gx._h, None, None, 0, C.byref(cnt)) == capi.FMGPU_ERR_UNSUPPORTED
    assert not gx.formats & capi.FMT_EXTRACT
    before = gx.device_bytes
    gx.accelerate_extract()
    assert gx.formats & capi.FMT_EXTRACT
    grown = gx.device_bytes - before
    nsamp = sum(len(x) // 16 + 1 for x in seqs)
    assert grown >= nsamp * 12 + len(seqs) * 28
    assert L.fmgpu_extract(gx._h, capi.ptr(r), 3, capi.ptr(out), total - 1, C.byref(cnt), None, None) == capi.FMGPU_ERR_CAPACITY
    assert cnt.value == total and (out == 0x5A).all()                           # the output is untouched
    assert L.fmgpu_extract(gx._h, capi.ptr(r), 3, capi.ptr(out), total, C.byref(cnt), None, None) == 0 and cnt.value == total
    assert out[:total].tobytes() == seqs[5].tobytes() + seqs[7][1:].tobytes() and (out[total:] == 0x5A).all()
    assert L.fmgpu_extract(gx._h, capi.ptr(r), 0, None, 0, C.byref(cnt), None, None) == 0 and cnt.value == 0
    for field, value in (("len", len(seqs[7])), ("seq_id", len(seqs)), ("seq_id", 1 << 40)):
        bad = r.copy()
        bad[field][2] = value                                                   # pos 1 + len_s, or an unknown seqId
        assert L.fmgpu_extract(gx._h, capi.ptr(bad), 3, capi.ptr(out), total + 8, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID, field
    edge = r.copy()
    edge["pos"][2], edge["len"][2] = len(seqs[7]), 0                            # pos = len_s, len 0: valid
    assert L.fmgpu_extract(gx._h, capi.ptr(edge), 3, capi.ptr(out), total + 8, C.byref(cnt), None, None) == 0
    ids = np.zeros(len(seqs), dtype=np.uint64)
    assert L.fmgpu_sequence_lengths(gx._h, capi.ptr(ids), capi.ptr(ids), len(seqs) - 1, C.byref(cnt)) == capi.FMGPU_ERR_CAPACITY and cnt.value == len(seqs)
    assert L.fmgpu_extract(gx._h, None, 3, capi.ptr(out), total, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_extract(gx._h, capi.ptr(r), 3, None, total, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    gx.accelerate_extract(True)                                                 # rebuilding replaces the table: the bytes do not add up twice
    assert gx.device_bytes == before + grown
    gx.accelerate_extract(False)
    assert gx.device_bytes == before and not gx.formats & capi.FMT_EXTRACT
    assert L.fmgpu_extract(gx._h, capi.ptr(r), 3, capi.ptr(out), total, C.byref(cnt), None, None) == capi.FMGPU_ERR_UNSUPPORTED
    nosa = fm.FMIndex.from_reference_arrays(**{k: v for k, v in oracle_arrays(fo.OraIndex.build("IB16", 5, seqs[:5], 4, False)).items() if k != "sparse"})
    with pytest.raises(fm.FmgpuError) as e:
        nosa.accelerate_extract()
    assert e.value.code == capi.FMGPU_ERR_INVALID


def test_save_load_and_clone(tmp_path):
    seqs = sequences(16, 5, seed=8, count=80, long=1500)
    gx = fm.BiFMIndex.from_sequences(seqs, 5, "IB16", 16).accelerate_extract()
    rng = np.random.default_rng(2)
    r = random_ranges([len(x) for x in seqs], {i: np.arange(0, len(x) + 1, 16) for i, x in enumerate(seqs)}, rng, count=500)
    want, off = gx.extract(r)
    path = str(tmp_path / "x.fmgpu")
    gx.save(path)
    for other in (fm.FMIndex.load(path), gx.clone()):
        assert not other.formats & capi.FMT_EXTRACT
        with pytest.raises(fm.FmgpuError) as e:
            other.extract(r)
        assert e.value.code == capi.FMGPU_ERR_UNSUPPORTED
        base = other.device_bytes
        other.accelerate_extract()
        assert other.device_bytes > base
        got, o = other.extract(r)
        assert got.tobytes() == want.tobytes() and np.array_equal(o, off)


# ------------------------------------------------------------------------------------------------ 6. size
def test_genome_like_text_both_widths():
    """a ~50 Mbp repeat-structured text: launches of many blocks and pieces, in both row widths"""
    torch = pytest.importorskip("torch")
    import bench
    from fmindex_collection_amd import datasets
    dev = torch.device("cuda", 0)
    scale = 50e6 / sum(bench.GRCH38_LENGTHS)
    lengths = [max(1000, int(l * scale)) for l in bench.GRCH38_LENGTHS]
    text, _ = datasets.genome_like_text(lengths, seed=23, device=dev)
    host = text.cpu().numpy()
    seq_off = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    seqs = [host[seq_off[i]: seq_off[i + 1]] for i in range(len(lengths))]
    for wide in (0, 1):
        with fm.options(force_wide=wide):
            gx = fm.FMIndex.from_sequences(seqs, 5, "IB16", 16)
        assert gx.row_bits == (64 if wide else 32)
        gx.accelerate_extract()
        ids, lens = gx.sequence_lengths()
        sym, off, st = gx.extract(ids, np.zeros_like(ids), lens, want_stats=True)
        assert sym.tobytes() == host.tobytes(), wide
        assert st.lf_steps == host.size
        rng = np.random.default_rng(wide)
        s = rng.integers(0, len(seqs), size=100_000)
        p = (rng.random(s.size) * (np.asarray(lengths)[s] - 200)).astype(np.int64)
        w, wo = gx.extract(s, p, np.full(s.size, 200))
        starts = seq_off[s] + p
        assert np.array_equal(w.reshape(-1, 200), host[starts[:, None] + np.arange(200)[None, :]])
        del gx
