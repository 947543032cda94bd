"""4-bit packed query batches on the device (include/fmgpu.h): fmgpu_queries_pack4 / unpack4 against the host packer, and the `_q4` search calls against
the byte calls and the oracle — the kernels that read nibbles themselves (k_exact_p, k_exact_a), the unpack route in front of every other kernel, every
placement of a packed buffer, both strands made on the device, and the refusal of alphabets that do not fit a nibble."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests.util import oracle_arrays
from tests.test_gpu_exact_window import build, texts, reads_for, foreign_reads

pytestmark = pytest.mark.gpu

COMP = np.array([0, 4, 3, 2, 1], dtype=np.uint8)


def device_copy(host, shift=0, fill=0xff, slack=48):
    """`host` at byte `shift` of a fresh device allocation whose other bytes are `fill`: (buffer to keep alive, device address of the copy)"""
    a = np.full(host.nbytes + shift + slack, fill, dtype=np.uint8)
    a[shift: shift + host.nbytes] = host.view(np.uint8).reshape(-1)
    buf = fm.DeviceBuffer.from_array(a)
    return buf, buf.ptr + shift


def both_strands(reads, sigma=5):
    out = []
    for r in reads:
        out.append(np.asarray(r, dtype=np.uint8))
        out.append(np.array([COMP[c] if c < sigma else 255 for c in r[::-1]], dtype=np.uint8))
    return out


# ------------------------------------------------------------------------------------------------------------------------ 1. the packer
def packer_batches():
    rng = np.random.default_rng(17)
    lengths = list(range(41)) + [101, 127, 128, 129, 300]
    out = {}
    for sigma in (5, 15):
        reads = []
        for m in rng.permutation(lengths):
            r = rng.integers(0, sigma, size=int(m), dtype=np.uint8)
            if m:
                for at, byte in zip((0, int(m) // 2, int(m) - 1), (sigma, 200, 255)):      # foreign bytes at the first, middle and last position (of some reads)
                    if rng.integers(0, 4) == 0:
                        r[at] = byte
            reads.append(r)
        reads.append(np.array([255], dtype=np.uint8)); reads.append(np.array([sigma, 1, 200, 2, 255], dtype=np.uint8))
        out[sigma] = reads
    out["odd"] = [rng.integers(0, 5, size=int(m), dtype=np.uint8) for m in rng.permutation([1, 3, 5, 7, 9, 11, 13, 15, 17, 33, 101, 129])]
    return out


def check_packer(queries, sigma, comp, want, where):
    got = fm.pack_queries_device(queries, sigma, comp)
    packed, qoff = got.host()
    assert got.nq == want.nq and np.array_equal(qoff, want.qoff), where
    assert packed.tobytes() == want.packed.tobytes(), where


@pytest.mark.parametrize("comp", [None, COMP], ids=["one_strand", "both_strands"])
def test_device_packer_equals_host_packer(comp):
    batches = packer_batches()
    for key, sigma in ((5, 5), (15, 15), ("odd", 5)):
        if comp is not None and sigma != 5:
            comp_s = np.concatenate([[0], np.arange(sigma - 1, 0, -1)]).astype(np.uint8)     # (any table will do: symbol c <-> sigma - c)
        else:
            comp_s = comp
        qbuf, qoff = fm.flatten(batches[key])
        want = fm.pack_queries((qbuf, qoff), sigma, comp_s)
        check_packer((qbuf, qoff), sigma, comp_s, want, (key, "host pointers"))
        dq, do = fm.DeviceBuffer.from_array(qbuf), fm.DeviceBuffer.from_array(qoff)
        check_packer((dq, do), sigma, comp_s, want, (key, "device pointers"))
        # the batch does not start at symbol 0
        sbuf, soff = np.concatenate([np.full(3, 9, dtype=np.uint8), qbuf]), qoff + np.uint64(3)
        check_packer((sbuf, soff), sigma, comp_s, want, (key, "qoff[0] = 3"))
        if key == 5:
            for shift in range(16):                                   # the byte buffer at every offset of a device allocation
                keep, at = device_copy(qbuf, shift)
                check_packer((at, qoff), sigma, comp_s, want, (key, "shift", shift))
                keep.free()
    # the C call's complement table in device memory, and unpack4 on the device
    qbuf, qoff = fm.flatten(batches[5])
    want = fm.pack_queries((qbuf, qoff), 5, comp)
    got = fm.pack_queries_device((qbuf, qoff), 5, None if comp is None else fm.DeviceBuffer.from_array(comp).to_array(np.uint8, 5))
    assert got.host()[0].tobytes() == want.packed.tobytes()
    total = int(want.qoff[-1])
    out = fm.DeviceBuffer(total + 8)
    capi.check(capi.lib().fmgpu_queries_unpack4(capi.ptr(got.packed), capi.ptr(got.qoff), got.nq, capi.ptr(out), None))
    capi.check(capi.lib().fmgpu_synchronize(None))
    assert np.array_equal(out.to_array(np.uint8, total), fm.unpack_queries(want)[0])
    host_out = np.zeros(total, dtype=np.uint8)
    capi.check(capi.lib().fmgpu_queries_unpack4(capi.ptr(want.packed), capi.ptr(want.qoff), want.nq, capi.ptr(host_out), None))
    assert np.array_equal(host_out, fm.unpack_queries(want)[0])


# ------------------------------------------------------------------------------------------------------------------------ 2. exact search, the kernels that read nibbles
@functools.lru_cache(maxsize=None)
def exact_case(kind="uniform"):
    seqs = texts(kind)
    ox = fo.OraIndex.build("IB16", 5, seqs, 4, False)
    qbuf, qoff = fm.flatten(reads_for(seqs, 5))
    olb, oln, ost = ox.search_exact(qbuf, qoff, want_steps=True)
    fq = fm.flatten(foreign_reads(seqs, 6))
    return seqs, ox, (qbuf, qoff), (olb, oln, ost), fq


def same_exact(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].lf_steps == b[2].lf_steps and a[2].hits == b[2].hits and \
        a[2].table_bytes == b[2].table_bytes and a[2].table_accesses == b[2].table_accesses and a[2].table_steps == b[2].table_steps


@pytest.mark.parametrize("pairs", [True, False], ids=["k_exact_p", "k_exact_a"])
@pytest.mark.parametrize("wide", [False, True], ids=["rows32", "rows64"])
def test_exact_search_reads_the_packed_form(wide, pairs):
    seqs, ox, (qbuf, qoff), (olb, oln, ost), fq = exact_case()
    gx = build(ox, wide, pairs=pairs)
    pq, pf = fm.pack_queries((qbuf, qoff), 5), fm.pack_queries(fq, 5)
    fbytes = fm.unpack_queries(pf)                                   # the foreign reads as the packed form holds them (255 for every byte >= 5)
    for lut_len in (0, 1, 7, 10):                                    # (without pairs the interval table sends the call through the unpack route)
        if lut_len:
            gx.accelerate(1, lut_len=lut_len, walk=0)
        for select in (0, capi.SEL_UNPACK_QUERIES):
            with fm.options(kernel_select=select):
                got = fm.search_no_errors.search(gx, pq, want_stats=True)
                byte = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
                assert np.array_equal(got[0], olb) and np.array_equal(got[1], oln) and got[2].lf_steps == int(ost.sum()), (lut_len, select)
                assert same_exact(got, byte), (lut_len, select)
                f4, f1 = fm.search_no_errors.search(gx, pf, want_stats=True), fm.search_no_errors.search(gx, fbytes, want_stats=True)
                assert not f4[1].any() and same_exact(f4, f1), (lut_len, select)
    gx.accelerate(1, lut_len=0, walk=0)
    for i in range(0, len(qoff) - 1, 37):                            # one read per batch
        if qoff[i + 1] == qoff[i]:
            continue
        one = fm.pack_queries((qbuf[qoff[i]: qoff[i + 1]], np.array([0, qoff[i + 1] - qoff[i]], dtype=np.uint64)), 5)
        a, b, s1 = fm.search_no_errors.search(gx, one, want_stats=True)
        assert (a[0], b[0], s1.lf_steps) == (olb[i], oln[i], int(ost[i])), i


def test_exact_search_on_a_text_without_symbol_4():
    seqs, ox, (qbuf, qoff), (olb, oln, ost), fq = exact_case("no_symbol_4")
    gx = build(ox, False)
    got = fm.search_no_errors.search(gx, fm.pack_queries((qbuf, qoff), 5), want_stats=True)
    assert np.array_equal(got[0], olb) and np.array_equal(got[1], oln) and got[2].lf_steps == int(ost.sum())


# ------------------------------------------------------------------------------------------------------------------------ 3. every placement of the packed buffer
@pytest.mark.parametrize("pairs", [True, False], ids=["k_exact_p", "k_exact_a"])
def test_packed_buffer_at_every_alignment(pairs):
    seqs, ox = exact_case()[:2]
    gx = build(ox, False, pairs=pairs)
    rng = np.random.default_rng(8)
    s = seqs[0]
    reads = []
    for m in list(range(1, 40)) + [101, 127, 128, 129, 150]:
        p = int(rng.integers(0, len(s) - m + 1))
        reads.append(s[p: p + m].copy())
    qbuf, qoff = fm.flatten(reads)
    olb, oln, ost = ox.search_exact(qbuf, qoff, want_steps=True)
    total = int(qoff[-1])
    for lead in (0, 1):                                              # the batch's first symbol is the low / the high nibble of its first byte
        nib = np.concatenate([np.full(lead, 15, dtype=np.uint8), qbuf[:total]])
        nib = np.concatenate([nib, np.full(nib.size & 1, 15, dtype=np.uint8)])            # (every nibble around the batch is 15, every byte around it 0xff)
        packed = (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)
        for shift in range(16):
            keep, at = device_copy(packed, shift)
            pq = fm.PackedQueries(at, qoff + np.uint64(lead))
            lb, ln, st = fm.search_no_errors.search(gx, pq, want_stats=True)
            assert np.array_equal(ln, oln) and np.array_equal(lb, olb) and st.lf_steps == int(ost.sum()), (lead, shift)
            keep.free()


# ------------------------------------------------------------------------------------------------------------------------ 4. exact search through the unpack route
def test_exact_search_behind_kstep_and_walk_tables():
    seqs, ox, (qbuf, qoff), (olb, oln, ost), fq = exact_case()
    pq, pf = fm.pack_queries((qbuf, qoff), 5), fm.pack_queries(fq, 5)
    fbytes = fm.unpack_queries(pf)
    for tables in (dict(kstep=3), dict(kstep=3, lut_len=6, walk=True)):
        gx = build(ox, False)
        gx.accelerate(**tables)
        got, byte = fm.search_no_errors.search(gx, pq, want_stats=True), fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
        assert np.array_equal(got[0], olb) and np.array_equal(got[1], oln) and same_exact(got, byte), tables
        assert same_exact(fm.search_no_errors.search(gx, pf, want_stats=True), fm.search_no_errors.search(gx, fbytes, want_stats=True)), tables


@pytest.mark.parametrize("layout,sigma,select", [("WAVELET", 12, 0), ("WAVELET", 12, capi.SEL_EXACT_ON_TREE), ("EPR16", 6, 0), ("WAVELET", 15, 0)])
def test_exact_search_on_alphabets_of_6_to_15(layout, sigma, select):
    rng = np.random.default_rng(23)
    seqs = [rng.integers(1, sigma, size=4000, dtype=np.uint8), rng.integers(1, sigma, size=700, dtype=np.uint8)]
    ox = fo.OraIndex.build(layout, sigma, seqs, 4, False)
    gx = fm.FMIndex.from_reference_arrays(**oracle_arrays(ox))
    if layout == "WAVELET":
        assert bool(gx.formats & capi.FMT_PLANES)
    reads = []
    for m in list(range(1, 20)) + [33, 64, 101]:
        for _ in range(3):
            p = int(rng.integers(0, 4000 - m + 1))
            r = seqs[0][p: p + m].copy()
            reads.append(r.copy())
            r[int(rng.integers(0, m))] = int(rng.integers(0, sigma)); reads.append(r.copy())
            r[int(rng.integers(0, m))] = [sigma, 200, 255][int(rng.integers(0, 3))]; reads.append(r)
    reads.append(np.zeros(0, dtype=np.uint8))
    qbuf, qoff = fm.flatten(reads)
    pq = fm.pack_queries((qbuf, qoff), sigma)
    ubytes = fm.unpack_queries(pq)
    clean = np.array([not (r >= sigma).any() for r in reads])        # (a byte outside the alphabet is undefined in the reference: the oracle never sees one)
    olb, oln = ox.search_exact(*fm.flatten([r for r, ok in zip(reads, clean) if ok]))
    with fm.options(kernel_select=select):
        got, byte = fm.search_no_errors.search(gx, pq, want_stats=True), fm.search_no_errors.search(gx, ubytes, want_stats=True)
    assert same_exact(got, byte)
    assert np.array_equal(got[0][clean], olb) and np.array_equal(got[1][clean], oln) and (oln > 0).sum() > 20


# ------------------------------------------------------------------------------------------------------------------------ 5. scheme searches
@functools.lru_cache(maxsize=None)
def scheme_case():
    rng = np.random.default_rng(31)
    base = rng.integers(1, 5, size=3000, dtype=np.uint8)
    seqs = [base, base[500:1500].copy(), rng.integers(1, 5, size=800, dtype=np.uint8)]
    seqs[1][rng.integers(0, 1000, size=15)] = rng.integers(1, 5, size=15)
    ox = fo.OraIndex.build("IB16", 5, seqs, 4, True)
    gx = fm.BiFMIndex.from_reference_arrays(**oracle_arrays(ox))

    def reads(lengths):
        out = []
        for i, m in enumerate(lengths):
            p = int(rng.integers(0, 3000 - m + 1))
            r = base[p: p + m].copy()
            for _ in range(i % 3):
                r[int(rng.integers(0, m))] = int(rng.integers(1, 5))
            if i % 19 == 0:
                r[int(rng.integers(0, m))] = 0                       # a delimiter
            if i % 23 == 0:
                r[int(rng.integers(0, m))] = [5, 9, 255][i % 3]      # a foreign symbol
            out.append(r)
        return out
    equal = fm.flatten(reads([32] * 240))
    ragged = fm.flatten(reads([int(m) for m in rng.integers(12, 60, size=200)]) + [np.zeros(0, dtype=np.uint8), np.array([1], dtype=np.uint8)])
    return ox, gx, equal, ragged


def raw_hits(gx, call, queries, scheme_struct, n, capacity):
    qbuf, qoff, nq = fm._queries(queries)
    out = np.zeros(max(capacity, 1), dtype=capi.HIT_DTYPE)
    cnt, st = C.c_uint64(), capi.Stats()
    rc = call(gx._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(scheme_struct), n, capi.ptr(out), capacity, C.byref(cnt), C.byref(st), None)
    if rc == 0:
        out = np.ascontiguousarray(out[: cnt.value])
        capi.check(capi.lib().fmgpu_hits_sort(capi.ptr(out), out.size, None))
    return rc, int(cnt.value), out, st


def scheme_struct(scheme, edit=False):
    pi, l, u = (fm._u64(x) for x in scheme)
    sc = capi.Scheme()
    sc.n_searches, sc.n_parts = pi.shape
    sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    sc.partition, sc.edit = None, 1 if edit else 0
    return sc, (pi, l, u)


def expanded_struct(scheme):
    pi, l, u = (fm._u64(x) for x in scheme)
    sc = capi.ExpandedScheme()
    sc.n_searches, sc.length = pi.shape
    sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    return sc, (pi, l, u)


SCHEME_CASES = ["lean", "no_lean", "ragged", "edit", "n3", "ng21"]


@pytest.mark.parametrize("case", SCHEME_CASES)
def test_scheme_searches_on_packed_batches(case):
    ox, gx, equal, ragged = scheme_case()
    L = capi.lib()
    queries = ragged if case == "ragged" else equal
    select, n = (capi.SEL_NO_LEAN if case == "no_lean" else 0), (3 if case == "n3" else capi.UINT64_MAX)
    if case == "ng21":
        sc, keep = expanded_struct(fm.search_scheme.expand(fm.search_scheme.pigeon_opt(0, 1), 32))
        calls = (L.fmgpu_search_ng21, L.fmgpu_search_ng21_q4)
    else:
        sc, keep = scheme_struct(fm.search_scheme.h2(3, 0, 1) if case == "edit" else fm.search_scheme.h2(4, 0, 2), edit=case == "edit")
        calls = (L.fmgpu_search_scheme, L.fmgpu_search_scheme_q4)
    pq = fm.pack_queries(queries, 5)
    ubytes = fm.unpack_queries(pq)
    with fm.options(kernel_select=select):
        rc1, c1, h1, s1 = raw_hits(gx, calls[0], ubytes, sc, n, 1 << 16)
        rc4, c4, h4, s4 = raw_hits(gx, calls[1], pq, sc, n, 1 << 16)
        dq = fm.PackedQueries(fm.DeviceBuffer.from_array(pq.packed), fm.DeviceBuffer.from_array(pq.qoff), pq.nq)
        rcd, cd, hd, sd = raw_hits(gx, calls[1], dq, sc, n, 1 << 16)
        assert rc1 == 0 and rc4 == 0 and rcd == 0 and c1 == c4 == cd and c1 > pq.nq // 2
        assert h1.tobytes() == h4.tobytes() == hd.tobytes()
        assert (s1.hits, s1.lf_steps) == (s4.hits, s4.lf_steps) == (sd.hits, sd.lf_steps)
        small = raw_hits(gx, calls[0], ubytes, sc, n, c1 // 2), raw_hits(gx, calls[1], pq, sc, n, c1 // 2)
        assert small[0][0] == small[1][0] == capi.FMGPU_ERR_CAPACITY and small[0][1] == small[1][1] == c1


# ------------------------------------------------------------------------------------------------------------------------ 6. both strands
def test_both_strands_made_on_the_device():
    ox, gx, equal, ragged = scheme_case()
    qbuf, qoff = equal
    reads = [qbuf[int(qoff[i]): int(qoff[i + 1])] for i in range(len(qoff) - 1)]
    host_both = fm.flatten(both_strands(reads))
    pq = fm.pack_queries_device((fm.DeviceBuffer.from_array(qbuf), fm.DeviceBuffer.from_array(qoff)), 5, COMP)
    assert pq.nq == 2 * len(reads)
    ubytes = fm.unpack_queries(fm.pack_queries(host_both, 5))        # (the host-made batch, foreign bytes as 255)
    a, b = fm.search_no_errors.search(gx, pq, want_stats=True), fm.search_no_errors.search(gx, ubytes, want_stats=True)
    assert same_exact(a, b) and (a[1] > 0).sum() > 20
    clean = np.repeat(np.array([not (r >= 5).any() for r in reads]), 2)     # (a byte outside the alphabet is undefined in the reference: the oracle never sees one)
    olb, oln = ox.search_exact(*fm.flatten([r for r, ok in zip(both_strands(reads), clean) if ok]))
    assert np.array_equal(a[0][clean], olb) and np.array_equal(a[1][clean], oln)
    sch = fm.search_scheme.h2(3, 0, 1)
    h4, hb = fm.search_ng26.search(gx, pq, sch), fm.search_ng26.search(gx, ubytes, sch)
    assert len(h4) > len(reads) // 2 and h4.tobytes() == hb.tobytes()      # (two reads in three carry at most one substitution: their forward strand is found)
    for errors in (0, 1):
        p4, pb = fm.search_locate(gx, pq, errors), fm.search_locate(gx, ubytes, errors)
        assert len(p4) > 20 and p4.tobytes() == pb.tobytes(), errors
    assert fm.search(gx, pq, 1).tobytes() == fm.search(gx, ubytes, 1).tobytes()
    assert fm.search_n(gx, pq, 1, 2).tobytes() == fm.search_n(gx, ubytes, 1, 2).tobytes()


# ------------------------------------------------------------------------------------------------------------------------ 7. refusal
def test_alphabets_beyond_15_are_refused():
    rng = np.random.default_rng(41)
    seqs = [rng.integers(1, 28, size=2000, dtype=np.uint8)]
    ox = fo.OraIndex.build("WAVELET", 28, seqs, 4, True)
    gx = fm.BiFMIndex.from_reference_arrays(**oracle_arrays(ox))
    L = capi.lib()
    packed, qoff = np.array([0x21, 0x43], dtype=np.uint8), np.array([0, 2, 4], dtype=np.uint64)
    lb, ln = np.full(2, 77, dtype=np.uint64), np.full(2, 77, dtype=np.uint64)
    st = capi.Stats(); st.lf_steps = 77
    assert L.fmgpu_search_exact_q4(gx._h, capi.ptr(packed), capi.ptr(qoff), 2, capi.ptr(lb), capi.ptr(ln), C.byref(st), None) == capi.FMGPU_ERR_UNSUPPORTED
    assert b"sigma" in L.fmgpu_last_error() and (lb == 77).all() and (ln == 77).all() and st.lf_steps == 77
    out, cnt = np.full(16, 7, dtype=capi.HIT_DTYPE), C.c_uint64(77)
    sc, keep = scheme_struct(fm.search_scheme.h2(3, 0, 1))
    assert L.fmgpu_search_scheme_q4(gx._h, capi.ptr(packed), capi.ptr(qoff), 2, C.byref(sc), capi.UINT64_MAX, capi.ptr(out), 16, C.byref(cnt), C.byref(st), None) == capi.FMGPU_ERR_UNSUPPORTED
    ex, keep2 = expanded_struct(fm.search_scheme.expand(fm.search_scheme.pigeon_opt(0, 1), 2))
    assert L.fmgpu_search_ng21_q4(gx._h, capi.ptr(packed), capi.ptr(qoff), 2, C.byref(ex), capi.UINT64_MAX, capi.ptr(out), 16, C.byref(cnt), C.byref(st), None) == capi.FMGPU_ERR_UNSUPPORTED
    assert cnt.value == 77 and st.lf_steps == 77 and out.tobytes() == np.full(16, 7, dtype=capi.HIT_DTYPE).tobytes()
    with pytest.raises(fm.FmgpuError):
        fm.search_no_errors.search(gx, fm.PackedQueries(packed, qoff))
