"""fmgpu_search_hamming_sm / fm.search_hamming_sm: with the identity matrix against fmgpu_search_scheme on the same handle, with IUPAC and protein matrices against the
plain-Python walk of tests/hamming_sm_model.py (records field for field, `seq` and the step count included) and its brute-force scorer.  Every check is exact.
Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, UINT64_MAX
from tests import hamming_sm_model as model
from tests.util import oracle_arrays

pytestmark = pytest.mark.gpu

LAYOUTS = [("IB16", 5), ("IB16", 21), ("WAVELET", 21), ("EPR16", 21)]
PROTEIN_EXTRA = {21: 5, 22: 13, 23: 4, 24: 7, 25: 12, 26: 17, 27: 19}      # the reference test's setCost calls on ScoringMatrix<28, 21>


# ------------------------------------------------------------------------------------------------ texts, indices, matrices (made once, never modified)
@functools.lru_cache(maxsize=None)
def sequences(sigma, small=False):
    rng = np.random.default_rng(300 + sigma + small)
    unit = rng.integers(1, sigma, size=7, dtype=np.uint8)
    if small:                                                       # <= 600 symbols: bounds what a read of N can enumerate
        return [rng.integers(1, sigma, size=400, dtype=np.uint8), np.tile(unit, 20), rng.integers(1, sigma, size=40, dtype=np.uint8)]
    return [rng.integers(1, sigma, size=3500, dtype=np.uint8), np.tile(unit, 40), rng.integers(1, sigma, size=50, dtype=np.uint8)]


@functools.lru_cache(maxsize=None)
def oracle(layout, sigma, small=False):
    return fo.OraIndex.build(layout, sigma, sequences(sigma, small), 2, True)


@functools.lru_cache(maxsize=None)
def handle(layout, sigma, wide, small=False):
    with fm.options(force_wide=wide):
        gx = fm.BiFMIndex.from_reference_arrays(**oracle_arrays(oracle(layout, sigma, small)))
    assert gx.row_bits == (64 if wide else 32)
    return gx


def iupac():
    return fm.ScoringMatrix.iupac_dna()


def protein():
    sm = fm.ScoringMatrix(28, 21)
    for q, r in PROTEIN_EXTRA.items():
        sm.set_cost(q, r, 0)
    return sm


def window(rng, seqs, sigma, m, subs=0, seq=0):
    s = seqs[seq]
    at = int(rng.integers(0, len(s) - m + 1))
    r = s[at: at + m].copy()
    for _ in range(subs):
        p = int(rng.integers(0, m))
        r[p] = (int(r[p]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1
    return r


def degenerate(rng, r, sigma, count, stray):
    """`count` positions of the read get a code that still holds the base, `stray` positions an arbitrary code of the query alphabet"""
    if sigma == 5:
        holds = {b: [5 + k for k, bases in enumerate(fm.ScoringMatrix.IUPAC.values()) if "ACGT"[b - 1] in bases] for b in range(1, 5)}
        top = 16
    else:
        holds = {r_: [q] for q, r_ in PROTEIN_EXTRA.items()}
        top = 28
    for p in rng.choice(len(r), size=min(count, len(r)), replace=False):
        if int(r[p]) in holds:
            r[p] = int(rng.choice(holds[int(r[p])]))
    for p in rng.choice(len(r), size=min(stray, len(r)), replace=False):
        r[p] = int(rng.integers(1, top))
    return r


@functools.lru_cache(maxsize=None)
def ragged_batch(sigma):
    """the read lengths at which the kernel takes another path: m = P, P + 1 (P = the scheme's parts), the wave-size neighbours, one read past the byte-staging budget (global-memory
    reads), an empty read and one shorter than P, and reads with degenerate positions; in the random text, the tandem repeat and the short sequence"""
    rng = np.random.default_rng(11 + sigma)
    seqs = sequences(sigma)
    P = scheme_for(sigma)[0].shape[1]
    reads = [window(rng, seqs, sigma, P), window(rng, seqs, sigma, P + 1, 1), degenerate(rng, window(rng, seqs, sigma, 63, 1), sigma, 4, 0),
             np.zeros(0, dtype=np.uint8), degenerate(rng, window(rng, seqs, sigma, 64, 2), sigma, 3, 1), window(rng, seqs, sigma, P - 1),
             degenerate(rng, window(rng, seqs, sigma, 65), sigma, 4, 1), degenerate(rng, window(rng, seqs, sigma, 300, 1), sigma, 4, 0)]
    for k in range(14):
        m = 20 + k % 5
        reads.append(degenerate(rng, window(rng, seqs, sigma, m, k % 3, seq=(0, 0, 1, 2)[k % 4]), sigma, 4, k % 3))
    return tuple(reads)


def scheme_for(sigma):
    return fo.scheme_h2(4, 0, 2) if sigma == 5 else fo.scheme_pigeon_opt(0, 1)


@functools.lru_cache(maxsize=None)
def ragged_model(sigma):
    """per read ([(lb, lb_rev, len, errors)], steps) of ragged_batch under the IUPAC / protein matrix"""
    sm = iupac() if sigma == 5 else protein()
    ox = oracle("IB16", sigma)
    return tuple(model.walk_read(ox, r, scheme_for(sigma), sm.free_mask, sm.cost_mask) for r in ragged_batch(sigma))


def assemble(per_read):
    recs = [(q, lb, lr, ln, e, seq) for q, (rs, _) in enumerate(per_read) for seq, (lb, lr, ln, e) in enumerate(rs)]
    return recs, sum(st for _, st in per_read)


def records(hits):
    return [(int(h["qidx"]), int(h["lb"]), int(h["lb_rev"]), int(h["len"]), int(h["errors"]), int(h["seq"])) for h in hits]


def run(gx, reads, scheme, sm, **kw):
    """reads: a sequence of reads, or flat=True: (qbuf, qoff)"""
    queries = reads if kw.pop("flat", False) else list(reads)
    hits, st = fm.search_hamming_sm.search(gx, queries, scheme, sm, want_stats=True, **kw)
    return records(hits), st


def check_model(gx, ox, reads, scheme, sm, **kw):
    want, steps = model.walk(ox, reads, scheme, sm.free_mask, sm.cost_mask, kw.get("partition"), kw.get("n", UINT64_MAX))
    got, st = run(gx, reads, scheme, sm, **kw)
    assert got == want
    assert st.lf_steps == steps and st.hits == len(want)
    return want


# ------------------------------------------------------------------------------------------------ 1. the identity matrix is fmgpu_search_scheme (Hamming)
@pytest.mark.parametrize("layout,sigma", LAYOUTS)
@pytest.mark.parametrize("wide", [0, 1])
def test_identity_matrix_is_search_scheme(layout, sigma, wide):
    gx = handle(layout, sigma, wide)
    seqs = sequences(sigma)
    sm = fm.ScoringMatrix(sigma)
    rng = np.random.default_rng(77)
    for scheme, m in ((fo.scheme_h2(4, 0, 2), 24), (fo.scheme_pigeon_opt(0, 1), 23), (fo.scheme_h2(5, 1, 3), 30)):
        reads = [window(rng, seqs, sigma, m, k % 3, seq=k % 2) for k in range(24)]      # (equal lengths: kernel_select = 0 takes the table-driven kernels where they serve)
        got, _ = run(gx, reads, scheme, sm)
        mine = sorted(r[:5] for r in got)
        assert len(mine) >= 12
        for select in (0, capi.SEL_GENERAL_DFS):
            with fm.options(kernel_select=select):
                hits = fm.search_ng26.search(gx, reads, scheme)
            assert sorted(r[:5] for r in records(hits)) == mine, select


# ------------------------------------------------------------------------------------------------ 2. + 3. IUPAC and (28, 21) matrices are the model; shapes
@pytest.mark.parametrize("layout,sigma", LAYOUTS)
@pytest.mark.parametrize("wide", [0, 1])
def test_matrix_batches_are_the_model(layout, sigma, wide):
    gx = handle(layout, sigma, wide)
    sm = iupac() if sigma == 5 else protein()
    reads = ragged_batch(sigma)
    want, steps = assemble(ragged_model(sigma))
    got, st = run(gx, reads, scheme_for(sigma), sm)
    assert got == want and st.lf_steps == steps and st.hits == len(want)
    # an empty result cannot pass: reads with several records, cursors of several rows, every error count, the long read found
    per_read = np.bincount([r[0] for r in want], minlength=len(reads))
    assert per_read.max() > 1 and per_read[3] == 0 and per_read[5] == 0 and per_read[7] >= 1
    assert any(r[3] > 1 for r in want) and {r[4] for r in want} == set(range(0, 3 if sigma == 5 else 2))
    assert st.table_accesses > 0 and st.table_bytes >= 12 * st.table_accesses and st.kernel_ms > 0


@functools.lru_cache(maxsize=None)
def many_reads():
    rng = np.random.default_rng(5)
    seqs = sequences(5)
    reads = []
    for k in range(257):
        r = window(rng, seqs, 5, 14 + k % 4, k % 3, seq=(0, 0, 0, 1)[k % 4])
        r[int(rng.integers(0, len(r)))] = 15 if k % 2 else int(rng.integers(5, 15))
        reads.append(r)
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def many_model():
    sm, ox = iupac(), oracle("IB16", 5)
    return tuple(model.walk_read(ox, r, scheme_for(5), sm.free_mask, sm.cost_mask) for r in many_reads())


@pytest.mark.parametrize("wide", [0, 1])
def test_batch_sizes_and_memory_spaces(wide):
    gx = handle("IB16", 5, wide)
    sm, scheme = iupac(), scheme_for(5)
    reads, per_read = many_reads(), many_model()
    for nq in (1, 63, 64, 65, 257):
        want, steps = assemble(per_read[:nq])
        got, st = run(gx, reads[:nq], scheme, sm)
        assert got == want and st.lf_steps == steps, nq
    assert len(want) > 200
    # qoff[0] = 13, host and device buffers, through the C ABI
    qbuf, qoff = fm.flatten(list(reads))
    qbuf = np.concatenate([np.full(13, 3, dtype=np.uint8), qbuf])
    qoff = qoff + np.uint64(13)
    got, st = run(gx, (qbuf, qoff), scheme, sm, flat=True)
    assert got == want and st.lf_steps == steps
    pi, l, u = (np.ascontiguousarray(x, dtype=np.uint64) for x in scheme)
    sc = capi.Scheme()
    sc.n_searches, sc.n_parts = pi.shape
    sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    m = sm._struct()
    count = len(want)
    dq, do, dh = fm.DeviceBuffer.from_array(qbuf), fm.DeviceBuffer.from_array(qoff), fm.DeviceBuffer((count + 1) * HIT_DTYPE.itemsize)
    cnt = C.c_uint64()
    L = capi.lib()
    for q_, o_ in ((dq, do), (dq, qoff), (qbuf, do)):
        capi.check(L.fmgpu_search_hamming_sm(gx._h, capi.ptr(q_), capi.ptr(o_), len(reads), C.byref(sc), C.byref(m), UINT64_MAX, capi.ptr(dh), count + 1, C.byref(cnt), None, None))
        assert cnt.value == count
        capi.check(L.fmgpu_hits_sort(capi.ptr(dh), count, None))
        assert records(dh.to_array(HIT_DTYPE, count)) == want
    for b in (dq, do, dh):
        b.free()


# ------------------------------------------------------------------------------------------------ 4. symbols
@pytest.mark.parametrize("wide", [0, 1])
def test_symbols(wide):
    gx, ox = handle("IB16", 5, wide), oracle("IB16", 5)
    seqs = sequences(5)
    scheme = scheme_for(5)
    rng = np.random.default_rng(9)
    base = [window(rng, seqs, 5, 22, k % 3, seq=k % 2) for k in range(10)]
    # a matrix with query_sigma = 200: byte c >= 16 stands for base 1 + c % 4 (free) and costs one error against the others; reads holding bytes 16 .. 199
    wide_sm = fm.ScoringMatrix(200, 5)
    for c in range(16, 200):
        for r in range(1, 5):
            wide_sm.set_cost(c, r, 0 if r == 1 + c % 4 else 1)
    reads = [r.copy() for r in base]
    for k, r in enumerate(reads):
        for p in rng.choice(len(r), size=6, replace=False):
            r[p] = 16 + 4 * int(rng.integers(0, 46)) + (int(r[p]) - 1 if k % 2 else int(rng.integers(0, 4)))
    reads[3][5] = 199
    want = check_model(gx, ox, reads, scheme, wide_sm)
    assert len(want) >= 5 and max(int(r.max()) for r in reads) == 199
    # bytes >= query_sigma and 255, and a code whose two masks are empty, pair with nothing: such a read has no record
    sm = iupac().set_unpairable(9)
    reads = [r.copy() for r in base]
    reads[0][7], reads[1][0], reads[2][21], reads[3][11], reads[4][3] = 16, 255, 200, 9, 15
    want = check_model(gx, ox, reads, scheme, sm)
    found = {r[0] for r in want}
    assert not found & {0, 1, 2, 3} and 4 in found and len(found) >= 5
    # query symbol 0: without pairs (the default), and as a code of its own
    reads = [r.copy() for r in base]
    for r in reads[:6]:
        r[int(rng.integers(0, len(r)))] = 0
    none = check_model(gx, ox, reads, scheme, iupac())
    zero_is_any = iupac()
    for r in range(1, 5):
        zero_is_any.set_cost(0, r, 0)
    some = check_model(gx, ox, reads, scheme, zero_is_any)
    assert not {r[0] for r in none} & set(range(6)) and {r[0] for r in some} >= set(range(6))
    # a free mask that contains text symbol 0: a match across a delimiter is reported
    n_or_end = iupac().set_cost(15, 0, 0)
    across = np.concatenate([seqs[0][-9:], np.array([15], dtype=np.uint8), seqs[1][:9]])
    want = check_model(gx, ox, [across, base[0]], scheme, n_or_end)
    hits = fm.search_hamming_sm.search(gx, [across, base[0]], scheme, n_or_end)
    pos = gx.locate_hits(hits)
    assert (0, 0, len(seqs[0]) - 9, 0) in {(int(p["qidx"]), int(p["seq_id"]), int(p["pos"]), int(p["errors"])) for p in pos}
    assert not [r for r in model.walk(ox, [across], scheme, iupac().free_mask, iupac().cost_mask)[0] if r[4] == 0]      # (without that bit: no exact match)


@pytest.mark.parametrize("wide", [0, 1])
def test_a_read_of_n_enumerates_the_text(wide):
    gx, ox = handle("IB16", 5, wide, True), oracle("IB16", 5, True)
    seqs = sequences(5, True)
    assert sum(len(s) for s in seqs) <= 600
    reads = [np.full(8, 15, dtype=np.uint8), seqs[0][10:30].copy(), np.array([15, 15, 1, 15, 15, 2, 15, 15, 15], dtype=np.uint8)]
    want = check_model(gx, ox, reads, scheme_for(5), iupac())
    eight = [r for r in want if r[0] == 0]
    text = model.joined(seqs)[0]
    distinct = {text[i: i + 8].tobytes() for i in range(len(text) - 7) if text[i: i + 8].all()}
    # h2(4, 0, 2) covers 0 errors once: every distinct 8-mer of the text is one record of the read, its rows the 8-mer's occurrences
    assert len(eight) == len(distinct) > 300 and sum(r[3] for r in eight) == sum(1 for i in range(len(text) - 7) if text[i: i + 8].all())
    assert all(r[4] == 0 for r in eight)


# ------------------------------------------------------------------------------------------------ 5. hit limit and capacity
@pytest.mark.parametrize("wide", [0, 1])
def test_hit_limit_and_capacity(wide):
    gx, ox = handle("IB16", 5, wide), oracle("IB16", 5)
    sm, scheme = iupac(), scheme_for(5)
    reads = list(ragged_batch(5))
    full, _ = assemble(ragged_model(5))
    for n in (1, 3):
        want = check_model(gx, ox, reads, scheme, sm, n=n)
        assert len(want) < len(full) and all(sum(r[3] for r in want if r[0] == q) <= n for q in range(len(reads)))
        assert any(sum(r[3] for r in want if r[0] == q) == n and sum(r[3] for r in full if r[0] == q) > n for q in range(len(reads)))
    got, st = run(gx, reads, scheme, sm, n=0)
    assert got == [] and st.lf_steps == 0
    # a capacity that is too small: the total comes back, and a retry with it succeeds
    qbuf, qoff = fm.flatten(reads)
    pi, l, u = (np.ascontiguousarray(x, dtype=np.uint64) for x in scheme)
    sc = capi.Scheme()
    sc.n_searches, sc.n_parts = pi.shape
    sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    m = sm._struct()
    L = capi.lib()
    count = len(full)
    out = np.full((count + 2) * HIT_DTYPE.itemsize, 0xA5, dtype=np.uint8).view(HIT_DTYPE)
    cnt = C.c_uint64()
    for cap in (0, 1, count - 1):
        rc = L.fmgpu_search_hamming_sm(gx._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), C.byref(sc), C.byref(m), UINT64_MAX, capi.ptr(out), cap, C.byref(cnt), None, None)
        assert rc == capi.FMGPU_ERR_CAPACITY and cnt.value == count, cap
        assert (out[cap:].view(np.uint8) == 0xA5).all()
    rc = L.fmgpu_search_hamming_sm(gx._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), C.byref(sc), C.byref(m), UINT64_MAX, capi.ptr(out), int(cnt.value), C.byref(cnt), None, None)
    assert rc == 0 and cnt.value == count and (out[count:].view(np.uint8) == 0xA5).all()
    hits = np.ascontiguousarray(out[:count])
    capi.check(L.fmgpu_hits_sort(capi.ptr(hits), count, None))
    assert records(hits) == full
    small, _ = run(gx, reads, scheme, sm, capacity=1)                  # the retry of the host layer
    assert small == full


# ------------------------------------------------------------------------------------------------ 6. partition and locate
@pytest.mark.parametrize("wide", [0, 1])
def test_partition_and_locate(wide):
    gx, ox = handle("IB16", 5, wide), oracle("IB16", 5)
    seqs = sequences(5)
    sm, scheme = iupac(), scheme_for(5)
    rng = np.random.default_rng(21)
    reads = [degenerate(rng, window(rng, seqs, 5, 24, k % 3, seq=k % 2), 5, 4, k % 2) for k in range(12)] + [window(rng, seqs, 5, 23)]
    uniform = check_model(gx, ox, reads, scheme, sm)
    want = check_model(gx, ox, reads, scheme, sm, partition=[3, 9, 5, 7])
    assert want and not any(r[0] == 12 for r in want) and any(r[0] == 12 for r in uniform)      # a read of another total length is skipped
    hits = fm.search_hamming_sm.search(gx, reads, scheme, sm, partition=[3, 9, 5, 7])
    pos = gx.locate_hits(hits)
    assert pos.size == sum(r[3] for r in want)
    got = {(int(p["qidx"]), int(p["seq_id"]), int(p["pos"]), int(p["errors"])) for p in pos}
    assert got == model.brute(seqs, reads[:12], sm.free_mask, sm.cost_mask, 0, 2) and len(got) >= 12


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors_leave_the_handle_healthy():
    gx = handle("IB16", 5, 0)
    seqs = sequences(5)
    rng = np.random.default_rng(3)
    reads = [window(rng, seqs, 5, 24, k % 3) for k in range(8)]
    scheme = scheme_for(5)
    before = fm.search_ng26.search(gx, reads, scheme)
    good, _ = run(gx, reads, scheme, iupac())
    qbuf, qoff = fm.flatten(reads)
    L = capi.lib()
    out, cnt = np.zeros(64, dtype=HIT_DTYPE), C.c_uint64()

    def scheme_struct(s, edit=0, keep=[]):
        pi, l, u = (np.ascontiguousarray(x, dtype=np.uint64) for x in s)
        keep.append((pi, l, u))
        sc = capi.Scheme()
        sc.n_searches, sc.n_parts = pi.shape
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        sc.edit = edit
        return sc

    def call(h, sc, m, n=UINT64_MAX):
        rc = L.fmgpu_search_hamming_sm(h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), C.byref(sc) if sc is not None else None, C.byref(m) if m is not None else None,
                                       n, capi.ptr(out), 64, C.byref(cnt), None, None)
        return rc, L.fmgpu_last_error().decode()

    ok = scheme_struct(scheme)
    sm = iupac()
    messages = set()

    def bad(rc_msg, code):
        assert rc_msg[0] == code, rc_msg
        assert rc_msg[1] and rc_msg[1] not in messages, rc_msg      # a message of its own
        messages.add(rc_msg[1])

    bad(call(gx._h, scheme_struct(scheme, edit=1), sm._struct()), capi.FMGPU_ERR_INVALID)
    bad(call(gx._h, ok, None), capi.FMGPU_ERR_INVALID)
    m = sm._struct()
    m.free_mask = None
    bad(call(gx._h, ok, m), capi.FMGPU_ERR_INVALID)
    for qs in (0, 257):
        m = sm._struct()
        m.query_sigma = qs
        rc = call(gx._h, ok, m)
        assert rc[0] == capi.FMGPU_ERR_INVALID and "query_sigma" in rc[1]
    high = iupac()
    high.cost_mask[7] |= np.uint32(1 << 5)                            # a text symbol >= sigma
    bad(call(gx._h, ok, high._struct()), capi.FMGPU_ERR_INVALID)
    both = iupac()
    both.cost_mask[6] |= both.free_mask[6]
    bad(call(gx._h, ok, both._struct()), capi.FMGPU_ERR_INVALID)
    # a bad scheme: the codes of fmgpu_search_scheme
    assert call(gx._h, None, sm._struct())[0] == capi.FMGPU_ERR_INVALID
    pi, l, u = scheme
    broken = (pi.copy(), l, u)
    broken[0][0, 0] = broken[0][0, 1]
    rc_sm = call(gx._h, scheme_struct(broken), sm._struct())
    rc_ng = L.fmgpu_search_scheme(gx._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), C.byref(scheme_struct(broken)), UINT64_MAX, capi.ptr(out), 64, C.byref(cnt), None, None)
    assert rc_sm[0] == rc_ng == capi.FMGPU_ERR_INVALID and rc_sm[1] == L.fmgpu_last_error().decode()
    # a unidirectional handle: the code and the message of fmgpu_search_scheme
    uni = fm.FMIndex.from_sequences(seqs, 5, "IB16", 4)
    rc_sm = call(uni._h, ok, sm._struct())
    rc_ng = L.fmgpu_search_scheme(uni._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), C.byref(ok), UINT64_MAX, capi.ptr(out), 64, C.byref(cnt), None, None)
    assert rc_sm[0] == rc_ng == capi.FMGPU_ERR_INVALID and rc_sm[1] == L.fmgpu_last_error().decode()
    # sigma > 32: the masks are one word
    big = fm.BiFMIndex.from_reference_arrays(**oracle_arrays(fo.OraIndex.build("IB16", 40, [rng.integers(1, 40, size=300, dtype=np.uint8)], 2, True)))
    bad(call(big._h, ok, fm.ScoringMatrix(5)._struct()), capi.FMGPU_ERR_UNSUPPORTED)
    # nq == 0 before the handle is looked at; null buffers
    assert L.fmgpu_search_hamming_sm(None, None, None, 0, None, None, 1, None, 0, C.byref(cnt), None, None) == 0 and cnt.value == 0
    assert L.fmgpu_search_hamming_sm(gx._h, None, capi.ptr(qoff), len(reads), C.byref(ok), C.byref(sm._struct()), 1, capi.ptr(out), 64, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    # the handle is healthy, and the existing call answers as before
    again, _ = run(gx, reads, scheme, iupac())
    assert again == good and len(good) >= 8
    after = fm.search_ng26.search(gx, reads, scheme)
    assert after.tobytes() == before.tobytes()
