"""fmgpu_search_hamming_sm without a GPU: the symbol, the masks of the Python ScoringMatrix, the argument checks that need no device, and the oracle of
tests/test_gpu_hamming_sm.py (tests/hamming_sm_model.py): the walk against the brute-force scorer and against the oracle's search_ng26."""
import ctypes as C
import functools

import numpy as np

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests import hamming_sm_model as model


def test_symbol_struct_and_abi_version():
    L = capi.lib()
    assert "fmgpu_search_hamming_sm" in capi.EXPORTS and hasattr(L, "fmgpu_search_hamming_sm")
    assert L.fmgpu_abi_version() == 6
    assert C.sizeof(capi.ScoringMatrix) == 24
    assert [f[0] for f in capi.ScoringMatrix._fields_] == ["query_sigma", "reserved", "free_mask", "cost_mask"]


def test_nq_zero_and_null_handle_without_a_device():
    L = capi.lib()
    cnt = C.c_uint64(99)
    st = capi.Stats()
    st.hits = 5
    # nq == 0 is decided before the handle is looked at
    assert L.fmgpu_search_hamming_sm(None, None, None, 0, None, None, 1, None, 0, C.byref(cnt), C.byref(st), None) == 0 and cnt.value == 0 and st.hits == 0
    assert L.fmgpu_search_hamming_sm(None, None, None, 0, None, None, 1, None, 0, None, None, None) == 0
    qbuf, qoff = np.array([1, 2, 3], dtype=np.uint8), np.array([0, 3], dtype=np.uint64)
    assert L.fmgpu_search_hamming_sm(None, capi.ptr(qbuf), capi.ptr(qoff), 1, None, None, 1, None, 0, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID


def bits(*ranks):
    return sum(1 << r for r in ranks)


def test_default_matrix_masks():
    sm = fm.ScoringMatrix(5)
    assert (sm.query_sigma, sm.ref_sigma) == (5, 5)
    assert sm.free_mask.tolist() == [0, 2, 4, 8, 16]
    assert sm.cost_mask.tolist() == [0, 0b11100, 0b11010, 0b10110, 0b01110]
    assert sm.free_mask.dtype == np.uint32 and sm.cost_mask.dtype == np.uint32
    one = fm.ScoringMatrix(1, 5)                                     # only the delimiter's row, and that pairs with nothing
    assert one.free_mask.tolist() == [0] and one.cost_mask.tolist() == [0]


def test_reference_test_matrix_masks():
    """the seven setCost calls of the reference's test on ScoringMatrix<28, 21>"""
    sm = fm.ScoringMatrix(28, 21)
    extra = {21: 5, 22: 13, 23: 4, 24: 7, 25: 12, 26: 17, 27: 19}
    for q, r in extra.items():
        sm.set_cost(q, r, 0)
    every = bits(*range(1, 21))
    assert sm.free_mask[0] == 0 and sm.cost_mask[0] == 0
    for q in range(1, 21):
        assert sm.free_mask[q] == 1 << q and sm.cost_mask[q] == every & ~(1 << q)
    for q, r in extra.items():
        assert sm.free_mask[q] == 1 << r and sm.cost_mask[q] == every & ~(1 << r)
    assert not (sm.free_mask & sm.cost_mask).any()
    sm.set_cost(21, 5, 1)                                            # and back: a pair sits in one list at a time
    assert sm.free_mask[21] == 0 and sm.cost_mask[21] == every
    sm.set_unpairable(21, 6)
    assert sm.cost_mask[21] == every & ~(1 << 6)
    sm.set_unpairable(22)
    assert sm.free_mask[22] == 0 and sm.cost_mask[22] == 0


def test_iupac_matrix_masks():
    sm = fm.ScoringMatrix.iupac_dna()
    assert (sm.query_sigma, sm.ref_sigma) == (16, 5)
    A, Cy, G, T = 1, 2, 3, 4
    want = [(), (A,), (Cy,), (G,), (T,), (A, G), (Cy, T), (Cy, G), (A, T), (G, T), (A, Cy), (Cy, G, T), (A, G, T), (A, Cy, T), (A, Cy, G), (A, Cy, G, T)]
    assert sm.free_mask.tolist() == [bits(*w) for w in want]
    assert sm.cost_mask.tolist() == [0] + [0b11110 & ~bits(*w) for w in want[1:]]
    assert list(fm.ScoringMatrix.IUPAC) == list("RYSWKMBDHVN")


# ------------------------------------------------------------------------------------------------ the model
@functools.lru_cache(maxsize=None)
def text_case(sigma):
    rng = np.random.default_rng(40 + sigma)
    unit = rng.integers(1, sigma, size=7, dtype=np.uint8)
    seqs = [rng.integers(1, sigma, size=1500, dtype=np.uint8), np.tile(unit, 40), rng.integers(1, sigma, size=60, dtype=np.uint8)]
    return seqs, fo.OraIndex.build("IB16", sigma, seqs, 2, True)


def windows(rng, seqs, sigma, count, lengths, max_subs):
    reads = []
    for k in range(count):
        s = seqs[k % 2]
        m = int(lengths[k % len(lengths)])
        at = int(rng.integers(0, len(s) - m + 1))
        r = s[at: at + m].copy()
        for _ in range(k % (max_subs + 1)):
            p = int(rng.integers(0, m))
            r[p] = (int(r[p]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1
        reads.append(r)
    return reads


def test_model_is_the_brute_force_on_an_iupac_batch():
    seqs, ox = text_case(5)
    sm = fm.ScoringMatrix.iupac_dna()
    rng = np.random.default_rng(5)
    reads = windows(rng, seqs, 5, 16, (20, 21, 22, 23, 24), 2)
    code_of = {frozenset(b): 5 + k for k, b in enumerate(fm.ScoringMatrix.IUPAC.values())}
    for r in reads:
        for p in rng.choice(len(r), size=4, replace=False):          # four degenerate positions that still hold the base ...
            base = "ACGT"[int(r[p]) - 1]
            r[p] = int(rng.choice([c for b, c in code_of.items() if base in b]))
        for p in rng.choice(len(r), size=int(rng.integers(0, 3)), replace=False):     # ... and up to two arbitrary codes
            r[p] = int(rng.integers(1, 16))
    scheme = fo.scheme_h2(4, 0, 2)
    recs, steps = model.walk(ox, reads, scheme, sm.free_mask, sm.cost_mask)
    got = model.located(ox, recs)
    assert got == model.brute(seqs, reads, sm.free_mask, sm.cost_mask, 0, 2)
    assert len(got) > len(reads) and steps > 0
    assert any(e == 2 for _, _, _, e in got) and any(ln > 1 for _, _, _, ln, _, _ in recs)
    # seq numbers the reports of a read from 0
    for q in range(len(reads)):
        assert [r[5] for r in recs if r[0] == q] == list(range(sum(1 for r in recs if r[0] == q)))


def test_model_with_the_identity_matrix_is_search_ng26():
    for sigma, scheme, m in ((5, fo.scheme_h2(4, 0, 2), 24), (5, fo.scheme_pigeon_opt(0, 1), 23), (21, fo.scheme_pigeon_opt(0, 1), 16), (5, fo.scheme_h2(5, 1, 3), 30)):
        seqs, ox = text_case(sigma)
        sm = fm.ScoringMatrix(sigma)
        reads = windows(np.random.default_rng(sigma + m), seqs, sigma, 10, (m,), 2)
        recs, _ = model.walk(ox, reads, scheme, sm.free_mask, sm.cost_mask)
        qbuf, qoff = fo.flatten_queries(reads)
        hits, _, _ = ox.search_ng26(qbuf, qoff, scheme, edit=False)
        want = sorted((int(h["qidx"]), int(h["lb"]), int(h["lb_rev"]), int(h["len"]), int(h["errors"])) for h in hits)
        assert sorted(r[:5] for r in recs) == want and len(want) >= 5


def test_model_clipping_is_search_n():
    """SearchNg26.h:412-420: the cursor that crosses n is cut to what is left, and the delegate's `true` ends the read's searches"""
    seqs, ox = text_case(5)
    sm = fm.ScoringMatrix.iupac_dna()
    scheme = fo.scheme_h2(4, 0, 2)
    read = seqs[1][3: 3 + 10].copy()                                  # inside the tandem repeat, with two N: several records, one of them a cursor of many rows
    read[2] = read[8] = 15
    full, _ = model.walk_read(ox, read, scheme, sm.free_mask, sm.cost_mask)
    big = max(range(len(full)), key=lambda i: full[i][2])
    assert len(full) >= 5 and 0 < big < len(full) - 1 and full[big][2] > 3
    before, total = sum(r[2] for r in full[:big]), sum(r[2] for r in full)
    for n in (1, 2, before, before + 1, before + full[big][2] - 1, before + full[big][2], total - 1, total, total + 5):
        got, _ = model.walk_read(ox, read, scheme, sm.free_mask, sm.cost_mask, n=n)
        want, ct = [], 0
        for lb, lr, ln, e in full:
            if ln + ct > n:
                ln = n - ct
            ct += ln
            want.append((lb, lr, ln, e))
            if ct == n:
                break
        assert got == want and sum(r[2] for r in got) == min(n, total)
    assert model.walk_read(ox, read, scheme, sm.free_mask, sm.cost_mask, n=0) == ([], 0)
    # a read shorter than the scheme has parts, and a partition that does not cover the read, produce nothing
    assert model.walk_read(ox, read[:3], scheme, sm.free_mask, sm.cost_mask) == ([], 0)
    assert model.walk_read(ox, read, scheme, sm.free_mask, sm.cost_mask, partition=[3, 3, 3, 3]) == ([], 0)
    assert model.walk_read(ox, read, scheme, sm.free_mask, sm.cost_mask, partition=[2, 3, 1, 4])[0]
