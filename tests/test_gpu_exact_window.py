"""k_exact_p with the read held in registers (QueryWindow) and the odd symbol of a read taken first, from C: intervals, miss rows and step counts
equal the oracle's one-symbol search — reads of every length from 1 to 300 (more than one window: the refill), ragged waves, delimiters and foreign
bytes at the first, middle and last position, substitutions that empty a pair, the interval table in front of the pair table, and 64-bit rows."""
import contextlib

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests.util import oracle_arrays

pytestmark = pytest.mark.gpu


def build(ox, wide, pairs=True):
    cls = fm.BiFMIndex if ox.bidirectional else fm.FMIndex
    opts = {}
    if wide:
        opts["force_wide"] = 1
    if not pairs:
        opts["pair_table"] = "0"
    with fm.options(**opts) if opts else contextlib.nullcontext():
        gx = cls.from_reference_arrays(**oracle_arrays(ox))
    assert gx.row_bits == (64 if wide else 32)
    return gx


def texts(kind):
    rng = np.random.default_rng(91)
    if kind == "uniform":
        base = rng.integers(1, 5, size=4000, dtype=np.uint8)
        # a few copies with sparse substitutions: long reads still match, and a substitution empties a pair deep into a read
        seqs = [base]
        for k in range(3):
            c = base.copy()
            c[rng.integers(0, len(c), size=20)] = rng.integers(1, 5, size=20)
            seqs.append(c)
        return seqs + [rng.integers(1, 5, size=int(rng.integers(1, 400)), dtype=np.uint8) for _ in range(20)]
    # no symbol 4 anywhere: an odd read that ends in 4 is empty after its first step ([C[4], C[5]) is empty)
    return [rng.integers(1, 4, size=int(rng.integers(300, 1500)), dtype=np.uint8) for _ in range(6)]


def reads_for(seqs, seed):
    rng = np.random.default_rng(seed)
    long_seqs = [s for s in seqs if len(s) >= 300]
    out = []
    for m in range(1, 301):                                   # every length, as a substring of the text and with substitutions
        s = long_seqs[int(rng.integers(0, len(long_seqs)))]
        p = int(rng.integers(0, len(s) - m + 1))
        q = s[p: p + m].copy()
        out.append(q.copy())
        for subs in (1, 2):
            r = q.copy()
            for _ in range(subs):
                r[int(rng.integers(0, m))] = int(rng.integers(1, 5))
            out.append(r)
        # a delimiter at the first, the middle and the last position
        for at in {0, m // 2, m - 1}:
            r = q.copy(); r[at] = 0; out.append(r)
    out += [np.array(x, dtype=np.uint8) for x in ([], [1], [4], [1, 4], [4, 4, 4], [0], [0, 1], [1, 0], [0, 1, 1], [1, 1, 0], [4] * 127, [4] * 128, [4] * 129)]
    # what follows a delimiter / crosses from one sequence into the next
    for s in seqs[:10]:
        out += [np.concatenate([s[-5:], [0], s[:4]]).astype(np.uint8), np.concatenate([[0], s[:7]]).astype(np.uint8)]
    order = rng.permutation(len(out))                          # ragged waves: short and long reads side by side in one wave
    return [out[i] for i in order]


def foreign_reads(seqs, seed):
    rng = np.random.default_rng(seed)
    s = max(seqs, key=len)
    out = []
    for m in (1, 2, 3, 8, 15, 16, 17, 64, 101, 127, 128, 129, 200, 255, 256, 257, 300):
        p = int(rng.integers(0, len(s) - m + 1))
        q = s[p: p + m].copy()
        for at in sorted({0, m // 2, m - 1}):
            for byte in (5, 9, 200, 255):
                r = q.copy(); r[at] = byte; out.append(r)
    return [out[i] for i in rng.permutation(len(out))]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("kind", ["uniform", "no_symbol_4"])
def test_pair_search_with_register_window(kind, wide):
    seqs = texts(kind)
    ox = fo.OraIndex.build("IB16", 5, seqs, 4, False)
    gx, gx_single = build(ox, wide), build(ox, wide, pairs=False)
    assert gx.device_bytes > gx_single.device_bytes          # the pair table is there: k_exact_p runs
    qbuf, qoff = fm.flatten(reads_for(seqs, 5))
    olb, oln, ost = ox.search_exact(qbuf, qoff, want_steps=True)
    lb, ln, st = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
    assert np.array_equal(ln, oln) and np.array_equal(lb, olb)
    assert st.lf_steps == int(ost.sum())
    assert (oln > 0).sum() > len(oln) // 10 and (olb[oln == 0] > 0).any()    # (hits, and misses that end on a row)
    # one read per batch: a wave of one lane, every length
    for i in range(0, len(qoff) - 1, 37):
        if qoff[i + 1] == qoff[i]:
            continue
        one = (qbuf[qoff[i]: qoff[i + 1]], np.array([0, qoff[i + 1] - qoff[i]], dtype=np.uint64))
        a, b, s1 = fm.search_no_errors.search(gx, one, want_stats=True)
        assert (a[0], b[0], s1.lf_steps) == (olb[i], oln[i], int(ost[i]))
    # bytes outside the alphabet (an empty interval here, undefined in the reference): the one-symbol kernel's rows and steps
    fq = fm.flatten(foreign_reads(seqs, 6))
    a = fm.search_no_errors.search(gx, fq, want_stats=True)
    b = fm.search_no_errors.search(gx_single, fq, want_stats=True)
    assert not a[1].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].lf_steps == b[2].lf_steps
    # the interval table in front of the pair table (up to 16 symbols of the window: lut lengths past the first word)
    for lut_len in (1, 7, 10):
        gx.accelerate(1, lut_len=lut_len, walk=0)
        assert bool(gx.formats & capi.FMT_INTERVALS)
        lb, ln, st = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
        assert np.array_equal(ln, oln) and np.array_equal(lb, olb) and st.lf_steps == int(ost.sum()), lut_len
        assert st.table_steps > 0
        c = fm.search_no_errors.search(gx, fq, want_stats=True)
        assert not c[1].any() and np.array_equal(c[0], b[0]) and c[2].lf_steps == b[2].lf_steps, lut_len
    gx.accelerate(1, lut_len=0, walk=0)


def test_pair_search_reads_at_every_alignment():
    """the window's 16-byte loads stay inside each read's own chunks: a batch whose reads start at every offset mod 16, with a byte buffer that
    itself starts at every offset of a device allocation"""
    torch = pytest.importorskip("torch")
    seqs = texts("uniform")
    ox = fo.OraIndex.build("IB16", 5, seqs, 4, False)
    gx = build(ox, False)
    rng = np.random.default_rng(8)
    s = seqs[0]
    reads = []
    for m in list(range(1, 40)) + [101, 127, 128, 129, 150]:
        p = int(rng.integers(0, len(s) - m + 1))
        reads.append(s[p: p + m].copy())
    qbuf, qoff = fm.flatten(reads)
    olb, oln, ost = ox.search_exact(qbuf, qoff, want_steps=True)
    for shift in range(16):
        dev = torch.zeros(len(qbuf) + 32, dtype=torch.uint8, device="cuda")
        dev[shift: shift + len(qbuf)] = torch.from_numpy(qbuf).to("cuda")
        torch.cuda.synchronize()
        lb, ln, st = fm.search_no_errors.search(gx, (dev.data_ptr() + shift, qoff), want_stats=True)     # (a device pointer: read in place)
        assert np.array_equal(ln, oln) and np.array_equal(lb, olb) and st.lf_steps == int(ost.sum()), shift
