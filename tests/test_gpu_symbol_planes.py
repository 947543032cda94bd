"""The symbol-plane table (Format S, k_exact_s) of the shipped library beyond its first super-block.  A line's sigma counts are B = flat_count_bits(sigma) bits wide
and relative to a super-block of 2^B rows: B = 24 at sigma = 29, 25 at sigma = 28 — 2^24 and 2^25 rows, which a device build reaches in a second.  The tests that compare
intervals with the oracle hold 10^4 .. 10^5 rows: one super-block, counts below 2^17.  Here the index has 1.7 x 10^7 .. 5 x 10^7 rows, so that

  * `row >> B` takes the values 0 and 1 in the builder (k_flat_counts, k_flat_super) and in the search (both interval ends, one or two super entries per step),
  * n = P - 1, P, P + 1 (P = 2^B) put the row `lb + len == n` before, on and behind the boundary (n = P: the last super-block is empty),
  * a text in which one symbol has 90 % of the positions sets the top bit of that symbol's field inside the first super-block, for a field at bit 0 of its word, for
    the last field and for one that straddles two 32-bit words.

The oracle's suffix sorter is too slow at this size.  The reference is a backward search in numpy on the BWT the device builder hands back (pinned against the oracle
by tests/test_gpu_bigbuild.py and tests/test_gpu_parity.py; its code knows nothing of Format S): LF(i, c) = #{keys < c n + i} over the sorted keys bwt[j] n + j — one
stable argsort and one searchsorted per step and interval end, all in int64.  The conditions on the reads are asserted on that reference before the device is asked, per
boundary k P inside the index: at least 5 intervals straddle it (lb < k P < lb + len), at least 100 have an end within 64 rows of it, at least 100 are single rows
beyond it, at least a quarter of the reads cut from the text end in super-block 1.

Times on an MI355X are printed per test (pytest -s) and listed in the docstring of test_beyond_the_first_super_block."""
import time

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi

pytestmark = pytest.mark.gpu

COUNT_BITS = {29: 24, 28: 25}             # flat_count_bits(sigma) of the shipped library (fmgpu_common.h): min(28, 704 / sigma)
SLEN_CUT = 30                             # symbols of a read cut from the text
WINDOW = 64                               # rows on either side of a boundary that the aimed reads stand on
DEPTH = 12                                # the aimed reads: every depth up to this one ...
AIM_DEPTHS = tuple(range(1, DEPTH + 1)) + (16, 24, 32, 48, 64, 96, 128, 192)      # ... and these


def straddling_symbol(sigma):
    """the first symbol above 1 whose count field lies in two 32-bit words"""
    B = COUNT_BITS[sigma]
    return next(d for d in range(2, sigma - 1) if (d * B) % 32 + B > 32)


class V:
    """a device tensor as the buffer object the host layer takes"""
    def __init__(self, t): self.t, self.ptr, self.nbytes = t, t.data_ptr(), t.numel() * t.element_size()


def make_text(torch, sigma, nseq, slen, dominant, seed):
    """nseq sequences of slen symbols over 1 .. sigma - 1, generated on the device.
    dominant = 0: every symbol equally frequent; half of the positions (chosen at random) hold the successor of the symbol before them (x -> x % (sigma - 1) + 1), the other
    half a random symbol — neighbouring rows of the index then share about 13 symbols instead of 5 (log_28 n), so that a dozen intervals of growing depth hold both rows
    beside a boundary, and a text position is still unique after 30 symbols.
    dominant = d: symbol d at 90 % of the positions, placed at random (no runs beyond chance), the others uniform over the rest."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(seed)
    total = nseq * slen
    if dominant:
        other = torch.randint(1, sigma - 1, (total,), generator=g, device=dev, dtype=torch.uint8)
        other += (other >= dominant).to(torch.uint8)               # 1 .. sigma - 1 without d
        text = torch.where(torch.rand(total, generator=g, device=dev) < 0.9, torch.full_like(other, dominant), other)
    else:
        fresh = torch.randint(0, sigma - 1, (total,), generator=g, device=dev, dtype=torch.int64)
        keep = torch.rand(total, generator=g, device=dev) < 0.5     # positions that hold a fresh symbol; the others continue the chain
        keep[0] = True
        at = torch.arange(total, device=dev, dtype=torch.int64)
        last = torch.cummax(torch.where(keep, at, torch.zeros_like(at)), 0).values      # the last fresh position at or before each position
        text = ((fresh[last] + (at - last)) % (sigma - 1) + 1).to(torch.uint8)
    # two sequences begin with eight times the largest symbol: the two last rows of the index share those eight symbols, so that with n = P + 1 rows, where P - 1 and P are
    # the last two, their common prefixes are intervals that straddle the boundary
    for at, then in ((0, 1), (5 * slen, 2)):
        text[at: at + 8] = sigma - 1
        text[at + 8] = then
    seq_off = torch.arange(nseq + 1, device=dev, dtype=torch.int64) * slen
    return text, seq_off


class Reference:
    """backward search on a BWT in numpy integers"""
    def __init__(self, bwt, sigma):
        self.n, self.sigma = len(bwt), sigma
        order = np.argsort(bwt, kind="stable").astype(np.int64)
        self.order = order
        self.keys = bwt[order].astype(np.int64) * self.n + order    # ascending: (symbol, row)
        self.C = np.concatenate([[0], np.cumsum(np.bincount(bwt, minlength=sigma).astype(np.int64))])

    def lf(self, c, rows):
        """C[c] + #{j < row : bwt[j] == c}"""
        return np.searchsorted(self.keys, np.asarray(c, dtype=np.int64) * self.n + np.asarray(rows, dtype=np.int64), side="left").astype(np.int64)

    def search(self, qbuf, qoff):
        """(lb, len, steps) per read: from (0, n), last symbol first, until the interval is empty; a byte outside the alphabet empties it to (0, 0)"""
        qoff = qoff.astype(np.int64)
        nq = len(qoff) - 1
        m = qoff[1:] - qoff[:-1]
        lb, ln, steps = np.zeros(nq, dtype=np.int64), np.full(nq, self.n, dtype=np.int64), np.zeros(nq, dtype=np.int64)
        alive = m > 0
        for t in range(int(m.max()) if nq else 0):
            idx = np.nonzero(alive & (m > t))[0]
            if not len(idx):
                break
            c = qbuf[qoff[1:][idx] - 1 - t].astype(np.int64)
            steps[idx] += 1
            ok = c < self.sigma
            bad = idx[~ok]
            lb[bad], ln[bad], alive[bad] = 0, 0, False
            idx, c = idx[ok], c[ok]
            a, b = self.lf(c, lb[idx]), self.lf(c, lb[idx] + ln[idx])
            lb[idx], ln[idx] = a, b - a
            alive[idx[b == a]] = False
        alive[:] = False
        return lb, ln, steps

    def aimed(self, row):
        """every read of depth 1 .. DEPTH (and of a few larger depths) whose interval meets rows [row - WINDOW, row + WINDOW].  The intervals of one depth partition the
        rows (LF is a permutation, the delimiter taken as a symbol), and the read of depth L that holds row r is the first L symbols of r's suffix: F[r], F[psi(r)], ...
        with psi = the inverse of LF = the stable order of the BWT.  (Growing the kept reads by a symbol in FRONT, and keeping those that still meet the window, loses
        them: a symbol in front sends a read's interval elsewhere in the table; one more symbol BEHIND splits it among its children.)  So every depth has exactly one
        read that holds `row`.  The larger depths are for texts whose neighbouring rows share more than DEPTH symbols (the skewed ones: about 80)"""
        rows = np.arange(max(0, row - WINDOW), min(row + WINDOW, self.n - 1) + 1, dtype=np.int64)
        spell = np.zeros((len(rows), AIM_DEPTHS[-1]), dtype=np.uint8)
        r = rows.copy()
        for t in range(AIM_DEPTHS[-1]):
            spell[:, t] = np.searchsorted(self.C, r, side="right") - 1        # F[r]: the symbol whose rows of the first column hold r
            r = self.order[r]
        out = []
        for depth in AIM_DEPTHS:
            out += list(np.unique(spell[:, :depth], axis=0))
        return out


def all_short_reads(sigma):
    """every string of 1, 2 and 3 symbols over 1 .. sigma - 1"""
    s = np.arange(1, sigma, dtype=np.uint8)
    a, b, c = np.meshgrid(s, s, s, indexing="ij")
    return [s[:, None], np.stack([a[..., 0].ravel(), b[..., 0].ravel()], axis=1), np.stack([a.ravel(), b.ravel(), c.ravel()], axis=1)]


def cut_reads(flat, nseq, slen, sigma, rng):
    """2 000 reads of 30 symbols from random places of the sequences, every tenth with one substitution; then a few with a delimiter, the byte sigma and 255, the
    empty read and reads of one symbol"""
    starts = rng.integers(0, nseq, size=2000) * slen + rng.integers(0, slen - SLEN_CUT + 1, size=2000)
    reads = flat[starts[:, None] + np.arange(SLEN_CUT)[None, :]].copy()
    for k in range(0, 2000, 10):
        j = int(rng.integers(0, SLEN_CUT))
        reads[k, j] = (int(reads[k, j]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1
    odd = []
    for k, byte in enumerate((0, sigma, 255, 0, sigma, 255)):
        q = reads[20 * k + 1].copy(); q[int(rng.integers(0, SLEN_CUT))] = byte; odd.append(q)
    odd += [np.zeros(0, dtype=np.uint8), np.array([1], dtype=np.uint8), np.array([sigma - 1], dtype=np.uint8), np.array([0], dtype=np.uint8), np.array([sigma], dtype=np.uint8)]
    return reads, starts, odd


# (sigma, n as nseq x (slen + 1), dominant symbol: 0 = none, "first", "last", "straddling"; row widths)
P29, P28 = 1 << 24, 1 << 25
CASES = [
    pytest.param(29, 65_793, 254, 0, (0, 1), id="sigma29-P-1"),             # 65 793 x 255 = 2^24 - 1
    pytest.param(29, 65_536, 255, 0, (0, 1), id="sigma29-P"),               # 65 536 x 256 = 2^24: row n opens the second, empty super-block
    pytest.param(29, 65_281, 256, 0, (0, 1), id="sigma29-P+1"),             # 65 281 x 257 = 2^24 + 1
    pytest.param(29, 100_261, 250, 0, (0, 1), id="sigma29-1.5P"),           # 100 261 x 251 = 25 165 511 rows
    pytest.param(28, 200_524, 250, 0, (0,), id="sigma28-1.5P"),             # 200 524 x 251 = 50 331 524 rows
    pytest.param(29, 100_261, 250, "first", (0,), id="sigma29-skewed-first"),
    pytest.param(29, 100_261, 250, "last", (0,), id="sigma29-skewed-last"),
    pytest.param(29, 100_261, 250, "straddling", (0, 1), id="sigma29-skewed-straddling"),
    pytest.param(28, 200_524, 250, "first", (0,), id="sigma28-skewed-first"),
    pytest.param(28, 200_524, 250, "last", (0,), id="sigma28-skewed-last"),
    pytest.param(28, 200_524, 250, "straddling", (0,), id="sigma28-skewed-straddling"),
]


def test_the_case_sizes_are_what_they_claim():
    """the three sizes around P are exactly P - 1, P, P + 1; the others hold one boundary and half a super-block behind it; the dominant symbols' fields lie
    where the test says"""
    sizes = [(p.values[0], p.values[1] * (p.values[2] + 1)) for p in CASES]
    assert [n for _, n in sizes[:3]] == [P29 - 1, P29, P29 + 1]
    for sigma, n in sizes[3:]:
        P = 1 << COUNT_BITS[sigma]
        assert P + P // 4 < n < 2 * P and n % P and n % 64
    for sigma, B in COUNT_BITS.items():
        assert B == min(28, 704 // sigma)
        d = straddling_symbol(sigma)
        assert (d * B) % 32 + B > 32 and ((sigma - 1) * B) % 32 + B <= 32


@pytest.mark.parametrize("sigma,nseq,slen,skew,widths", CASES)
def test_beyond_the_first_super_block(sigma, nseq, slen, skew, widths):
    """Exact search on an index of n = nseq (slen + 1) rows built on the device (Wavelet): lb, len and the step count of every read equal the numpy reference's, through
    k_exact_s, through the tree (k_exact_m), with an interval table in front and with that table switched off by selection; the handle is larger than one made with
    symbol_planes = 0 by exactly the table's lines and super entries; 1 000 single-row reads, located, spell themselves in the text.

    Measured on an MI355X, per case, all of it (text, two builds per row width, reference, reads, four searches per row width, locate): 0.56 .. 0.80 s at sigma = 29
    (1.7 x 10^7 and 2.5 x 10^7 rows, uniform and skewed, one or two row widths), 0.85 .. 1.20 s at sigma = 28 (5.0 x 10^7 rows); 2.9 s for the case that runs first and
    initialises the device.  A device build took 0.01 .. 0.06 s, skewed texts included; the numpy reference (argsort and keys) 0.16 .. 0.55 s.  No case had to shrink.

    Bounds that a case cannot meet by construction (the others hold as the module states them):
      n = P - 1: every row and every interval end lies in super-block 0 — no boundary inside, none of the four bounds applies; the case pins the largest count of the
                 first super-block and the row lb + len = n = P - 1.
      n = P:     the boundary is row n itself: intervals end ON it (lb + len = n) and none reaches beyond — "straddle" and "single rows beyond" and "cut reads in sb >= 1"
                 cannot hold; at least 100 interval ends within 64 rows of it is asserted.
      n = P + 1: one row lies beyond the boundary: "100 single rows beyond" and "a quarter of the cut reads in sb >= 1" cannot hold; the straddling intervals are the
                 common prefixes of the last two rows (>= 5 asserted, as everywhere), and at least 100 ends within 64 rows."""
    torch = pytest.importorskip("torch")
    B = COUNT_BITS[sigma]
    P = 1 << B
    n = nseq * (slen + 1)
    d = {0: 0, "first": 1, "last": sigma - 1, "straddling": straddling_symbol(sigma)}[skew]
    t0 = time.perf_counter()
    text, seq_off = make_text(torch, sigma, nseq, slen, d, seed=1000 * sigma + d)
    flat = text.cpu().numpy()
    times = {}
    ref = reads = None
    for wide in widths:
        where = (sigma, n, skew, "64-bit rows" if wide else "32-bit rows")
        t1 = time.perf_counter()
        with fm.options(force_wide=wide):
            gx = fm.FMIndex.from_sequences((V(text), V(seq_off)), sigma, "WAVELET", 16, keep_host=True)
            torch.cuda.synchronize()
            times["build%d" % wide] = time.perf_counter() - t1
            with fm.options(symbol_planes=0):
                tree = fm.FMIndex.from_sequences((V(text), V(seq_off)), sigma, "WAVELET", 16)
        assert gx.n == n and gx.row_bits == (64 if wide else 32), where
        # Format S was built, with a super entry per symbol and super-block — the last one empty where n is a multiple of P
        assert gx.formats & capi.FMT_PLANES and not tree.formats & capi.FMT_PLANES, where
        assert gx.device_bytes - tree.device_bytes == (n // 64 + 1) * 128 + ((n >> B) + 1) * sigma * (8 if wide else 4), where
        tree.close()
        if ref is None:                                              # the reference and the reads: once per text (the BWT does not depend on the row width)
            t1 = time.perf_counter()
            bwt = gx.built_array(0)
            assert len(bwt) == n and int(bwt.max()) < sigma
            ref = Reference(bwt, sigma)
            assert np.array_equal(gx.built_array(2, np.uint64).astype(np.int64), ref.C), where
            times["reference"] = time.perf_counter() - t1
            t1 = time.perf_counter()
            rng = np.random.default_rng(sigma * 100 + d)
            cut, starts, odd = cut_reads(flat, nseq, slen, sigma, rng)
            boundaries = [k * P for k in range(1, n // P + 1)]       # (n = P: the boundary is row n)
            aimed = [q for b in sorted(set(boundaries + [n])) for q in ref.aimed(b)]     # (and at the last rows: lb + len = n)
            reads = [q for block in all_short_reads(sigma) for q in block] + aimed + list(cut) + odd
            first_cut = len(reads) - len(odd) - len(cut)
            qbuf, qoff = fm.flatten(reads)
            wlb, wln, wst = ref.search(qbuf, qoff)
            times["reads"] = time.perf_counter() - t1
            # ---- what the batch reaches, on the reference alone
            clb, cln = wlb[first_cut: first_cut + len(cut)], wln[first_cut: first_cut + len(cut)]
            assert int((cln[np.arange(len(cut)) % 10 != 0] >= 1).all()), "a read cut from the text is not found by the reference"
            for b in boundaries:
                straddle = int(((wlb < b) & (b < wlb + wln)).sum())
                beside = int(((wln > 0) & ((np.abs(wlb - b) <= WINDOW) | (np.abs(wlb + wln - b) <= WINDOW))).sum())
                beyond = int(((wln == 1) & (wlb >= b)).sum())
                cut_beyond = int((clb >> B >= 1).sum())
                print("sigma %d n %d (%s), boundary %d: %d reads; %d intervals straddle it, %d end within %d rows, %d single rows beyond, %d of %d cut reads end in sb >= 1"
                      % (sigma, n, skew or "uniform", b, len(reads), straddle, beside, WINDOW, beyond, cut_beyond, len(cut)))
                assert beside >= 100, where
                if b < n:
                    assert straddle >= 5, where
                if n - b > 1:
                    assert beyond >= 100 and 4 * cut_beyond >= len(cut), where
            if n == P - 1:
                assert not boundaries and int((wlb + wln).max()) == n
            if n == P:
                assert int(((wln > 0) & (wlb + wln == n)).sum()) >= DEPTH, "intervals that end on row n = P"
            if d:                                                    # the dominant symbol's field has its top bit set before the first super-block ends
                top = int(ref.lf(d, min(n, P) // 64 * 64 - 64) - ref.lf(d, 0))
                print("symbol %d: %d rows before the last line of super-block 0 (2^%d = %d), field at bit %d of its word" % (d, top, B - 1, 1 << (B - 1), (d * B) % 32))
                assert top >= 1 << (B - 1), where
            want = (wlb.astype(np.uint64), wln.astype(np.uint64), int(wst.sum()))
        # ---- the device
        t1 = time.perf_counter()

        def check(path):
            lb, ln, st = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
            bad = np.nonzero((lb != want[0]) | (ln != want[1]))[0]
            assert not len(bad), (where, path, "%d reads differ" % len(bad), [(reads[k].tolist(), int(lb[k]), int(ln[k]), int(want[0][k]), int(want[1][k])) for k in bad[:4]])
            assert st.lf_steps == want[2], (where, path, st.lf_steps, want[2])
            return st
        for name, sel in (("k_exact_s", 0), ("k_exact_m", capi.SEL_EXACT_ON_TREE)):
            with fm.options(kernel_select=sel):
                check(name)
        gx.accelerate(0, lut_len=2, walk=0)
        assert gx.formats & capi.FMT_INTERVALS
        for name, sel in (("interval table + k_exact_s", 0), ("interval table switched off", capi.SEL_NO_EXACT_LUT)):
            with fm.options(kernel_select=sel):
                st = check(name)
            assert (st.table_steps > 0) == (sel == 0), (where, name)
        gx.accelerate(0, lut_len=0, walk=0)
        # ---- independent of the BWT: single-row reads, located, spell themselves in the text
        one = np.nonzero(cln == 1)[0][:1000]
        assert len(one) == 1000
        seq, pos, steps = gx.locate(clb[one].astype(np.uint64))
        at = seq.astype(np.int64) * slen + pos.astype(np.int64) + steps.astype(np.int64)
        assert np.array_equal(flat[at[:, None] + np.arange(SLEN_CUT)[None, :]], cut[one]), (where, "located reads")
        times["device%d" % wide] = time.perf_counter() - t1
        gx.close()
    times["all"] = time.perf_counter() - t0
    print("sigma %d n %d (%s): " % (sigma, n, skew or "uniform") + ", ".join("%s %.2f s" % kv for kv in times.items()))
