"""The two kernels that sit directly on the occurrence tables: fmgpu_cursor_extend with a symbol per cursor (extendLeft(c) / extendRight(c), the only search-side
reader of prefix_rank(b, c) - prefix_rank(a, c)) and fmgpu_search_exact_depth — on every layout, in both row widths, on FMIndex and BiFMIndex handles.

One collection per alphabet (sigma = 5, 28, 255): two sequences of 900 and 437 symbols, 1 339 rows — five 256-row super-blocks of the 8-bit layouts, 21 blocks, the
last one partly filled.  The expected values come from an IB16 oracle index, once per (sigma, bidirectional); the answers depend neither on layout nor on row width.

  walk      300 walkers seeded from text positions (and the root, two empty cursors and the last row) take 12 single-symbol steps, left or right; the oracle drives, so
            every round is an independent comparison of lb, lb_rev and len.  Beside the oracle stands the plain count: where the pattern holds no delimiter the new
            len is the number of windows of the text that equal it (test_the_oracle_walk_counts_windows checks the oracle against it without a device).
  chain     the device fed with its own outputs ends at the oracle's final cursors.
  forms     extend(.., None)[i, c] == extend(.., symb = c)[i]; stepping a read's symbols from the root reproduces search_no_errors.search.
  guard     cursors outside the index and symbols outside the alphabet give {0, 0, 0} beside untouched neighbours; argument errors; device buffers on a stream.
  depth     fmgpu_search_exact_depth against tests/cursor_model.depth_model, also from the native readers (expand_dna = 0) and on an index of one row.
  creation  a BiFMIndex whose two strings differ in layout is refused."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests.cursor_model import depth_model
from tests.util import make_text, sample_reads, occurrences, oracle_arrays
from tests.test_gpu_parity import LAYOUTS
from tests.test_gpu_superblocks import family
from tests.golden.make_golden import super_period

gpu = pytest.mark.gpu

SIGMAS = (5, 28, 255)
N_ROWS = 900 + 437 + 2
WALKERS, ROUNDS = 300, 12
NONE = 2 ** 64 - 1


# ------------------------------------------------------------------------------------------------ inputs and expectations (no device)
@functools.lru_cache(maxsize=None)
def collection(sigma):
    """the sequences, the IB16 oracle index (rate 4, bidirectional), what OraIndex.from_bwt needs for another layout, and the text with its delimiters"""
    seqs = [make_text(900, sigma, seed=3), make_text(437, sigma, seed=4)]
    ox = fo.OraIndex.build("IB16", sigma, seqs, 4, True)
    n = ox.n
    assert n == N_ROWS
    for p in {super_period(l, sigma) for l in LAYOUTS} - {None}:
        assert n % p, "the reference's first search step is wrong where n is a multiple of a super-block period"
    fw, rv = ox.bwt_string(), ox.bwt_string(rev=True)
    bwt = np.fromiter((fw.symbol(i) for i in range(n)), dtype=np.uint8, count=n)
    bwt_rev = np.fromiter((rv.symbol(i) for i in range(n)), dtype=np.uint8, count=n)
    has, seq, pos = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for i in range(n):
        v = ox.single_locate_step(i)
        if v is not None:
            has[i], seq[i], pos[i] = 1, v[0], v[1]
    text = np.concatenate([seqs[0], [0], seqs[1], [0]]).astype(np.uint8)
    return seqs, ox, (bwt, bwt_rev, has, seq, pos), text


@functools.lru_cache(maxsize=None)
def layout_oracle(layout, sigma, bidir):
    _, ox, (bwt, bwt_rev, has, seq, pos), _ = collection(sigma)
    return ox if layout == "IB16" and bidir else fo.OraIndex.from_bwt(layout, sigma, bwt, bwt_rev if bidir else None, has, seq, pos)


def handle(layout, sigma, bidir, wide, **opts):
    with fm.options(force_wide=wide, **opts):
        gx = (fm.BiFMIndex if bidir else fm.FMIndex).from_reference_arrays(**oracle_arrays(layout_oracle(layout, sigma, bidir)))
    assert gx.row_bits == (64 if wide else 32) and gx.n == N_ROWS and gx.bidirectional == bidir
    return gx


@functools.lru_cache(maxsize=None)
def seeds(sigma):
    """the walkers' seed reads, of lengths 1 to 40 (200 from the first sequence, 100 from the second), and where each one stands in the text: its anchor occurrence"""
    seqs, _, _, text = collection(sigma)
    reads, starts = [], []
    for s, count in ((0, 200), (1, 100)):
        for r in sample_reads(seqs[s], count, 40, seed=11 + s + sigma):
            starts.append(int(occurrences(text, r)[0][0]))
            reads.append(r[: 1 + len(reads) % 40].copy())
    assert len(reads) == WALKERS
    return reads, starts


def searched(ox, read):
    """the oracle's cursor of a read, stepped leftwards from the root through every symbol (the cursor may end empty)"""
    cur = ox.cursor()
    for c in read[::-1]:
        cur = ox.extend_left(cur, int(c))
    return cur


@functools.lru_cache(maxsize=None)
def walk(sigma, bidir):
    """ROUNDS rounds of (right[w], symb[w], inp[w], out[w], plain[w]): the oracle's cursors before and after the step of every walker, and the number of windows of
    the text equal to the walker's new pattern (-1: the pattern holds a delimiter, or the walker is a cursor without a pattern)"""
    ox = layout_oracle("IB16", sigma, bidir)
    n = ox.n
    text = collection(sigma)[3]
    rng = np.random.default_rng(7000 + 2 * sigma + bidir)
    cur, pat, left, right = [], [], [], []                       # left / right: the text positions beside the walker's window at its anchor
    for r, p in zip(*seeds(sigma)):
        c = searched(ox, r)
        cur.append((c.lb, c.lb_rev, c.len)); pat.append([int(v) for v in r]); left.append(p - 1); right.append(p + len(r))
    rev = (lambda v: v) if bidir else (lambda v: 0)
    cur.append((0, 0, n)); pat.append([]); left.append(449); right.append(450)        # the root cursor, anchored in the middle of the first sequence
    for c in ((0, 0, 0), (n, rev(n), 0), (n - 1, rev(n - 1), 1)):                     # empty at both ends of the index; the last row alone
        cur.append(c); pat.append(None); left.append(None); right.append(None)
    rounds = []
    for _ in range(ROUNDS):
        W = len(cur)
        go_right = (rng.random(W) < 0.5) & bool(bidir)
        true, uniform = rng.random(W) < 0.8, rng.integers(0, sigma, size=W)
        rd = {"right": go_right, "symb": np.zeros(W, dtype=np.uint8), "inp": np.array(cur, dtype=np.uint64), "out": np.zeros((W, 3), dtype=np.uint64),
              "plain": np.full(W, -1, dtype=np.int64)}
        for w in range(W):
            c = int(uniform[w])
            if pat[w] is not None:
                j = right[w] if go_right[w] else left[w]
                if true[w]:
                    c = int(text[j]) if 0 <= j < len(text) else 0
                if go_right[w]:
                    pat[w] = pat[w] + [c]; right[w] += 1
                else:
                    pat[w] = [c] + pat[w]; left[w] -= 1
                if 0 not in pat[w]:
                    rd["plain"][w] = len(occurrences(text, np.array(pat[w], dtype=np.uint8))[0])
            nc = (ox.extend_right if go_right[w] else ox.extend_left)(fo.Cursor(*(int(v) for v in cur[w])), c)
            cur[w] = (nc.lb, nc.lb_rev, nc.len)
            rd["symb"][w], rd["out"][w] = c, cur[w]
        rounds.append(rd)
    return rounds


def test_the_oracle_walk_counts_windows():
    """CPU only: on every step whose pattern holds no delimiter the oracle's new len is the number of windows of the text equal to the pattern (left steps prepend the
    symbol, right steps append it) — and the walk is what it claims: cursors that live for several rounds, empty results, both directions, delimiter steps"""
    for sigma in SIGMAS:
        for bidir in (False, True):
            rounds = walk(sigma, bidir)
            checked = alive = empty = rights = delims = 0
            for r, rd in enumerate(rounds):
                m = rd["plain"] >= 0
                bad = np.nonzero(m & (rd["out"][:, 2] != rd["plain"].astype(np.uint64)))[0]
                assert not len(bad), ("the oracle's len differs from the plain count", sigma, bidir, r, bad[:8].tolist())
                checked += int(m.sum()); alive += int((rd["out"][:, 2] > 0).sum()); empty += int((rd["out"][:, 2] == 0).sum())
                rights += int(rd["right"].sum()); delims += int((rd["symb"] == 0).sum())
                assert (rd["inp"][:, 0] + rd["inp"][:, 2] <= N_ROWS).all() and (rd["inp"][:, 1] + rd["inp"][:, 2] <= N_ROWS).all()
            print("sigma %d %s: %d steps checked against the plain count, %d results alive, %d empty, %d to the right, %d with the delimiter; alive after the last round: %d"
                  % (sigma, "BiFMIndex" if bidir else "FMIndex", checked, alive, empty, rights, delims, int((rounds[-1]["out"][:, 2] > 0).sum())))
            assert checked >= 2000 and alive >= 800 and empty >= 300 and delims >= (20 if sigma == 5 else 1) and (rights >= 1000) == bidir
            assert int((rounds[5]["out"][:, 2] > 0).sum()) >= 30, "too few cursors live for several rounds"


def test_the_depth_model_on_the_oracle():
    """CPU only: the depth model against the oracle's exact search — a read whose search ends with several rows has depth length + 1, any other read a depth within
    1 .. length; a read that ends empty was emptied no later than the search stopped"""
    for sigma in SIGMAS:
        inside = [k for k, r in enumerate(depth_batch(sigma)) if not (r >= sigma).any()]  # (a byte >= sigma is out of bounds for the reference's search, and for the oracle's)
        reads = [depth_batch(sigma)[k] for k in inside]
        ox = layout_oracle("IB16", sigma, True)
        want = expected_depth(sigma)[inside]
        lb, ln, st = ox.search_exact(*fm.flatten(reads), want_steps=True)
        lens = np.array([len(r) for r in reads], dtype=np.uint64)
        assert np.array_equal(want > lens, ln > 1) and (want[ln > 1] == lens[ln > 1] + 1).all(), sigma
        assert (want[(ln <= 1) & (lens > 0)] >= 1).all() and (want[ln == 0] <= st[ln == 0]).all(), sigma
        assert want[[len(r) == 0 for r in reads]].tolist() == [1]
        alien = [k for k, r in enumerate(depth_batch(sigma)) if (r >= sigma).any()]
        assert len(alien) == WALKERS and (expected_depth(sigma)[alien] <= [len(depth_batch(sigma)[k]) for k in alien]).all()
        print("sigma %d: %d reads, depth min %d max %d, %d beyond their length" % (sigma, len(reads), want.min(), want.max(), int((want > lens).sum())))


# ------------------------------------------------------------------------------------------------ the walk
def device_round(gx, rd, inp):
    """one batched single-symbol call per direction on the cursors `inp`: (W, 3), lb_rev = 0 on a unidirectional handle"""
    bidir = gx.bidirectional
    got = np.zeros((len(inp), 3), dtype=np.uint64)
    for right in (False, True) if bidir else (False,):
        m = rd["right"] == right
        if not m.any():
            continue
        olb, orev, olen = gx.extend(inp[m, 0], inp[m, 1] if bidir else None, inp[m, 2], symb=rd["symb"][m], right=right)
        got[m, 0], got[m, 2] = olb, olen
        if bidir:
            got[m, 1] = orev
        else:
            assert orev is None
    return got


def differing(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8].tolist()


@gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_single_symbol_steps_against_the_oracle_walk(layout, wide):
    """every round of the oracle's walk: lb, lb_rev and len of every cursor, empty results included (they carry the reference's lb); the new len against the plain window
    count; then the chain — the device fed with its own outputs ends at the oracle's final cursors"""
    for sigma in SIGMAS:
        for bidir in (False, True):
            where = (layout, sigma, "BiFMIndex" if bidir else "FMIndex", "64-bit rows" if wide else "32-bit rows")
            gx = handle(layout, sigma, bidir, wide)
            rounds = walk(sigma, bidir)
            chain = rounds[0]["inp"]
            for r, rd in enumerate(rounds):
                got = device_round(gx, rd, rd["inp"])
                assert np.array_equal(got, rd["out"]), ("round", r, where, differing(got, rd["out"]))        # (lb_rev: zeros on both sides of a unidirectional handle)
                m = rd["plain"] >= 0
                assert np.array_equal(got[m, 2], rd["plain"][m].astype(np.uint64)), ("len differs from the plain window count", r, where)
                chain = device_round(gx, rd, chain)
            assert np.array_equal(chain, rounds[-1]["out"]), ("chain", where, differing(chain, rounds[-1]["out"]))


@gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_both_forms_and_the_search_agree(layout, wide):
    """form identity on the cursors of round 3: extend(.., None)[i, c] == extend(.., symb = c)[i] for every c and both directions, and both equal the oracle's all-symbols
    step; search identity: a read's symbols stepped leftwards from the root, last symbol first, until the first empty cursor, reproduce search_no_errors.search"""
    for sigma in SIGMAS:
        seqs = collection(sigma)[0]
        reads = sample_reads(seqs[0], 100, 20, seed=21, mutate=1, sigma=sigma)           # every other read carries a substitution
        queries = fm.flatten(reads)
        for bidir in (False, True):
            where = (layout, sigma, "BiFMIndex" if bidir else "FMIndex", "64-bit rows" if wide else "32-bit rows")
            gx = handle(layout, sigma, bidir, wide)
            ox = layout_oracle("IB16", sigma, bidir)
            cur = walk(sigma, bidir)[3]["inp"]
            lb, rev, ln = cur[:, 0], (cur[:, 1] if bidir else None), cur[:, 2]
            for right in (False, True) if bidir else (False,):
                alb, arev, alen = gx.extend(lb, rev, ln, None, right=right)
                assert alb.shape == (len(cur), sigma) and (arev is None) == (not bidir)
                for k in range(0, len(cur), 7):                                          # the all-symbols form against the oracle's, on every 7th cursor
                    step = (ox.extend_right_all if right else ox.extend_left_all)(fo.Cursor(*(int(v) for v in cur[k])))
                    want = np.array([(c.lb, c.lb_rev, c.len) for c in step], dtype=np.uint64)
                    got = np.stack([alb[k], arev[k] if bidir else np.zeros(sigma, dtype=np.uint64), alen[k]], axis=1)
                    assert np.array_equal(got, want), ("all-symbols form", where, right, k)
                for c in range(sigma):
                    olb, orev, olen = gx.extend(lb, rev, ln, symb=c, right=right)
                    same = np.array_equal(olb, alb[:, c]) and np.array_equal(olen, alen[:, c]) and (not bidir or np.array_equal(orev, arev[:, c]))
                    assert same, ("the two forms differ", where, "right" if right else "left", c)
            slb, sln = fm.search_no_errors.search(gx, queries)
            olb, oln = ox.search_exact(*queries)
            assert np.array_equal(slb, olb) and np.array_equal(sln, oln), ("exact search", where)
            assert int((sln > 0).sum()) >= 40 and int((sln == 0).sum()) >= 40
            R = np.stack(reads)
            cl, cr, cn = np.zeros(len(R), dtype=np.uint64), np.zeros(len(R), dtype=np.uint64), np.full(len(R), N_ROWS, dtype=np.uint64)
            for j in range(R.shape[1]):
                live = np.nonzero(cn > 0)[0]
                if not len(live):
                    break
                nl, nr, nn = gx.extend(cl[live], cr[live] if bidir else None, cn[live], symb=R[live, R.shape[1] - 1 - j])
                cl[live], cn[live] = nl, nn
                if bidir:
                    cr[live] = nr
            assert np.array_equal(cl, slb) and np.array_equal(cn, sln), ("stepping a read's symbols differs from the exact search", where)


# ------------------------------------------------------------------------------------------------ the guard, the errors, device buffers
GUARD_LAYOUTS = ("IB8", "IB16", "IBP16", "EPR8", "EPRV2_16", "WAVELET", "EPRV3_8", "EPRV5", "IEPRV7", "FBV_512_64K")


def raw_extend(gx, direction, count, lb, rev, ln, symb, olb, orev, oln, stream=None):
    return capi.lib().fmgpu_cursor_extend(gx._h, direction, count, capi.ptr(lb), capi.ptr(rev), capi.ptr(ln), capi.ptr(symb), capi.ptr(olb), capi.ptr(orev), capi.ptr(oln), stream)


@gpu
@pytest.mark.parametrize("wide", [0, 1])
def test_cursors_outside_the_index_yield_zeros(wide):
    """fmgpu_index.hip computes `valid` before any table is read: lb > n, lb + len > n (also where the sum wraps), len = 2^64 - 1, lb_rev + len > n, symb = sigma and
    symb = 255 each give {0, 0, 0}, in all sigma slots of the all-symbols form; the valid cursors between them keep their oracle values.  A unidirectional handle
    ignores lb_rev, whatever it holds"""
    n = N_ROWS
    outside = [(n + 1, 0, 0), (n - 3, 0, 5), (0, 0, NONE), (1, 0, NONE), (NONE, 0, 1), (NONE, 0, NONE), (0, n - 3, 5), (0, n + 1, 0), (5, NONE, 2)]
    for layout in GUARD_LAYOUTS:
        for sigma in SIGMAS:
            for bidir in (False, True):
                where = (layout, sigma, "BiFMIndex" if bidir else "FMIndex", "64-bit rows" if wide else "32-bit rows")
                gx = handle(layout, sigma, bidir, wide)
                rd = walk(sigma, bidir)[3]
                bad = np.array([c for c in outside if bidir or c[1] == 0], dtype=np.uint64)
                ok = np.concatenate([rd["inp"][:40], rd["inp"][-4:]])
                at = np.arange(len(ok) + len(bad)) % 5 == 2                              # the cursors outside stand between the valid ones
                at[np.nonzero(at)[0][len(bad):]] = False
                assert at.sum() == len(bad)
                cur = np.zeros((len(at), 3), dtype=np.uint64)
                cur[at], cur[~at] = bad, ok
                okc = np.concatenate([rd["symb"][:40], rd["symb"][-4:]])
                for right in (False, True) if bidir else (False,):
                    ox = layout_oracle("IB16", sigma, bidir)
                    want1 = np.zeros((len(cur), 3), dtype=np.uint64)
                    symb = np.zeros(len(cur), dtype=np.uint8)
                    symb[~at] = okc
                    symb[at] = 1
                    over = np.nonzero(~at)[0][3::9]                                      # valid cursors with a symbol outside the alphabet
                    symb[over[0::2]], symb[over[1::2]] = min(sigma, 255), 255
                    wantall = np.zeros((len(cur), sigma, 3), dtype=np.uint64)
                    for k in np.nonzero(~at)[0]:
                        c0 = fo.Cursor(*(int(v) for v in cur[k]))
                        wantall[k] = [(c.lb, c.lb_rev, c.len) for c in (ox.extend_right_all if right else ox.extend_left_all)(c0)]
                        if symb[k] < sigma:
                            nc = (ox.extend_right if right else ox.extend_left)(c0, int(symb[k]))
                            want1[k] = (nc.lb, nc.lb_rev, nc.len)
                    assert (want1[~at][:, 2] > 0).sum() >= 5 and len(over) >= 4
                    olb, orev, oln = gx.extend(cur[:, 0], cur[:, 1] if bidir else None, cur[:, 2], symb=symb, right=right)
                    got = np.stack([olb, orev if bidir else np.zeros_like(olb), oln], axis=1)
                    assert np.array_equal(got, want1), ("single-symbol form", where, right, differing(got, want1))
                    olb, orev, oln = gx.extend(cur[:, 0], cur[:, 1] if bidir else None, cur[:, 2], None, right=right)
                    got = np.stack([olb, orev if bidir else np.zeros_like(olb), oln], axis=2)
                    assert np.array_equal(got, wantall), ("all-symbols form", where, right)
                    assert not got[at].any()
                if not bidir:                                                            # lb_rev of a unidirectional handle: ignored, and out_lb_rev receives zeros
                    junk = np.full(len(cur), NONE, dtype=np.uint64)
                    olb, orev, oln = (np.full(len(cur), NONE, dtype=np.uint64) for _ in range(3))
                    assert raw_extend(gx, 0, len(cur), np.ascontiguousarray(cur[:, 0]), junk, np.ascontiguousarray(cur[:, 2]), symb, olb, orev, oln) == 0
                    assert np.array_equal(np.stack([olb, orev, oln], axis=1), want1), ("lb_rev is not ignored", where)


@gpu
def test_argument_errors_of_cursor_extend():
    """FMGPU_ERR_INVALID for a direction other than 0 and 1, for direction 1 on an FMIndex (the message names a BiFMIndex), for a null lb, len, out_lb or out_len, and on
    a BiFMIndex for a null lb_rev or out_lb_rev (an FMIndex takes both as null); count == 0 returns 0 with every pointer null"""
    bx, ux = handle("IB16", 5, True, 0), handle("IB16", 5, False, 0)
    a = np.zeros(4, dtype=np.uint64)
    ln = np.full(4, 3, dtype=np.uint64)
    o = [np.zeros(4 * 5, dtype=np.uint64) for _ in range(3)]
    assert raw_extend(bx, 2, 4, a, a, ln, None, *o) == capi.FMGPU_ERR_INVALID
    assert raw_extend(bx, -1, 4, a, a, ln, None, *o) == capi.FMGPU_ERR_INVALID
    assert raw_extend(ux, 1, 4, a, a, ln, None, *o) == capi.FMGPU_ERR_INVALID
    assert "BiFMIndex" in capi.lib().fmgpu_last_error().decode()
    with pytest.raises(fm.FmgpuError) as ei:
        ux.extend(a, None, ln, symb=1, right=True)
    assert ei.value.code == capi.FMGPU_ERR_INVALID
    for gx in (bx, ux):
        for missing in (0, 2, 4, 6):                                                     # lb, len, out_lb, out_len
            args = [a, a, ln, None, *o]
            args[missing] = None
            assert raw_extend(gx, 0, 4, *args) == capi.FMGPU_ERR_INVALID, (gx.bidirectional, missing)
    for missing in (1, 5):                                                               # lb_rev, out_lb_rev: a BiFMIndex needs them, an FMIndex does not
        args = [a, a, ln, None, *o]
        args[missing] = None
        assert raw_extend(bx, 0, 4, *args) == capi.FMGPU_ERR_INVALID, missing
        assert raw_extend(ux, 0, 4, *args) == 0, missing
    for gx in (bx, ux):
        for direction in (0, 1) if gx.bidirectional else (0,):
            assert raw_extend(gx, direction, 0, None, None, None, None, None, None, None) == 0
    olb, orev, oln = ux.extend(a, None, ln, None)                                        # and the handles still answer
    assert orev is None and olb.shape == (4, 5)


@gpu
def test_cursor_steps_with_device_buffers_on_a_caller_stream():
    """all seven arrays in HBM, the call on a non-default stream: complete once that stream is synchronised, and equal to the host-buffer call — one call per form
    (streams from the HIP runtime libfmgpu.so itself is linked against, as test_calls_on_caller_streams_with_device_buffers does)"""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    try:
        for layout, sigma in (("IB16", 5), ("WAVELET", 28), ("EPR16", 255)):
            gx = handle(layout, sigma, True, 0)
            rd = walk(sigma, True)[3]
            cur, count = rd["inp"], len(rd["inp"])
            for right in (0, 1):
                for symb in (rd["symb"], None):
                    fan = 1 if symb is not None else sigma
                    want = gx.extend(cur[:, 0], cur[:, 1], cur[:, 2], symb=symb, right=bool(right))
                    ins = [fm.DeviceBuffer.from_array(np.ascontiguousarray(cur[:, k])) for k in range(3)]
                    ds = fm.DeviceBuffer.from_array(symb) if symb is not None else None
                    outs = [fm.DeviceBuffer.from_array(np.full(count * fan, NONE, dtype=np.uint64)) for _ in range(3)]
                    rc = capi.lib().fmgpu_cursor_extend(gx._h, right, count, C.c_void_p(ins[0].ptr), C.c_void_p(ins[1].ptr), C.c_void_p(ins[2].ptr),
                                                        C.c_void_p(ds.ptr) if ds else None, C.c_void_p(outs[0].ptr), C.c_void_p(outs[1].ptr), C.c_void_p(outs[2].ptr), st)
                    assert rc == 0, capi.lib().fmgpu_last_error()
                    assert hip.hipStreamSynchronize(st) == 0
                    for got, w in zip(outs, want):
                        assert np.array_equal(got.to_array(np.uint64, count * fan), w.reshape(-1)), (layout, sigma, right, fan)
                    assert int((want[2] > 0).sum()) >= 5
    finally:
        hip.hipStreamDestroy(st)


# ------------------------------------------------------------------------------------------------ the depth profile
@functools.lru_cache(maxsize=None)
def depth_batch(sigma):
    """the walkers' seed reads (lengths 1 to 40), the same with one substitution, with a delimiter inside, with a byte >= sigma (sigma itself and 255), an empty read,
    and one read of 300 symbols"""
    seqs = collection(sigma)[0]
    reads = seeds(sigma)[0]
    rng = np.random.default_rng(900 + sigma)
    subst, delim, alien = [], [], []
    for k, r in enumerate(reads):
        q = r.copy(); j = int(rng.integers(0, len(q))); q[j] = (int(q[j]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1; subst.append(q)
        q = r.copy(); q[int(rng.integers(0, len(q)))] = 0; delim.append(q)
        q = r.copy(); q[int(rng.integers(0, len(q)))] = 255 if k % 2 else min(sigma, 255); alien.append(q)
    return reads + subst + delim + alien + [np.zeros(0, dtype=np.uint8), seqs[0][100:400].copy()]


@functools.lru_cache(maxsize=None)
def expected_depth(sigma):
    return depth_model(layout_oracle("IB16", sigma, True), depth_batch(sigma))


def depth_handles(layout, sigma, wide):
    yield "BiFMIndex", handle(layout, sigma, True, wide)
    yield "FMIndex", handle(layout, sigma, False, wide)
    if sigma == 5 and family(layout) != "A":                                             # EPR / EPRV2 / Wavelet answer from their native readers, not from the Format A shadow
        yield "FMIndex, not expanded", handle(layout, sigma, False, wide, expand_dna=0)
        yield "BiFMIndex, not expanded", handle(layout, sigma, True, wide, expand_dna=0)


@gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_depth_profile_against_the_model(layout, wide):
    """out_depth of the whole batch on FMIndex and BiFMIndex handles of the layout (sigma = 5: also with expand_dna = 0), from offset 0 and behind 7 other bytes"""
    for sigma in SIGMAS:
        reads = depth_batch(sigma)
        want = expected_depth(sigma)
        qbuf, qoff = fm.flatten(reads)
        shifted = (np.concatenate([np.full(7, 1, dtype=np.uint8), qbuf]), qoff + np.uint64(7))                 # the same batch behind 7 other bytes: qoff[0] != 0
        for name, gx in depth_handles(layout, sigma, wide):
            where = (layout, sigma, name, "64-bit rows" if wide else "32-bit rows")
            got = fm.search_no_errors.depth(gx, (qbuf, qoff))
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.uint64), want), (where, np.nonzero(got != want)[0][:8].tolist())
            got = fm.search_no_errors.depth(gx, shifted)
            assert np.array_equal(got.astype(np.uint64), want), ("qoff[0] = 7", where, np.nonzero(got != want)[0][:8].tolist())


@gpu
@pytest.mark.parametrize("wide", [0, 1])
def test_depth_on_one_row_and_its_argument_errors(wide):
    """an index of one row (a single empty sequence): nothing is consumed of any read; nq == 0 returns 0; a null out_depth with nq > 0 is FMGPU_ERR_INVALID"""
    ox = fo.OraIndex.build("IB16", 5, [np.zeros(0, dtype=np.uint8)], 1, False)
    assert ox.n == 1
    with fm.options(force_wide=wide):
        gx = fm.FMIndex.from_reference_arrays(**oracle_arrays(ox))
    assert gx.n == 1 and gx.row_bits == (64 if wide else 32)
    reads = [np.zeros(0, dtype=np.uint8), np.array([1], dtype=np.uint8), np.array([0], dtype=np.uint8), np.array([2, 9, 255, 1], dtype=np.uint8)]
    assert np.array_equal(depth_model(ox, reads), np.zeros(len(reads), dtype=np.uint64))
    assert fm.search_no_errors.depth(gx, reads).tolist() == [0] * len(reads)
    qbuf, qoff = fm.flatten(reads)
    L = capi.lib()
    for hx in (gx, handle("IB16", 5, True, wide)):
        assert L.fmgpu_search_exact_depth(hx._h, None, None, 0, None, None) == 0
        assert L.fmgpu_search_exact_depth(hx._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), None, None) == capi.FMGPU_ERR_INVALID
        assert len(fm.search_no_errors.depth(hx, reads)) == len(reads)


# ------------------------------------------------------------------------------------------------ creation
@gpu
def test_a_bifmindex_of_two_layouts_is_refused():
    """BiFMIndex<String> has one String type; the kernels choose their reader by bwt's layout and would read bwt_rev through an empty view.  Creation refuses the pair
    (no search or cursor call is made on such a handle)"""
    seqs = [make_text(300, 6, seed=5), make_text(120, 6, seed=6)]
    arrays = {layout: oracle_arrays(fo.OraIndex.build(layout, 6, seqs, 4, True)) for layout in ("IB16", "EPR16")}
    for fw, rv in (("IB16", "EPR16"), ("EPR16", "IB16")):
        with pytest.raises(fm.FmgpuError) as ei:
            fm.BiFMIndex.from_reference_arrays(bwt=arrays[fw]["bwt"], C_array=arrays[fw]["C_array"], bwt_rev=arrays[rv]["bwt_rev"], sparse=arrays[fw]["sparse"])
        assert ei.value.code == capi.FMGPU_ERR_INVALID and fw in str(ei.value) and rv in str(ei.value), str(ei.value)
    for layout in arrays:
        gx = fm.BiFMIndex.from_reference_arrays(**arrays[layout])
        assert gx.bidirectional and gx.layout == layout and gx.n == 422
