"""The occurrence tables of the device where their counters start anew: the super-block boundaries of the reference layouts (every 256 / 65 536 rows, 65 520 or
65 532 for InterleavedEPR, the 2^8 and 2^16 levels of EPRV4 / EPRV5 / InterleavedEPRV7, the l1 / l0 pair of FlattenedBitvectors2L) and the super-blocks of the
64-bit-row build (2^30 rows in the shipped library; 2^16 in the development build libfmgpu_dev_ss16.so, which the last tests run in a child process).

  1. String_c at the edges: rank / prefix_rank / symbol of every layout at sizes P - 1, P, P + 1, 2 P + 300 around its super-block period P, on the rows beside
     every boundary, against the oracle and against the plain count #{j < i : text[j] == c} (a numpy cumulative sum, independent of the oracle).
  2. Searches aimed at the edges: a collection of 131 371 rows (two 16-bit boundaries, the EPR periods beside them), reads cut from the suffixes of the rows
     beside each boundary — exact search through every kernel selection, scheme searches (Hamming, edit, ng21, backtracking, SMEMs, scoring matrix), cursor
     steps (all symbols at once and one symbol per call), the depth profile, locate, locate_hits and extract, per layout, alphabet and row width, against the CPU walk of the oracle.
  3. The same check list with 64-bit rows on super-blocks of 2^16 rows (three of them), so that the super tables of Formats A / P / M, the builder's, the
     locate kernels' and the lean kernel's LDS copy are read beyond their first entry.
  4. The symbol-plane table (Format S, k_exact_s) in that build: count fields of 16 bits in both row widths, three super-blocks — exact search by every selection
     and with interval tables at sigma = 6, 21, 25, 26, 28, 29, the super table in LDS and through L2, workgroups of 256 and 512 lanes, and skewed collections that
     set a field's top bit before each boundary.  (The shipped field widths at their real boundaries: tests/test_gpu_symbol_planes.py.)

The reference's own rank(n, .) at n = k P counts the closed super-block twice: pinned in QUIRK_ROW."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, POSITION_DTYPE
from tests import smem_brute as sb
from tests.cursor_model import depth_model, single_steps
from tests.util import make_text, oracle_arrays, string_arrays
from tests.test_gpu_parity import LAYOUTS, HIT_KEYS, mutated_queries
from tests.golden.make_golden import EDGE_SIGMAS, super_period, edge_sizes, edge_text, edge_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. String_c at the edges
def family(layout):
    """which reader answers fmgpu_string_query: "R" = InterleavedEPR blocks in place (OccR<false>), "R2" = InterleavedEPRV2 blocks in place (OccR<true>),
    "M" = the multi-ary tree of a Wavelet, "A" = everything converted to the one-symbol block table"""
    return "R" if layout in ("EPR8", "EPR16", "EPR32") else "R2" if layout.startswith("EPRV2_") else "M" if layout == "WAVELET" else "A"


# what the device returns on row i = n of a string of n = k P rows, where the reference (and the oracle, bit for bit) counts the closed super-block twice:
# "oracle" = the reference's doubled value, "plain" = the count in the text.  The in-place readers do the reference's arithmetic on the reference's arrays;
# the converter of EPRV3 (k_convert_hier) adds the same super-block and block counters.  No kernel was changed to get these.
QUIRK_ROW = {"A": "oracle", "R": "oracle", "R2": "oracle"}
QUIRK_LAYOUTS = ("EPR8", "EPR16", "EPRV2_8", "EPRV2_16", "EPRV3_8", "EPRV3_16")


@functools.lru_cache(maxsize=None)
def oracle_against_plain(layout, sigma, n):
    """the oracle's all_ranks_and_prefix_ranks on the probed rows against the plain count: (rows below n where they differ, the oracle's ranks and prefix
    ranks of row n, whether row n differs).  Shared by both row widths; the tables themselves are too large to keep"""
    text = edge_text(sigma, n)
    rows, _ = edge_rows(layout, sigma, n)
    rank, prefix = plain_counts(text, sigma, rows)
    ork, opr = fo.OraString(layout, sigma, text).all_ranks_rows(rows)
    differ = np.nonzero((ork != rank).any(axis=1) | (opr != prefix).any(axis=1))[0]
    below = [int(rows[k]) for k in differ if rows[k] < n]
    return below, ork[-1].copy(), opr[-1].copy(), bool(len(differ) and rows[differ[-1]] == n)


def plain_counts(text, sigma, rows):
    """#{j < i : text[j] == c} and #{j < i : text[j] < c} for the rows i: the high-precision reference, integers from a cumulative sum"""
    n = len(text)
    cum = np.zeros((n + 1, sigma), dtype=np.uint32)
    cum[np.arange(1, n + 1), text] = 1
    np.cumsum(cum, axis=0, out=cum)
    rank = cum[rows.astype(np.int64)].astype(np.uint64)
    return rank, np.cumsum(rank, axis=1) - rank


def device_tables(gx, rows, symbols):
    """rank and prefix_rank of every (row, symbol) pair, in pieces of 2^22 queries"""
    rank = np.empty((len(rows), len(symbols)), dtype=np.uint64)
    prefix = np.empty_like(rank)
    step = max(1, (1 << 22) // len(symbols))
    for a in range(0, len(rows), step):
        idx = np.repeat(rows[a: a + step], len(symbols))
        sym = np.tile(symbols, len(rows[a: a + step]))
        rank[a: a + step] = gx.rank(idx, sym).reshape(-1, len(symbols))
        prefix[a: a + step] = gx.prefix_rank(idx, sym).reshape(-1, len(symbols))
    return rank, prefix


@gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_string_concept_at_super_block_edges(layout, wide):
    """rank / prefix_rank / symbol on the rows within 130 of every multiple of the super-block period, of 65 536 and of the inner level sizes, every 509th row,
    n - 1 and n — all symbols on the boundary rows (every 17th on the others for sigma = 255).  Three assertions: the oracle equals the plain count below row n;
    the device equals the plain count below row n; on row n the device equals the oracle, or what QUIRK_ROW pins where the reference counts twice"""
    seen = 0
    for sigma in EDGE_SIGMAS:
        all_symbols = np.arange(sigma, dtype=np.uint8)
        few_symbols = all_symbols if sigma <= 28 else np.unique(np.concatenate([all_symbols[::17], all_symbols[-1:]]))
        for n in edge_sizes(layout, sigma):
            where = (layout, sigma, n, "64-bit rows" if wide else "32-bit rows")
            text = edge_text(sigma, n)
            rows, near = edge_rows(layout, sigma, n)
            s = fo.OraString(layout, sigma, text)
            C_arr = np.array([int(np.count_nonzero(text < c)) for c in range(sigma + 1)], dtype=np.uint64)
            with fm.options(force_wide=wide):
                gx = fm.FMIndex.from_reference_arrays(bwt=string_arrays(s), C_array=C_arr)
            assert gx.row_bits == (64 if wide else 32)
            below, orank_n, oprefix_n, doubled = oracle_against_plain(layout, sigma, n)
            assert not below, ("the oracle differs from the plain count below row n", where, below[:8])
            assert doubled == (n % (super_period(layout, sigma) or 1 << 40) == 0 and layout in QUIRK_LAYOUTS), where
            prank, pprefix = plain_counts(text, sigma, rows)
            for part, symbols in ((near, all_symbols), (~near, few_symbols)):
                if not part.any():
                    continue
                grank, gprefix = device_tables(gx, rows[part], symbols)
                under = rows[part] < n
                for what, got, plain in (("rank", grank, prank[part][:, symbols]), ("prefix_rank", gprefix, pprefix[part][:, symbols])):
                    bad = np.argwhere(got[under] != plain[under])
                    assert not len(bad), (what, "differs from the plain count", where, [(int(rows[part][under][r]), int(symbols[c])) for r, c in bad[:8]])
                if not under.all():                              # row n is the last probed row
                    assert rows[part][-1] == n
                    want = "oracle" if not doubled else QUIRK_ROW[family(layout)]
                    want_rank, want_prefix = (orank_n, oprefix_n) if want == "oracle" else (prank[-1], pprefix[-1])
                    if doubled:
                        print("row n = %d of %s sigma %d (%s): device rank %s, oracle %s, plain %s" % (n, layout, sigma, where[3], grank[-1][:4], orank_n[:4], prank[-1][:4]))
                        seen += 1
                    assert np.array_equal(grank[-1], want_rank[symbols]) and np.array_equal(gprefix[-1], want_prefix[symbols]), ("row n", want, where)
            at = rows[rows < n]
            assert np.array_equal(gx.symbol(at), text[at.astype(np.int64)].astype(np.uint64)), ("symbol", where)
    assert (seen > 0) == (layout in QUIRK_LAYOUTS)


# ------------------------------------------------------------------------------------------------ 2. searches aimed at the edges
N_ROWS = 131_371
BOUNDARIES = (65_520, 65_532, 65_536, 131_040, 131_064, 131_072)     # two super-blocks of 65 520 (EPR, 3 bits), 65 532 (EPR, 5 bits) and 65 536 rows
AIM_OFFSETS = (-65, -64, -63, -2, -1, 0, 1, 2, 63, 64, 65)
AIM_LENGTHS = (1, 2, 3, 5, 8, 12, 20, 40)
SCHEMES = {"h2": lambda: fm.search_scheme.h2(3, 0, 1), "pigeon": lambda: fm.search_scheme.pigeon_opt(0, 1)}
PLANES_EXTRA_SIGMAS = (25, 26, 29)                                   # alphabets of part 4 (exact search on the symbol-plane table) beyond EDGE_SIGMAS
SKEWED = ((29, 1), (29, 28))                                         # (sigma, dominant symbol) of part 4's skewed collections: the first symbol and the last


def skewed_text(n, sigma, dominant, seed):
    """n symbols: `dominant` at 90 % of the positions, placed at random (no runs beyond chance), the other symbols of 1 .. sigma - 1 uniform over the rest"""
    rng = np.random.default_rng(seed)
    other = rng.integers(1, sigma - 1, size=n, dtype=np.uint8)
    other += other >= dominant
    return np.where(rng.random(n) < 0.9, np.uint8(dominant), other).astype(np.uint8)


def collection(sigma, dominant=0):
    return _collection(sigma, dominant)


@functools.lru_cache(maxsize=None)
def _collection(sigma, dominant):
    """two sequences of 100 000 and 31 369 symbols, sorted once: the oracle index (IB16, rate 4, bidirectional) and what OraIndex.from_bwt needs for another layout
    (dominant = d: the skewed collection of part 4, symbol d at 90 % of the positions)"""
    seqs = [make_text(100_000, sigma, seed=3), make_text(31_369, sigma, seed=4)] if not dominant else [skewed_text(100_000, sigma, dominant, 3), skewed_text(31_369, sigma, dominant, 4)]
    ox = fo.OraIndex.build("IB16", sigma, seqs, 4, True)
    n = ox.n
    assert n == N_ROWS
    for p in {super_period(l, s) for l in LAYOUTS for s in EDGE_SIGMAS} - {None}:
        assert n % p, "the reference's first search step is wrong where n is a multiple of a super-block period"
    fw, rv = ox.bwt_string(), ox.bwt_string(rev=True)
    bwt = np.fromiter((fw.symbol(i) for i in range(n)), dtype=np.uint8, count=n)
    bwt_rev = np.fromiter((rv.symbol(i) for i in range(n)), dtype=np.uint8, count=n)
    has, seq, pos = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for i in range(n):
        v = ox.single_locate_step(i)
        if v is not None:
            has[i], seq[i], pos[i] = 1, v[0], v[1]
    return seqs, ox, (bwt, bwt_rev, has, seq, pos)


def text_position(ox, row):
    seq, pos, steps = ox.locate(int(row))
    return int(seq), int(pos + steps)


def batch(sigma, dominant=0):
    return _batch(sigma, dominant)


@functools.lru_cache(maxsize=None)
def _batch(sigma, dominant):
    """(reads, rows of the aimed reads): per row beside a boundary the first L symbols of its suffix, the same with one substitution and with a delimiter,
    and 500 reads from random places"""
    seqs, ox, _ = collection(sigma, dominant)
    rng = np.random.default_rng(1000 + sigma)
    aimed, rows = [], []
    for b in BOUNDARIES:
        for d in AIM_OFFSETS:
            seq, p = text_position(ox, b + d)
            for L in AIM_LENGTHS:
                if len(seqs[seq][p: p + L]):
                    aimed.append(seqs[seq][p: p + L].copy()); rows.append(b + d)
    subst, delim = [], []
    for r in aimed:
        q = r.copy(); j = int(rng.integers(0, len(q))); q[j] = (int(q[j]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1; subst.append(q)
        q = r.copy(); q[int(rng.integers(0, len(q)))] = 0; delim.append(q)
    return aimed + subst + delim + mutated_queries(seqs, 500, 1, 60, 1, seed=sigma, sigma=sigma), np.array(rows, dtype=np.uint64)


def hit_matrix(hits):
    return np.stack([np.asarray(hits[k]).astype(np.uint64) for k in HIT_KEYS], axis=1) if len(hits) else np.zeros((0, len(HIT_KEYS)), dtype=np.uint64)


def hit_records(qidx, lb, ln):
    h = np.zeros(len(lb), dtype=HIT_DTYPE)
    h["qidx"], h["lb"], h["len"] = qidx, lb, ln
    return h


def subsets(sigma):
    """which reads a search takes: scheme searches need a symbol per part (reads of 5 and more); one batch per length for the equal-length kernels"""
    reads, _ = batch(sigma)
    lens = np.array([len(r) for r in reads])
    clean = np.array([0 not in r for r in reads])                # (a scoring matrix pairs the delimiter with nothing: its batch holds none)
    return {"ragged": np.nonzero(lens >= 5)[0], "len20": np.nonzero(lens == 20)[0], "len40": np.nonzero(lens == 40)[0], "len20_clean": np.nonzero((lens == 20) & clean)[0]}


def flat(sigma, which):
    reads, _ = batch(sigma)
    return fm.flatten([reads[i] for i in subsets(sigma)[which]])


@functools.lru_cache(maxsize=None)
def expected(sigma):
    """every answer of the check list from the CPU walk of the oracle (extract and locate_hits: from the text and the oracle's locate), once per alphabet:
    the answers do not depend on the layout the BWT is held in, nor on the row width"""
    seqs, ox, _ = collection(sigma)
    reads, rows = batch(sigma)
    E = {}
    qbuf, qoff = fm.flatten(reads)
    lb, ln, st = ox.search_exact(qbuf, qoff, want_steps=True)
    E["exact"] = np.stack([lb, ln])
    E["exact_steps"] = np.array([int(st.sum())], dtype=np.uint64)
    for sname, make in SCHEMES.items():
        for which in ("ragged", "len20", "len40"):
            q = flat(sigma, which)
            for edit in (False, True):
                hits, _, nodes = ox.search_ng26(q[0], q[1], make(), edit=edit, cap=1 << 21)
                key = "%s/%s/%s" % ("edit" if edit else "hamming", sname, which)
                E[key], E[key + "#nodes"] = hit_matrix(hits), np.array([nodes], dtype=np.uint64)
    q = flat(sigma, "len20")
    hits, _, nodes = ox.search_ng21(q[0], q[1], fm.search_scheme.expand(SCHEMES["pigeon"](), 20), cap=1 << 21)
    E["ng21/len20"], E["ng21/len20#nodes"] = hit_matrix(hits), np.array([nodes], dtype=np.uint64)
    few = fm.flatten([reads[i] for i in subsets(sigma)["ragged"][::12]])
    E["backtracking"] = hit_matrix(ox.search_backtracking(few[0], few[1], 1)[0])
    q = flat(sigma, "len20_clean")
    m = hit_matrix(ox.search_ng26(q[0], q[1], SCHEMES["h2"](), edit=False, cap=1 << 21)[0])
    E["matrix/len20"] = m[np.lexsort(m.T[::-1])]                 # the identity matrix is the Hamming search; the order of the records within a read is its own
    seeds = [reads[i] for i in subsets(sigma)["len40"][::3]]
    brute = sb.Batch(seqs, seeds, sigma)
    want = brute.seeds()
    slb, sln = ox.search_exact(*fm.flatten([seeds[q][b: b + l] for q, b, l, _, _ in want]))
    E["smems"] = np.array([[q, b, l, s, r, int(slb[k]), int(sln[k])] for k, (q, b, l, s, r) in enumerate(want)], dtype=np.uint64).reshape(-1, 7)
    E["smems#lengths"] = np.array(brute.lengths, dtype=np.uint64)
    E["smems#steps"] = np.array([brute.steps], dtype=np.uint64)
    # cursors whose first or last row lies within 2 rows of a boundary, from the Hamming hits; all symbols, to the left and to the right
    h = E["hamming/h2/ragged"]
    close = np.zeros(len(h), dtype=bool)
    for b in BOUNDARIES:
        close |= (np.abs(h[:, 1].astype(np.int64) - b) <= 2) | (np.abs((h[:, 1] + h[:, 3]).astype(np.int64) - b) <= 2)
    cur = np.unique(h[close][:, 1:4], axis=0)
    assert len(cur) >= 20, "too few cursors beside a boundary"
    E["cursors"] = cur
    for right in (False, True):
        out = np.zeros((len(cur), sigma, 3), dtype=np.uint64)
        for k, (a, r, l) in enumerate(cur):
            step = (ox.extend_right_all if right else ox.extend_left_all)(fo.Cursor(int(a), int(r), int(l)))
            out[k] = [(c.lb, c.lb_rev, c.len) for c in step]
        E["extend/right" if right else "extend/left"] = out
        E["extend1/right" if right else "extend1/left"] = single_steps(ox, cur, right)         # extendLeft(c) / extendRight(c): one oracle call per cursor and symbol
    E["depth"] = depth_model(ox, reads)
    # locate: every row within 130 of a boundary
    near = np.unique(np.concatenate([np.arange(b - 130, b + 131) for b in BOUNDARIES])).astype(np.uint64)
    near = near[near < N_ROWS]
    E["locate_rows"] = near
    E["locate"] = np.array([ox.locate(int(r)) for r in near], dtype=np.uint64)
    # locate_hits: the exact intervals that straddle a boundary, as hit records
    straddle = np.zeros(len(lb), dtype=bool)
    for b in BOUNDARIES:
        straddle |= (lb < b) & (b < lb + ln)
    idx = np.nonzero(straddle & (ln <= 4096))[0]
    E["straddling"] = np.stack([idx.astype(np.uint64), lb[idx], ln[idx]], axis=1)
    pos = []
    for k, (q, a, l) in enumerate(E["straddling"]):
        for r in range(int(a), int(a + l)):
            s_, p_ = text_position(ox, r)
            pos.append((int(q), s_, p_, 0, k))
    E["locate_hits"] = np.array(pos, dtype=np.uint64).reshape(-1, 5)
    # extract: windows of up to 48 symbols that end at the text position of a row beside a boundary
    rng = []
    for r in near[::5]:
        s_, p_ = text_position(ox, r)
        w = min(48, p_)
        if w:
            rng.append((s_, p_ - w, w))
    E["ranges"] = np.array(rng, dtype=np.uint64)
    E["extract"] = np.concatenate([seqs[s_][p_: p_ + w] for s_, p_, w in rng])
    return E


def test_the_batch_is_what_it_claims():
    """CPU only: every aimed read's interval contains its row; at least 100 intervals straddle a boundary (lb < b < lb + len), at least 20 begin or end exactly
    on one, at least 100 are a single row — for each of the six alphabets and for the three that only the symbol-plane checks of part 4 add (its skewed collections: see there)"""
    for sigma, dominant in [(s, 0) for s in EDGE_SIGMAS + PLANES_EXTRA_SIGMAS]:
        seqs, ox, _ = collection(sigma, dominant)
        reads, rows = batch(sigma, dominant)
        lb, ln = ox.search_exact(*fm.flatten(reads[: len(rows)]))
        assert ((lb <= rows) & (rows < lb + ln)).all(), sigma
        straddle = sum(int(((lb < b) & (b < lb + ln)).sum()) for b in BOUNDARIES)
        on_edge = sum(int(((lb == b) | (lb + ln == b)).sum()) for b in BOUNDARIES)
        one_row = int((ln == 1).sum())
        print("sigma %d%s: %d aimed reads, %d straddle a boundary, %d begin or end on one, %d are one row" % (sigma, ", symbol %d dominant" % dominant if dominant else "", len(rows), straddle, on_edge, one_row))
        assert straddle >= 100 and on_edge >= 20 and one_row >= 100, (sigma, dominant, straddle, on_edge, one_row)


def exact_selections(sigma, wide):
    """the kernel selections of exact search that the suite uses, where they choose another kernel"""
    out = [("default", 0)]
    if sigma == 5:
        out.append(("one_symbol", capi.SEL_EXACT_ONE_SYMBOL))
        if not wide:
            out.append(("no_sample_chain", capi.SEL_NO_SAMPLE_CHAIN))
    if 6 <= sigma <= 29:
        out.append(("on_tree", capi.SEL_EXACT_ON_TREE))
    return out


def exact_tables(sigma, wide):
    """(kstep, lut_len, walk) as test_exact_search_with_kstep_accelerator and test_wide_exact_search_and_locate parametrise them, the interval table capped at 2^22 entries"""
    if wide:
        combos = ((1, 4, 0), (1, 0, 1), (1, 3, 2), (0, 2, 1))
    else:
        k = 3 if sigma in (5, 6) else 2 if sigma == 4 else 1
        combos = ((k, 4, 0), (k, 0, 1), (k, 5, 1), (1, 3, 1), (1, 2, 0), (k, 4, 2), (1, 0, 2))
    cap = 1
    while (sigma - 1) ** (cap + 1) <= 1 << 22:
        cap += 1
    return [(ks, min(lut, cap), walk) for ks, lut, walk in combos]


def exact_of(gx, queries):
    lb, ln, st = fm.search_no_errors.search(gx, queries, want_stats=True)
    return np.stack([lb, ln]), np.array([st.lf_steps], dtype=np.uint64)


def collect_exact_and_locate(gx, sigma, tag, R):
    """the checks that depend on how the handle was created: exact search by every selection, locate by both kernels"""
    reads, _ = batch(sigma)
    E = expected(sigma)
    queries = fm.flatten(reads)
    for name, sel in exact_selections(sigma, gx.row_bits == 64):
        with fm.options(kernel_select=sel):
            R["exact@%s/%s" % (tag, name)], R["exact_steps@%s/%s" % (tag, name)] = exact_of(gx, queries)
    for name, sel in (("quad", 0), ("per_lane", capi.SEL_LOCATE_PER_LANE)):
        with fm.options(kernel_select=sel):
            R["locate@%s/%s" % (tag, name)] = np.stack(gx.locate(E["locate_rows"]), axis=1)
    hits = hit_records(E["straddling"][:, 0], E["straddling"][:, 1], E["straddling"][:, 2])
    pos = gx.locate_hits(hits, capacity=len(E["locate_hits"]) + 16)
    R["locate_hits@%s" % tag] = np.stack([pos[k].astype(np.uint64) for k in ("qidx", "seq_id", "pos", "errors", "hit")], axis=1).reshape(-1, 5)


def collect(gx, sigma, R=None, tag="default"):
    """the whole check list on one handle: name@kernel-path -> what the device returned (compare() names the path that differs)"""
    R = {} if R is None else R
    wide = gx.row_bits == 64
    reads, _ = batch(sigma)
    E = expected(sigma)
    queries = fm.flatten(reads)
    collect_exact_and_locate(gx, sigma, tag, R)
    if sigma <= 15:                                              # the 4-bit form, packed on the host and on the device
        R["exact@%s/q4" % tag], R["exact_steps@%s/q4" % tag] = exact_of(gx, fm.pack_queries(queries, sigma))
        R["exact@%s/q4_device" % tag], _ = exact_of(gx, fm.pack_queries_device(queries, sigma))
    # scheme searches: equal-length batches (lean / fast / fast-edit kernels) and the ragged whole (general kernels), LF table on and off, prefix and walk tables
    def schemes(path, which_list, edit_list=(False, True)):
        for sname, make in SCHEMES.items():
            for which in which_list:
                for edit in edit_list:
                    hits, st = fm.search_ng26.search(gx, flat(sigma, which), make(), want_stats=True, edit=edit, capacity=1 << 21)
                    key = "%s/%s/%s" % ("edit" if edit else "hamming", sname, which)
                    R["%s@%s/%s" % (key, tag, path)], R["%s#nodes@%s/%s" % (key, tag, path)] = hit_matrix(hits), np.array([st.lf_steps], dtype=np.uint64)
    schemes("lf", ("ragged", "len20", "len40"))
    with fm.options(kernel_select=capi.SEL_GENERAL_DFS):
        schemes("general", ("len20",))
    if sigma == 5:                                               # the equal-length Hamming kernels of a sigma = 5 index, one by one
        for path, sel in (("lean_on_format_a", capi.SEL_LEAN_FORMAT_A), ("fast_plain", capi.SEL_NO_LEAN)):
            with fm.options(kernel_select=sel):
                schemes(path, ("len20", "len40"), (False,))
    q20 = flat(sigma, "len20")
    hits, st = fm.search_ng21.search(gx, q20, fm.search_scheme.expand(SCHEMES["pigeon"](), 20), want_stats=True, capacity=1 << 21)
    R["ng21/len20@%s" % tag], R["ng21/len20#nodes@%s" % tag] = hit_matrix(hits), np.array([st.lf_steps], dtype=np.uint64)
    few = fm.flatten([reads[i] for i in subsets(sigma)["ragged"][::12]])
    R["backtracking@%s" % tag] = hit_matrix(fm.search_backtracking.search(gx, few, 1))
    if sigma <= 32:
        m = hit_matrix(fm.search_hamming_sm.search(gx, flat(sigma, "len20_clean"), SCHEMES["h2"](), fm.ScoringMatrix(sigma), capacity=1 << 21))
        R["matrix/len20@%s" % tag] = m[np.lexsort(m.T[::-1])]
    seeds = [reads[i] for i in subsets(sigma)["len40"][::3]]
    sh, spans, lengths, st = fm.search_smems(gx, seeds, want_lengths=True, want_stats=True)
    R["smems@%s" % tag] = np.stack([sh["qidx"], spans["qbeg"], spans["qlen"], sh["seq"], sh["len"], sh["lb"], sh["len"]], axis=1).astype(np.uint64).reshape(-1, 7)
    R["smems#lengths@%s" % tag], R["smems#steps@%s" % tag] = np.asarray(lengths).astype(np.uint64), np.array([st.lf_steps], dtype=np.uint64)
    cur = E["cursors"]
    for right in (False, True):
        olb, orev, olen = gx.extend(cur[:, 0], cur[:, 1], cur[:, 2], None, right=right)
        R["extend/%s@%s" % ("right" if right else "left", tag)] = np.stack([olb, orev, olen], axis=2)
        one = [gx.extend(cur[:, 0], cur[:, 1], cur[:, 2], symb=c, right=right) for c in range(sigma)]      # the single-symbol form, one batched call per symbol
        R["extend1/%s@%s" % ("right" if right else "left", tag)] = np.stack([np.stack(step, axis=1) for step in one], axis=1)
    R["depth@%s" % tag] = fm.search_no_errors.depth(gx, queries).astype(np.uint64)
    gx.accelerate_lf(False)
    schemes("no_lf", ("ragged", "len20"))
    R["locate@%s/no_lf" % tag] = np.stack(gx.locate(E["locate_rows"]), axis=1)
    gx.accelerate_lf(True)
    if not wide:                                                 # what only the 32-bit-row build offers
        gx.accelerate_search(min(4, exact_tables(sigma, wide)[0][1]), 3)      # (the prefix table capped like the interval table: sigma = 255 takes 2 symbols)
        schemes("prefix_walk3", ("ragged", "len20"))
        gx.accelerate_search(0, 0)
        gx.accelerate_locate()
        R["locate@%s/answer_table" % tag] = np.stack(gx.locate(E["locate_rows"]), axis=1)
        gx.accelerate_locate(False)
    gx.accelerate_extract()
    rg = E["ranges"]
    R["extract@%s" % tag] = gx.extract(rg[:, 0], rg[:, 1], rg[:, 2])[0]
    gx.accelerate_extract(False)
    for ks, lut, walk in exact_tables(sigma, wide):
        gx.accelerate(ks, lut_len=lut, walk=walk)
        path = "%s/kstep%d_lut%d_walk%d" % (tag, ks, lut, walk)
        R["exact@" + path], R["exact_steps@" + path] = exact_of(gx, queries)
    gx.accelerate(0)
    R["exact@%s/tables_dropped" % tag], _ = exact_of(gx, queries)
    return R


def compare(R, sigma, where):
    """every array of R against the oracle's; the message lists the kernel paths that differ"""
    E = expected(sigma)
    bad = []
    for name in sorted(R):
        want, got = E[name.split("@")[0]], R[name]
        if got.shape != want.shape:
            bad.append((name, "shape", got.shape, want.shape))
        elif not np.array_equal(got, want):
            bad.append((name, "first differences at", np.argwhere(got != want)[:3].tolist()))
    assert not bad, (where, bad[:12])
    return len(R)


def variant_options(layout, sigma):
    """creation options that put another table under the searches of this layout and alphabet"""
    out = []
    if sigma == 5:
        out += [("no_pair_table", {"pair_table": 0}), ("no_fused_locate", {"fused_locate": 0})]
        if family(layout) != "A":
            out.append(("not_expanded", {"expand_dna": 0, "pair_table": 0}))
    if sigma == 4:
        out.append(("no_fused_locate", {"fused_locate": 0}))
    if 6 <= sigma <= 29 and family(layout) != "A":
        out.append(("no_symbol_planes", {"symbol_planes": 0}))
    return out


def layout_oracle(layout, sigma, dominant=0):
    seqs, ox, arrays = collection(sigma, dominant)
    return ox if layout == "IB16" else fo.OraIndex.from_bwt(layout, sigma, *arrays)


def check_layout(layout, sigma, wide):
    lx = layout_oracle(layout, sigma)
    with fm.options(force_wide=wide):
        gx = fm.BiFMIndex.from_reference_arrays(**oracle_arrays(lx))
    assert gx.row_bits == (64 if wide else 32) and gx.n == N_ROWS
    R = collect(gx, sigma)
    for tag, opts in variant_options(layout, sigma):
        with fm.options(force_wide=wide, **opts):
            vx = fm.BiFMIndex.from_reference_arrays(**oracle_arrays(lx))
        collect_exact_and_locate(vx, sigma, tag, R)
    return R


@gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("sigma", EDGE_SIGMAS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_searches_at_super_block_edges(layout, sigma, wide):
    R = check_layout(layout, sigma, wide)
    assert compare(R, sigma, (layout, sigma, "64-bit rows" if wide else "32-bit rows")) > 40


BUILT = [("IB16", 5), ("IB16", 28), ("IB16", 255), ("WAVELET", 6), ("WAVELET", 21), ("WAVELET", 28)]


def check_built(layout, sigma, wide, sorter=0):
    seqs, _, _ = collection(sigma)
    with fm.options(force_wide=wide, suffix_sorter=sorter, bucket_rows=0 if sorter < 2 else 40_000):
        gx = fm.BiFMIndex.from_sequences(seqs, sigma, layout, 4)
    assert gx.row_bits == (64 if wide else 32) and gx.n == N_ROWS
    return collect(gx, sigma, tag="built%d" % sorter)


@gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("layout,sigma", BUILT)
def test_device_built_index_at_super_block_edges(layout, sigma, wide):
    R = check_built(layout, sigma, wide)
    assert compare(R, sigma, (layout, sigma, "built on the device", "64-bit rows" if wide else "32-bit rows")) > 40


# ------------------------------------------------------------------------------------------------ 3. 64-bit rows on super-blocks of 2^16 rows
DEV_CASES = [("IB16", 5), ("WAVELET", 28), ("EPRV2_16", 6), ("IB16", 255)]
DEV_SHIFT = 16

_CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "oracle"))
import ctypes
import numpy as np
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests import test_gpu_superblocks as t
layout, sigma, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
shift = capi.lib().fmgpu_dev_super_shift()
assert shift == t.DEV_SHIFT and t.N_ROWS >> shift == 2, shift
R = t.check_layout(layout, sigma, 1)
if layout in ("IB16", "WAVELET"):
    for sorter in (1, 2):
        R.update(t.check_built(layout, sigma, 1, sorter))
try:
    fm.BiFMIndex.from_reference_arrays(**t.oracle_arrays(t.layout_oracle(layout, sigma))).save(out + ".idx")
    refused = 0
except fm.FmgpuError as e:
    refused = int(e.code == capi.FMGPU_ERR_UNSUPPORTED)
try:
    fm.FMIndex.load(out + ".idx")
    refused = 0
except fm.FmgpuError as e:
    refused &= int(e.code == capi.FMGPU_ERR_UNSUPPORTED)
R["refuses_files"] = np.array([refused])
np.savez(out, **R)
print("EDGES_DONE", shift, len(R))
"""


@gpu
@pytest.mark.parametrize("layout,sigma", DEV_CASES)
def test_wide_super_blocks_of_2_16_rows(layout, sigma, tmp_path):
    """the check list of part 2 with force_wide = 1 in the development build whose wide super-blocks hold 2^16 rows: 131 371 rows are three of them, so every
    `row >> kSuperShift` of the 64-bit-row kernels takes the values 0, 1 and 2 and the aimed reads stand on both boundaries.  One child process (the library is
    chosen at import); the parent compares what it wrote with the oracle, so a difference names its kernel path"""
    lib = os.path.join(ROOT, "fmindex-collection_amd", "libfmgpu_dev_ss%d.so" % DEV_SHIFT)
    assert os.path.exists(lib), "libfmgpu_dev_ss16.so is not built (make -C fmindex-collection_amd/csrc DEV=1 SUPER_SHIFT=16)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FMGPU_")}
    env["FMGPU_LIBRARY"] = lib
    path = str(tmp_path / "edges.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT), layout, str(sigma), path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "EDGES_DONE %d" % DEV_SHIFT in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = dict(np.load(path))
    assert got.pop("refuses_files")[0] == 1, "the development build with small super-blocks must refuse to write and to read index files"
    assert compare(got, sigma, (layout, sigma, "64-bit rows, super-blocks of 2^16 rows")) > 40
    if layout in ("IB16", "WAVELET"):
        assert any(k.endswith("built2/default") for k in got) and any(k.endswith("built1/default") for k in got)


# ------------------------------------------------------------------------------------------------ 4. the symbol-plane table on super-blocks of 2^16 rows
# In the development build with SUPER_SHIFT = 16 the count fields of Format S are min(shipped width, 16) = 16 bits wide in both row widths (fmgpu_common.h,
# flat_count_bits): 131 371 rows are three of its super-blocks, a count reaches 2^16 - 64, and the aimed reads stand on both boundaries — against the oracle.
# (A 16-bit field never lies in two 32-bit words: the straddling store and load are what tests/test_gpu_symbol_planes.py reaches at the shipped widths.)
PLANES_CASES = {6: ("WAVELET", "EPR16", "EPRV2_16"), 21: ("WAVELET",), 25: ("WAVELET",), 26: ("WAVELET",), 28: ("WAVELET", "EPR16", "EPRV2_16"), 29: ("WAVELET",)}
# the development knobs that choose among result-identical paths of k_exact_s: (environment, lanes of a workgroup, the super table staged in LDS)
PLANES_KNOBS = {"default": ({}, 512, True), "super_through_l2": ({"FMGPU_DEV_FLAT_SUPER_MAX": "0"}, 512, False),
                "lanes_256": ({"FMGPU_DEV_FLAT_LANES": "256"}, 256, True), "lanes_512": ({"FMGPU_DEV_FLAT_LANES": "512"}, 512, True)}


@functools.lru_cache(maxsize=None)
def expected_exact(sigma, dominant=0):
    """the oracle's intervals and step count of the batch: what every path of part 4 must return"""
    _, ox, _ = collection(sigma, dominant)
    lb, ln, st = ox.search_exact(*fm.flatten(batch(sigma, dominant)[0]), want_steps=True)
    return {"exact": np.stack([lb, ln]), "exact_steps": np.array([int(st.sum())], dtype=np.uint64)}


def planes_tables(sigma, wide):
    """an interval table alone in front of the symbol planes (k_exact_s starts from its entry), then the combinations of exact_tables (a k-step table puts Format A under
    the search: the planes must hand over and take back)"""
    return [(0, 1, 0), (0, 2, 0), (0, 3, 0)] + exact_tables(sigma, wide)[:3]


PLANES_PATHS = 2 * 2 + 3 * 2 * 2 + 3 * 2 + 1                          # arrays per handle: (intervals, steps) by 2 selections, 3 x 2 + 3 table paths; tables dropped


def collect_planes(gx, sigma, dominant, tag, R):
    """exact search of the batch by every selection and with interval tables, on a handle that holds the symbol-plane table"""
    assert gx.formats & capi.FMT_PLANES and gx.n == N_ROWS, tag
    queries = fm.flatten(batch(sigma, dominant)[0])
    for name, sel in exact_selections(sigma, gx.row_bits == 64):
        with fm.options(kernel_select=sel):
            R["exact@%s/%s" % (tag, name)], R["exact_steps@%s/%s" % (tag, name)] = exact_of(gx, queries)
    for ks, lut, walk in planes_tables(sigma, gx.row_bits == 64):
        gx.accelerate(ks, lut_len=lut, walk=walk)
        for name, sel in (("", 0), ("_off", capi.SEL_NO_EXACT_LUT)) if ks == 0 else (("", 0),):
            with fm.options(kernel_select=sel):
                path = "%s/kstep%d_lut%d_walk%d%s" % (tag, ks, lut, walk, name)
                R["exact@" + path], R["exact_steps@" + path] = exact_of(gx, queries)
    gx.accelerate(0)
    R["exact@%s/tables_dropped" % tag], _ = exact_of(gx, queries)


def check_planes(sigma, dominant=0):
    """every layout of PLANES_CASES[sigma] in both row widths, from the oracle's arrays and (Wavelet) built on the device by two suffix sorters"""
    R = {}
    seqs, _, _ = collection(sigma, dominant)
    for layout in PLANES_CASES[sigma] if not dominant else ("WAVELET",):
        lx = layout_oracle(layout, sigma, dominant)
        for wide in (0, 1):
            with fm.options(force_wide=wide):
                gx = fm.FMIndex.from_reference_arrays(bwt=oracle_arrays(lx)["bwt"], C_array=oracle_arrays(lx)["C_array"])
                assert gx.row_bits == (64 if wide else 32)
                collect_planes(gx, sigma, dominant, "%s/rows%d/arrays" % (layout, gx.row_bits), R)
                for sorter in (1, 2) if layout == "WAVELET" else ():
                    with fm.options(suffix_sorter=sorter, bucket_rows=0 if sorter < 2 else 40_000):
                        bx = fm.FMIndex.from_sequences(seqs, sigma, layout, 4)
                    collect_planes(bx, sigma, dominant, "%s/rows%d/built%d" % (layout, bx.row_bits, sorter), R)
    return R


_CHILD_PLANES = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "oracle"))
import ctypes as C
import numpy as np
from fmindex_collection_amd import capi
from tests import test_gpu_superblocks as t
sigma, dominant, knob, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
L = capi.lib()
assert L.fmgpu_dev_super_shift() == t.DEV_SHIFT and t.N_ROWS >> t.DEV_SHIFT == 2
R = t.check_planes(sigma, dominant)
lanes, super_lds, bits = C.c_uint32(), C.c_uint32(), C.c_uint32()
launches = L.fmgpu_dev_flat_launch(C.byref(lanes), C.byref(super_lds), C.byref(bits))
R["launch"] = np.array([launches, lanes.value, super_lds.value, bits.value])
np.savez(out, **R)
print("PLANES_DONE", len(R))
"""


def run_planes_child(sigma, dominant, knob, tmp_path):
    """check_planes in a child process that holds the development build with super-blocks of 2^16 rows and the knob's environment; what the child's last k_exact_s
    launch took (fmgpu_dev_flat_launch) is asserted here: the paths a knob chooses among return the same intervals"""
    lib = os.path.join(ROOT, "fmindex-collection_amd", "libfmgpu_dev_ss%d.so" % DEV_SHIFT)
    assert os.path.exists(lib), "libfmgpu_dev_ss16.so is not built (make -C fmindex-collection_amd/csrc DEV=1 SUPER_SHIFT=16)"
    extra, lanes, in_lds = PLANES_KNOBS[knob]
    env = {k: v for k, v in os.environ.items() if not k.startswith("FMGPU_")}
    env.update(extra, FMGPU_LIBRARY=lib)
    path = str(tmp_path / "planes.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD_PLANES % (ROOT, ROOT), str(sigma), str(dominant), knob, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "PLANES_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = dict(np.load(path))
    launches, got_lanes, got_super, got_bits = (int(v) for v in got.pop("launch"))
    nsb = (N_ROWS >> DEV_SHIFT) + 1
    assert launches > 0 and got_lanes == lanes and got_bits == DEV_SHIFT and got_super == (nsb * sigma if in_lds else 0), (knob, launches, got_lanes, got_super, got_bits)
    E = expected_exact(sigma, dominant)
    bad = [(name, np.argwhere(got[name] != E[name.split("@")[0]])[:3].tolist()) for name in sorted(got) if not np.array_equal(got[name], E[name.split("@")[0]])]
    assert not bad, (sigma, dominant, knob, bad[:12])
    return got


@gpu
@pytest.mark.parametrize("knob", list(PLANES_KNOBS))
@pytest.mark.parametrize("sigma", list(PLANES_CASES))
def test_symbol_planes_on_super_blocks_of_2_16_rows(sigma, knob, tmp_path):
    """exact search on Format S with 16-bit count fields and three super-blocks, 32- and 64-bit rows: a Wavelet at sigma = 6, 21, 25, 26, 28, 29 (from the oracle's arrays
    and built on the device), EPR16 and EPRV2_16 blocks at sigma = 6 and 28 — every kernel selection, interval tables in front, against the oracle; then the same list
    with the super table read through L2 and with workgroups of 256 and of 512 lanes forced, one child process each"""
    got = run_planes_child(sigma, 0, knob, tmp_path)
    handles = 2 * (3 + (len(PLANES_CASES[sigma]) - 1))                # per row width: the Wavelet from arrays and built twice, the EPR layouts from arrays
    assert len(got) == handles * PLANES_PATHS, (len(got), handles)
    assert any("rows32/built2/default" in k for k in got) and any("rows64/arrays/on_tree" in k for k in got)


@gpu
@pytest.mark.parametrize("sigma,dominant", SKEWED)
def test_symbol_planes_with_full_count_fields(sigma, dominant, tmp_path):
    """the skewed collection: one symbol holds 90 % of the 131 371 rows, so that its 16-bit count has the top bit set before each of the two boundaries (asserted on
    the oracle's BWT) — the first symbol (its field in the upper half of a word) and the last one (in the lower half); exact search only, both row widths"""
    _, _, arrays = collection(sigma, dominant)
    bwt = arrays[0]
    for b in (1 << DEV_SHIFT, 2 << DEV_SHIFT):
        inside = int(np.count_nonzero(bwt[b - (1 << DEV_SHIFT): b - 64] == dominant))
        assert inside >= 1 << (DEV_SHIFT - 1), (b, inside)
    E = expected_exact(sigma, dominant)["exact"]                     # the batch on the oracle: wide intervals over the boundaries, and single rows
    straddle = sum(int(((E[0] < b) & (b < E[0] + E[1])).sum()) for b in (1 << DEV_SHIFT, 2 << DEV_SHIFT))
    assert straddle >= 100 and int((E[1] == 1).sum()) >= 100, (straddle, int((E[1] == 1).sum()))
    assert len(run_planes_child(sigma, dominant, "default", tmp_path)) == 6 * PLANES_PATHS
