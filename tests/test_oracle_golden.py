"""The oracle (oracle/fmoracle.c) against every golden vector of the reference for this path, against vectors produced by
the real reference headers, and against brute force.  CPU only."""
import json
import os
import zlib

import numpy as np
import pytest

import fmoracle as fo
from tests.util import make_text, occurrences, sample_reads
from tests.golden.make_golden import live_string_cases, string_digests, edge_string_cases, edge_digests

GOLD = os.path.join(os.path.dirname(__file__), "golden")
REF = json.load(open(os.path.join(GOLD, "reference_tests.json")))
REFSTR = json.load(open(os.path.join(GOLD, "ref_strings.json")))
REFSCH = json.load(open(os.path.join(GOLD, "ref_schemes.json")))
REFLIVE = json.load(open(os.path.join(GOLD, "ref_strings_live.json")))["layouts"]
REFEDGES = json.load(open(os.path.join(GOLD, "ref_strings_live_edges.json")))["layouts"]

ALL_LAYOUTS = list(fo.LAYOUTS)


def naive_rank(text, idx, c):
    return int(np.count_nonzero(np.asarray(text[:idx]) == c))


def naive_prefix(text, idx, c):
    return int(np.count_nonzero(np.asarray(text[:idx]) < c))


# ------------------------------------------------------------------------------------------------ strings
@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_hallo_welt_hand_counted(layout):
    """string/unittest.cpp:52-312 — every hand counted rank / prefix_rank value"""
    g = REF["hallo_welt"]
    s = fo.OraString(layout, g["sigma"], g["text"])
    assert s.size() == 10
    for i, c in enumerate(g["text"]):
        assert s.symbol(i) == c
    for idx, sym, val in g["rank"]:
        assert s.rank(idx, sym) == val, (idx, sym)
    for idx, sym, val in g["prefix_rank"]:
        assert s.prefix_rank(idx, sym) == val, (idx, sym)
    for idx in range(10):
        rs, prs = s.all_ranks_and_prefix_ranks(idx)
        for sym in (32, 72, 87, 97, 101, 108, 111, 116, 122):
            assert rs[sym] == s.rank(idx, sym) and prs[sym] == s.prefix_rank(idx, sym)


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_long_text_crossing_255(layout):
    """string/unittest.cpp:314-398 — 310 symbols, naive counts for every idx and symbol"""
    g = REF["long_text"]
    text = np.array(g["text"], dtype=np.uint8)
    s = fo.OraString(layout, g["sigma"], text)
    assert s.size() == len(text) == 310
    for i in range(len(text)):
        assert s.symbol(i) == text[i]
    present = sorted(set(text.tolist())) + [1, 200]
    for idx in range(0, len(text) + 1):
        rs, prs = s.all_ranks_and_prefix_ranks(idx)
        for sym in present:
            assert s.rank(idx, sym) == naive_rank(text, idx, sym) == rs[sym]
            assert s.prefix_rank(idx, sym) == naive_prefix(text, idx, sym) == prs[sym]


@pytest.mark.parametrize("case", REFSTR["cases"], ids=lambda c: f"{c['layout']}-s{c['sigma']}-n{c['n']}")
def test_strings_against_real_reference_vectors(case):
    """tables and layout bytes produced by the REAL reference headers (tests/golden/ref_strings.json)"""
    text = make_text(case["n"], case["sigma"], seed=case["seed"], lo=0)
    s = fo.OraString(case["layout"], case["sigma"], text)
    rk, pr = s.rank_table()
    assert zlib.crc32(rk.tobytes()) == case["rank_crc"]
    assert zlib.crc32(pr.tobytes()) == case["prefix_rank_crc"]
    assert rk[-1].tolist() == case["rank_last_row"] and pr[-1].tolist() == case["prefix_last_row"]
    sym = np.array([s.symbol(i) for i in range(case["n"])], dtype=np.uint8)
    assert zlib.crc32(sym.tobytes()) == case["symbol_crc"] and np.array_equal(sym, text)
    if case["layout"] in fo.HIER_LAYOUTS:
        assert [zlib.crc32(a.tobytes()) for a in s.level_fields()] == case["level_crc"]
        assert [int(a.size) for a in s.level_fields()] == case["level_bytes"]
    elif case["layout"] != "WAVELET":
        assert s.block_stride() == case["block_stride"]
        cnt, words, sup = s.block_fields()
        assert (cnt.shape[0], sup.shape[0]) == (case["n_blocks"], case["n_super"])
        assert zlib.crc32(cnt.tobytes()) == case["counts_crc"]
        assert zlib.crc32(words.tobytes()) == case["words_crc"]
        assert zlib.crc32(sup.tobytes()) == case["super_crc"]
    else:
        nn = 1 << max(1, (case["sigma"] - 1).bit_length())
        crc = [zlib.crc32(b"".join(s.raw(4 * k + j).tobytes() for j in range(4))) for k in range(nn)]
        assert crc == case["node_crc"]
    if case.get("rank_table"):
        assert rk.tolist() == case["rank_table"]


@pytest.mark.parametrize("layout", fo.REF_UNBUILDABLE)
def test_flattened_bitvectors_against_text_counts(layout):
    """FlattenedBitvectors2L.h cannot be compiled here (it includes ../utils.h: libsais, mmser) — the restatement is pinned by the
    reference's String unit-test vectors above (hallo welt, 310 symbols) and by counting in the text, around the 512 / 2048 / 65 536
    block edges; its array layout is restated from the source text only (parity of the BYTES unpinned)."""
    rng = np.random.default_rng(7)
    for sigma, n in ((5, 0), (5, 1), (5, 513), (5, 2048), (5, 66000), (28, 2100), (256, 700), (2, 130), (28, 2 * 65536 + 300)):
        text = rng.integers(0, sigma, size=n, dtype=np.uint8)
        s = fo.OraString(layout, sigma, text)
        l1_bits = int(layout.split("_")[1]); bitct = max(1, (sigma - 1).bit_length())
        bits, l0, l1 = s.raw(0), s.raw(1), s.raw(2)
        nsuper = n // 65536 + 1
        assert l0.size == nsuper * (sigma + 1) * 8 and l1.size == nsuper * (65536 // l1_bits) * (sigma + 1) * 2
        assert bits.size == nsuper * (65536 // l1_bits) * bitct * l1_bits // 8
        for i in (list(range(n + 1)) if n <= 2100 else list(range(0, n + 1, 1021)) + [n, 65535, 65536, 65537] + [131071, 131072, 131073] * (n > 131073)):
            for c in range(0, sigma, 1 if sigma <= 28 else 51):
                assert s.rank(i, c) == naive_rank(text, i, c) and s.prefix_rank(i, c) == naive_prefix(text, i, c)


@pytest.mark.parametrize("layout", [l for l in ALL_LAYOUTS if l not in fo.REF_UNBUILDABLE])
def test_strings_live_against_real_reference(layout):
    """comparison with the answers of the reference headers compiled in place (recorded in ref_strings_live.json by make_golden.py), incl. the
    16-bit super-block boundaries: the block arrays (shape and values), rank and prefix_rank at every probed index and symbol, every symbol"""
    want = REFLIVE[layout]
    got = [(sigma, n, string_digests(fo.OraString(layout, sigma, text), layout, sigma, n, idxs)) for sigma, n, text, idxs in live_string_cases(layout)]
    assert [(w["sigma"], w["n"]) for w in want] == [(sigma, n) for sigma, n, _ in got]
    for w, (sigma, n, d) in zip(want, got):
        for k in ("blocks", "rank", "prefix_rank", "symbol"):
            assert d.get(k) == w.get(k), (layout, sigma, n, k)


@pytest.mark.parametrize("layout", [l for l in ALL_LAYOUTS if l not in fo.REF_UNBUILDABLE])
def test_strings_live_edges_against_real_reference(layout):
    """the same comparison at the super-block boundaries of every layout and alphabets of 4, 6, 21, 28 and 255 symbols (ref_strings_live_edges.json): sizes P - 1,
    P, P + 1 and 2 P + 300 around the layout's super-block period P, rows beside every boundary and row n — rank and prefix_rank symbol by symbol,
    the ranks of all_ranks_and_prefix_ranks and symbol.  At n = k P the reference's own rank(n, .) counts the closed super-block twice: pinned as it is"""
    want = REFEDGES[layout]
    got = [(sigma, n, edge_digests(fo.OraString(layout, sigma, text), sigma, n, rows, symbols)) for sigma, n, text, rows, symbols in edge_string_cases(layout)]
    assert [(w["sigma"], w["n"]) for w in want] == [(sigma, n) for sigma, n, _ in got]
    for w, (sigma, n, d) in zip(want, got):
        for k in ("rank", "prefix_rank", "all_ranks", "symbol"):
            assert d[k] == w[k], (layout, sigma, n, k)


# ------------------------------------------------------------------------------------------------ search schemes
def _eq(a, b):
    return all(np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y) for x, y in zip(a, b))


def test_schemes_against_real_reference_vectors():
    for g in REFSCH["h2"]:
        s = fo.scheme_h2(g["N"], g["minK"], g["K"])
        assert _eq(s, (g["pi"], g["l"], g["u"])), g
        assert fo.scheme_is_valid(s) == g["valid"] and fo.scheme_is_complete(s, g["minK"], g["K"]) == g["complete"]
        assert fo.scheme_node_count_hamming(s, 5) == pytest.approx(g["nodeCount_sigma5"], rel=1e-12)
    for name, fn in (("pigeon_opt", fo.scheme_pigeon_opt), ("pigeon_trivial", fo.scheme_pigeon_trivial)):
        for g in REFSCH[name]:
            s = fn(g["minK"], g["K"])
            assert _eq(s, (g["pi"], g["l"], g["u"])) and fo.scheme_is_complete(s, g["minK"], g["K"]) == g["complete"]
    for g in REFSCH["backtracking"]:
        assert _eq(fo.scheme_backtracking(g["N"], g["minK"], g["K"]), (g["pi"], g["l"], g["u"]))
    for g in REFSCH["expand"]:
        e = fo.scheme_expand(fo.scheme_h2(g["N"], 0, g["K"]), g["len"])
        assert e[0].shape[0] == g["searches"] and zlib.crc32(b"".join(x.tobytes() for x in e)) == g["crc"], g
        h = fo.scheme_limit_to_hamming(e)
        assert zlib.crc32(b"".join(x.tobytes() for x in h)) == g["hamming_crc"]
    for g in REFSCH["limitToHamming"]:
        h = fo.scheme_limit_to_hamming(fo.scheme_h2(g["N"], 0, g["K"]))
        assert h[1].tolist() == g["l"] and h[2].tolist() == g["u"]
    for g in REFSCH["partition"]:
        assert fo.uniform_partition(g["parts"], g["total"]).tolist() == g["out"]


def test_scheme_reference_test_cases():
    """search_scheme/expand.cpp:11-60 and checkGeneratorsIsComplete.cpp:48-60"""
    for c in REF["expand"]["cases"]:
        sch = tuple(np.array([x], dtype=np.uint64) for x in c["in"])
        e = fo.scheme_expand(sch, c["len"])
        assert fo.scheme_is_valid(e) and _eq(e, tuple(np.array([x], dtype=np.uint64) for x in c["out"]))
    for N in range(1, 10):
        for minK in range(0, min(N, 5)):
            for maxK in range(minK, min(N, 5)):
                assert fo.scheme_is_complete(fo.scheme_h2(N, minK, maxK), minK, maxK), (N, minK, maxK)


# ------------------------------------------------------------------------------------------------ index fixtures
def _sampled_index(layout, g, rule, bidir):
    bwt, sa = np.array(g["bwt"], dtype=np.uint8), np.array(g["sa"], dtype=np.uint64)
    has = np.array([rule(i, int(sa[i])) for i in range(len(sa))], dtype=np.uint8)
    rev = np.array(g["bwtRev"], dtype=np.uint8) if bidir else None
    return fo.OraIndex.from_bwt(layout, g["sigma"], bwt, rev, has, np.zeros(len(sa), dtype=np.uint64), sa), has, sa


SAMPLINGS = {"full": lambda i, s: True, "every2nd_row": lambda i, s: i % 2 == 0 or s == 0, "odd_rows": lambda i, s: i % 2 == 1,
             "every2nd_text": lambda i, s: s % 2 == 0}


@pytest.mark.parametrize("layout", ["IB16", "IBP16", "EPR16", "EPRV2_16", "WAVELET"])
@pytest.mark.parametrize("fixture,bidir", [("fmindex_hallo", False), ("bifmindex_hallo", True), ("bifmindex_long", True)])
def test_index_locate_fixtures(layout, fixture, bidir):
    """fmindex/checkFMIndex.cpp:15-110, fmindex/checkBiFMIndex.cpp:13-105, :136-222"""
    g = REF[fixture]
    for name, rule in SAMPLINGS.items():
        if fixture == "bifmindex_long" and name == "odd_rows":
            continue
        x, has, sa = _sampled_index(layout, g, rule, bidir)
        assert x.n == len(sa)
        for i in range(len(sa)):
            seq, pos, off = x.locate(i)
            assert seq == 0 and pos + off == sa[i], (name, i)
            step = x.single_locate_step(i)
            assert (step == (0, int(sa[i]))) if has[i] else (step is None)
            if name == "full":
                assert off == 0


@pytest.mark.parametrize("bidir", [False, True])
def test_cursor_fixture(bidir):
    """fmindex/checkFMIndexCursor.cpp:13-66, fmindex/checkBiFMIndexCursor.cpp:12-103"""
    g = REF["cursor"]
    x = fo.OraIndex.build("IB16", g["sigma"], g["data"], g["sampling_rate"], bidir)
    cur = x.cursor()
    assert (cur.lb, cur.len) == (0, x.n) and x.n == 8
    left_all = x.extend_left_all(cur)
    for sym, count, lb in g["extend"]:
        c = x.extend_left(cur, sym)
        assert (c.len, c.lb) == (count, lb)
        if bidir:
            c = x.extend_right(cur, sym)
            assert (c.len, c.lb) == (count, lb)
    for sym in range(g["sigma"]):
        c = x.extend_left(cur, sym)
        assert (c.lb, c.len) == (left_all[sym].lb, left_all[sym].len)
    if bidir:
        right_all = x.extend_right_all(cur)
        for sym in range(g["sigma"]):
            c = x.extend_right(cur, sym)
            assert (c.lb, c.len) == (right_all[sym].lb, right_all[sym].len)


def _located(x, hits):
    out = []
    for h in hits:
        for r in range(int(h["lb"]), int(h["lb"] + h["len"])):
            s, p, o = x.locate(r)
            out.append([int(h["qidx"]), s, p + o])
    return sorted(out)


def test_search_fixtures():
    """search/checkSearches.cpp:23-72, :104-117, :1482-1505; search/checkSearchBacktracking.cpp:295-327"""
    g = REF["searches"]
    qbuf, qoff = fo.flatten_queries(g["queries"])
    for bidir in (False, True):
        x = fo.OraIndex.build("IB16", g["sigma"], g["input"], g["sampling_rate"], bidir)
        hits, _ = x.search_backtracking(qbuf, qoff, 1)
        assert _located(x, hits) == g["backtracking_k1"]
        lb, ln = x.search_exact(qbuf, qoff)
        assert ln.tolist() == [0, 0] and g["no_errors"] == []
    x = fo.OraIndex.build("IB16", g["sigma"], g["input"], g["sampling_rate"], True)
    # fmc::search<false>(index, queries, 1, ...): h2(2, 0, 1) for length-2 queries + limitToHamming (CachedSearchScheme.h:26-30)
    sch = fo.scheme_limit_to_hamming(fo.scheme_h2(2, 0, 1))
    hits, _, _ = x.search_ng26(qbuf, qoff, sch)
    assert _located(x, hits) == g["hamming_k1_facade"]
    hits, _, _ = x.search_ng26(qbuf, qoff, fo.scheme_pigeon_opt(0, 1))
    assert _located(x, hits) == g["backtracking_k1"]


def test_collection_fixture():
    """search/checkSearchBacktracking.cpp:12-40, :42-102 — BWT rows, 'A' interval and the locate table"""
    for key in ("collection", "single"):
        g = REF[key]
        x = fo.OraIndex.build("IB16", g["sigma"], g["input"], g["sampling_rate"], True)
        assert [x.bwt_string().symbol(i) for i in range(x.n)] == g["bwt"]
        qbuf, qoff = fo.flatten_queries([[ord("A")]])
        hits, _ = x.search_backtracking(qbuf, qoff, 0)
        assert len(hits) == 1 and (hits[0]["lb"], hits[0]["len"], hits[0]["errors"]) == (g["query_A"]["lb"], g["query_A"]["count"], 0)
        if "locate" in g:
            for i, (seq, pos) in enumerate(g["locate"]):
                s, p, o = x.locate(i)
                assert (s, p + o) == (seq, pos)


# ------------------------------------------------------------------------------------------------ brute force
def _concat(seqs):
    t = []
    for s in seqs:
        t += list(s) + [0]
    return np.array(t, dtype=np.uint8)


@pytest.mark.parametrize("layout", ["IB16", "EPR16", "EPRV2_16", "WAVELET", "IBP16"])
def test_exact_intervals_match_text_scan(layout):
    rng = np.random.default_rng(5)
    seqs = [rng.integers(1, 5, size=n, dtype=np.uint8) for n in (700, 45, 1300)]
    seqs[1][:20] = seqs[0][100:120]                       # shared substrings -> multi-occurrence intervals
    x = fo.OraIndex.build(layout, 5, seqs, 4, True)
    text = _concat(seqs)
    queries = [text[s: s + m] for s, m in ((3, 5), (100, 20), (100, 12), (742, 3), (800, 40))] + [np.array([1, 2, 3, 4, 1, 1, 1, 2, 2], dtype=np.uint8)]
    qbuf, qoff = fo.flatten_queries(queries)
    lb, ln = x.search_exact(qbuf, qoff)
    for q, query in enumerate(queries):
        pos, _ = occurrences(text, query)
        pos = [p for p in pos if 0 not in text[p: p + len(query)]]
        assert ln[q] == len(pos)
        found = sorted(x.locate(int(r))[1] + x.locate(int(r))[2] + int(np.cumsum([0] + [len(s) + 1 for s in seqs])[x.locate(int(r))[0]]) for r in range(int(lb[q]), int(lb[q] + ln[q])))
        assert found == sorted(int(p) for p in pos)


@pytest.mark.parametrize("layout,batch,threads", [("IB16", 32, 1), ("WAVELET", 7, 3), ("EPRV5", 1, 2), ("IB16", 300, 2)])
def test_batched_exact_search_equals_one_at_a_time(layout, batch, threads):
    """search/SearchNoErrors.h:28-86 (round-robin over a batch of cursors) answers what :12-26 answers, ragged and empty queries included"""
    rng = np.random.default_rng(77)
    text = rng.integers(1, 5, size=30000, dtype=np.uint8)
    x = fo.OraIndex.build(layout, 5, [text], 8, False)
    queries = []
    for i in range(9000):
        m = int(rng.integers(0, 60))
        s = int(rng.integers(0, len(text) - 60))
        q = text[s: s + m].copy()
        if m and i % 3 == 0:
            q[int(rng.integers(0, m))] = rng.integers(1, 5)
        queries.append(q)
    qbuf, qoff = fo.flatten_queries(queries)
    lb, ln = x.search_exact(qbuf, qoff)
    blb, bln = x.search_exact_batched(qbuf, qoff, batch, threads)
    assert np.array_equal(ln, bln) and np.array_equal(lb, blb)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ng26_equals_backtracking_equals_text_scan(k):
    """h2(k+2, 0, k) with a uniform partition is complete and non-redundant: same multiset as naive backtracking and as a
    scan of the text (the explicit-scheme overload is the k-mismatch contract)"""
    rng = np.random.default_rng(100 + k)
    base = rng.integers(1, 5, size=400, dtype=np.uint8)
    seqs = [np.concatenate([base, base[50:250], rng.integers(1, 5, size=300, dtype=np.uint8)]), base[::-1].copy()]
    text = _concat(seqs)
    x = fo.OraIndex.build("IB16", 5, seqs, 1, True)
    queries = []
    for i in range(60):
        m = int(rng.integers(k + 2, 40))
        s = int(rng.integers(0, len(seqs[0]) - m))
        q = seqs[0][s: s + m].copy()
        for _ in range(int(rng.integers(0, k + 2))):
            q[int(rng.integers(0, m))] = rng.integers(1, 5)
        queries.append(q)
    qbuf, qoff = fo.flatten_queries(queries)
    sch = fo.scheme_h2(k + 2, 0, k)
    nh, qc, _ = x.search_ng26(qbuf, qoff, sch)
    bh, _ = x.search_backtracking(qbuf, qoff, k)
    key = lambda h: sorted(zip(h["qidx"].tolist(), h["lb"].tolist(), h["len"].tolist(), h["errors"].tolist()))
    assert key(nh) == key(bh)
    assert qc.sum() == len(nh)
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs])
    for q, query in enumerate(queries):
        pos, mism = occurrences(text, query, k)
        ok = [(int(p), int(e)) for p, e in zip(pos, mism) if 0 not in text[p: p + len(query)]]
        got = []
        for h in nh[nh["qidx"] == q]:
            for r in range(int(h["lb"]), int(h["lb"] + h["len"])):
                s, p, o = x.locate(r)
                got.append((int(starts[s]) + p + o, int(h["errors"])))
        assert sorted(got) == sorted(ok), q


# ------------------------------------------------------------------------------------------------ edit distance
def test_edit_distance_fixtures():
    """search/checkSearches.cpp:1093-1121, :1148-1171 (search_ng26::search, Edit = true by default, pigeon_opt(0,1)) and :1422-1466
    (fmc::search<true> / search_n<true>: h2(2,0,1) for length-2 queries, CachedSearchScheme.h:16-36): same located multiset"""
    g = REF["searches_edit"]
    x = fo.OraIndex.build("IB16", g["sigma"], g["input"], g["sampling_rate"], True)
    for key, sch in (("ng26_pigeon_opt_CD_DB", fo.scheme_pigeon_opt(0, 1)), ("ng26_pigeon_opt_n3", fo.scheme_pigeon_opt(0, 1)),
                     ("facade_k1", fo.scheme_h2(2, 0, 1)), ("facade_k1_n3", fo.scheme_h2(2, 0, 1))):
        c = g[key]
        qbuf, qoff = fo.flatten_queries(c["queries"])
        hits, _, _ = x.search_ng26(qbuf, qoff, sch, max_hits=c.get("n", fo.UINT64_MAX), edit=True)
        assert _located(x, hits) == c["expected"], key


REF_SEARCH = np.load(os.path.join(GOLD, "ref_search_intervals.npz"))
from tests.golden.make_golden import REF_SEARCH_CASES  # noqa: E402  (the case table: layout, sigma, text size and seed, reads)


@pytest.mark.parametrize("name", sorted(REF_SEARCH_CASES))
def test_search_intervals_from_the_real_reference_rank(name):
    """tests/golden/ref_search_intervals.npz was computed by backward search over the REAL reference's rank functions
    (tests/golden/make_golden.py::ref_search_intervals; config0_ib16 = BASELINE.json configs[0]); the restatement's searches — one query at
    a time and the 32-way interleaved form — must reproduce every (lb, len), on the restatement of the same occurrence-table layout"""
    layout, sigma, tn, seed, nreads, rl = REF_SEARCH_CASES[name]
    want = REF_SEARCH[name]
    text = make_text(tn, sigma, seed=seed)
    x = fo.OraIndex.build(layout, sigma, [text], 16, False)
    qbuf, qoff = fo.flatten_queries(sample_reads(text, nreads, rl, seed=1, mutate=1, sigma=sigma))
    lb, ln = x.search_exact(qbuf, qoff, nthreads=4)
    assert np.array_equal(ln, want[:, 1]) and np.array_equal(lb, want[:, 0])
    blb, bln = x.search_exact_batched(qbuf, qoff, 32, 4)
    assert np.array_equal(bln, want[:, 1]) and np.array_equal(blb, want[:, 0])
    assert int((want[:, 1] > 0).sum()) >= len(want) // 2


def test_ng21_fixtures():
    """search/checkSearches.cpp:422-525: search_ng21::search / search_n / search_best / search_best_n over expand(pigeon_opt(..), 2)"""
    g = REF["searches_ng21"]
    x = fo.OraIndex.build("IB16", g["sigma"], g["input"], g["sampling_rate"], True)
    qbuf, qoff = fo.flatten_queries(g["queries"])
    m = len(g["queries"][0])
    ex = lambda a: fo.scheme_expand(fo.scheme_pigeon_opt(*a), m)
    hits, _, _ = x.search_ng21(qbuf, qoff, ex(g["search"]["scheme"]))
    assert _located(x, hits) == g["search"]["expected"]
    hits, _, _ = x.search_ng21(qbuf, qoff, ex(g["search_n"]["scheme"]), max_hits=g["search_n"]["n"])
    assert _located(x, hits) == g["search_n"]["expected"]
    hits, _ = x.search_ng21_best(qbuf, qoff, [ex(a) for a in g["search_best"]["schemes"]])
    assert _located(x, hits) == g["search_best"]["expected"]
    hits, _ = x.search_ng21_best(qbuf, qoff, [ex(a) for a in g["search_best_n"]["schemes"]], max_hits=g["search_best_n"]["n"])
    assert _located(x, hits) == g["search_best_n"]["expected"]


@pytest.mark.parametrize("k", [1, 2])
def test_ng21_sound_and_covering(k):
    """search_ng21 reports cursors of alignments with at most k edits: every reported occurrence is within its error count of the query,
    and every text substring within edit distance k has a reported occurrence starting at most k positions away (it prunes equivalent
    alignments like search_ng26<Edit = true>, SearchNg21.h:97-98)"""
    rng = np.random.default_rng(70 + k)
    seqs = [rng.integers(1, 5, size=260, dtype=np.uint8), rng.integers(1, 5, size=120, dtype=np.uint8)]
    text = _concat(seqs)
    x = fo.OraIndex.build("IB16", 5, seqs, 1, True)
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs])
    m = 12
    queries = []
    for i in range(25):
        p = int(rng.integers(0, len(seqs[0]) - m - 2)); q = list(seqs[0][p: p + m + 2])
        for _ in range(int(rng.integers(0, k + 1))):
            op = int(rng.integers(0, 3)); at = int(rng.integers(1, m - 1))
            if op == 0: q[at] = int(rng.integers(1, 5))
            elif op == 1: del q[at]
            else: q.insert(at, int(rng.integers(1, 5)))
        queries.append(np.array(q[:m], dtype=np.uint8))
    qbuf, qoff = fo.flatten_queries(queries)
    hits, _, _ = x.search_ng21(qbuf, qoff, fo.scheme_expand(fo.scheme_pigeon_opt(0, k), m))
    found = {}
    for h in hits:
        for r in range(int(h["lb"]), int(h["lb"] + h["len"])):
            s_, p_, o_ = x.locate(r)
            at = int(starts[s_]) + p_ + o_
            e = int(h["errors"])
            assert e <= k
            assert any(at + ln <= len(text) and 0 not in text[at: at + ln] and _edit_distance(list(queries[int(h["qidx"])]), list(text[at: at + ln])) <= e
                       for ln in range(max(1, m - e), m + e + 1)), (h, at)
            found.setdefault(int(h["qidx"]), set()).add(at)
    for qi, q in enumerate(queries):
        for at in range(len(text)):
            for ln in range(m - k, m + k + 1):
                sub = text[at: at + ln]
                if len(sub) == ln and 0 not in sub and _edit_distance(list(q), list(sub)) <= k:
                    assert any(abs(at - f) <= k for f in found.get(qi, ())), (qi, at, ln)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ng26_full_state_machine_equals_hamming_reduction(k):
    """the line-by-line restatement (nge_*, Edit = false) and the Hamming reduction of SURVEY appendix A (ng_*) agree hit by hit,
    in callback order, and in the number of cursor extensions"""
    rng = np.random.default_rng(k)
    base = rng.integers(1, 5, size=500, dtype=np.uint8)
    seqs = [np.concatenate([base, base[100:300]]), rng.integers(1, 5, size=200, dtype=np.uint8)]
    x = fo.OraIndex.build("IB16", 5, seqs, 2, True)
    queries = []
    for i in range(150):
        m = int(rng.integers(k + 2, 45)); p = int(rng.integers(0, len(seqs[0]) - m)); q = seqs[0][p: p + m].copy()
        for _ in range(int(rng.integers(0, k + 2))):
            q[int(rng.integers(0, m))] = rng.integers(1, 5)
        queries.append(q)
    qbuf, qoff = fo.flatten_queries(queries)
    for sch in (fo.scheme_h2(k + 2, 0, k), fo.scheme_pigeon_opt(0, k), fo.scheme_backtracking(2, 0, k)):
        for n in (fo.UINT64_MAX, 2):
            a, qa, na = x.search_ng26(qbuf, qoff, sch, max_hits=n)
            b, qb, nb = x.search_ng26(qbuf, qoff, sch, max_hits=n, edit=False)
            assert a.tobytes() == b.tobytes() and np.array_equal(qa, qb) and na == nb


def _edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


@pytest.mark.parametrize("k", [1, 2])
def test_edit_distance_sound_and_covering(k):
    """Edit = true reports cursors, not alignments, and prunes equivalent alignments (SearchNg26.h:146-147, :103: no deletion /
    substitution at either end), so the checkable properties are: every reported occurrence lies within its reported error count of
    the query for some length in [m - e, m + e]; and every text substring within edit distance k of the query has a reported
    occurrence starting at most k positions away."""
    rng = np.random.default_rng(40 + k)
    seqs = [rng.integers(1, 5, size=260, dtype=np.uint8), rng.integers(1, 5, size=120, dtype=np.uint8)]
    text = _concat(seqs)
    x = fo.OraIndex.build("IB16", 5, seqs, 1, True)
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs])
    queries = []
    for i in range(25):
        m = int(rng.integers(k + 3, 16)); p = int(rng.integers(0, len(seqs[0]) - m - 2)); q = list(seqs[0][p: p + m])
        for _ in range(int(rng.integers(0, k + 1))):
            op = int(rng.integers(0, 3)); j = int(rng.integers(0, len(q)))
            if op == 0: q[j] = int(rng.integers(1, 5))
            elif op == 1: q.insert(j, int(rng.integers(1, 5)))
            elif len(q) > k + 3: del q[j]
        queries.append(np.array(q, dtype=np.uint8))
    qbuf, qoff = fo.flatten_queries(queries)
    hits, _, _ = x.search_ng26(qbuf, qoff, fo.scheme_h2(k + 2, 0, k), edit=True)
    assert len(hits) > 0
    for qi, q in enumerate(queries):
        m = len(q)
        rep = []
        for h in hits[hits["qidx"] == qi]:
            e = int(h["errors"])
            assert e <= k
            for r in range(int(h["lb"]), int(h["lb"] + h["len"])):
                s, p, o = x.locate(r)
                g = int(starts[s]) + p + o
                rep.append(g)
                best = min(_edit_distance(list(text[g: g + L]), list(q)) for L in range(max(0, m - e), m + e + 1) if g + L <= len(text))
                assert best <= e, (qi, g, e, best)
        rep = set(rep)
        for g in range(len(text)):
            for L in range(max(1, m - k), m + k + 1):
                sub = text[g: g + L]
                if len(sub) < L or 0 in sub:
                    continue
                if _edit_distance(list(sub), list(q)) <= k:
                    assert any(abs(g - r) <= k for r in rep), (qi, g, L)


def test_search_n_clips_like_the_reference():
    """search_ng26 search_n semantics (SearchNg26.h:407-423): stop after exactly n rows, clip the last cursor"""
    seqs = [np.array([1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 3], dtype=np.uint8)]
    x = fo.OraIndex.build("IB16", 5, seqs, 1, True)
    qbuf, qoff = fo.flatten_queries([[1, 2], [2, 1, 2]])
    sch = fo.scheme_pigeon_opt(0, 1)
    full, _, _ = x.search_ng26(qbuf, qoff, sch)
    for n in (1, 2, 3, 5, 100):
        hits, qc, _ = x.search_ng26(qbuf, qoff, sch, max_hits=n)
        for q in range(2):
            tot_full = int(full[full["qidx"] == q]["len"].sum())
            assert int(hits[hits["qidx"] == q]["len"].sum()) == min(n, tot_full)


def test_suffix_array_and_bwt_small():
    text = np.array([2, 1, 3, 1, 2, 1, 0, 2, 1, 0], dtype=np.uint8)
    sa = np.zeros(len(text), dtype=np.uint64)
    assert fo.lib().ora_suffix_array(fo._p8(text), len(text), fo._p64(sa)) == 0
    naive = sorted(range(len(text)), key=lambda i: bytes(text[i:].tolist()))
    assert sa.tolist() == naive


# ------------------------------------------------------------------------------------------------ the sampled suffix array's parts, from the reference's own tests
@pytest.mark.parametrize("which", ["dense_vector", "dense_multi_vector"])
def test_dense_vector_reference_cases(which):
    """checkDenseVector.cpp:8-82, checkDenseMultiVector.cpp:8-89 — every value reads back, for vectors made from a list (largest value and gcd taken from the
    values), with a given largest value and divisor + push_back, and by concat (divisor = gcd of both sides': 5 where the test asserts it)"""
    for c in REF[which]["cases"]:
        if c["concat"]:
            left, right = fo.OraDenseVector(c["inputs"][0]), fo.OraDenseVector(c["inputs"][1])
            v = fo.OraDenseVector.concat(left, right)
            want = c["inputs"][0] + c["inputs"][1]
        elif "largest_divisor" in c:
            v = fo.OraDenseVector(c["inputs"][0], *c["largest_divisor"])
            want = c["inputs"][0]
            assert v.common_divisor == c["largest_divisor"][1] and v.bits == (c["largest_divisor"][0] // c["largest_divisor"][1]).bit_length()
        else:
            v = fo.OraDenseVector(c["inputs"][0])
            want = c["inputs"][0]
            assert v.common_divisor == int(np.gcd.reduce(np.array(want, dtype=np.int64))) and v.bits == (max(want) // v.common_divisor).bit_length()
        assert len(v) == len(want) and [v[i] for i in range(len(want))] == want, c["name"]
        if "common_divisor" in c:
            assert v.common_divisor == c["common_divisor"], c["name"]
    # the same values as the two fields of a SparseArray (what an index holds): every second row carries (a, b)
    a, b = REF[which]["cases"][1]["inputs"][0], REF[which]["cases"][2]["inputs"][0]
    has = np.zeros(2 * len(a), dtype=np.uint8); has[::2] = 1
    sp = fo.OraSparse(has, np.repeat(a, 2), np.repeat(b, 2))
    assert [sp.value(2 * i) for i in range(len(a))] == list(zip(a, b)) and all(sp.value(2 * i + 1) is None for i in range(len(a)))


def test_bitvector2l_reference_vectors():
    """bitvector/unittest.cpp:14-140 (run there over Bitvector2L_512_64k, the presence bitvector of the sampled suffix array): symbol and rank of the 14-bit text,
    rank at every checked index of the 512-bit text (rank(512) is the first to read an L1 counter other than block 0's)"""
    g = REF["bitvector"]
    sp = fo.OraSparse(g["short"]["bits"])
    for i, v in g["short"]["symbol"]:
        assert (sp.value(i) is not None) == bool(v)
    for i, v in g["short"]["rank"]:
        assert sp.rank(i) == v, i
    bits = g["long"]["bits"]
    sp = fo.OraSparse(bits + [0] * 8)                               # (rank(512) needs a 513th position: the reference's Bitvector2L always holds one more block)
    assert len(bits) == 512 and len(g["long"]["rank"]) == 32 * 17
    for i, v in enumerate(bits):
        assert (sp.value(i) is not None) == bool(v)
    for i, v in g["long"]["rank"]:
        assert sp.rank(i) == v, i


def test_csa_reference_vectors():
    """suffixarray/checkCSA.cpp:9-81: the suffix array of Hello$World$ and, for sampling rates 3, 4, 5 and 8, which rows carry a value and the (sequence,
    position) they answer — through the oracle's suffix sorter, its SparseArray and the LF walk of locate for the rows in between"""
    g = REF["csa"]
    seqs = [np.array(s_, dtype=np.uint8) for s_ in g["sequences"]]
    text = np.concatenate([np.concatenate([s_, [0]]) for s_ in seqs]).astype(np.uint8)
    sa = np.zeros(len(text), dtype=np.uint64)
    assert fo.lib().ora_suffix_array(fo._p8(text), len(text), fo._p64(sa)) == 0 and sa.tolist() == g["sa"]
    starts = np.concatenate([[0], np.cumsum([len(s_) + 1 for s_ in seqs])])
    seq_of = np.searchsorted(starts, sa, side="right") - 1
    pos_of = sa - starts[seq_of]
    bwt = text[(sa.astype(np.int64) - 1) % len(text)]
    for rate, rows in g["sampling"].items():
        has = (pos_of % int(rate) == 0).astype(np.uint8)
        assert sorted(r for r, _, _ in rows) == np.nonzero(has)[0].tolist(), rate      # the reference samples exactly the rows whose position is a multiple of the rate
        sp = fo.OraSparse(has, seq_of, pos_of)
        for r, s_, p_ in rows:
            assert sp.value(r) == (s_, p_), (rate, r)
        x = fo.OraIndex.from_bwt("IB16", g["sigma"], bwt, None, has, seq_of.astype(np.uint64), pos_of.astype(np.uint64))
        for r in range(len(sa)):
            s_, p_, st = x.locate(r)
            assert (s_, p_ + st) == (int(seq_of[r]), int(pos_of[r])), (rate, r)


def test_scheme_counts_and_validity_reference_cases():
    """search_scheme/nodeCount.cpp:13-34, isValid.cpp:10-65, isComplete.cpp:10-35, checkGenerators.cpp:21-132 through the oracle's restatements"""
    g = REF["node_count"]
    for n in range(g["zero_errors"]["n_from"], g["zero_errors"]["n_to"] + 1, 7):
        assert fo.scheme_node_count_hamming(fo.scheme_backtracking(n, 0, 0), g["sigma"]) == n
        assert fo.scheme_node_count_hamming(fo.scheme_expand(fo.scheme_backtracking(1, 0, 0), n), g["sigma"]) == n
    for count, N, minK, K, sigma in g["known"]:
        assert fo.scheme_node_count_hamming(fo.scheme_backtracking(N, minK, K), sigma) == count
    as_scheme = lambda c: tuple(np.array([c[k]], dtype=np.uint64) for k in ("pi", "l", "u"))
    for c in REF["is_valid"]["cases"]:
        assert bool(fo.scheme_is_valid(as_scheme(c))) == c["expected"], c
    for c in REF["is_complete"]["cases"]:
        assert bool(fo.scheme_is_complete(as_scheme(c), *c["args"])) == c["expected"], c
    gv = REF["generators_valid"]
    for N in range(gv["backtracking"]["N"][0], gv["backtracking"]["N"][1] + 1):
        for minK in range(0, 10):
            for maxK in range(minK, 10):
                assert fo.scheme_is_valid(fo.scheme_backtracking(N, minK, maxK))
        for minK in range(0, min(N, 10)):
            for maxK in range(minK, min(N, 10)):
                assert fo.scheme_is_valid(fo.scheme_h2(N, minK, maxK)), (N, minK, maxK)
    for minK in range(0, 20):
        for maxK in range(minK, 20):
            assert fo.scheme_is_valid(fo.scheme_pigeon_trivial(minK, maxK)) and fo.scheme_is_valid(fo.scheme_pigeon_opt(minK, maxK))
