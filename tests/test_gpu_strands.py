"""The both-strand calls on the device (include/fmgpu.h): fmgpu_queries_strands against the NumPy restatement, the pair ladder against tests/strands_model.py fed from
the single-scheme calls, fmgpu_map_strands against fmgpu_map on the doubled batch and against search_best_pairs -> hits_sort -> locate_hits, and the two feed calls
against fmgpu_map_strands.  Expected values come only from existing calls and the NumPy model.  Run with -m gpu on an MI355X.

The text: make_text(6000, 5) with a palindrome A + revcomp(A) planted (both strands of that read are found at stratum 0) and, for a 40-symbol segment X of the text
and X' = X with two substitutions, revcomp(X') planted elsewhere: read X' is found forward only at stratum 2 and on strand 1 at stratum 0 — where the pair ladder and
the independent ladder must differ.  The read of 5 000 symbols (several blocks of the strands kernel) is part of the strands batches and of the exact-kind map; the
ladders run on the reads of up to 70 symbols."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, POSITION_DTYPE
from tests import strands_model as model
from tests.util import make_text

pytestmark = pytest.mark.gpu
UNLIMITED = fm.UINT64_MAX
DNA5 = np.array([0, 4, 3, 2, 1], dtype=np.uint8)
BLOCK_LEN = 30
LENGTHS = [0, 0, 1, 2, 3, 7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 55, 60, 63, 64, 65, 66, 67, 68, 69, 70, 70, 70, 5, 9, 11, 13, 21, 27, 39, 43, 58, 40, 36, 24]


def revcomp(r):
    table = np.arange(256, dtype=np.uint8)
    table[:5] = DNA5
    return table[np.asarray(r, dtype=np.uint8)[::-1]]


@functools.lru_cache(maxsize=None)
def text():
    """(the indexed text, the palindrome read, the read X')"""
    t = make_text(6000, 5, seed=41).copy()
    a = t[1000:1020].copy()
    pal = np.concatenate([a, revcomp(a)])
    t[3000:3040] = pal
    xp = t[2000:2040].copy()
    for p in (7, 29):
        xp[p] = xp[p] % 4 + 1
    t[5000:5040] = revcomp(xp)
    return t, pal, xp


@functools.lru_cache(maxsize=None)
def index(kind):
    cls = fm.BiFMIndex if kind.startswith("bi") else fm.FMIndex
    with fm.options(force_wide=1 if kind.endswith("_wide") else 0):
        gx = cls.from_sequences([text()[0]], 5, "IB16", 4)
    assert gx.row_bits == (64 if kind.endswith("_wide") else 32)
    return gx


@functools.lru_cache(maxsize=None)
def reads_of(which):
    """"ladder": the reads of LENGTHS — cut from the text with 0 / 1 / 2 substitutions, as they are or reverse-complemented, or random; bytes 0, 5 and 255 inside a few —
    and the palindrome and X'.  "all": those and the read of 5 000 symbols.  "block": 20 reads of BLOCK_LEN symbols (what the ng21 ladder is expanded for)."""
    rng = np.random.default_rng(9)
    t, pal, xp = text()

    def cut(m, subs, flip):
        at = int(rng.integers(0, len(t) - m + 1))
        r = t[at: at + m].copy()
        for p in rng.choice(m, size=min(subs, m), replace=False) if m else []:
            r[p] = (int(r[p]) - 1 + int(rng.integers(1, 4))) % 4 + 1
        return revcomp(r) if flip else r

    if which == "block":
        return [cut(BLOCK_LEN, i % 3, i % 2 == 1) if i % 5 != 4 else rng.integers(1, 5, size=BLOCK_LEN, dtype=np.uint8) for i in range(20)]
    reads = []
    for i, m in enumerate(LENGTHS):
        r = cut(m, (i // 4) % 3, i % 2 == 1) if i % 4 != 3 else rng.integers(1, 5, size=m, dtype=np.uint8)
        if m >= 40 and i % 5 == 0:
            r[m // 2] = (0, 5, 255)[(i // 5) % 3]
        reads.append(r)
    reads += [pal.copy(), xp.copy()]
    if which == "all":
        reads.insert(7, t[500:5500].copy())
    return reads


def shifted(reads, shift):
    """the flat batch with qoff[0] = shift (bytes the batch does not own in front of it)"""
    qbuf, qoff = fm.flatten(reads)
    return np.concatenate([np.full(shift, 7, dtype=np.uint8), qbuf]), qoff + np.uint64(shift)


# ---------------------------------------------------------------------------------------------------------------- fmgpu_queries_strands
def strands_call(qbuf, qoff, nq, comp, out, out_qoff):
    return capi.lib().fmgpu_queries_strands(capi.ptr(qbuf), capi.ptr(qoff), nq, capi.ptr(comp), len(comp), capi.ptr(out), capi.ptr(out_qoff), None)


@pytest.mark.parametrize("shift", [0, 3, 16])
def test_queries_strands_equals_the_numpy_restatement(shift):
    reads = reads_of("all") + [np.array([4, 255, 1], dtype=np.uint8)]
    qbuf, qoff = shifted(reads, shift)
    nq = len(reads)
    total = 2 * (int(qoff[-1]) - shift)
    assert total > 3 * 4096 and total % 16 != 0                         # several blocks, one read across them, a partial last chunk
    for comp in (DNA5[:1].copy(), DNA5, np.array([0, 4, 3, 2, 1, 5], dtype=np.uint8), (255 - np.arange(256)).astype(np.uint8)):
        wq, wo = fm.both_strands((qbuf, qoff), comp)
        assert wq.size == total
        # host in, host out
        out, off = np.full(total + 3, 77, dtype=np.uint8), np.full(2 * nq + 2, 77, dtype=np.uint64)
        assert strands_call(qbuf, qoff, nq, comp, out, off) == 0, capi.lib().fmgpu_last_error()
        assert np.array_equal(out[:total], wq) and np.array_equal(off[:-1], wo) and (out[total:] == 77).all() and off[-1] == 77
    comp = DNA5
    wq, wo = fm.both_strands((qbuf, qoff), comp)
    # device in, device out (the facade), and the mixed cases
    dq, do = capi.DeviceBuffer.from_array(qbuf), capi.DeviceBuffer.from_array(qoff)
    oq, oo = fm.both_strands_device((dq, do), comp)
    assert np.array_equal(oq.to_array(np.uint8, total), wq) and np.array_equal(oo.to_array(np.uint64, 2 * nq + 1), wo)
    out, off = np.zeros(total, dtype=np.uint8), np.zeros(2 * nq + 1, dtype=np.uint64)
    assert strands_call(dq, do, nq, comp, out, off) == 0 and np.array_equal(out, wq) and np.array_equal(off, wo)
    oq2, oo2 = fm.both_strands_device((qbuf, qoff), comp)
    assert np.array_equal(oq2.to_array(np.uint8, total), wq) and np.array_equal(oo2.to_array(np.uint64, 2 * nq + 1), wo)
    # a device output that is not 16-byte aligned
    raw = capi.DeviceBuffer(total + 32)
    assert strands_call(dq, do, nq, comp, raw.ptr + 5, oo2) == 0
    assert np.array_equal(raw.to_array(np.uint8, total + 5)[5:], wq)


def test_queries_strands_small_batches():
    one = [np.array([1, 2, 2, 4, 5, 255, 0, 3], dtype=np.uint8)]
    for reads in (one, [one[0][:1]], [np.zeros(0, dtype=np.uint8)] * 5, [make_text(16, 5, seed=3)], [make_text(8, 5, seed=4), np.zeros(0, dtype=np.uint8), make_text(40, 5, seed=5)]):
        qbuf, qoff = fm.flatten(reads)
        wq, wo = fm.both_strands(reads, DNA5)
        oq, oo = fm.both_strands_device((qbuf, qoff), DNA5)
        assert np.array_equal(oq.to_array(np.uint8, wq.size), wq) and np.array_equal(oo.to_array(np.uint64, wo.size), wo)
    # no read, device offsets: out_qoff[0] = 0
    oo = capi.DeviceBuffer.from_array(np.full(2, 9, dtype=np.uint64))
    assert strands_call(None, None, 0, DNA5, None, oo) == 0 and oo.to_array(np.uint64, 2).tolist() == [0, 9]
    # decreasing offsets are found on the device, before a symbol is read
    qbuf, qoff = fm.flatten([make_text(20, 5, seed=6)] * 3)
    bad = qoff.copy()
    bad[2] = 5
    out, off = np.zeros(200, dtype=np.uint8), np.zeros(7, dtype=np.uint64)
    assert strands_call(qbuf, bad, 3, DNA5, out, off) == capi.FMGPU_ERR_INVALID and b"non-decreasing" in capi.lib().fmgpu_last_error()


# ---------------------------------------------------------------------------------------------------------------- the pair ladder
def ladder_of(mode):
    if mode == "ng21":
        return [fm.search_scheme.expand(fm.search_scheme.pigeon_opt(k, k), BLOCK_LEN) for k in range(3)]
    return [fm.search_scheme.h2(k + 2, 0, k) for k in range(3)]


@functools.lru_cache(maxsize=None)
def doubled(mode):
    """the doubled batch the ladders run on, as a list of reads"""
    q, o = fm.both_strands(reads_of("block" if mode == "ng21" else "ladder"), DNA5)
    return [q[int(o[i]): int(o[i + 1])] for i in range(len(o) - 1)]


def single_scheme_search(gx, mode, n):
    dreads = doubled(mode)

    def search(i, sel):
        sub = fm.flatten([dreads[int(q)] for q in sel])
        if mode == "ng21":
            return fm.search_ng21.search(gx, sub, ladder_of(mode)[i], n=n)
        return fm.search_ng26.search(gx, sub, ladder_of(mode)[i], None, n, edit=(mode == "edit"))
    return search


def best(gx, mode, n, pairs, **kw):
    batch = fm.flatten(doubled(mode))
    if mode == "ng21":
        return fm.search_ng21.search_best(gx, batch, ladder_of(mode), n, pairs=pairs, **kw)
    return fm.search_best(gx, batch, None, n, edit=(mode == "edit"), schemes=[(s, None) for s in ladder_of(mode)], pairs=pairs, **kw)


@pytest.mark.parametrize("ix", ["bi", "bi_wide"])
@pytest.mark.parametrize("mode", ["hamming", "edit", "ng21"])
def test_pair_ladder_equals_the_model(ix, mode):
    gx = index(ix)
    nq = len(doubled(mode))
    for n in (UNLIMITED, 1, 3):
        hits, stratum, stats = best(gx, mode, n, True, want_stratum=True, want_stats=True)
        rec, want_stratum, searched = model.pair_ladder(nq, 3, single_scheme_search(gx, mode, n))
        assert hits.tobytes() == model.callback_order(rec).tobytes(), (n,)
        assert np.array_equal(stratum, want_stratum) and np.array_equal(stratum[0::2], stratum[1::2])
        assert sum(s.hits for s in stats) == len(hits)
        # a sub-multiset of the independent ladder's records on the same batch
        ihits, istratum = best(gx, mode, n, False, want_stratum=True)
        mine, theirs = sorted(map(tuple, hits.tolist())), sorted(map(tuple, ihits.tolist()))
        assert all(mine.count(x) <= theirs.count(x) for x in set(mine)) and len(mine) <= len(theirs)
        assert np.array_equal(np.minimum(istratum[0::2], istratum[1::2]), stratum[0::2])
        if mode != "ng21":
            assert len(mine) < len(theirs)                               # X': its forward strand is not searched again
            xq = nq - 2                                                  # X' is the last read: reads nq - 2 and nq - 1 of the doubled batch
            assert stratum[xq:].tolist() == [0, 0] and istratum[xq:].tolist() == [2, 0]
            assert not (hits["qidx"] == xq).any() and (ihits["qidx"] == xq).any() and (hits["qidx"] == xq + 1).any()
            pq = nq - 4                                                  # the palindrome: both strands at stratum 0
            assert stratum[pq: pq + 2].tolist() == [0, 0] and (hits["qidx"] == pq).any() and (hits["qidx"] == pq + 1).any()
    assert mode == "ng21" or all(int((want_stratum == k).sum()) >= 2 for k in (0, 1, 2, 255)), np.bincount(want_stratum)


def test_pair_ladder_capacity_and_device_buffers():
    gx = index("bi")
    L = capi.lib()
    qbuf, qoff = fm.flatten(doubled("hamming"))
    nq = len(qoff) - 1
    hits, stratum = best(gx, "hamming", UNLIMITED, True, want_stratum=True)
    what, keep = fm._map_query(None, ladder_of("hamming"), False, False, UNLIMITED, False, 0)
    schemes = C.cast(what.schemes, C.POINTER(capi.Scheme))
    total = len(hits)
    first = int((stratum[hits["qidx"].astype(np.int64)] == 0).sum())      # the records of stratum 0
    for cap in (0, first - 1, first, total - 1):
        out, cnt = np.zeros(max(cap, 1), dtype=HIT_DTYPE), C.c_uint64()
        rc = L.fmgpu_search_best_pairs(gx._h, capi.ptr(qbuf), capi.ptr(qoff), nq, schemes, 3, UNLIMITED, capi.ptr(out), cap, C.byref(cnt), None, None, None)
        assert rc == capi.FMGPU_ERR_CAPACITY and cap < cnt.value <= total, (cap, cnt.value)      # the records up to and including the stratum that overflowed
        assert cap >= first or cnt.value == first
    # device buffers in and out
    dq, do = capi.DeviceBuffer.from_array(qbuf), capi.DeviceBuffer.from_array(qoff)
    dh, ds = capi.DeviceBuffer(total * 40), capi.DeviceBuffer(nq)
    cnt = C.c_uint64()
    assert L.fmgpu_search_best_pairs(gx._h, capi.ptr(dq), capi.ptr(do), nq, schemes, 3, UNLIMITED, capi.ptr(dh), total, C.byref(cnt), capi.ptr(ds), None, None) == 0
    assert cnt.value == total and L.fmgpu_hits_sort(capi.ptr(dh), total, None) == 0
    assert dh.to_array(HIT_DTYPE, total).tobytes() == hits.tobytes() and np.array_equal(ds.to_array(np.uint8, nq), stratum)
    del keep


# ---------------------------------------------------------------------------------------------------------------- fmgpu_map_strands
MODES = {"exact": dict(errors=0), "hamming": dict(schemes="ladder", edit=False), "edit": dict(schemes="ladder", edit=True), "ng21": dict(schemes="ladder", ng21=True)}


def map_args(mode):
    kw = dict(MODES[mode])
    if kw.get("schemes") == "ladder":
        kw["schemes"] = ladder_of(mode)
    return kw


def forward_reads(mode):
    return reads_of("block" if mode == "ng21" else "all" if mode == "exact" else "ladder")


@functools.lru_cache(maxsize=None)
def expected(ix, mode, pair, n=UNLIMITED):
    """(P, H, stratum) from the existing calls: pair 0 — fmgpu_map on the NumPy-doubled batch; pair 1 — search_best_pairs -> hits_sort -> locate_hits"""
    gx = index(ix)
    batch = fm.both_strands(forward_reads(mode), DNA5)
    if not pair or mode == "exact":
        pos, hits, stratum = fm.map_reads(gx, batch, n=n, want_hits=True, want_stratum=True, **map_args(mode))
    else:
        hits, stratum = best(gx, mode, n, True, want_stratum=True)
        pos = gx.locate_hits(hits) if len(hits) else np.zeros(0, dtype=POSITION_DTYPE)
    return np.ascontiguousarray(pos), np.ascontiguousarray(hits), np.ascontiguousarray(stratum)


def same(got, want):
    pos, hits, stratum = got
    P, H, S = want
    assert hits.tobytes() == H.tobytes() and np.ascontiguousarray(pos).tobytes() == P.tobytes() and np.array_equal(stratum, S)
    return True


@pytest.mark.parametrize("ix,mode", [("bi", "hamming"), ("bi", "edit"), ("bi", "ng21"), ("bi_wide", "hamming"), ("bi_wide", "ng21"), ("bi", "exact"), ("fm", "exact"),
                                     ("bi_wide", "exact")])
def test_map_strands_equals_map_on_the_doubled_batch_and_the_pair_composition(ix, mode):
    gx = index(ix)
    reads = forward_reads(mode)
    for pair in (False, True):
        for n in (UNLIMITED, 3):
            want = expected(ix, mode, pair, n)
            assert len(want[0]) >= len(want[1]) > 0
            for shift in (0, 3, 16) if n == UNLIMITED else (0,):
                got = fm.map_reads(gx, shifted(reads, shift), n=n, want_hits=True, want_stratum=True, strands=DNA5, pair=pair, **map_args(mode))
                assert same(got, want), (pair, n, shift)
    if mode == "exact":                                                  # no ladder: pair changes nothing
        assert same(expected(ix, mode, True), expected(ix, mode, False))
    else:
        assert len(expected(ix, mode, True)[1]) <= len(expected(ix, mode, False)[1])
    # strand 1 of a read cut from the text as it is lies nowhere; strand 0 of the palindrome and its strand 1 lie at the same place
    if mode in ("hamming", "edit"):
        P = expected(ix, mode, True)[0]
        nq2 = 2 * len(reads)
        a, b = P[P["qidx"] == nq2 - 4], P[P["qidx"] == nq2 - 3]
        assert 3000 in a["pos"].tolist() and 3000 in b["pos"].tolist()
        x = P[P["qidx"] == nq2 - 1]
        assert x["pos"].tolist() == [5000] and x["errors"].tolist() == [0] and not (P["qidx"] == nq2 - 2).any()


@pytest.mark.parametrize("mode", ["hamming", "exact"])
def test_map_strands_growth_path_no_locate_and_device_batches(mode):
    gx = index("bi")
    reads = forward_reads(mode)
    qbuf, qoff = fm.flatten(reads)
    for pair in (False, True):
        want = expected("bi", mode, pair)
        assert same(fm.map_reads(gx, (qbuf, qoff), want_hits=True, want_stratum=True, strands="dna5", pair=pair, first_records=1, **map_args(mode)), want)
        pos, hits, stratum = fm.map_reads(gx, (qbuf, qoff), want_hits=True, want_stratum=True, strands="dna5", pair=pair, locate=False, **map_args(mode))
        assert len(pos) == 0 and hits.tobytes() == want[1].tobytes() and np.array_equal(stratum, want[2])
        dq, do = capi.DeviceBuffer.from_array(qbuf), capi.DeviceBuffer.from_array(qoff)
        assert same(fm.map_reads(gx, (dq, do), want_hits=True, want_stratum=True, strands="dna5", pair=pair, **map_args(mode)), want)
    # the position buffer too small: the exact total and FMGPU_ERR_CAPACITY
    what, keep = fm._map_query(0 if mode == "exact" else None, None if mode == "exact" else ladder_of(mode), False, False, UNLIMITED, True, 0)
    st = capi.Strands(DNA5.ctypes.data_as(capi.u8p), 5, 1)
    cnt, hcnt = C.c_uint64(), C.c_uint64()
    pos = np.zeros(4, dtype=POSITION_DTYPE)
    rc = capi.lib().fmgpu_map_strands(gx._h, capi.ptr(qbuf), capi.ptr(qoff), len(reads), C.byref(what), C.byref(st), capi.ptr(pos), 4, C.byref(cnt), None, 0, C.byref(hcnt),
                                      None, None, None, None)
    want = expected("bi", mode, True)
    assert rc == capi.FMGPU_ERR_CAPACITY and cnt.value == len(want[0]) and hcnt.value == len(want[1])
    del keep


# ---------------------------------------------------------------------------------------------------------------- the feeds
@pytest.mark.parametrize("mode", ["hamming", "ng21", "exact"])
def test_feed_map_strands_equals_map_strands(mode):
    gx = index("bi")
    reads = forward_reads(mode)
    qbuf, qoff = fm.flatten(reads)
    forward_bytes = int(qoff[-1])
    for chunk in (1, 7, 0):
        with fm.Feed(gx, chunk_reads=chunk, slots=2, host_threads=2) as feed:
            for pair in (False, True):
                want = expected("bi", mode, pair)
                got = feed.map((qbuf, qoff), want_hits=True, want_stratum=True, strands=DNA5, pair=pair, **map_args(mode))
                assert same(got, want), (chunk, pair)
                info = feed.info()
                assert info["chunks"] == (-(-len(reads) // chunk) if chunk else 1)
                assert info["uploaded_bytes"] == forward_bytes + 8 * (len(reads) + info["chunks"])       # the forward strand and its offsets: nothing of strand 1
            before = feed.info()["device_bytes"]
            assert same(feed.map((qbuf, qoff), want_hits=True, want_stratum=True, strands=DNA5, pair=True, **map_args(mode)), expected("bi", mode, True))
            assert feed.info()["device_bytes"] == before                 # the doubled buffers only ever grow
            # the feed still serves a plain call
            plain = feed.map((qbuf, qoff), want_hits=True, want_stratum=True, **map_args(mode))
            assert same(plain, tuple(np.ascontiguousarray(a) for a in fm.map_reads(gx, (qbuf, qoff), want_hits=True, want_stratum=True, **map_args(mode))))


def file_text(fmt, mode):
    """the forward reads as FASTA (multi-line records) or FASTQ; a symbol outside 1 .. 4 is written as N"""
    out = []
    for i, r in enumerate(forward_reads(mode)):
        eol = b"\r\n" if i % 3 == 1 else b"\n"
        seq = "".join("ACGT"[int(v) - 1] if 1 <= int(v) <= 4 else "N" for v in r).encode()
        if fmt == "fasta":
            width = 1 + (7 * i) % 23
            out.append(b">read%d some text" % i + eol + b"".join(seq[k: k + width] + eol for k in range(0, len(seq), width)))
        else:
            out.append(b"@q%d" % i + eol + seq + eol + b"+" + eol + bytes((33 + (i + k) % 60) for k in range(len(seq))) + eol)
    return b"".join(out)


TABLE = None


def table():
    global TABLE
    if TABLE is None:
        TABLE = fm.symbol_table("ACGT", 1, True, fm.FOREIGN)
    return TABLE


def text_agrees(m, pq, want):
    P, H, S = want
    assert m.reads == pq.reads and m.symbols == pq.symbols and m.consumed == pq.consumed and m.foreign == pq.foreign
    assert m.hits.tobytes() == H.tobytes() and np.ascontiguousarray(m.positions).tobytes() == P.tobytes() and np.array_equal(m.stratum, S) and len(m.stratum) == 2 * pq.reads
    assert m.names.tobytes() == pq.names.tobytes() and m.quals.tobytes() == pq.quals.tobytes()
    assert np.array_equal(m.lens, np.diff(pq.qoff.astype(np.int64)).astype(np.uint64))


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
@pytest.mark.parametrize("mode", ["hamming", "exact"])
def test_feed_map_text_strands_equals_map_strands_on_the_parsed_batch(fmt, mode):
    gx = index("bi")
    data = file_text(fmt, mode)
    pq = fm.parse_queries(data, fmt, table(), want_names=True, want_quals=True)
    assert pq.reads == len(forward_reads(mode)) and pq.foreign > 0
    kw = dict(want_hits=True, want_stratum=True, want_names=True, want_quals=True, want_lens=True)
    with fm.Feed(gx, slots=2, host_threads=2) as feed:
        for pair in (False, True):
            want = tuple(np.ascontiguousarray(a) for a in fm.map_reads(gx, pq.batch, want_hits=True, want_stratum=True, strands=DNA5, pair=pair, **map_args(mode)))
            assert len(want[0]) > 0
            for B in (16, 257, 0):
                m = feed.map_text(data, fmt, table(), chunk_bytes=B, strands=DNA5, pair=pair, **kw, **map_args(mode))
                text_agrees(m, pq, want)
                assert feed.info()["uploaded_bytes"] == len(data)        # the text and nothing else: the second strand never crosses the bus
            # `final` split over two calls: the first call consumes what it proves complete, the second takes the rest
            cut = len(data) * 2 // 3
            m1 = feed.map_text(data[:cut], fmt, table(), final=False, chunk_bytes=257, strands=DNA5, pair=pair, **kw, **map_args(mode))
            m2 = feed.map_text(data[m1.consumed:], fmt, table(), final=True, chunk_bytes=257, strands=DNA5, pair=pair, **kw, **map_args(mode))
            assert 0 < m1.reads < pq.reads and m1.reads + m2.reads == pq.reads
            h2, p2 = m2.hits.copy(), np.ascontiguousarray(m2.positions).copy()
            h2["qidx"] += np.uint64(2 * m1.reads)
            p2["qidx"] += np.uint64(2 * m1.reads)
            p2["hit"] += np.uint32(len(m1.hits))
            assert np.concatenate([m1.hits, h2]).tobytes() == want[1].tobytes() and np.concatenate([np.ascontiguousarray(m1.positions), p2]).tobytes() == want[0].tobytes()
            assert np.array_equal(np.concatenate([m1.stratum, m2.stratum]), want[2])
        # a text error still names the whole-file line
        lines = data.split(b"\n")
        bad_line = len(lines) * 3 // 4 // 4 * 4 if fmt == "fastq" else 0
        if fmt == "fastq":
            lines[bad_line] = b"!" + lines[bad_line][1:]
            with pytest.raises(fm.TextError) as e:
                feed.map_text(b"\n".join(lines), fmt, table(), chunk_bytes=64, strands=DNA5, pair=True, **map_args(mode))
            assert e.value.line == bad_line
        # the feed still serves a plain fmgpu_feed_map_text call, with unchanged results
        plain = feed.map_text(data, fmt, table(), chunk_bytes=257, **kw, **map_args(mode))
        want = tuple(np.ascontiguousarray(a) for a in fm.map_reads(gx, pq.batch, want_hits=True, want_stratum=True, **map_args(mode)))
        assert plain.hits.tobytes() == want[1].tobytes() and np.ascontiguousarray(plain.positions).tobytes() == want[0].tobytes() and np.array_equal(plain.stratum, want[2])
        assert len(plain.stratum) == pq.reads
