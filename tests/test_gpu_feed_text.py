"""fmgpu_feed_map_text on the device (include/fmgpu.h): the raw bytes of a read file through a feed.  Every expected value is what the existing calls give for the
whole text — fm.map_reads(fm.parse_queries(text)) plus that parse's spans and lengths; tests/feed_text_model.py (proved equal to the whole-text contract on the CPU
by tests/test_feed_text_host.py) gives the number of windows and the text errors.  Indices and ladders are those of tests/test_gpu_map.py.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE, POSITION_DTYPE, TEXT_SPAN_DTYPE
from tests import feed_text_model as pieces
from tests import parse_model as model
from tests.parse_model import LINES, FASTA, FASTQ
from tests.test_gpu_map import BLOCK_LEN, batch, index, ladder_of, sigma_of

pytestmark = pytest.mark.gpu
FORMATS = {"lines": LINES, "fasta": FASTA, "fastq": FASTQ}
WINDOWS = (16, 64, 257, 4096, 1 << 20)                                # 16: below every record (the headroom grows); 64, 257: records cut at every line role; 2^20: one window
LETTERS28 = "".join(chr(65 + i) for i in range(27))                   # ranks 1 .. 27 of the sigma = 28 index: 'A' .. '['


def table_of(sigma):
    if sigma == 5:
        return fm.symbol_table("ACGT", 1, True, fm.FOREIGN, drop=b"-", extra={"$": 0})
    return fm.symbol_table(LETTERS28, 1, False, fm.FOREIGN, drop=b"-")


@functools.lru_cache(maxsize=None)
def file_text(fmt, sigma, block):
    """the reads of tests/test_gpu_map.batch as a read file: LF and CRLF line ends mixed, a foreign byte for every symbol outside 1 .. sigma - 1, dropped bytes ('-')
    here and there, lower case (sigma = 5), the empty reads of the batch, multi-line FASTA records and empty lines (FASTA), and a last record without a newline.
    block: only the 20 reads of BLOCK_LEN symbols (what the ng21 ladder is expanded for)"""
    reads = batch(sigma)[0]
    reads = reads[-20:] if block else reads
    letters = "ACGT" if sigma == 5 else LETTERS28
    out = []
    for i, r in enumerate(reads):
        eol = b"\r\n" if i % 3 == 1 else b"\n"
        s = "".join(letters[int(v) - 1] if 1 <= int(v) < sigma else "n?"[i % 2] for v in r)
        if sigma == 5 and i % 4 == 2:
            s = s.lower()
        if i % 5 == 3 and len(s) > 2:
            s = s[:2] + "-" + s[2:] + "-"
        seq = s.encode()
        if fmt == LINES:
            out.append(seq + eol)
        elif fmt == FASTA:
            width = 1 + (7 * i) % 23
            rows = [seq[k: k + width] for k in range(0, len(seq), width)]
            out.append(b">read%d some text" % i + eol + b"".join(row + eol for row in rows) + (b"\n" if i % 7 == 0 else b""))
        else:
            out.append(b"@q%d" % i + eol + seq + eol + (b"+" if i % 2 else b"+q%d" % i) + eol + bytes((33 + (i + k) % 60) for k in range(len(seq))) + eol)
    text = b"".join(out)
    return text[: -len(eol)]                                          # the last record ends the file without a newline


MODES = {"exact": dict(errors=0), "hamming": dict(schemes="ladder", edit=False), "edit": dict(schemes="ladder", edit=True), "ng21": dict(schemes="ladder", ng21=True)}


def map_args(mode):
    kw = dict(MODES[mode])
    if kw.get("schemes") == "ladder":
        kw["schemes"] = ladder_of(mode)
    return kw


@functools.lru_cache(maxsize=None)
def expected(ix, fmt, mode, final=1):
    """(P, H, stratum, names, quals, lens, ParsedQueries) of the whole text through the existing calls"""
    sigma = sigma_of(ix)
    text = file_text(fmt, sigma, mode == "ng21")
    pq = fm.parse_queries(text, fmt, table_of(sigma), final=bool(final), want_names=True, want_quals=True)
    assert pq.reads >= 19 and (mode != "ng21" or set(np.diff(pq.qoff.astype(np.int64)).tolist()) == {BLOCK_LEN})
    pos, hits, stratum = fm.map_reads(index(ix), pq.batch, want_hits=True, want_stratum=True, **map_args(mode))
    assert len(hits) > 0 and len(pos) >= len(hits)
    return np.ascontiguousarray(pos), hits, stratum, pq.names, pq.quals, np.diff(pq.qoff.astype(np.int64)).astype(np.uint64), pq


def agrees(m, want):
    P, H, S, names, quals, lens, pq = want
    assert m.reads == pq.reads and m.symbols == pq.symbols and m.consumed == pq.consumed and m.foreign == pq.foreign
    assert m.hits.tobytes() == H.tobytes() and m.positions.tobytes() == P.tobytes()
    assert np.array_equal(m.stratum, S) and np.array_equal(m.lens, lens)
    assert m.names.tobytes() == names.tobytes() and m.quals.tobytes() == quals.tobytes()


@pytest.mark.parametrize("slots", [2, 4])
@pytest.mark.parametrize("mode", ["exact", "hamming", "edit", "ng21"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_every_output_equals_the_whole_text_calls(fmt, mode, slots):
    fmt = FORMATS[fmt]
    text = file_text(fmt, 5, mode == "ng21")
    want = expected("bi", fmt, mode)
    with fm.Feed(index("bi"), slots=slots, host_threads=3) as feed:
        for B in WINDOWS:
            m = feed.map_text(text, fmt, table_of(5), chunk_bytes=B, want_hits=True, want_stratum=True, want_names=True, want_quals=True, want_lens=True, **map_args(mode))
            agrees(m, want)
            info = feed.info()
            assert info["chunks"] == pieces.windows(len(text), B) == -(-len(text) // B)
            assert info["uploaded_bytes"] == len(text) == info["staged_bytes"] - result_bytes(m)
        # a second call on the same feed: the same results, and no buffer grows
        before = feed.info()["device_bytes"]
        for B in WINDOWS:
            agrees(feed.map_text(text, fmt, table_of(5), chunk_bytes=B, want_hits=True, want_stratum=True, want_names=True, want_quals=True, want_lens=True, **map_args(mode)), want)
        assert feed.info()["device_bytes"] == before


def result_bytes(m):
    """what crosses the pinned slots on the way back when no output is pinned"""
    return m.hits.nbytes + m.positions.nbytes + m.reads * (1 + 16 + 16 + 8)


@pytest.mark.parametrize("ix,mode", [("bi_wide", "hamming"), ("bi_wide", "exact"), ("fm", "exact"), ("wavelet", "exact")])
def test_the_other_indices(ix, mode):
    sigma = sigma_of(ix)
    for fmt in (FASTA, FASTQ):
        text = file_text(fmt, sigma, False)
        want = expected(ix, fmt, mode)
        with fm.Feed(index(ix), slots=2) as feed:
            for B in (16, 257):
                agrees(feed.map_text(text, fmt, table_of(sigma), chunk_bytes=B, want_hits=True, want_stratum=True, want_names=True, want_quals=True, want_lens=True,
                                     **map_args(mode)), want)


def raw(feed, text, fmt, what, cap, hcap, rcap, final=1, B=64, pos=None, hits=None, stratum=None, names=None, quals=None, lens=None, nbytes=None, table=None):
    """the C call -> (rc, result, P buffer, P count, H buffer, H count, stratum, names, quals, lens); an array given as False is passed as NULL"""
    def buf(given, n, dtype, fill=0):
        return None if given is False else (np.full(max(n, 1), fill, dtype=dtype) if given is None else given)
    pos, hits = buf(pos, cap, POSITION_DTYPE), buf(hits, hcap, HIT_DTYPE)
    stratum, names, quals, lens = buf(stratum, rcap, np.uint8, 77), buf(names, rcap, TEXT_SPAN_DTYPE), buf(quals, rcap, TEXT_SPAN_DTYPE), buf(lens, rcap, np.uint64)
    cnt, hcnt, res = C.c_uint64(12345), C.c_uint64(12345), capi.ParseResult()
    table = table_of(5) if table is None else table
    rc = capi.lib().fmgpu_feed_map_text(feed._f, capi.ptr(text), len(text) if nbytes is None else nbytes, fmt, final, capi.ptr(table), B, C.byref(what),
                                        capi.ptr(pos), cap, C.byref(cnt), capi.ptr(hits), hcap, C.byref(hcnt), capi.ptr(stratum), capi.ptr(names), capi.ptr(quals), capi.ptr(lens),
                                        rcap, C.byref(res), None, None)
    return rc, res, pos, int(cnt.value), hits, int(hcnt.value), stratum, names, quals, lens


def query(mode, locate=True):
    kw = map_args(mode)
    return fm._map_query(kw.get("errors"), kw.get("schemes"), kw.get("ng21", False), kw.get("edit", True), fm.UINT64_MAX, locate, 0)


def test_pinned_text_and_outputs_are_used_in_place():
    text = file_text(FASTQ, 5, False)
    P, H, S, names, quals, lens, pq = expected("bi", FASTQ, "hamming")
    what, keep = query("hamming")
    bufs = [capi.PinnedBuffer(max(n, 8)) for n in (len(text), P.nbytes, H.nbytes, pq.reads, names.nbytes, quals.nbytes, lens.nbytes)]
    ptext = bufs[0].array(np.uint8, len(text))
    ptext[:] = np.frombuffer(text, dtype=np.uint8)
    outs = [b.array(dt, n) for b, dt, n in zip(bufs[1:], (POSITION_DTYPE, HIT_DTYPE, np.uint8, TEXT_SPAN_DTYPE, TEXT_SPAN_DTYPE, np.uint64),
                                               (len(P), len(H), pq.reads, pq.reads, pq.reads, pq.reads))]
    with fm.Feed(index("bi"), slots=2) as feed:
        for B in (64, 257):
            for o in outs:
                o.view(np.uint8)[:] = 0x5A
            rc, res, pos, cnt, hits, hcnt, stratum, gn, gq, gl = raw(feed, ptext, FASTQ, what, len(P), len(H), pq.reads, B=B, pos=outs[0], hits=outs[1], stratum=outs[2],
                                                                       names=outs[3], quals=outs[4], lens=outs[5])
            assert rc == 0, capi.lib().fmgpu_last_error()
            assert (cnt, hcnt, res.reads, res.symbols, res.consumed, res.foreign) == (len(P), len(H), pq.reads, pq.symbols, pq.consumed, pq.foreign)
            assert pos.tobytes() == P.tobytes() and hits.tobytes() == H.tobytes() and np.array_equal(stratum, S)
            assert gn.tobytes() == names.tobytes() and gq.tobytes() == quals.tobytes() and np.array_equal(gl, lens)
            info = feed.info()
            assert info["staged_bytes"] == 0 and info["uploaded_bytes"] == len(text) and info["chunks"] == -(-len(text) // B)
        # pageable text, pinned outputs: only the text crosses a pinned slot
        rc = raw(feed, np.frombuffer(text, dtype=np.uint8), FASTQ, what, len(P), len(H), pq.reads, B=257, pos=outs[0], hits=outs[1], stratum=outs[2], names=outs[3],
                 quals=outs[4], lens=outs[5])[0]
        assert rc == 0 and feed.info()["staged_bytes"] == len(text)
    del outs, ptext, keep
    for b in bufs:
        b.free()


def test_without_locate_and_without_read_arrays():
    text = np.frombuffer(file_text(FASTA, 5, False), dtype=np.uint8)
    P, H, S, names, quals, lens, pq = expected("bi", FASTA, "edit")
    what, keep = query("edit", locate=False)
    with fm.Feed(index("bi"), slots=2) as feed:
        rc, res, pos, cnt, hits, hcnt, stratum, *_ = raw(feed, text, FASTA, what, 0, len(H), pq.reads, B=257, pos=False)
        assert rc == 0 and cnt == 0 and hcnt == len(H) and hits.tobytes() == H.tobytes() and np.array_equal(stratum, S) and res.reads == pq.reads
        # every read-indexed array NULL: read_capacity is ignored
        what, keep = query("edit")
        rc, res, pos, cnt, hits, hcnt, *_ = raw(feed, text, FASTA, what, len(P), 0, 0, B=64, hits=False, stratum=False, names=False, quals=False, lens=False)
        assert rc == 0 and cnt == len(P) and pos.tobytes() == P.tobytes() and hcnt == len(H) and res.reads == pq.reads
        # bytes == 0: zero counts and a zero result
        rc, res, pos, cnt, hits, hcnt, *_ = raw(feed, text, FASTA, what, 4, 4, 4, nbytes=0)
        assert rc == 0 and (cnt, hcnt, res.reads, res.symbols, res.consumed, res.foreign, res.error_line, res.error_offset) == (0,) * 8
        # a device pointer in any argument: the feed rule
        dev = fm.DeviceBuffer(64)
        rc = capi.lib().fmgpu_feed_map_text(feed._f, capi.ptr(dev), 64, FASTA, 1, capi.ptr(table_of(5)), 0, C.byref(what), capi.ptr(pos), 4, C.byref(C.c_uint64()), None, 0,
                                            None, None, None, None, None, 0, C.byref(capi.ParseResult()), None, None)
        assert rc == capi.FMGPU_ERR_INVALID and b"host memory only" in capi.lib().fmgpu_last_error()
    del keep


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_not_final_and_the_call_behind_it(fmt):
    """final == 0: consumed is the whole-text parse's; the call from there with final = 1 gives the rest.  Its qidx count from 0 and its spans are relative to the bytes
    it was given: the first call's read count and `consumed` are added here, and its position records index its own hit list: the first call's hit count is added."""
    fmt = FORMATS[fmt]
    text = np.frombuffer(file_text(fmt, 5, False), dtype=np.uint8)
    cut = len(text) * 2 // 3
    P, H, S, names, quals, lens, pq = expected("bi", fmt, "hamming")
    head = fm.parse_queries(text[:cut], fmt, table_of(5), final=False)
    assert 0 < head.consumed < cut and 0 < head.reads < pq.reads
    what, keep = query("hamming")
    with fm.Feed(index("bi"), slots=2) as feed:
        for B in (64, 257):
            a = raw(feed, text[:cut], fmt, what, len(P), len(H), pq.reads, final=0, B=B)
            assert a[0] == 0 and (a[1].consumed, a[1].reads, a[1].symbols, a[1].foreign) == (head.consumed, head.reads, head.symbols, head.foreign)
            b = raw(feed, text[head.consumed:], fmt, what, len(P), len(H), pq.reads, final=1, B=B)
            assert b[0] == 0 and a[1].reads + b[1].reads == pq.reads and a[1].consumed + b[1].consumed == pq.consumed
            ra, rb = a[1].reads, b[1].reads
            pos_b, hits_b = b[2][: b[3]].copy(), b[4][: b[5]].copy()
            pos_b["qidx"] += ra
            pos_b["hit"] += a[5]
            hits_b["qidx"] += ra
            assert np.concatenate([a[2][: a[3]], pos_b]).tobytes() == P.tobytes() and np.concatenate([a[4][: a[5]], hits_b]).tobytes() == H.tobytes()
            assert np.array_equal(np.concatenate([a[6][:ra], b[6][:rb]]), S) and np.array_equal(np.concatenate([a[9][:ra], b[9][:rb]]), lens)
            for k, whole, shifted in ((7, names, fmt != LINES), (8, quals, fmt == FASTQ)):
                tail = b[k][:rb].copy()
                if shifted:
                    tail["offset"] += head.consumed
                assert np.concatenate([a[k][:ra], tail]).tobytes() == whole.tobytes()
    del keep


def test_capacities_one_below_need_report_exact_totals():
    text = np.frombuffer(file_text(FASTQ, 5, False), dtype=np.uint8)
    P, H, S, names, quals, lens, pq = expected("bi", FASTQ, "hamming")
    what, keep = query("hamming")
    L = capi.lib()
    with fm.Feed(index("bi"), slots=2) as feed:
        for short, word in (((1, 0, 0), b"position buffer"), ((0, 1, 0), b"hit buffer"), ((0, 0, 1), b"read arrays")):
            rc, res, pos, cnt, hits, hcnt, *_ = raw(feed, text, FASTQ, what, len(P) - short[0], len(H) - short[1], pq.reads - short[2], B=257)
            assert rc == capi.FMGPU_ERR_CAPACITY and word in L.fmgpu_last_error()
            assert (cnt, hcnt, res.reads, res.symbols, res.consumed, res.foreign) == (len(P), len(H), pq.reads, pq.symbols, pq.consumed, pq.foreign)
            assert feed.info()["chunks"] == -(-len(text) // 257)                       # every piece still ran
        agrees_raw = raw(feed, text, FASTQ, what, len(P), len(H), pq.reads, B=257)     # and the exact totals fit
        assert agrees_raw[0] == 0 and agrees_raw[2].tobytes() == P.tobytes() and agrees_raw[4].tobytes() == H.tobytes()
    del keep


def broken(kind):
    """(format, text) with one text error behind the first windows of 64 and of 257 bytes"""
    text = bytearray(file_text(FASTQ, 5, False))
    lines, _ = model.split_lines(bytes(text), True)
    if kind == "separator":
        l = next(l for l, (s, e) in enumerate(lines) if l % 4 == 2 and s > 300)
        text[lines[l][0]] = ord("-")
    elif kind == "quality":
        l = next(l for l, (s, e) in enumerate(lines) if l % 4 == 3 and s > 300 and e - s > 3)
        del text[lines[l][0]]
    else:
        return FASTA, b"\n\r\nACGT\n" + file_text(FASTA, 5, False)
    return FASTQ, bytes(text)


@pytest.mark.parametrize("kind", ["separator", "quality", "text before the first header"])
def test_text_errors_name_the_line_of_the_whole_text(kind):
    fmt, text = broken(kind)
    good = np.frombuffer(file_text(fmt, 5, False), dtype=np.uint8)
    P, H, S, names, quals, lens, pq = expected("bi", fmt, "hamming")
    what, keep = query("hamming")
    L = capi.lib()
    with fm.Feed(index("bi"), slots=2) as feed:
        for B in (64, 257):
            want = pieces.parse_pieces(text, fmt, table_of(5), 1, B)
            whole = model.parse(text, fmt, table_of(5), 1)
            assert want.error_line is not None and (want.error_line, want.error_offset, want.reads, want.consumed) == (whole.error_line, whole.error_offset, whole.reads, whole.consumed)
            assert fmt == FASTA or want.error_offset > 257                             # in a piece other than the first
            rc, res, *_ = raw(feed, np.frombuffer(text, dtype=np.uint8), fmt, what, len(P), len(H), pq.reads, B=B)
            assert rc == capi.FMGPU_ERR_INVALID
            msg = L.fmgpu_last_error()
            assert msg.startswith(b"text error in line %d (0-based, byte offset %d)" % (want.error_line, want.error_offset)), msg
            assert (res.error_line, res.error_offset, res.reads, res.symbols, res.consumed, res.foreign) == \
                (want.error_line, want.error_offset, len(want.reads), want.symbols, want.consumed, want.foreign)
            # the feed serves a good call afterwards
            ok = raw(feed, good, fmt, what, len(P), len(H), pq.reads, B=B)
            assert ok[0] == 0 and ok[2].tobytes() == P.tobytes() and ok[4].tobytes() == H.tobytes()
        with pytest.raises(fm.TextError) as e:
            feed.map_text(text, fmt, table_of(5), chunk_bytes=64, schemes=ladder_of("hamming"), edit=False)
        assert (e.value.line, e.value.offset) == (whole.error_line, whole.error_offset)
    del keep


def test_python_mirrors_on_a_file(tmp_path):
    text = file_text(FASTQ, 5, False)
    path = tmp_path / "reads.fastq"
    path.write_bytes(text)
    want = expected("bi", FASTQ, "edit")
    with fm.Feed(index("bi")) as feed:
        m = feed.map_file(str(path), "fastq", table_of(5), chunk_bytes=257, want_hits=True, want_stratum=True, want_names=True, want_quals=True, want_lens=True, **map_args("edit"))
        agrees(m, want)
        assert fm.ParsedQueries.texts(text, m.names)[:2] == [b"q0", b"q1"]
        # capacities that are too small: the call runs once more with the exact totals the capacity error reports
        m = feed.map_text(bytearray(text), FASTQ, table_of(5), chunk_bytes=64, want_hits=True, want_stratum=True, want_names=True, want_quals=True, want_lens=True,
                          capacities=(3, 2, 1), **map_args("edit"))
        agrees(m, want)
        # without locate there are no positions
        m = feed.map_text(bytearray(text), FASTQ, table_of(5), chunk_bytes=4096, locate=False, want_hits=True, **map_args("edit"))
        assert len(m.positions) == 0 and m.hits.tobytes() == want[1].tobytes() and m.stratum is None and m.names is None and m.reads == want[6].reads
        (tmp_path / "empty").write_bytes(b"")
        m = feed.map_file(str(tmp_path / "empty"), FASTQ, table_of(5), errors=0)
        assert m.reads == 0 and len(m.positions) == 0
