"""fmgpu_feed_map_text (include/fmgpu.h) on the host: the exported symbol, the argument checks that come before any use of the device, the window / piece / headroom
arithmetic of fmgpu_feed_host.h as a stand-alone program (plain and under the address and undefined-behaviour sanitizers; nothing is loaded into python), and the
piece rule in plain Python (tests/feed_text_model.py) against the whole-text contract (tests/parse_model.py): pieces with a carry give the whole-text parse."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests import feed_text_model as pieces
from tests import parse_model as model
from tests.parse_model import LINES, FASTA, FASTQ
from tests.test_parse_host import CASES, CHUNK_TEXTS, DNA, DNA_DROP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_feed_text_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_feed_text_host")
WINDOWS = (16, 17, 64, 257, 4096)


def test_symbol_is_exported_and_the_abi_stays():
    L = capi.lib()
    assert "fmgpu_feed_map_text" in capi.EXPORTS and hasattr(L, "fmgpu_feed_map_text")
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        header = f.read()
    assert "int fmgpu_feed_map_text(fmgpu_feed_t f, const uint8_t* text, uint64_t bytes, int32_t format, int32_t final," in header
    assert L.fmgpu_abi_version() == 6 and "#define FMGPU_ABI_VERSION 6" in header
    assert len(capi.OPTIONS) == 13 and "FMGPU_OPT_COUNT_ = 13" in header.replace("  ", " ")
    assert hasattr(fm.Feed, "map_text") and hasattr(fm.Feed, "map_file")


def _call(f, text, nbytes, fmt, table, chunk_bytes, what, out, cap, cnt, hits, hcap, result, final=1):
    return capi.lib().fmgpu_feed_map_text(f, capi.ptr(text), nbytes, fmt, final, capi.ptr(table), chunk_bytes, None if what is None else C.byref(what),
                                          capi.ptr(out), cap, None if cnt is None else C.byref(cnt), capi.ptr(hits), hcap, None, None, None, None, None, 0,
                                          None if result is None else C.byref(result), None, None)


def test_argument_checks_need_no_device():
    """every check is made on a block of zero bytes in place of a feed (no feed exists without a device): each returns its own message before the feed is looked at,
    and the feed check itself comes before the device is"""
    L = capi.lib()
    not_a_feed = np.zeros(4096, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    text = np.frombuffer(b"AC\nGT\n", dtype=np.uint8)
    pos, hits = np.zeros(4, dtype=fm.POSITION_DTYPE), np.zeros(4, dtype=fm.HIT_DTYPE)
    what, _ = fm._map_query(0, None, False, True, fm.UINT64_MAX, True, 0)
    res, cnt = capi.ParseResult(), C.c_uint64(7)

    def refused(word, *args, **kw):
        assert _call(*args, **kw) == capi.FMGPU_ERR_INVALID
        assert word in L.fmgpu_last_error(), L.fmgpu_last_error()

    good = [not_a_feed, text, text.size, LINES, DNA, 0, what, pos, 4, cnt, hits, 4, res]
    refused(b"feed is null", *([None] + good[1:]))                               # null f
    refused(b"not a feed", *good)                                                # ... or no feed at all
    refused(b"result", *(good[:12] + [None]))                                    # null result
    refused(b"symbol_of", *(good[:4] + [None] + good[5:]))                       # null symbol_of
    refused(b"what is null", *(good[:6] + [None] + good[7:]))                    # null what
    refused(b"out_count", *(good[:9] + [None] + good[10:]))                      # null out_count
    refused(b"text is null", *(good[:1] + [None] + good[2:]))                    # null text, bytes > 0
    refused(b"out", *(good[:7] + [None] + good[8:]))                             # null out, capacity > 0
    refused(b"out_hits", *(good[:10] + [None] + good[11:]))                      # null out_hits, hits_capacity > 0
    for fmt in (3, -1):
        refused(b"unknown text format", *(good[:3] + [fmt] + good[4:]))
    for b in (1, 15):
        refused(b"chunk_bytes", *(good[:5] + [b] + good[6:]))
    bad = capi.MapQuery()
    bad.kind, bad.max_hits_per_query = 77, 1
    refused(b"kind", *(good[:6] + [bad] + good[7:]))                             # what fmgpu_feed_map refuses in `what`
    bad.kind, bad.n_schemes = capi.MAP_SCHEME, 0
    refused(b"n_schemes", *(good[:6] + [bad] + good[7:]))
    assert cnt.value == 0                                                        # (the counts are reset on every path)
    # bytes == 0 on a real feed returns 0 with zero counts and a zero result: tests/test_gpu_feed_text.py


def test_window_arithmetic_as_a_program_plain_and_under_the_sanitizers():
    base = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", SRC, "-o", EXE]
    for extra in (["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]):
        subprocess.run(base + extra, check=True)
        r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "all checks passed" in r.stdout


def crlf(text):
    return text.replace(b"\r\n", b"\n").replace(b"\n", b"\r\n")


def same(a, b):
    assert (a.error_line, a.error_offset) == (b.error_line, b.error_offset)
    assert a.reads == b.reads and a.consumed == b.consumed and a.foreign == b.foreign
    if a.error_line is None:
        assert a.names == b.names and a.quals == b.quals


TEXTS = [(name, fmt, text) for name, fmt, _, text, _, _, _ in CASES] + [("chunk text %d" % fmt, fmt, text) for fmt, text in CHUNK_TEXTS.items()]


@pytest.mark.parametrize("B", WINDOWS)
def test_pieces_give_the_whole_text_parse(B):
    """every text of tests/test_parse_host.py, as it is and with CRLF line ends, under both tables and both `final` flags; error lines and offsets are the whole text's"""
    for name, fmt, text in TEXTS:
        for variant in (text, crlf(text), text * 3, crlf(text) + text):
            for table in (DNA, DNA_DROP):
                for final in (1, 0):
                    whole = model.parse(variant, fmt, table, final)
                    got = pieces.parse_pieces(variant, fmt, table, final, B)
                    same(got, whole)
                    assert got.windows == -(-len(variant) // B), name


def test_pieces_where_only_later_bytes_settle_a_line():
    """the two places where a piece that is not final cannot be parsed to its end (tests/feed_text_model.settled), cut at every byte: windows of 16 bytes and more,
    so a prefix of 15 - k filler bytes puts byte k of the text on a window's edge"""
    cases = [(FASTA, b"\r\n\r\n>a\r\nAC\r\n\r\n>b\r\nGT\r\n"),
             (FASTA, b"\n\r\nAC\r\n>a\nGT\n"),                                   # a text error behind a lone "\r\n"
             (FASTQ, b"@a\nAC\n+\nII\n" + b"\n" * 9),                            # empty lines at the very end: discarded, however many
             (FASTQ, b"@a\nAC\n+\nII\n" + b"\r\n" * 6),
             (FASTQ, b"@a\nAC\n+\nII\n@b\n\n+\n\n\n\n\n"),                       # the last record loses its empty quality line: truncated, line 4
             (FASTQ, b"@a\nAC\n+\nII\n" + b"\n" * 5 + b"@b\nA\n+\nI\n"),         # empty lines that are no end: a bad record, line 4
             (FASTQ, b"@a\n\n+\n\n@b\nA\n+\nI\n")]
    for fmt, text in cases:
        for pad in range(16):
            filler = {FASTA: b"\n" * pad, FASTQ: b"@p\n" + b"A" * pad + b"\n+\n" + b"I" * pad + b"\n"}[fmt]
            for final in (1, 0):
                whole = model.parse(filler + text, fmt, DNA, final)
                for B in (16, 17, 31):
                    same(pieces.parse_pieces(filler + text, fmt, DNA, final, B), whole)


def test_pieces_random_cuts():
    rng = np.random.default_rng(11)
    for fmt, text in CHUNK_TEXTS.items():
        whole = model.parse(text, fmt, DNA, 1)
        for B in rng.integers(16, len(text) + 5, size=40):
            same(pieces.parse_pieces(text, fmt, DNA, 1, int(B)), whole)
