"""fmgpu_positions_sam and fmgpu_sam_header (include/fmgpu.h) on the host: the symbols and the struct, every argument check that comes before the first use of the
device, the calls without a line, the header call against the plain-Python model of tests/sam_model.py, and that model against hand-written lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import POSITION_DTYPE, TEXT_SPAN_DTYPE
from tests import sam_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def last_error():
    return capi.lib().fmgpu_last_error()


def test_the_symbols_exist_and_the_abi_version_stays():
    L = capi.lib()
    for name in ("fmgpu_positions_sam", "fmgpu_sam_header"):
        assert name in capi.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header())
    assert L.fmgpu_abi_version() == 6 and re.search(r"#define FMGPU_ABI_VERSION 6\b", header())


def test_the_struct_mirrors_the_header():
    body = re.search(r"typedef struct fmgpu_sam_spec \{(.*?)\} fmgpu_sam_spec;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            names += [re.sub(r"\[\d+\]", "", first.split()[-1]).lstrip("*")] + [re.sub(r"\[\d+\]", "", m.strip()).lstrip("*") for m in more]
    S = capi.SamSpec
    assert C.sizeof(S) == 72
    assert [f[0] for f in S._fields_] == names == ["qbuf", "qoff", "nq", "char_of", "strands", "read_names", "quals", "seq_names", "cigar", "emit_unmapped",
                                                    "secondary_seq", "mapq_unique", "mapq_multi", "reserved"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 65, 66, 67, 68, 69]


CHAR_OF = fm.char_table("dna5")
QBUF = np.array([1, 2, 3, 4], dtype=np.uint8)
QOFF = np.array([0, 2, 4], dtype=np.uint64)
COMP = np.array(fm.DNA5_COMPLEMENT, dtype=np.uint8)


def spec(qbuf=QBUF, qoff=QOFF, nq=2, char_of=CHAR_OF, strands=None, read_names=None, quals=None, seq_names=None, cigar=1, emit_unmapped=1, secondary_seq=0,
         reserved=(0, 0, 0)):
    p = lambda a: a if a is None or isinstance(a, C.c_void_p) else capi.ptr(a)          # noqa: E731
    return capi.SamSpec(p(qbuf), p(qoff), nq, p(char_of), None if strands is None else C.pointer(strands), None if read_names is None else C.pointer(read_names),
                        None if quals is None else C.pointer(quals), None if seq_names is None else C.pointer(seq_names), cigar, emit_unmapped, secondary_seq, 60, 0,
                        (C.c_uint8 * 3)(*reserved))


def test_argument_checks_come_before_the_device():
    L = capi.lib()
    rec = np.zeros(2, dtype=POSITION_DTYPE)
    out = np.full(64, 0xAA, dtype=np.uint8)
    garbage = C.c_void_p(0x10)                                           # never read through: the checks come first
    nbytes, nlines = C.c_uint64(7), C.c_uint64(7)
    names = np.zeros(4, dtype=np.uint8)
    spans = np.zeros(1, dtype=TEXT_SPAN_DTYPE)

    def call(s, positions=capi.ptr(rec), count=2, out_=capi.ptr(out), capacity=64, out_bytes=C.byref(nbytes)):
        return L.fmgpu_positions_sam(positions, count, None if s is None else C.byref(s), out_, capacity, out_bytes, None, C.byref(nlines), None)

    no_bytes = capi.NameTable(None, 4, capi.ptr(spans).value, 1)
    no_spans = capi.NameTable(capi.ptr(names).value, 4, None, 1)
    cases = [
        (lambda: call(None), b"spec is null"),
        (lambda: call(spec(char_of=None)), b"char_of is null"),
        (lambda: call(spec(), out_bytes=None), b"out_bytes is null"),
        (lambda: call(spec(qbuf=None)), b"qbuf is null while nq > 0"),
        (lambda: call(spec(qoff=None)), b"qoff is null while nq > 0"),
        (lambda: call(spec(), positions=None), b"positions is null while count > 0"),
        (lambda: call(spec(), out_=None), b"out is null while capacity > 0"),
        (lambda: call(spec(cigar=2)), b"cigar must be 0 or 1"),
        (lambda: call(spec(emit_unmapped=2)), b"emit_unmapped must be 0 or 1"),
        (lambda: call(spec(secondary_seq=255)), b"secondary_seq must be 0 or 1"),
        (lambda: call(spec(reserved=(0, 0, 1))), b"reserved must be 0"),
        (lambda: call(spec(reserved=(1, 0, 0))), b"reserved must be 0"),
        (lambda: call(spec(strands=capi.Strands(None, 5, 0))), b"strands has a null complement"),
        (lambda: call(spec(strands=capi.Strands(COMP.ctypes.data_as(capi.u8p), 0, 0))), b"strands->n must be in [1, 256]"),
        (lambda: call(spec(strands=capi.Strands(COMP.ctypes.data_as(capi.u8p), 257, 0))), b"strands->n must be in [1, 256]"),
        (lambda: call(spec(read_names=no_bytes)), b"the read_names table has no bytes but n_bytes > 0"),
        (lambda: call(spec(read_names=no_spans)), b"the read_names table has no spans but count > 0"),
        (lambda: call(spec(quals=no_bytes)), b"the quals table has no bytes but n_bytes > 0"),
        (lambda: call(spec(quals=no_spans)), b"the quals table has no spans but count > 0"),
        (lambda: call(spec(seq_names=no_bytes)), b"the seq_names table has no bytes but n_bytes > 0"),
        (lambda: call(spec(seq_names=no_spans)), b"the seq_names table has no spans but count > 0"),
        # the same with no record, and with no read: the checks do not depend on either
        (lambda: call(spec(reserved=(0, 9, 0)), positions=None, count=0), b"reserved must be 0"),
        (lambda: call(spec(qbuf=None, qoff=None, nq=0, cigar=3)), b"cigar must be 0 or 1"),
        (lambda: call(spec(char_of=None, qbuf=None, qoff=None, nq=0), positions=None, count=0), b"char_of is null"),
        # garbage pointers behind a bad spec are never looked at
        (lambda: call(spec(qbuf=garbage, qoff=garbage, reserved=(0, 1, 0)), positions=garbage, out_=garbage), b"reserved must be 0"),
    ]
    messages = set()
    for run, word in cases:
        nbytes.value = 7
        assert run() == capi.FMGPU_ERR_INVALID and word in last_error(), (word, last_error())
        messages.add(last_error())
    assert len(messages) >= 19                                           # each check has a message of its own
    assert (out == 0xAA).all()
    # the bound on the lines: refused before anything is staged
    for count, nq, emit in (((1 << 32) - 256, 0, 0), (0, (1 << 32) - 256, 0), (0, (1 << 32) - 256, 1), (1 << 31, 1 << 31, 1)):
        assert call(spec(qbuf=garbage, qoff=garbage, nq=nq, emit_unmapped=emit), positions=garbage, count=count, out_=None, capacity=0) == capi.FMGPU_ERR_UNSUPPORTED
        assert b"2^32 - 256" in last_error()


def test_no_line_returns_zero_behind_the_checks():
    L = capi.lib()
    nbytes, nlines = C.c_uint64(7), C.c_uint64(7)
    off = np.full(3, 9, dtype=np.uint64)
    none = spec(qbuf=None, qoff=None, nq=0)
    assert L.fmgpu_positions_sam(None, 0, C.byref(none), None, 0, C.byref(nbytes), capi.ptr(off), C.byref(nlines), None) == 0
    assert nbytes.value == 0 and nlines.value == 0 and off.tolist() == [0, 9, 9]
    nbytes.value = nlines.value = 7
    quiet = spec(emit_unmapped=0)                                        # two reads, no record, no unmapped lines
    assert L.fmgpu_positions_sam(None, 0, C.byref(quiet), None, 0, C.byref(nbytes), None, None, None) == 0 and nbytes.value == 0
    # the Python layer: no line, no text
    empty = (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert fm.format_sam(np.zeros(0, dtype=POSITION_DTYPE), empty) == b""
    text, offsets = fm.format_sam(np.zeros(0, dtype=POSITION_DTYPE), (QBUF, QOFF), emit_unmapped=False, want_line_offsets=True)
    assert text == b"" and offsets.tolist() == [0]


def test_the_header_call_matches_the_model():
    names = [b"chr1 homo sapiens", b"chr2\tx", b"chrM", b"scaffold_17"]
    lengths = [248956422, 1, 16569, (1 << 40) + 7]
    for program in (None, "fmgpu-example"):
        want = model.sam_header(names, lengths, None if program is None else program.encode())
        assert fm.sam_header(names, lengths, program) == want
    assert fm.sam_header([], []) == b"@HD\tVN:1.6\tSO:unknown\n"
    assert fm.sam_header(names[2:3], lengths[2:3], "p") == b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chrM\tLN:16569\n@PG\tID:p\n"
    for bad in ([b"chr1", b""], [b"chr1", b" late"], [b"\tx"]):
        with pytest.raises(fm.FmgpuError) as e:
            fm.sam_header(bad, [1] * len(bad))
        assert e.value.code == capi.FMGPU_ERR_INVALID and "sequence %d has an empty name" % (len(bad) - 1) in str(e.value)
        with pytest.raises(model.SamError):
            model.sam_header(bad, [1] * len(bad))
    # the counting call, an exact capacity, and one byte short
    L = capi.lib()
    data, spans = fm.pack_names(names)
    table = capi.NameTable(capi.ptr(data).value, data.size, capi.ptr(spans).value, len(names))
    lens = np.array(lengths, dtype=np.uint64)
    want = model.sam_header(names, lengths, b"id")
    nbytes = C.c_uint64(0)
    assert L.fmgpu_sam_header(C.byref(table), capi.ptr(lens), 4, b"id", None, 0, C.byref(nbytes)) == 0 and nbytes.value == len(want)
    out = np.full(len(want) + 4, 0xAA, dtype=np.uint8)
    nbytes.value = 0
    assert L.fmgpu_sam_header(C.byref(table), capi.ptr(lens), 4, b"id", capi.ptr(out), len(want) - 1, C.byref(nbytes)) == capi.FMGPU_ERR_CAPACITY
    assert nbytes.value == len(want) and (out == 0xAA).all()
    assert L.fmgpu_sam_header(C.byref(table), capi.ptr(lens), 4, b"id", capi.ptr(out), len(want), C.byref(nbytes)) == 0
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xAA).all()
    assert L.fmgpu_sam_header(None, capi.ptr(lens), 4, None, None, 0, C.byref(nbytes)) == capi.FMGPU_ERR_INVALID and b"seq_names is null while nseq > 0" in last_error()
    assert L.fmgpu_sam_header(C.byref(table), capi.ptr(lens), 5, None, None, 0, C.byref(nbytes)) == capi.FMGPU_ERR_INVALID and b"fewer than nseq rows" in last_error()
    assert L.fmgpu_sam_header(C.byref(table), capi.ptr(lens), 4, None, None, 0, None) == capi.FMGPU_ERR_INVALID and b"out_bytes is null" in last_error()


def records(rows):
    return np.array([(q, s, p, e, 0) for q, s, p, e in rows], dtype=POSITION_DTYPE)


def test_the_model_writes_the_lines_of_the_header_text():
    """one read unique, one multi, one on strand 1, one unmapped, one with m = 0; written by hand"""
    reads = [[1, 2, 3, 4, 255], [1, 1, 2], [1, 2, 2, 4], [3, 3], []]
    qbuf, qoff = fm.flatten(reads)
    names = (b"r0 first/1r1\tx@@r4", [(0, 10), (10, 4), (14, 0), (14, 2), (16, 2)])
    quals = (b"ABCDEFGHIJKL!!", [(0, 5), (5, 3), (8, 4), (12, 2), (14, 0)])
    seqs = (b"chr1 the firstchrM", [(0, 14), (14, 4)])
    # qidx counts both strands: read 0 once on strand 0; read 1 three times, twice with one error (strand 0 then 1) and once with two; read 2 on strand 1; read 4 (empty)
    rec = records([(0, 0, 99, 0), (2, 1, 5, 2), (2, 0, 7, 1), (3, 1, 9, 1), (5, 0, 0, 3), (8, 1, 41, 0)])
    text, off = model.format_sam(rec, qbuf, qoff, CHAR_OF, fm.DNA5_COMPLEMENT, names, quals, seqs)
    want = [b"r0\t0\tchr1\t100\t60\t5M\t*\t0\t0\tACGTN\tABCDE\tNM:i:0\tNH:i:1\n",
            b"r1\t256\tchrM\t6\t0\t3M\t*\t0\t0\t*\t*\tNM:i:2\tNH:i:3\n",
            b"r1\t0\tchr1\t8\t0\t3M\t*\t0\t0\tAAC\tFGH\tNM:i:1\tNH:i:3\n",
            b"r1\t272\tchrM\t10\t0\t3M\t*\t0\t0\t*\t*\tNM:i:1\tNH:i:3\n",
            b"*\t16\tchr1\t1\t60\t4M\t*\t0\t0\tAGGT\tLKJI\tNM:i:3\tNH:i:1\n",
            b"@@\t4\t*\t0\t0\t*\t*\t0\t0\tGG\t!!\n",
            b"r4\t0\tchrM\t42\t60\t*\t*\t0\t0\t*\t*\tNM:i:0\tNH:i:1\n"]
    assert text == b"".join(want)
    assert off == [sum(len(w) for w in want[:k]) for k in range(len(want) + 1)]
    # secondary_seq: the secondary records carry their own strand's SEQ and QUAL; cigar = 0; no tables; no unmapped lines
    text, _ = model.format_sam(rec[1:4], qbuf, qoff, CHAR_OF, fm.DNA5_COMPLEMENT, cigar=0, emit_unmapped=0, secondary_seq=1, mapq_unique=40, mapq_multi=3)
    assert text == (b"1\t256\t1\t6\t3\t*\t*\t0\t0\tAAC\t*\tNM:i:2\tNH:i:3\n1\t0\t0\t8\t3\t*\t*\t0\t0\tAAC\t*\tNM:i:1\tNH:i:3\n"
                    b"1\t272\t1\t10\t3\t*\t*\t0\t0\tGTT\t*\tNM:i:1\tNH:i:3\n")
    # without strands the read is qidx itself
    text, _ = model.format_sam(records([(3, 7, 0, 0)]), qbuf, qoff, CHAR_OF, emit_unmapped=0)
    assert text == b"3\t0\t7\t1\t60\t2M\t*\t0\t0\tGG\t*\tNM:i:0\tNH:i:1\n"
    # what the device refuses, in the header's order
    for bad, who, index, what in ((records([(0, 0, 0, 0), (10, 0, 0, 0)]), "record", 1, "range"), (records([(2, 0, 0, 0), (1, 0, 0, 0)]), "record", 1, "order")):
        with pytest.raises(model.SamError) as e:
            model.format_sam(bad, qbuf, qoff, CHAR_OF, fm.DNA5_COMPLEMENT)
        assert (e.value.code, e.value.who, e.value.index, e.value.what) == (model.INVALID, who, index, what)
    with pytest.raises(model.SamError) as e:
        model.format_sam(rec, qbuf, qoff, CHAR_OF, fm.DNA5_COMPLEMENT, quals=(b"ABCD", [(0, 4)] * 5))
    assert (e.value.who, e.value.index, e.value.what) == ("record", 0, "quals len")
    with pytest.raises(model.SamError) as e:
        model.format_sam(rec, qbuf, qoff, CHAR_OF, fm.DNA5_COMPLEMENT, read_names=(b"ab", [(0, 1)] * 3))
    assert (e.value.who, e.value.index, e.value.what) == ("unmapped read", 3, "read_names row")
    # what is too long is judged by the stated sizes, and an invalid line anywhere goes first
    big = 1 << 31
    with pytest.raises(model.SamError) as e:
        model.format_sam(records([(0, 0, 0, 0)]), qbuf, [0, big, big + 2], CHAR_OF, fm.DNA5_COMPLEMENT)
    assert (e.value.code, e.value.who, e.value.index, e.value.what) == (model.UNSUPPORTED, "record", 0, "read")
    with pytest.raises(model.SamError) as e:
        model.format_sam(records([(1, 0, 0, 0)]), qbuf, [0, big - 1], CHAR_OF, fm.DNA5_COMPLEMENT, quals=(b"ab", [(0, big - 1)], big))
    assert (e.value.code, e.value.what) == (model.UNSUPPORTED, "line")
    with pytest.raises(model.SamError) as e:
        model.format_sam(records([(0, 0, 0, 0), (2, 9, 0, 0)]), qbuf, [0, big, big + 2], CHAR_OF, fm.DNA5_COMPLEMENT, seq_names=(b"ab", [(0, 2)]))
    assert (e.value.code, e.value.who, e.value.index, e.value.what) == (model.INVALID, "record", 1, "seq_names row")
