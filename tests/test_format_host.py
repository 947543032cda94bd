"""fmgpu_positions_format (include/fmgpu.h) on the host: the symbol and the two structs, every argument check that comes before the first use of the device, count == 0,
the plain-Python model of tests/format_model.py against printf on hand-made records, and the name-packing helper of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import POSITION_DTYPE, TEXT_SPAN_DTYPE
from tests import format_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def last_error():
    return capi.lib().fmgpu_last_error()


def test_the_symbol_exists_and_abi_version_and_option_count_stay():
    L = capi.lib()
    assert "fmgpu_positions_format" in capi.EXPORTS and hasattr(L, "fmgpu_positions_format")
    assert re.search(r"\bint\s+fmgpu_positions_format\s*\(", header())
    assert L.fmgpu_abi_version() == 6 and re.search(r"#define FMGPU_ABI_VERSION 6\b", header())
    assert re.search(r"FMGPU_OPT_COUNT_ = 13\b", header()) and len(capi.OPTIONS) == 13


def struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[\d+\]", "", d.split()[-1]).lstrip("*") for d in body.split(";") if d.strip()]


def test_the_structs_mirror_the_header():
    assert C.sizeof(capi.FormatSpec) == 40 and C.sizeof(capi.NameTable) == 32
    assert [f[0] for f in capi.FormatSpec._fields_] == struct_fields("fmgpu_format_spec") == \
        ["n_cols", "cols", "sep", "strand_shift", "name_stop", "reserved", "pos_add", "read_names", "seq_names"]
    S = capi.FormatSpec
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 4, 12, 13, 14, 15, 16, 24, 32]
    assert [f[0] for f in capi.NameTable._fields_] == struct_fields("fmgpu_name_table") == ["bytes", "n_bytes", "spans", "count"]
    assert [getattr(capi.NameTable, f[0]).offset for f in capi.NameTable._fields_] == [0, 8, 16, 24]
    for name, code in capi.COLUMNS.items():
        assert re.search(r"#define FMGPU_COL_%s\s+%d\b" % (name.upper(), code), header()), name
    assert sorted(capi.COLUMNS.values()) == list(range(9))
    assert (model.QIDX, model.SEQ_ID, model.POS, model.ERRORS, model.HIT, model.READ, model.STRAND, model.READ_NAME, model.SEQ_NAME) == \
        tuple(capi.COLUMNS[k] for k in ("qidx", "seq_id", "pos", "errors", "hit", "read", "strand", "read_name", "seq_name"))


def spec(cols=(0, 1, 2, 3), n_cols=None, sep=32, strand_shift=0, name_stop=0, reserved=0, read_names=None, seq_names=None):
    cols = list(cols) + [0] * (8 - len(cols))
    return capi.FormatSpec(len([c for c in cols]) if n_cols is None else n_cols, (C.c_uint8 * 8)(*cols), sep, strand_shift, name_stop, reserved, 0,
                           None if read_names is None else C.pointer(read_names), None if seq_names is None else C.pointer(seq_names))


def test_argument_checks_come_before_the_device():
    L = capi.lib()
    rec = np.zeros(2, dtype=POSITION_DTYPE)
    out = np.full(64, 0xAA, dtype=np.uint8)
    garbage = C.c_void_p(0x10)                                           # never read through: the checks come first
    nbytes = C.c_uint64(7)
    names = np.zeros(4, dtype=np.uint8)
    spans = np.zeros(1, dtype=TEXT_SPAN_DTYPE)

    def call(s, positions=capi.ptr(rec), out_=capi.ptr(out), capacity=64, out_bytes=C.byref(nbytes)):
        return L.fmgpu_positions_format(positions, 2, None if s is None else C.byref(s), out_, capacity, out_bytes, None, None)

    good4 = lambda **kw: spec(n_cols=4, **kw)                            # noqa: E731
    cases = [
        (lambda: call(None), b"spec is null"),
        (lambda: call(good4(), positions=None), b"positions is null"),
        (lambda: call(good4(), out_bytes=None), b"out_bytes is null"),
        (lambda: call(good4(), out_=None), b"out is null while capacity > 0"),
        (lambda: call(spec(n_cols=0)), b"n_cols must be in [1, 8]"),
        (lambda: call(spec(n_cols=9)), b"n_cols must be in [1, 8]"),
        (lambda: call(spec(n_cols=-1)), b"n_cols must be in [1, 8]"),
        (lambda: call(spec(cols=(0, 9), n_cols=2)), b"unknown column code 9"),
        (lambda: call(spec(cols=(0, 1, 255), n_cols=3)), b"unknown column code 255"),
        (lambda: call(good4(strand_shift=2)), b"strand_shift must be 0 or 1"),
        (lambda: call(good4(name_stop=2)), b"name_stop must be 0 or 1"),
        (lambda: call(good4(reserved=1)), b"reserved must be 0"),
        (lambda: call(spec(cols=(7,), n_cols=1)), b"a read_names column needs the read_names table"),
        (lambda: call(spec(cols=(0, 8), n_cols=2)), b"a seq_names column needs the seq_names table"),
        (lambda: call(spec(cols=(7,), n_cols=1, read_names=capi.NameTable(None, 4, capi.ptr(spans).value, 1))), b"the read_names table has no bytes but n_bytes > 0"),
        (lambda: call(spec(cols=(7,), n_cols=1, read_names=capi.NameTable(capi.ptr(names).value, 4, None, 1))), b"the read_names table has no spans but count > 0"),
        (lambda: call(spec(cols=(8,), n_cols=1, seq_names=capi.NameTable(None, 1, None, 0))), b"the seq_names table has no bytes but n_bytes > 0"),
        (lambda: call(spec(cols=(8,), n_cols=1, seq_names=capi.NameTable(None, 0, None, 3))), b"the seq_names table has no spans but count > 0"),
        # garbage pointers behind a bad spec are never looked at
        (lambda: call(spec(n_cols=0), positions=garbage, out_=garbage), b"n_cols must be in [1, 8]"),
        (lambda: call(good4(reserved=9), positions=garbage, out_=garbage), b"reserved must be 0"),
    ]
    messages = set()
    for run, word in cases:
        nbytes.value = 7
        assert run() == capi.FMGPU_ERR_INVALID and word in last_error(), (word, last_error())
        messages.add(last_error())
    assert len(messages) >= 16                                           # each check has a message of its own
    # a column code beyond n_cols is not looked at; a table nobody asks for is not either (the call then goes on to the device, which is not tried here)
    assert (out == 0xAA).all()
    # 2^32 records: refused before anything is staged
    assert L.fmgpu_positions_format(garbage, 1 << 32, C.byref(good4()), None, 0, C.byref(nbytes), None, None) == capi.FMGPU_ERR_UNSUPPORTED
    assert b"grid limit" in last_error()


def test_no_record_returns_zero_before_anything_is_looked_at():
    L = capi.lib()
    nbytes = C.c_uint64(7)
    off = np.full(3, 9, dtype=np.uint64)
    garbage = C.c_void_p(0x10)
    assert L.fmgpu_positions_format(None, 0, None, None, 0, C.byref(nbytes), capi.ptr(off), None) == 0
    assert nbytes.value == 0 and off.tolist() == [0, 9, 9]
    nbytes.value = 7
    bad = spec(n_cols=0, reserved=3)
    assert L.fmgpu_positions_format(garbage, 0, C.byref(bad), garbage, 5, C.byref(nbytes), None, None) == 0 and nbytes.value == 0
    assert L.fmgpu_positions_format(None, 0, None, None, 0, None, None, None) == 0
    # the Python layer: no record, no text
    assert fm.format_positions(np.zeros(0, dtype=POSITION_DTYPE)) == b""
    text, offsets = fm.format_positions(np.zeros(0, dtype=POSITION_DTYPE), want_line_offsets=True)
    assert text == b"" and offsets.tolist() == [0]


def records(rows):
    return np.array(rows, dtype=POSITION_DTYPE)


def test_the_model_equals_printf_on_hand_made_records():
    rec = records([(0, 0, 0, 0, 0), (9, 10, 99, 100, 7), (123456, 7, 123456789, 2, 1), ((1 << 64) - 1, 1 << 32, (1 << 32) - 1, (1 << 32) - 1, 5)])
    text, off = model.format_positions(rec)
    want = b"".join(b"%d %d %d %d\n" % (int(r["qidx"]), int(r["seq_id"]), int(r["pos"]), int(r["errors"])) for r in rec)
    assert text == want and text.splitlines()[2] == b"123456 7 123456789 2" and len(b"123456 7 123456789 2\n") == 21
    assert off[0] == 0 and off[-1] == len(text) and [text[off[i]: off[i + 1]] for i in range(4)] == want.splitlines(keepends=True)
    assert model.format_positions(rec, (0, 1, 2))[0] == b"".join(b"%d %d %d\n" % (int(r["qidx"]), int(r["seq_id"]), int(r["pos"])) for r in rec)
    assert model.format_positions([], (0,)) == (b"", [0])
    # pos_add wraps mod 2^64; a column twice; tabs
    one = records([(5, 1, (1 << 64) - 1, 0, 3)])
    assert model.format_positions(one, (2, 2, 4), b"\t", pos_add=1)[0] == b"0\t0\t3\n"
    assert model.format_positions(one, (2,), pos_add=(1 << 64) - 1)[0] == b"%d\n" % ((1 << 64) - 2)


def test_the_model_strands_and_names():
    rec = records([(4, 1, 10, 0, 0), (5, 0, 20, 1, 1), (0, 1, 30, 2, 2)])
    reads = (b"r0 first\tx" + b"r1" + b" r2", [(0, 10), (10, 2), (12, 3)])
    seqs = (b"chr1chrM extra", [(0, 4), (4, 10)])
    cols = (model.READ_NAME, model.SEQ_NAME, model.POS, model.STRAND, model.READ, model.ERRORS)
    assert model.format_positions(rec, cols, b"\t", 1, True, 1, reads, seqs)[0] == b"\tchrM\t11\t+\t2\t0\n\tchr1\t21\t-\t2\t1\nr0\tchrM\t31\t+\t0\t2\n"
    assert model.format_positions(rec[2:], cols, b" ", 0, False, 0, reads, seqs)[0] == b"r0 first\tx chrM extra 30 + 0 2\n"
    # strand_shift 0: every qidx is its own read and the strand is '+'
    assert model.format_positions(rec[:2], (model.READ, model.STRAND), b" ", 0)[0] == b"4 +\n5 +\n"
    # the lowest offending record, and INVALID in front of UNSUPPORTED
    with pytest.raises(model.FormatError) as e:
        model.format_positions(rec, (model.READ_NAME,), read_names=reads)
    assert (e.value.code, e.value.record, e.value.what) == (model.INVALID, 0, "row")
    with pytest.raises(model.FormatError) as e:
        model.format_positions(rec, (model.SEQ_NAME,), seq_names=(b"chr1", [(0, 4), (2, 3)]))
    assert (e.value.code, e.value.record, e.value.what) == (model.INVALID, 0, "span")
    with pytest.raises(model.FormatError) as e:
        model.format_positions(rec[1:], (model.SEQ_NAME,), seq_names=(b"chr1", [(0, 4), (2, 3)]))
    assert (e.value.code, e.value.record) == (model.INVALID, 1)


def test_pack_names_and_the_python_facade_without_a_device():
    data, spans = fm.pack_names([b"ab", "", "xyz", b"q r"])
    assert data.tobytes() == b"abxyzq r" and spans.dtype == TEXT_SPAN_DTYPE and spans.tolist() == [(0, 2), (2, 0), (2, 3), (5, 3)]
    assert fm.ParsedQueries.texts(data, spans) == [b"ab", b"", b"xyz", b"q r"]
    data, spans = fm.pack_names([])
    assert data.size == 0 and spans.size == 0
    table, keep = fm._name_table([b"ab", b"c"])
    assert (table.n_bytes, table.count) == (3, 2) and table.bytes == keep[0].ctypes.data and table.spans == keep[1].ctypes.data
    table, keep = fm._name_table((b"abc", np.array([(1, 2)], dtype=TEXT_SPAN_DTYPE)))
    assert (table.n_bytes, table.count) == (3, 1)
    rec = records([(1, 2, 3, 4, 5)])
    with pytest.raises(ValueError):
        fm.format_positions(rec, columns=())
    with pytest.raises(ValueError):
        fm.format_positions(rec, columns=("qidx",) * 9)
    with pytest.raises(ValueError):
        fm.format_positions(rec, sep="ab")
    with pytest.raises(ValueError):
        fm.format_positions(rec, columns=("read_name",))
    with pytest.raises(KeyError):
        fm.format_positions(rec, columns=("nonsense",))
