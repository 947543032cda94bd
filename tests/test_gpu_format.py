"""fmgpu_positions_format on the device (include/fmgpu.h): every output is compared byte for byte with the plain-Python model of tests/format_model.py.  The shapes are the
smallest at which the kernels can go wrong: digit boundaries, tiles of 256 records and 16-byte pieces, every output alignment, a name longer than a workgroup's LDS window.
Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import POSITION_DTYPE, TEXT_SPAN_DTYPE, DeviceBuffer
from tests import format_model as model

pytestmark = pytest.mark.gpu
NAMES = ["qidx", "seq_id", "pos", "errors", "hit", "read", "strand", "read_name", "seq_name"]
U64, U32 = (1 << 64) - 1, (1 << 32) - 1


def check(rec, columns=("qidx", "seq_id", "pos", "errors"), sep=" ", strands=False, name_stop=False, pos_add=0, read_names=None, seq_names=None, device_names=False, **kw):
    """format_positions against the model; the text"""
    want, woff = model.format_positions(rec, [capi.COLUMNS[c] for c in columns], sep.encode(), 1 if strands else 0, name_stop, pos_add, read_names, seq_names)
    tables = {}
    for key, t in (("read_names", read_names), ("seq_names", seq_names)):
        if t is not None:
            data, spans = np.frombuffer(bytes(t[0]), dtype=np.uint8), np.asarray(t[1], dtype=TEXT_SPAN_DTYPE)
            tables[key] = (DeviceBuffer.from_array(data), DeviceBuffer.from_array(spans)) if device_names and data.size >= 8 and spans.size else (data, spans)
    got, off = fm.format_positions(rec, columns=columns, sep=sep, strands=strands, name_stop=name_stop, pos_add=pos_add, want_line_offsets=True, **tables, **kw)
    assert got == want, (columns, len(rec), got[:200], want[:200])
    assert off.tolist() == woff
    return got


@functools.lru_cache(maxsize=None)
def boundary_records():
    """fields that run through 0, 9, 10, 99, 100, ..., 10^k - 1, 10^k for every k up to 19, and 2^32 - 1, 2^32, 2^64 - 1 (the 32-bit fields: what fits, and 2^32 - 1)"""
    wide = sorted({0, U32, 1 << 32, U64} | {10 ** k for k in range(20)} | {10 ** k - 1 for k in range(1, 20)})
    narrow = [v for v in wide if v <= U32]
    n = len(wide)
    rec = np.zeros(n, dtype=POSITION_DTYPE)
    rec["qidx"] = np.array(wide, dtype=np.uint64)
    rec["seq_id"] = np.array(wide[::-1], dtype=np.uint64)
    rec["pos"] = np.array(wide[n // 2:] + wide[: n // 2], dtype=np.uint64)
    rec["errors"] = np.array([narrow[i % len(narrow)] for i in range(n)], dtype=np.uint32)
    rec["hit"] = np.array([narrow[-1 - i % len(narrow)] for i in range(n)], dtype=np.uint32)
    return rec


def test_digit_boundaries():
    rec = boundary_records()
    text = check(rec, ("qidx", "seq_id", "pos", "errors", "hit"))
    assert b"18446744073709551615" in text and b" 4294967295\n" in text and text.startswith(b"0 18446744073709551615 ")
    # pos_add that wraps: 2^64 - 1 + 1 = 0, 10^19 + (2^64 - 10^19) = 0, and one that carries into a new digit
    for add in (1, U64, (1 << 64) - 10 ** 19, 1 << 63):
        check(rec, ("pos", "qidx"), pos_add=add)
    # exactly the example's line, and the three-column file of the other modes
    assert check(rec) == b"".join(b"%d %d %d %d\n" % (int(r["qidx"]), int(r["seq_id"]), int(r["pos"]), int(r["errors"])) for r in rec)
    check(rec, ("qidx", "seq_id", "pos"))


def random_records(count, seed, reads=None, seqs=None):
    """random field widths: every number of digits is as likely as any other, so lines straddle every 16-byte piece and every workgroup's range"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(count, dtype=POSITION_DTYPE)

    for name, bits in (("qidx", 64), ("seq_id", 64), ("pos", 64), ("errors", 32), ("hit", 32)):
        width = rng.integers(1, bits + 1, size=count).astype(np.uint64)                  # the bit length of every value
        v = rng.integers(0, U64, size=count, dtype=np.uint64, endpoint=True) >> (np.uint64(64) - width)
        v[rng.integers(0, count, size=max(1, count // 16))] = 0
        rec[name] = v.astype(rec[name].dtype)
    if reads is not None:
        rec["qidx"] = rng.integers(0, reads, size=count)
    if seqs is not None:
        rec["seq_id"] = rng.integers(0, seqs, size=count)
    return rec


@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 3 * 256 + 1, 5000])
def test_tile_and_piece_boundaries(count):
    rec = random_records(count, seed=count)
    check(rec, ("qidx", "seq_id", "pos", "errors"))
    check(rec, ("errors",))                                              # short lines: many per 16-byte piece
    check(rec, ("qidx", "seq_id", "pos", "errors", "hit", "pos", "qidx", "seq_id"), pos_add=12345)      # long lines


def make_spec(columns, sep=" ", strand_shift=0, name_stop=0, pos_add=0, read_names=None, seq_names=None):
    cols = [capi.COLUMNS[c] for c in columns]
    return capi.FormatSpec(len(cols), (C.c_uint8 * 8)(*(cols + [0] * (8 - len(cols)))), ord(sep), strand_shift, name_stop, 0, pos_add,
                           None if read_names is None else C.pointer(read_names), None if seq_names is None else C.pointer(seq_names))


def raw(pos, count, spec, out, capacity, off=None):
    n = C.c_uint64(123)
    rc = capi.lib().fmgpu_positions_format(capi.ptr(pos), count, C.byref(spec), capi.ptr(out), capacity, C.byref(n), capi.ptr(off), None)
    return rc, int(n.value)


def test_every_output_alignment_and_the_guard_bytes():
    rec = random_records(700, seed=3)
    cols = ("qidx", "seq_id", "pos", "errors")
    want, _ = model.format_positions(rec, [capi.COLUMNS[c] for c in cols])
    spec, dpos = make_spec(cols), DeviceBuffer.from_array(rec)
    guard = 64
    for shift in range(16):
        fill = np.full(guard + 16 + len(want) + guard, 0xAA, dtype=np.uint8)
        buf = DeviceBuffer.from_array(fill)
        assert buf.ptr % 256 == 0
        rc, n = raw(dpos, len(rec), spec, buf.ptr + guard + shift, len(want))
        assert rc == 0 and n == len(want), capi.lib().fmgpu_last_error()
        back = buf.to_array(np.uint8, fill.size)
        assert back[guard + shift: guard + shift + n].tobytes() == want, shift
        assert (back[: guard + shift] == 0xAA).all() and (back[guard + shift + n:] == 0xAA).all(), shift
    # records at an odd multiple of 8 bytes: no 16-byte loads there
    pad = DeviceBuffer.from_array(np.concatenate([np.zeros(8, dtype=np.uint8), rec.view(np.uint8)]))
    out = np.zeros(len(want), dtype=np.uint8)
    assert raw(pad.ptr + 8, len(rec), spec, out, len(want)) == (0, len(want)) and out.tobytes() == want


def test_columns():
    reads = (b"alpha beta" + b"r1\tx" + b"gamma", [(0, 10), (10, 4), (14, 5)])
    seqs = (b"chr1chr22 len=5", [(0, 4), (4, 11)])
    rec = random_records(300, seed=9, reads=6, seqs=2)
    for col in NAMES:                                                    # every column code alone: n_cols = 1
        check(rec, (col,), strands=True, read_names=reads, seq_names=seqs)
    for sep in (" ", "\t"):
        check(rec, tuple(NAMES[:8]), sep=sep, strands=True, read_names=reads, seq_names=seqs)          # n_cols = 8
        check(rec, ("seq_name", "pos", "seq_name", "read_name", "read_name", "pos"), sep=sep, strands=True, name_stop=True, read_names=reads, seq_names=seqs, pos_add=1)
    # strand_shift 0: read = qidx, the strand is always '+'; a read_names row indexed by qidx itself
    rec0 = random_records(300, seed=10, reads=3, seqs=2)
    text = check(rec0, ("read", "strand", "read_name", "qidx"), read_names=reads, seq_names=seqs)
    assert b"-" not in text
    text = check(rec, ("read", "strand", "read_name", "qidx"), strands=True, read_names=reads)
    assert b" - " in text and b" + " in text


@functools.lru_cache(maxsize=None)
def long_names():
    """names of 0, 1, 15, 16, 17, 300 and 70 000 bytes (the last makes a tile larger than any LDS window); blanks at byte 0, in the middle and nowhere"""
    rng = np.random.default_rng(17)
    names = [bytes(rng.integers(33, 127, size=m, dtype=np.uint8)) for m in (0, 1, 15, 16, 17, 300, 70000)]
    names += [b" starts with a blank", b"middle\tblank here", b"no_blank_at_all", b"x" * 40 + b" " + b"y" * 40, bytes(rng.integers(33, 127, size=200, dtype=np.uint8)) + b"\t" + b"z" * 100]
    return fm.pack_names(names), len(names)


@pytest.mark.parametrize("device_names", [False, True])
def test_names_of_every_length(device_names):
    (data, spans), n = long_names()
    rec = random_records(600, seed=21, reads=n, seqs=n)
    rec["qidx"][rec["qidx"] == 6] = 5
    rec["qidx"][[50, 150, 250, 350, 450, 550]] = 6                       # the 70 000-byte name: six times as a read name
    rec["seq_id"][rec["seq_id"] == 6] = 4
    rec["seq_id"][[100, 420]] = 6                                        # ... and twice as a sequence name
    for stop in (False, True):
        text = check(rec, ("read_name", "seq_name", "pos", "errors"), sep="\t", name_stop=stop, read_names=(data, spans), seq_names=(data, spans), device_names=device_names)
        assert len(text) > 8 * 70000
    check(rec[:3], ("seq_name", "read_name", "seq_name"), read_names=(data, spans), seq_names=(data, spans), device_names=device_names)
    # both strands: the row is qidx >> 1
    check(rec, ("read_name", "strand", "qidx"), strands=True, name_stop=True, read_names=(data, spans), device_names=device_names)


def test_memory_combinations():
    rec = random_records(777, seed=5)
    cols = ("qidx", "seq_id", "pos", "errors")
    want, woff = model.format_positions(rec, [capi.COLUMNS[c] for c in cols])
    spec, dpos = make_spec(cols), DeviceBuffer.from_array(rec)
    for pos in (rec, dpos):
        for dev_out in (False, True):
            for dev_off in (False, True):
                out = DeviceBuffer(len(want)) if dev_out else np.zeros(len(want), dtype=np.uint8)
                off = DeviceBuffer((len(rec) + 1) * 8) if dev_off else np.zeros(len(rec) + 1, dtype=np.uint64)
                assert raw(pos, len(rec), spec, out, len(want), off) == (0, len(want)), capi.lib().fmgpu_last_error()
                assert (out.to_array(np.uint8, len(want)) if dev_out else out).tobytes() == want
                assert (off.to_array(np.uint64, len(rec) + 1) if dev_off else off).tolist() == woff
    # the Python layer with device records and a device result
    (buf, n), off = fm.format_positions(dpos, device=True, want_line_offsets=True)
    assert n == len(want) and buf.to_array(np.uint8, n).tobytes() == want and off.tolist() == woff
    # no record and a device out_line_off: one zero
    doff = DeviceBuffer.from_array(np.full(2, 9, dtype=np.uint64))
    assert raw(None, 0, spec, None, 0, doff) == (0, 0) and doff.to_array(np.uint64, 2).tolist() == [0, 9]


def test_capacity_and_the_counting_call():
    rec = random_records(600, seed=6)
    cols = ("qidx", "pos", "hit")
    want, woff = model.format_positions(rec, [capi.COLUMNS[c] for c in cols])
    spec = make_spec(cols)
    for dev in (False, True):
        sentinel = np.full(len(want), 0xAA, dtype=np.uint8)
        out = DeviceBuffer.from_array(sentinel) if dev else sentinel.copy()
        off = np.zeros(len(rec) + 1, dtype=np.uint64)
        rc, n = raw(rec, len(rec), spec, out, len(want) - 1, off)
        assert rc == capi.FMGPU_ERR_CAPACITY and n == len(want) and off.tolist() == woff
        assert ((out.to_array(np.uint8, len(want)) if dev else out) == 0xAA).all()
        assert raw(rec, len(rec), spec, out, len(want), None) == (0, len(want))          # exactly enough
        assert (out.to_array(np.uint8, len(want)) if dev else out).tobytes() == want
    off = np.zeros(len(rec) + 1, dtype=np.uint64)
    assert raw(rec, len(rec), spec, None, 0, off) == (0, len(want)) and off.tolist() == woff


def test_device_side_errors_name_the_lowest_record():
    L = capi.lib()
    (data, spans), n = fm.pack_names([b"one", b"two", b"three"]), 3
    rec = random_records(900, seed=8, reads=3, seqs=3)
    sentinel = np.full(1 << 16, 0xAA, dtype=np.uint8)
    off0 = np.full(len(rec) + 1, 7, dtype=np.uint64)
    for dev in (False, True):
        for what in ("row", "span"):
            r, sp = rec.copy(), spans.copy()
            if what == "row":
                r["qidx"][[700, 333]] = (3, 1 << 40)                     # beyond the table, at two records
            else:
                sp["len"][1] = 9                                         # 3 + 9 > 11 bytes
                r["qidx"] = 0
                r["qidx"][[801, 258]] = 1
            with pytest.raises(model.FormatError) as e:
                model.format_positions(r, (model.READ_NAME, model.POS), read_names=(data, sp))
            lowest = 333 if what == "row" else 258
            assert (e.value.code, e.value.record, e.value.what) == (model.INVALID, lowest, what)
            keep = (DeviceBuffer.from_array(data), DeviceBuffer.from_array(sp)) if dev else (data, sp)
            table = capi.NameTable(capi.ptr(keep[0]).value, data.size, capi.ptr(keep[1]).value, 3)
            spec = make_spec(("read_name", "pos"), read_names=table)
            out = DeviceBuffer.from_array(sentinel) if dev else sentinel.copy()
            off = off0.copy()
            rc, _ = raw(r, len(r), spec, out, sentinel.size, off)
            assert rc == capi.FMGPU_ERR_INVALID and (b"record %d " % lowest) in L.fmgpu_last_error(), L.fmgpu_last_error()
            assert ((out.to_array(np.uint8, sentinel.size) if dev else out) == 0xAA).all() and (off == 7).all()
            # the next call on the same thread succeeds
            check(rec, ("read_name", "pos"), read_names=(data, spans))
    # a span of 2^31 bytes (inside a table that says it is that large: the measuring pass reads no name byte without name_stop)
    big = np.array([(0, 1 << 31)], dtype=TEXT_SPAN_DTYPE)
    keep = (DeviceBuffer.from_array(data), DeviceBuffer.from_array(big))
    table = capi.NameTable(keep[0].ptr, (1 << 31) + 5, keep[1].ptr, 1)
    one = np.zeros(2, dtype=POSITION_DTYPE)
    rc, _ = raw(one, 2, make_spec(("seq_name",), seq_names=table), None, 0)
    assert rc == capi.FMGPU_ERR_UNSUPPORTED and b"record 0 " in L.fmgpu_last_error() and b"2^31" in L.fmgpu_last_error()


def test_chained_behind_map_reads():
    from tests.test_gpu_map import batch, index
    gx = index("bi")
    _, qbuf, qoff = batch(5)
    pos = fm.map_reads(gx, (qbuf, qoff), errors=1, edit=False)
    assert len(pos) > 20
    check(pos)
    check(pos, ("read", "seq_name", "pos", "errors", "hit"), sep="\t", pos_add=1, seq_names=(b"s0s1s2", [(0, 2), (2, 2), (4, 2)]))
    dpos = DeviceBuffer.from_array(pos)
    assert fm.format_positions(dpos) == model.format_positions(pos)[0]


def test_chained_behind_map_text_with_both_strands_and_read_names():
    from tests.test_gpu_strands import file_text, index, map_args, table
    gx = index("bi")
    for fmt in ("fasta", "fastq"):
        data = file_text(fmt, "hamming")
        with fm.Feed(gx, slots=2, host_threads=2) as feed:
            m = feed.map_text(data, fmt, table(), want_names=True, strands="dna5", pair=True, chunk_bytes=257, **map_args("hamming"))
        pos = np.ascontiguousarray(m.positions)
        assert len(pos) > 20 and (pos["qidx"] & 1).any() and not (pos["qidx"] & 1).all()
        cols = ("read_name", "seq_id", "pos", "strand", "errors")
        got = fm.format_positions(pos, columns=cols, sep="\t", strands=True, read_names=(data, m.names), name_stop=True, pos_add=1)
        want = model.format_positions(pos, [capi.COLUMNS[c] for c in cols], b"\t", 1, True, 1, read_names=(data, m.names))[0]
        assert got == want
        first = want.split(b"\n")[0].split(b"\t")
        assert first[0] == (b"read%d" if fmt == "fasta" else b"q%d") % (int(pos[0]["qidx"]) >> 1) and first[3] in (b"+", b"-")
