"""fmgpu_positions_sam on the device (include/fmgpu.h): every output, text and line offsets both, is compared byte for byte with the plain-Python model of
tests/sam_model.py.  The shapes are the smallest at which the kernels can go wrong: read lengths around the 16-byte pieces and the 64 lanes of a wave, a read longer than a
workgroup's window, record counts around the 256 lanes of a workgroup, every output alignment, unmapped reads at every place, one read with thousands of records.  One
end-to-end test (FASTQ text -> parse -> both-strand Hamming ladder -> SAM) checks the lines against the indexed text instead of the model.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import POSITION_DTYPE, TEXT_SPAN_DTYPE, DeviceBuffer
from tests import sam_model as model

pytestmark = pytest.mark.gpu
DNA5 = np.array(fm.DNA5_COMPLEMENT, dtype=np.uint8)
CHAR_OF = fm.char_table("dna5")
CODES = {model.INVALID: capi.FMGPU_ERR_INVALID, model.UNSUPPORTED: capi.FMGPU_ERR_UNSUPPORTED}
LENGTHS = [0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 101, 255, 256, 257, 20000]


def make_batch(lengths, seed, prefix=0):
    """(qbuf, qoff, read names, quals, seq names): random reads over 1 .. 4 with a few 255, names with blanks and empty ones, a quality string per read (none for every
    seventh); `prefix` bytes in front of the first read (qoff[0] = prefix)"""
    rng = np.random.default_rng(seed)
    reads = [rng.integers(1, 5, size=m).astype(np.uint8) for m in lengths]
    for r in reads:
        if r.size:
            r[rng.integers(0, r.size, size=1 + r.size // 50)] = 255
    qbuf = np.concatenate([np.full(prefix, 7, dtype=np.uint8)] + reads + [np.zeros(1, dtype=np.uint8)])
    qoff = (prefix + np.concatenate([[0], np.cumsum(lengths)])).astype(np.uint64)
    names = [b"" if i % 11 == 5 else b" hidden" if i % 11 == 7 else b"read_%d/1 len=%d\tx" % (i, m) if i % 2 else b"r%d" % i for i, m in enumerate(lengths)]
    quals = [b"" if i % 7 == 6 else bytes(rng.integers(33, 127, size=m).astype(np.uint8)) for i, m in enumerate(lengths)]
    seqs = [b"chr1 the first", b"", b"chrM", b"scaffold_0123456789_0123456789_0123456789_0123456789_0123456789_0123456789\tlong"]
    return qbuf, qoff, fm.pack_names(names), fm.pack_names(quals), fm.pack_names(seqs)


def make_records(per_read, seed, strands=True, errors=3, nseq=4, strand=None):
    """per_read[r] records for read r, in read order: random strand (or `strand`), seq_id, pos of every digit count, errors below `errors` (ties are common)"""
    rng = np.random.default_rng(seed)
    reads = np.repeat(np.arange(len(per_read), dtype=np.uint64), per_read)
    rec = np.zeros(reads.size, dtype=POSITION_DTYPE)
    st = rng.integers(0, 2, size=reads.size).astype(np.uint64) if strand is None else np.full(reads.size, strand, dtype=np.uint64)
    rec["qidx"] = 2 * reads + st if strands else reads
    rec["seq_id"] = rng.integers(0, nseq, size=reads.size)
    rec["pos"] = rng.integers(0, (1 << 63) - 1, size=reads.size, dtype=np.uint64) >> rng.integers(0, 63, size=reads.size).astype(np.uint64)
    rec["errors"] = rng.integers(0, errors, size=reads.size)
    rec["hit"] = np.arange(reads.size)
    return rec


def table_model(t):
    """(data, spans) or (data, spans, stated n_bytes) as the model takes it"""
    return None if t is None else (t[0].tobytes(), [(int(s["offset"]), int(s["len"])) for s in t[1]]) + tuple(t[2:])


def on_device(t):
    data, spans = t
    return (DeviceBuffer.from_array(np.concatenate([data, np.zeros(8, dtype=np.uint8)])), DeviceBuffer.from_array(spans)) if spans.size else t


def check(rec, qbuf, qoff, strands=True, read_names=None, quals=None, seq_names=None, device=(), **kw):
    """format_sam against the model, text and line offsets; `device`: which of "positions", "queries", "read_names", "quals", "seq_names" lie in device memory"""
    mkw = {k: (1 if v else 0) for k, v in kw.items() if k != "mapq"}
    if "mapq" in kw:
        mkw["mapq_unique"], mkw["mapq_multi"] = kw["mapq"]
    want, woff = model.format_sam(rec, qbuf, qoff, CHAR_OF, DNA5 if strands else None, table_model(read_names), table_model(quals), table_model(seq_names), **mkw)
    tables = {k: (on_device(t) if k in device and t is not None else t) for k, t in (("read_names", read_names), ("quals", quals), ("seq_names", seq_names))}
    queries = (DeviceBuffer.from_array(qbuf), DeviceBuffer.from_array(qoff)) if "queries" in device else (qbuf, qoff)
    positions = DeviceBuffer.from_array(rec) if "positions" in device and len(rec) else rec
    got, off = fm.format_sam(positions, queries, strands="dna5" if strands else None, want_line_offsets=True, **tables, **kw)
    assert off.tolist() == woff
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError((len(got), len(want), at, got[max(at - 80, 0): at + 40], want[max(at - 80, 0): at + 40]))
    return got


@pytest.mark.parametrize("strand", [0, 1])
def test_read_lengths_around_pieces_waves_and_the_window(strand):
    qbuf, qoff, names, quals, seqs = make_batch(LENGTHS, seed=1)
    rec = make_records([1] * len(LENGTHS), seed=2 + strand, strand=strand)
    text = check(rec, qbuf, qoff, read_names=names, quals=quals, seq_names=seqs)
    assert text.count(b"\n") == len(LENGTHS) and b"\t20000M\t" in text and b"N" in text
    assert (b"\t16\t" in text) == bool(strand)
    check(rec, qbuf, qoff, read_names=names, quals=quals, seq_names=seqs, device=("positions", "queries", "read_names", "quals", "seq_names"))
    # both strands of every read, the secondary ones with their SEQ: a line of every length at two places of the text
    both = make_records([2] * len(LENGTHS), seed=4)
    both["qidx"] = 2 * (both["qidx"] >> np.uint64(1)) + ((np.arange(both.size, dtype=np.uint64) + np.uint64(strand)) & np.uint64(1))
    check(both, qbuf, qoff, quals=quals, secondary_seq=True)


@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 5000])
def test_record_counts_around_the_workgroup(count):
    rng = np.random.default_rng(count)
    lengths = rng.integers(0, 70, size=count).tolist()
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=count)
    rec = make_records([1] * count, seed=count + 1)
    check(rec, qbuf, qoff, read_names=names, quals=quals, seq_names=seqs)
    check(rec, qbuf, qoff, device=("positions", "queries"))                   # short lines: hundreds per window when the reads are short
    # the same records on a batch of empty reads: lines of about 30 bytes, more than 256 of them in a window
    empty = make_batch([0] * count, seed=count)
    check(rec, empty[0], empty[1], cigar=False)


def raw_spec(qbuf, qoff, nq, strands=None, read_names=None, quals=None, seq_names=None, cigar=1, emit_unmapped=1, secondary_seq=0):
    keep = []

    def table(t):
        if t is None:
            return None
        if len(t) == 3:                                                      # a table that states more bytes than it holds: device memory, used in place
            data, spans = DeviceBuffer.from_array(np.concatenate([t[0], np.zeros(8, dtype=np.uint8)])), DeviceBuffer.from_array(t[1])
            nt = capi.NameTable(data.ptr, t[2], spans.ptr, len(t[1]))
            keep.append((nt, data, spans))
            return C.pointer(nt)
        data, spans = t
        nt = capi.NameTable(capi.ptr(data).value, data.nbytes if isinstance(data, np.ndarray) else data.nbytes - 8, capi.ptr(spans).value,
                            spans.nbytes // TEXT_SPAN_DTYPE.itemsize)
        keep.append((nt, data, spans))
        return C.pointer(nt)
    spec = capi.SamSpec(capi.ptr(qbuf), capi.ptr(qoff), nq, CHAR_OF.ctypes.data, None if strands is None else C.pointer(strands), table(read_names), table(quals),
                        table(seq_names), cigar, emit_unmapped, secondary_seq, 60, 0, (C.c_uint8 * 3)(0, 0, 0))
    return spec, keep


def raw(pos, count, spec, out, capacity, off=None):
    n, lines = C.c_uint64(123), C.c_uint64(123)
    rc = capi.lib().fmgpu_positions_sam(capi.ptr(pos), count, C.byref(spec), capi.ptr(out), capacity, C.byref(n), capi.ptr(off), C.byref(lines), None)
    return rc, int(n.value), int(lines.value)


def test_every_output_alignment_and_the_guard_bytes():
    lengths = [101, 0, 33, 64, 7, 150, 16, 1] * 25
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=5)
    rec = make_records([(r % 3) for r in range(len(lengths))], seed=6)
    want, woff = model.format_sam(rec, qbuf, qoff, CHAR_OF, DNA5, table_model(names), table_model(quals), table_model(seqs))
    assert len(want) > 2 * 16384
    st = capi.Strands(DNA5.ctypes.data_as(capi.u8p), 5, 0)
    dq, do, dpos = DeviceBuffer.from_array(qbuf), DeviceBuffer.from_array(qoff), DeviceBuffer.from_array(rec)
    spec, keep = raw_spec(dq, do, len(lengths), st, names, quals, seqs)
    guard = 64
    for shift in range(16):
        fill = np.full(guard + 16 + len(want) + guard, 0xAA, dtype=np.uint8)
        buf = DeviceBuffer.from_array(fill)
        assert buf.ptr % 256 == 0
        rc, n, lines = raw(dpos, len(rec), spec, buf.ptr + guard + shift, len(want))
        assert rc == 0 and n == len(want) and lines == len(woff) - 1, capi.lib().fmgpu_last_error()
        back = buf.to_array(np.uint8, fill.size)
        assert back[guard + shift: guard + shift + n].tobytes() == want, shift
        assert (back[: guard + shift] == 0xAA).all() and (back[guard + shift + n:] == 0xAA).all(), shift
    # records at an odd multiple of 8 bytes: no 16-byte loads there
    pad = DeviceBuffer.from_array(np.concatenate([np.zeros(8, dtype=np.uint8), rec.view(np.uint8)]))
    out = np.zeros(len(want), dtype=np.uint8)
    assert raw(pad.ptr + 8, len(rec), spec, out, len(want))[:2] == (0, len(want)) and out.tobytes() == want


@pytest.mark.parametrize("prefix", [1, 3, 15, 17])
def test_a_batch_that_starts_at_an_odd_offset(prefix):
    lengths = [16, 32, 101, 5, 0, 64, 48]
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=7, prefix=prefix)
    assert int(qoff[0]) == prefix
    rec = make_records([2] * len(lengths), seed=8)
    for device in ((), ("queries",)):
        check(rec, qbuf, qoff, quals=quals, secondary_seq=True, device=device)


@pytest.mark.parametrize("pattern", ["first", "last", "runs", "all", "none"])
def test_unmapped_reads_at_every_place(pattern):
    n = 40
    per_read = {"first": [0] + [1] * (n - 1), "last": [2] * (n - 1) + [0], "runs": [0 if 5 <= r < 12 or 20 <= r < 23 or r in (30, 38, 39) else 1 + r % 2 for r in range(n)],
                "all": [0] * n, "none": [1] * n}[pattern]
    qbuf, qoff, names, quals, seqs = make_batch([(37 * r) % 120 for r in range(n)], seed=9)
    rec = make_records(per_read, seed=10)
    assert (len(rec) == 0) == (pattern == "all")
    text = check(rec, qbuf, qoff, read_names=names, quals=quals, seq_names=seqs)
    assert text.count(b"\t4\t*\t0\t0\t*\t*\t0\t0\t") == per_read.count(0)
    quiet = check(rec, qbuf, qoff, read_names=names, quals=quals, seq_names=seqs, emit_unmapped=False)
    assert quiet.count(b"\n") == len(rec) and (pattern != "all" or quiet == b"")
    check(rec, qbuf, qoff, device=("positions", "queries"))


def test_one_read_with_thousands_of_records_among_reads_with_one():
    lengths = [50, 101, 75] + [40] * 20
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=11)
    per_read = [1, 3000, 1] + [1, 0] * 10
    for secondary_seq in (False, True):
        text = check(make_records(per_read, seed=12, errors=2), qbuf, qoff, read_names=names, quals=quals, seq_names=seqs, secondary_seq=secondary_seq)
        assert text.count(b"NH:i:3000\n") == 3000


def test_ties_for_the_primary_record_and_the_switches():
    lengths = [30, 31, 32, 33, 34, 35]
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=13)
    rec = make_records([3, 3, 3, 3, 1, 2], seed=14)
    rec["errors"] = [0, 1, 2,  2, 1, 1,  3, 3, 3,  5, 4, 5,  9,  0, 0]       # unique first; a tie behind a worse record; all equal; unique in the middle; alone; a pair
    for cigar in (False, True):
        for secondary_seq in (False, True):
            text = check(rec, qbuf, qoff, quals=quals, cigar=cigar, secondary_seq=secondary_seq, mapq=(42, 7))
            lines = [l.split(b"\t") for l in text.splitlines()]
            assert [int(l[1]) & 256 for l in lines] == [0, 256, 256,  256, 0, 256,  0, 256, 256,  256, 0, 256,  0,  0, 256]
            assert [int(l[4]) for l in lines] == [42, 7, 7,  7, 7, 7,  7, 7, 7,  7, 42, 7,  42,  7, 7]
            assert all((l[5] == b"*") != cigar for l in lines)
            assert all((l[9] == b"*") == (bool(int(l[1]) & 256) and not secondary_seq) for l in lines)


def test_every_optional_table_given_and_missing_in_host_and_device_memory():
    lengths = [20, 0, 64, 101, 17, 3]
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=15)
    rec = make_records([1, 1, 2, 0, 1, 3], seed=16)
    for mask in range(8):
        given = {k: t for bit, (k, t) in enumerate((("read_names", names), ("quals", quals), ("seq_names", seqs))) if mask >> bit & 1}
        check(rec, qbuf, qoff, **given)
        check(rec, qbuf, qoff, device=tuple(given) + ("queries", "positions"), **given)
    plain = make_records([1, 1, 2, 0, 1, 3], seed=17, strands=False)          # without strands: read = qidx, never flag 16
    text = check(plain, qbuf, qoff, strands=False, read_names=names, quals=quals, seq_names=seqs)
    assert all(not int(l.split(b"\t")[1]) & 16 for l in text.splitlines())


def refused(rec, qbuf, qoff, **kw):
    """the call and the model refuse the same offender with the same code"""
    tables = {k: kw.get(k) for k in ("read_names", "quals", "seq_names")}
    with pytest.raises(model.SamError) as want:
        model.format_sam(rec, qbuf, qoff, CHAR_OF, DNA5, *(table_model(t) for t in tables.values()))
    out = np.full(4096, 0xAA, dtype=np.uint8)
    off = np.full(len(rec) + len(qoff) + 1, 9, dtype=np.uint64)
    st = capi.Strands(DNA5.ctypes.data_as(capi.u8p), 5, 0)
    spec, keep = raw_spec(qbuf, qoff, len(qoff) - 1, st, **tables)
    rc, n, lines = raw(rec, len(rec), spec, out, out.size, off)
    message = capi.lib().fmgpu_last_error().decode()
    assert rc == CODES[want.value.code] and want.value.names in message, (message, str(want.value))
    assert (out == 0xAA).all() and (off == 9).all() and n == 0 and lines == 0
    return want.value


def test_device_checks_name_the_lowest_offender():
    lengths = [10, 20, 0, 30, 5, 12]
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=18)
    good = make_records([2, 1, 1, 0, 2, 1], seed=19)
    nq = len(lengths)
    bad = good.copy(); bad["qidx"][[3, 5]] = 2 * nq + 1                       # a read >= nq: the lowest such record, before anything else
    bad["qidx"][1] = 0
    assert (refused(bad, qbuf, qoff).index, refused(bad, qbuf, qoff).what) == (3, "range")
    bad = good.copy(); bad["qidx"][[2, 4]] = 1                                 # below its predecessor's (the strand bit does not count)
    bad["qidx"][1] = 0
    assert refused(bad, qbuf, qoff).what == "order" and refused(bad, qbuf, qoff).index == 4
    down = qoff.copy(); down[2] += 3; down[5] -= 40                            # reads 2 and 4 end before they start
    e = refused(good, qbuf, down)
    assert (e.who, e.index, e.what) == ("read", 2, "qoff")
    short = lambda t, k: (t[0], t[1][:k])                                      # noqa: E731
    beyond = lambda t, row: (t[0], np.array([(s["offset"], s["len"] + (t[0].size if i == row else 0)) for i, s in enumerate(t[1])], dtype=TEXT_SPAN_DTYPE))  # noqa: E731
    e = refused(good, qbuf, qoff, read_names=short(names, 3))                  # row 3 is an unmapped read's
    assert (e.who, e.index, e.what) == ("unmapped read", 3, "read_names row")
    e = refused(good, qbuf, qoff, read_names=beyond(names, 1))
    assert (e.who, e.index, e.what) == ("record", 2, "read_names span")
    e = refused(good, qbuf, qoff, quals=short(quals, 4), read_names=names)
    assert (e.who, e.index, e.what) == ("record", 4, "quals row")
    e = refused(good, qbuf, qoff, quals=beyond(quals, 0))
    assert (e.who, e.index, e.what) == ("record", 0, "quals span")
    wrong = quals[1].copy(); wrong["len"][1] -= 1; wrong["len"][5] += 1        # neither 0 nor m
    e = refused(good, qbuf, qoff, quals=(quals[0], wrong))
    assert (e.who, e.index, e.what) == ("record", 2, "quals len")
    far = good.copy(); far["seq_id"][[3, 6]] = 4
    e = refused(far, qbuf, qoff, seq_names=seqs)
    assert (e.who, e.index, e.what) == ("record", 3, "seq_names row")
    e = refused(good, qbuf, qoff, seq_names=beyond(seqs, int(good["seq_id"][5])))
    assert e.what == "seq_names span" and e.index == int(np.flatnonzero(good["seq_id"] == good["seq_id"][5])[0])
    # a refused call leaves the library usable
    check(good, qbuf, qoff, read_names=names, quals=quals, seq_names=seqs)


def test_what_is_too_long_is_unsupported_and_an_invalid_line_goes_first():
    """Sizes of 2^31 and more are refused by what qoff and the spans state, in the pass that measures the lines: no byte of such a read or span is read (the batch is
    staged behind the read-back only, a table that states more than it holds lies in device memory and is used in place)."""
    qbuf = np.array([1, 2, 3, 4, 1, 2, 3, 4], dtype=np.uint8)
    big, spans = 1 << 31, lambda *rows: np.array(list(rows), dtype=TEXT_SPAN_DTYPE)          # noqa: E731
    short = np.frombuffer(b"abcdefgh", dtype=np.uint8)
    records = lambda *rows: np.array([(q, s, 7, 0, 0) for q, s in rows], dtype=POSITION_DTYPE)          # noqa: E731
    # a read of 2^31 symbols: unmapped, and with a record
    long_read = np.array([0, 4, 4 + big, 8 + big], dtype=np.uint64)
    e = refused(records((0, 0), (4, 1)), qbuf, long_read)
    assert (e.code, e.who, e.index, e.what) == (model.UNSUPPORTED, "unmapped read", 1, "read")
    e = refused(records((0, 0), (3, 1), (4, 1)), qbuf, long_read)
    assert (e.code, e.who, e.index, e.what) == (model.UNSUPPORTED, "record", 1, "read")
    assert "2^31" in capi.lib().fmgpu_last_error().decode()
    # a name, a quality and a sequence name span of 2^31 bytes, each in a table that says it is that large
    qoff = np.array([0, 4, 8], dtype=np.uint64)
    rec = records((0, 0), (1, 1), (2, 1))
    e = refused(rec, qbuf, qoff, read_names=(short, spans((0, 3), (0, big)), big + 5))
    assert (e.code, e.who, e.index, e.what) == (model.UNSUPPORTED, "record", 2, "read_names long")
    e = refused(rec[:2], qbuf, qoff, quals=(short, spans((0, 4), (0, big)), big + 5))
    assert (e.code, e.who, e.index, e.what) == (model.UNSUPPORTED, "unmapped read", 1, "quals long")
    e = refused(rec, qbuf, qoff, seq_names=(short, spans((0, 3), (1, big)), big + 5))
    assert (e.code, e.who, e.index, e.what) == (model.UNSUPPORTED, "record", 1, "seq_names long")
    # a line of 2^32 bytes: SEQ and QUAL of 2^31 - 1 bytes each, both below the limit of a read and of a span
    e = refused(records((1, 0)), qbuf, np.array([0, big - 1], dtype=np.uint64), quals=(short, spans((0, big - 1)), big + 5))
    assert (e.code, e.who, e.index, e.what) == (model.UNSUPPORTED, "record", 0, "line")
    assert "2^32" in capi.lib().fmgpu_last_error().decode()
    # an invalid line anywhere goes first: the too-long read is record 0's, the sequence name row beyond its table record 2's
    e = refused(records((0, 0), (2, 1), (3, 4)), qbuf, np.array([0, big, big + 4], dtype=np.uint64), seq_names=(short, spans((0, 3), (3, 3))))
    assert (e.code, e.who, e.index, e.what) == (model.INVALID, "record", 2, "seq_names row")
    # and the lowest of several too-long lines is named
    e = refused(records((0, 0), (2, 0)), qbuf, np.array([0, big, 2 * big + 1, 2 * big + 5], dtype=np.uint64))
    assert (e.code, e.who, e.index, e.what) == (model.UNSUPPORTED, "record", 0, "read")
    # a refused call leaves the library usable
    check(rec, qbuf, qoff)


def test_a_capacity_one_byte_short_leaves_out_untouched_with_exact_counts():
    lengths = [101] * 300
    qbuf, qoff, names, quals, seqs = make_batch(lengths, seed=20)
    rec = make_records([r % 3 for r in range(300)], seed=21)
    want, woff = model.format_sam(rec, qbuf, qoff, CHAR_OF, DNA5, table_model(names), table_model(quals), table_model(seqs))
    st = capi.Strands(DNA5.ctypes.data_as(capi.u8p), 5, 0)
    spec, keep = raw_spec(qbuf, qoff, 300, st, names, quals, seqs)
    for device in (False, True):
        fill = np.full(len(want) + 32, 0xAA, dtype=np.uint8)
        out = DeviceBuffer.from_array(fill) if device else fill
        off = np.full(len(woff), 9, dtype=np.uint64)
        rc, n, lines = raw(rec, len(rec), spec, out, len(want) - 1, off)
        assert rc == capi.FMGPU_ERR_CAPACITY and n == len(want) and lines == len(woff) - 1 and off.tolist() == woff
        assert ((out.to_array(np.uint8, fill.size) if device else out) == 0xAA).all()
        assert raw(rec, len(rec), spec, None, 0) == (0, len(want), len(woff) - 1)          # the counting call
        rc, n, lines = raw(rec, len(rec), spec, out, len(want), off)
        assert rc == 0 and (out.to_array(np.uint8, fill.size) if device else out)[:n].tobytes() == want


def long_names(count, rng):
    """names of 100 .. 400 bytes without a blank; every third gets one in its second half (QNAME and RNAME end in front of it)"""
    names = []
    for i in range(count):
        name = bytearray(rng.integers(33, 127, size=int(rng.integers(100, 401))).astype(np.uint8).tobytes())
        if i % 3 == 1:
            name[int(rng.integers(len(name) // 2, len(name)))] = b" \t"[i % 2]
        names.append(bytes(name))
    return names


def test_names_that_cross_the_window_edges():
    """QNAME and RNAME are copied by their lane, the part inside the workgroup's 16 KiB window: long names on short reads, so that names lie across the edges between
    windows.  That some do is asserted from the model's text alone, for each of the two output alignments, before the device is asked."""
    rng = np.random.default_rng(31)
    nq, window = 300, 16384
    qbuf, qoff, _, quals, _ = make_batch(rng.integers(0, 60, size=nq).tolist(), seed=32)
    names, seqs = fm.pack_names(long_names(nq, rng)), fm.pack_names(long_names(40, rng))
    rec = make_records([(1, 1, 2, 0)[r % 4] for r in range(nq)], seed=33, nseq=40)
    assert len(rec) == 300
    want, woff = model.format_sam(rec, qbuf, qoff, CHAR_OF, DNA5, table_model(names), table_model(quals), table_model(seqs))
    assert len(want) > 4 * window + 16                                        # at least four edges at either alignment
    st = capi.Strands(DNA5.ctypes.data_as(capi.u8p), 5, 0)
    dq, do, dpos = DeviceBuffer.from_array(qbuf), DeviceBuffer.from_array(qoff), DeviceBuffer.from_array(rec)
    spec, keep = raw_spec(dq, do, nq, st, names, quals, seqs)
    guard = 64
    for shift in (0, 5):
        # windows are cut at multiples of 16384 counted from the 16-byte piece of the output address that holds the first byte: the edges in bytes of the text
        edges = range(window - shift, len(want), window)
        assert len(edges) >= 4
        crossing = {"QNAME": 0, "RNAME": 0}
        for l in range(len(woff) - 1):
            f = want[woff[l]: woff[l + 1]].split(b"\t")
            for field, start, n in (("QNAME", woff[l], len(f[0])), ("RNAME", woff[l] + len(f[0]) + len(f[1]) + 2, len(f[2]))):
                crossing[field] += any(start < e < start + n for e in edges)
        assert crossing["QNAME"] >= 1 and crossing["RNAME"] >= 1, (shift, crossing)
        fill = np.full(guard + 16 + len(want) + guard, 0xAA, dtype=np.uint8)
        buf = DeviceBuffer.from_array(fill)
        assert buf.ptr % 256 == 0
        rc, n, lines = raw(dpos, len(rec), spec, buf.ptr + guard + shift, len(want))
        assert rc == 0 and n == len(want) and lines == len(woff) - 1, capi.lib().fmgpu_last_error()
        back = buf.to_array(np.uint8, fill.size)
        assert back[guard + shift: guard + shift + n].tobytes() == want, shift
        assert (back[: guard + shift] == 0xAA).all() and (back[guard + shift + n:] == 0xAA).all(), shift


def test_fastq_to_sam_end_to_end_against_the_indexed_text():
    """Does not lean on the model: FASTQ bytes -> parse_queries -> map_reads (both strands, the pair ladder of Hamming schemes k = 0 .. 2) -> format_sam; every mapped
    line is held against the text that was indexed."""
    rng = np.random.default_rng(77)
    texts = [rng.integers(1, 5, size=n).astype(np.uint8) for n in (6000, 3500, 4500)]
    seq_names = [b"chrA test", b"chrB", b"chrC\tx"]
    letters = np.frombuffer(b"$ACGT", dtype=np.uint8)
    comp = np.array(fm.DNA5_COMPLEMENT, dtype=np.uint8)
    reads, planted = [], []
    for i in range(400):
        t = int(rng.integers(0, 3)); m = int(rng.integers(40, 61)); at = int(rng.integers(0, texts[t].size - m + 1))
        r = texts[t][at: at + m].copy()
        for j in rng.choice(m, size=int(rng.integers(0, 3)), replace=False):
            r[j] = 1 + (r[j] - 1 + int(rng.integers(1, 4))) % 4
        reverse = i % 2 == 1
        planted.append((t, at, m, reverse))
        reads.append(comp[r[::-1]] if reverse else r)
    reads += [rng.integers(1, 5, size=60).astype(np.uint8) for _ in range(20)]
    order = rng.permutation(len(reads))
    quals = [bytes(rng.integers(33, 127, size=len(r)).astype(np.uint8)).replace(b"@", b"A") for r in reads]
    fastq = b"".join(b"@read%d extra\n%s\n+\n%s\n" % (k, letters[reads[k]].tobytes(), quals[k]) for k in order)
    pq = fm.parse_queries(fastq, "fastq", fm.symbol_table.dna5(), device=True, want_names=True, want_quals=True)
    assert pq.reads == 420 and pq.foreign == 0
    gx = fm.BiFMIndex.from_sequences(texts, 5, "IB16", 16)
    positions = fm.map_reads(gx, pq.batch, errors=2, edit=False, strands="dna5", pair=True)
    text = fm.format_sam(positions, pq.batch, strands="dna5", read_names=(fastq, pq.names), quals=(fastq, pq.quals), seq_names=seq_names, secondary_seq=True)
    assert fm.sam_header(seq_names, [t.size for t in texts], "test").count(b"@SQ") == 3
    value = {c: i for i, c in enumerate(b"$ACGT")}
    by_name = {b"chrA": 0, b"chrB": 1, b"chrC": 2}
    primaries, mapped = {}, set()
    lines = text.splitlines()
    assert len(lines) >= 420 and text.endswith(b"\n")
    for line in lines:
        f = line.split(b"\t")
        k = int(f[0][4:])
        flag = int(f[1])
        if flag & 4:
            assert len(f) == 11 and f[9] == letters[reads[k]].tobytes() and f[10] == quals[k]
            primaries[k] = primaries.get(k, 0) + 1
            continue
        assert len(f) == 13
        m, pos, t = len(f[9]), int(f[3]) - 1, texts[by_name[f[2]]]
        assert f[5] == b"%dM" % m and m == len(reads[k])
        window = t[pos: pos + m]
        assert window.size == m
        seq = np.array([value[c] for c in f[9]], dtype=np.uint8)
        assert int((seq != window).sum()) == int(f[11][5:]) <= 2 and f[11].startswith(b"NM:i:")
        assert seq.tobytes() == (comp[reads[k][::-1]] if flag & 16 else reads[k]).tobytes()
        assert f[10] == (quals[k][::-1] if flag & 16 else quals[k])
        primaries[k] = primaries.get(k, 0) + (0 if flag & 256 else 1)
        mapped.add(k)
    assert sorted(primaries) == list(range(420)) and set(primaries.values()) == {1}          # each read has exactly one line without flag 256
    # the condition: a planted read lies within two substitutions of the text at its place, on its strand, so the ladder k = 0 .. 2 must find it
    for k, (t, at, m, reverse) in enumerate(planted):
        forward = comp[reads[k][::-1]] if reverse else reads[k]
        assert int((forward != texts[t][at: at + m]).sum()) <= 2
        assert k in mapped, k
