"""fmgpu_queries_parse / fm.parse_queries / fm.parse_stream on the device against the plain-Python restatement of the contract (tests/parse_model.py), field for
field: every check is exact.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests import parse_model as model
from tests.parse_model import LINES, FASTA, FASTQ
from tests.test_parse_host import CASES, CHUNK_TEXTS, DNA, DNA_DROP

pytestmark = pytest.mark.gpu

FORMATS = [LINES, FASTA, FASTQ]
SENT = 0xEEEEEEEEEEEEEEEE
SPAN = capi.TEXT_SPAN_DTYPE


@functools.lru_cache(maxsize=None)
def want_for(text, fmt, final, table_key):
    return model.parse(text, fmt, TABLES[table_key], final)


TABLES = {"dna": DNA, "drop": DNA_DROP}


def sentinel_spans(count):
    a = np.zeros(count, dtype=SPAN)
    a["offset"] = a["len"] = SENT
    return a


def device_parse(text_ptr, n, fmt, final, table, symbol_capacity=None, read_capacity=None, device_out=False, spans=True):
    """one call with sentinel-filled outputs of n (+ 1) entries -> (rc, result, qbuf, qoff, names, quals) as host arrays"""
    qbuf, qoff = np.full(n + 1, 0xEE, dtype=np.uint8), np.full(n + 2, SENT, dtype=np.uint64)
    names, quals = (sentinel_spans(n + 1), sentinel_spans(n + 1)) if spans else (None, None)
    outs = [qbuf, qoff, names, quals]
    bufs = [fm.DeviceBuffer.from_array(a) if device_out and a is not None else a for a in outs]
    res = capi.ParseResult()
    rc = capi.lib().fmgpu_queries_parse(text_ptr, n, fmt, final, capi.ptr(table), capi.ptr(bufs[0]), n if symbol_capacity is None else symbol_capacity,
                                        capi.ptr(bufs[1]), n if read_capacity is None else read_capacity, capi.ptr(bufs[2]), capi.ptr(bufs[3]), C.byref(res), None)
    if device_out:
        outs = [None if a is None else b.to_array(a.dtype, a.size) for a, b in zip(outs, bufs)]
    return (rc, res, *outs)


def untouched(qbuf, qoff, names, quals, symbols=0, entries=0, reads=0):
    ok = bool(np.all(qbuf[symbols:] == 0xEE) and np.all(qoff[entries:] == SENT))
    for spans in (names, quals):
        if spans is not None:
            ok = ok and bool(np.all(spans["offset"][reads:] == SENT) and np.all(spans["len"][reads:] == SENT))
    return ok


def check(text, fmt, final, table_key="dna", text_ptr=None, **kw):
    """the device call on `text` equals the model in every field; outputs beyond what it owes are untouched"""
    want = want_for(bytes(text), fmt, int(bool(final)), table_key)
    data = np.frombuffer(bytes(text), dtype=np.uint8)
    rc, res, qbuf, qoff, names, quals = device_parse(capi.ptr(data) if text_ptr is None else text_ptr, len(text), fmt, final, TABLES[table_key], **kw)
    got = (int(res.reads), int(res.symbols), int(res.consumed), int(res.foreign))
    assert got == (len(want.reads), want.symbols, want.consumed, want.foreign), (got, text[:80])
    if want.error_line is not None:
        assert rc == capi.FMGPU_ERR_INVALID and (int(res.error_line), int(res.error_offset)) == (want.error_line, want.error_offset)
        assert ("line %d" % want.error_line).encode() in capi.lib().fmgpu_last_error()
        assert untouched(qbuf, qoff, names, quals)
        return want
    assert rc == 0, capi.lib().fmgpu_last_error()
    assert (int(res.error_line), int(res.error_offset)) == (0, 0)
    nr, ns = len(want.reads), want.symbols
    assert qbuf[:ns].tobytes() == want.qbuf.tobytes() and np.array_equal(qoff[: nr + 1], want.qoff)
    assert untouched(qbuf, qoff, names, quals, ns, nr + 1, nr)
    if names is not None:
        assert [(int(s["offset"]), int(s["len"])) for s in names[:nr]] == [tuple(s) for s in want.names]
        assert [(int(s["offset"]), int(s["len"])) for s in quals[:nr]] == [tuple(s) for s in want.quals]
    return want


# ------------------------------------------------------------------------------------------------ texts
def long_text(fmt):
    """several thousand bytes of well-formed text with records of many shapes"""
    return b"".join(CHUNK_TEXTS[fmt].replace(b"read", b"r%d_" % k).replace(b"@q", b"@s%d." % k) + (b"\n" if fmt != FASTQ else b"") for k in range(16))


def fastq_of_size(n):
    """a well-formed FASTQ of exactly n bytes (n >= 17): records of long_text, the last one's name padded"""
    body, at = long_text(FASTQ), 0
    while True:                                                     # the longest prefix of whole records that leaves room for a last record
        nxt = at
        for _ in range(4):
            nxt = body.index(b"\n", nxt) + 1
        if nxt > n - 17:
            break
        at = nxt
    rest = n - at                                                   # "@" name "\n" seq "\n+\n" qual "\n": 6 + len(name) + 2 len(seq)
    seq = b"ACGTTGCAAC"[: min(5, (rest - 6) // 2)]
    name = b"x" * (rest - 6 - 2 * len(seq))
    text = body[:at] + b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
    assert len(text) == n
    return text


SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025, 4097]


@pytest.mark.parametrize("fmt", FORMATS)
def test_buffer_sizes_at_the_lane_wave_and_block_boundaries(fmt):
    body = long_text(fmt)
    assert len(body) > 4097
    for n in SIZES:
        for final in (0, 1):                                        # (a FASTQ prefix with final = 1 is usually a truncated file: the error and the counts in front of it)
            check(body[:n], fmt, final)
        if fmt == FASTQ and n >= 17:
            assert check(fastq_of_size(n), fmt, 1).error_line is None
    for one in (b"A", b">", b"@", b"\r"):                             # single bytes of every kind
        for final in (0, 1):
            check(one, fmt, final)


def test_a_line_longer_than_several_blocks():
    seq = bytes(np.random.default_rng(1).choice(list(b"ACGTN"), size=5000).astype(np.uint8))
    assert check(seq + b"\n", LINES, 1).symbols == 5000
    assert check(seq, LINES, 1).symbols == 5000
    assert check(seq, LINES, 0).symbols == 0
    assert check(b">long one\n" + seq + b"\n>next\nAC\n", FASTA, 1).symbols == 5002
    assert check(b">long one\n" + seq + b"\n>next\nAC\n", FASTA, 0).symbols == 5000
    assert check(b"@long\n" + seq + b"\n+\n" + seq + b"\n@n\nA\n+\n@\n", FASTQ, 1).symbols == 5001


def test_empty_lines_newlines_only_and_many_short_lines():
    for fmt in FORMATS:
        for final in (0, 1):
            check(b"\n" * 300, fmt, final)
            check(b"\n", fmt, final)
            check(b"\r\n" * 77, fmt, final)
    check(b"AC\n" + b"\n" * 300 + b"GT\n", LINES, 1)
    check(b">a\n" + b"\n" * 300 + b"GT\n" + b"\n" * 300, FASTA, 1)
    check(b"@a\nAC\n+\nII\n" + b"\n" * 300, FASTQ, 1)
    record = b">forty lines\n" + b"".join(b"ACGTACG"[: 1 + i % 7] + b"\n" for i in range(40))
    assert len(check(record, FASTA, 1).reads[0]) == sum(1 + i % 7 for i in range(40))
    check(record + b">b\nA\n", FASTA, 0)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_written_cases(case):
    _, fmt, final, text, reads, consumed, error = case
    want = check(text, fmt, final)
    assert want.consumed == consumed and (error is None) == (want.error_line is None)      # (the host test pins the model on these)


def test_drop_and_foreign():
    text = b"@r1 first\nAC-G T\n+\nIIIIII\n@r2\nNNA\n+\nIII\n"
    want = check(text, FASTQ, 1, "drop")
    assert want.foreign == 2 and want.symbols == 7
    check(b">n1 d\r\nA-C \r\n -\n>n2\nNN-N\n", FASTA, 1, "drop")
    check(b"A C\n- -\nxAy\n", LINES, 1, "drop")
    check(long_text(FASTA).replace(b"T", b"-").replace(b"G", b"n"), FASTA, 1, "drop")


@pytest.mark.parametrize("fmt", FORMATS)
def test_chunking_law(fmt):
    """parse(text[:c], final = 0) then parse(text[consumed:], final = 1) gives the reads of the whole parse, for every cut c"""
    text = CHUNK_TEXTS[fmt]
    whole = check(text, fmt, 1)
    for cut in range(len(text) + 1):
        head = check(text[:cut], fmt, 0, spans=False)
        tail = check(text[head.consumed:], fmt, 1, spans=False)
        assert head.error_line is None and tail.error_line is None and head.reads + tail.reads == whole.reads, cut


def test_counting_call_and_capacity():
    L = capi.lib()
    for fmt in FORMATS:
        text = long_text(fmt)
        want = want_for(text, fmt, 1, "dna")
        data, res = np.frombuffer(text, dtype=np.uint8), capi.ParseResult()
        assert L.fmgpu_queries_parse(capi.ptr(data), len(text), fmt, 1, capi.ptr(DNA), None, 0, None, 0, None, None, C.byref(res), None) == 0
        counts = (len(want.reads), want.symbols, want.consumed, want.foreign)
        assert (res.reads, res.symbols, res.consumed, res.foreign) == counts
        for ncap, rcap in ((want.symbols - 1, len(want.reads)), (want.symbols, len(want.reads) - 1), (0, 0)):
            rc, res, qbuf, qoff, names, quals = device_parse(capi.ptr(data), len(text), fmt, 1, DNA, ncap, rcap)
            assert rc == capi.FMGPU_ERR_CAPACITY and (res.reads, res.symbols, res.consumed, res.foreign) == counts
            assert untouched(qbuf, qoff, names, quals)
        rc, res, qbuf, qoff, names, quals = device_parse(capi.ptr(data), len(text), fmt, 1, DNA, want.symbols, len(want.reads))      # exactly enough
        assert rc == 0 and qbuf[: want.symbols].tobytes() == want.qbuf.tobytes() and np.array_equal(qoff[: len(want.reads) + 1], want.qoff)


@pytest.mark.parametrize("fmt", FORMATS)
def test_memory_spaces(fmt):
    """host, pinned and device text, at every alignment of a device pointer; host and device outputs"""
    text = long_text(fmt)[:1500] if fmt != FASTQ else fastq_of_size(1500)
    data = np.frombuffer(text, dtype=np.uint8)
    pinned = fm.PinnedBuffer.from_array(data)
    check(text, fmt, 1, text_ptr=C.c_void_p(pinned.ptr))
    check(text, fmt, 1, text_ptr=C.c_void_p(pinned.ptr), device_out=True)
    check(text, fmt, 1, device_out=True)
    for lead in (0, 1, 5, 15, 16, 31):
        dev = fm.DeviceBuffer.from_array(np.concatenate([np.full(lead, ord(">"), dtype=np.uint8), data, np.full(40, ord("\n"), dtype=np.uint8)]))
        check(text, fmt, 1, text_ptr=C.c_void_p(dev.ptr + lead), device_out=bool(lead & 1))
        check(text[:777], fmt, 0, text_ptr=C.c_void_p(dev.ptr + lead))
    pinned.free()


def test_parse_queries_takes_bytes_arrays_tensors_and_device_buffers():
    import torch
    text = long_text(FASTQ)
    want = want_for(text, FASTQ, 1, "dna")
    data = np.frombuffer(text, dtype=np.uint8)
    tensor = torch.from_numpy(data.copy())
    for source in (text, data, tensor, tensor.pin_memory(), tensor.cuda(), fm.DeviceBuffer.from_array(data)):
        for device in (False, True):
            got = fm.parse_queries(source, "fastq", DNA, device=device, want_names=True, want_quals=True)
            qbuf = got.qbuf.to_array(np.uint8, got.symbols) if device else got.qbuf[: got.symbols]
            qoff = got.qoff.to_array(np.uint64, got.reads + 1) if device else got.qoff
            assert qbuf.tobytes() == want.qbuf.tobytes() and np.array_equal(qoff, want.qoff)
            assert (got.reads, got.symbols, got.consumed, got.foreign) == (len(want.reads), want.symbols, len(text), want.foreign)
            assert fm.ParsedQueries.texts(text, got.names) == [text[o: o + n] for o, n in want.names]
            assert fm.ParsedQueries.texts(text, got.quals) == [text[o: o + n] for o, n in want.quals]
    with pytest.raises(fm.TextError, match="line 6") as err:
        fm.parse_queries(b"@a\nAC\n+\nII\n@b\nGT\n-\nII\n", fm.FASTQ, DNA)
    assert (err.value.line, err.value.offset) == (6, 17)
    empty = fm.parse_queries(b"", "lines", DNA)
    assert empty.reads == 0 and empty.qoff.tolist() == [0]


# ------------------------------------------------------------------------------------------------ end to end
LETTERS = b"$ACGT"


@functools.lru_cache(maxsize=None)
def index_and_reads():
    from tests.test_gpu_smems import sequences
    seqs = sequences(5, False)
    rng = np.random.default_rng(11)
    src = seqs[0]
    reads = [src[a: a + l].copy() for a, l in ((int(rng.integers(0, len(src) - 60)), int(rng.integers(1, 60))) for _ in range(40))]
    reads[7] = np.array([1, 2, 3, 4] * 9, dtype=np.uint8)           # a read that need not occur, an empty one
    reads[9] = reads[9][:0]
    return fm.BiFMIndex.from_sequences(seqs, 5, "IB16", 4), reads


def as_text(reads, fmt):
    out = []
    for i, r in enumerate(reads):
        s = bytes(LETTERS[c] for c in r)
        if fmt == FASTQ:
            out.append(b"@read %d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
        else:
            out.append(b">read %d\n" % i + b"".join(s[k: k + 17] + b"\n" for k in range(0, len(s), 17)))
    return b"".join(out)


@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_parsed_device_batch_feeds_search_map_and_pack(fmt):
    gx, reads = index_and_reads()
    host = fm.flatten(reads)
    parsed = fm.parse_queries(as_text(reads, fmt), fmt, DNA, device=True)
    assert parsed.reads == len(reads) and parsed.foreign == 0
    lb, ln = fm.search_no_errors.search(gx, parsed.batch)
    wlb, wln = fm.search_no_errors.search(gx, host)
    assert np.array_equal(ln, wln) and np.array_equal(lb[ln > 0], wlb[wln > 0]) and int((ln > 0).sum()) > 20
    pos = fm.map_reads(gx, parsed.batch, errors=1, edit=False)
    assert pos.tobytes() == fm.map_reads(gx, host, errors=1, edit=False).tobytes() and len(pos) > 0
    comp = [0, 4, 3, 2, 1]
    packed, poff = fm.pack_queries_device(parsed.batch, 5, comp).host()
    want = fm.pack_queries(host, 5, comp)
    assert packed.tobytes() == want.packed.tobytes() and np.array_equal(poff, want.qoff)


def test_parse_stream():
    rng = np.random.default_rng(3)
    parts = []
    for i in range(150):
        s = bytes(rng.choice(list(b"ACGTN"), size=int(rng.integers(20, 101))).astype(np.uint8))
        parts.append(b"@read%d/1\n%s\n+\n%s\n" % (i, s, bytes(rng.integers(33, 74, size=len(s)).astype(np.uint8))))
    text = b"".join(parts)
    assert 15_000 < len(text) < 30_000
    want = want_for(text, FASTQ, 1, "dna")
    for chunk_bytes in (1 << 10, 4 << 10, 1 << 16):
        batches = list(fm.parse_stream(io.BytesIO(text), "fastq", DNA, chunk_bytes=chunk_bytes, want_names=True, want_quals=True))
        assert len(batches) == 1 if chunk_bytes > len(text) else len(batches) > 3
        reads, names, quals = [], [], []
        for b in batches:
            reads += [b.qbuf[int(b.qoff[r]): int(b.qoff[r + 1])].tobytes() for r in range(b.reads)]
            names += b.name_texts
            quals += b.qual_texts
        assert reads == want.reads and sum(b.foreign for b in batches) == want.foreign
        assert names == [text[o: o + n] for o, n in want.names] and quals == [text[o: o + n] for o, n in want.quals]
    with pytest.raises(ValueError, match="no complete read"):
        list(fm.parse_stream(io.BytesIO(text), "fastq", DNA, chunk_bytes=64, max_chunk_bytes=128))
    grown = list(fm.parse_stream(io.BytesIO(text), "fastq", DNA, chunk_bytes=64, max_chunk_bytes=1 << 12))
    assert sum(b.reads for b in grown) == len(want.reads)
