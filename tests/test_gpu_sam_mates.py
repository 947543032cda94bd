"""fmgpu_positions_sam_mates on the device (include/fmgpu.h): every output, text and line offsets both, is compared byte for byte with the plain-Python model of
tests/sam_mates_model.py.  The shapes are the smallest at which the kernels can go wrong: read lengths around the 16-byte pieces and the 64 lanes of a wave, a read longer
than a workgroup's window, fragment counts around the 256 lines of a workgroup, every output alignment, the six situations of a fragment at every place, pairs in any
order, with ties and by the thousand.  One end-to-end test (two FASTQ texts -> parse -> both-strand mapping -> join -> paired SAM) checks the lines against the indexed
text instead of the model.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import MATE_PAIR_DTYPE, POSITION_DTYPE, TEXT_SPAN_DTYPE, DeviceBuffer
from tests import sam_mates_model as model

pytestmark = pytest.mark.gpu
DNA5 = np.array(fm.DNA5_COMPLEMENT, dtype=np.uint8)
CHAR_OF = fm.char_table("dna5")
CODES = {model.INVALID: capi.FMGPU_ERR_INVALID, model.UNSUPPORTED: capi.FMGPU_ERR_UNSUPPORTED}
LENGTHS = [0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 101, 255, 256, 257, 20000]
PROPER, SAME_SEQ, OTHER_SEQ, ONLY_A, ONLY_B, NEITHER = 1, 2, 3, 4, 5, 6
SEQS = fm.pack_names([b"chr1 the first", b"", b"chrM", b"scaffold_0123456789_0123456789_0123456789_0123456789_0123456789_0123456789\tlong"])
WINDOW = 16384


def random_slots(classes, seed, strand=None, most=3):
    """per slot (2f: mate A of fragment f, 2f + 1: mate B) its records (strand, seq_id, pos, errors), and the pairs (fragment, record of A, record of B, both counted
    inside their slot) by the fragment's situation: PROPER has one to four pairs, SAME_SEQ every record on one sequence and no pair, OTHER_SEQ the two mates on
    different sequences, ONLY_A / ONLY_B records of one mate, NEITHER none.  Errors are small, so ties are common; pos has every digit count"""
    rng = np.random.default_rng(seed)
    slots, pairs = [], []

    def some(count, seqs):
        return [(int(rng.integers(0, 2)) if strand is None else strand, int(rng.choice(seqs)), int(rng.integers(0, (1 << 62) - 1) >> rng.integers(0, 62)),
                 int(rng.integers(0, 3))) for _ in range(count)]
    for f, c in enumerate(classes):
        na = int(rng.integers(1, most + 1)) if c in (PROPER, SAME_SEQ, OTHER_SEQ, ONLY_A) else 0
        nb = int(rng.integers(1, most + 1)) if c in (PROPER, SAME_SEQ, OTHER_SEQ, ONLY_B) else 0
        s = int(rng.integers(0, 4))
        slots += [some(na, [s] if c in (SAME_SEQ, OTHER_SEQ) else [0, 1, 2, 3]), some(nb, [s] if c == SAME_SEQ else [(s + 1) % 4] if c == OTHER_SEQ else [0, 1, 2, 3])]
        if c == PROPER:
            combos = [(a, b) for a in range(na) for b in range(nb)]
            pairs += [(f,) + combos[k] for k in sorted(rng.choice(len(combos), size=min(len(combos), int(rng.integers(1, 5))), replace=False))]
    return slots, pairs


def make_reads(lengths, seed):
    rng = np.random.default_rng(seed)
    reads = [rng.integers(1, 5, size=m).astype(np.uint8) for m in lengths]
    for r in reads:
        if r.size:
            r[rng.integers(0, r.size, size=1 + r.size // 50)] = 255
    return reads, [b"" if i % 7 == 6 else bytes(rng.integers(33, 127, size=m).astype(np.uint8)) for i, m in enumerate(lengths)]


def flat(reads, prefix):
    """(qbuf, qoff) with `prefix` bytes in front of the first read (qoff[0] = prefix) and a byte behind the last"""
    qbuf = np.concatenate([np.full(prefix, 7, dtype=np.uint8)] + list(reads) + [np.zeros(1, dtype=np.uint8)])
    return qbuf, (prefix + np.concatenate([[0], np.cumsum([len(r) for r in reads])])).astype(np.uint64)


def frag_name(f):
    return b"" if f % 11 == 5 else b" hidden" if f % 11 == 7 else b"/1" if f % 11 == 8 else b"frag_%d/1 pos=%d\tx" % (f, f) if f % 2 else b"f%d/2" % f if f % 3 == 0 else b"f%d" % f


def build(slots, pairs, lengths, interleaved=False, strands=True, seed=0, prefix=(3, 5), shuffle=False):
    """the arguments of the call (and of the model) from records per slot: lengths[l] = the length of the read of slot l"""
    n = len(slots) // 2
    reads, quals = make_reads(lengths, seed + 1000)
    case = dict(interleaved=interleaved, strands=strands, n=n, seq_names=SEQS)

    def array(rows):
        rec = np.zeros(len(rows), dtype=POSITION_DTYPE)
        for i, (read, (st, seq, pos, err)) in enumerate(rows):
            rec[i] = ((2 * read + st) if strands else read, seq, pos, err, i)
        return rec
    first = [0] * (2 * n)                                      # the index of each slot's first record in its array
    if interleaved:
        rows = [(l, r) for l in range(2 * n) for r in slots[l]]
        at = 0
        for l in range(2 * n):
            first[l], at = at, at + len(slots[l])
        case.update(rec_a=array(rows), rec_b=None, batch_a=flat(reads, prefix[0]), batch_b=None, quals_a=fm.pack_names(quals), quals_b=None,
                    read_names=fm.pack_names([frag_name(l >> 1) if l % 2 == 0 else b"mate_b_%d/2" % l for l in range(2 * n)]))
    else:
        for side in range(2):
            at = 0
            for f in range(n):
                first[2 * f + side], at = at, at + len(slots[2 * f + side])
        case.update(rec_a=array([(f, r) for f in range(n) for r in slots[2 * f]]), rec_b=array([(f, r) for f in range(n) for r in slots[2 * f + 1]]),
                    batch_a=flat(reads[0::2], prefix[0]), batch_b=flat(reads[1::2], prefix[1]), quals_a=fm.pack_names(quals[0::2]), quals_b=fm.pack_names(quals[1::2]),
                    read_names=fm.pack_names([frag_name(f) for f in range(n)]))
    prs = np.zeros(len(pairs), dtype=MATE_PAIR_DTYPE)
    for i, (f, a, b) in enumerate(pairs):
        prs[i] = (f, 12345, first[2 * f] + a, first[2 * f + 1] + b, 99, 7)          # tlen, errors and flags are not read
    if shuffle:
        prs = prs[np.random.default_rng(seed + 2000).permutation(len(prs))]
    case["pairs"] = prs
    return case


def table_model(t):
    """(data, spans) or (data, spans, stated n_bytes) as the model takes it"""
    return None if t is None else (t[0].tobytes(), [(int(s["offset"]), int(s["len"])) for s in t[1]]) + tuple(t[2:])


def expected(case, tables=("read_names", "quals_a", "quals_b", "seq_names"), **kw):
    mkw = {k: (1 if v else 0) for k, v in kw.items() if k != "mapq"}
    if "mapq" in kw:
        mkw["mapq_unique"], mkw["mapq_multi"] = kw["mapq"]
    given = {k: table_model(case[k]) for k in tables if case[k] is not None}
    return model.format_sam_mates(case["rec_a"], case["batch_a"], case["rec_b"], case["batch_b"], case["pairs"], CHAR_OF, DNA5 if case["strands"] else None,
                                  case["interleaved"], **given, **mkw)


def dev(a):
    return DeviceBuffer.from_array(a) if a is not None and a.size else a


def on_device(t):
    data, spans = t
    return (DeviceBuffer.from_array(np.concatenate([data, np.zeros(8, dtype=np.uint8)])), DeviceBuffer.from_array(spans)) if spans.size else t


def check(case, tables=("read_names", "quals_a", "quals_b", "seq_names"), device=False, **kw):
    """format_sam_mates against the model, text and line offsets; device: every array (positions, pairs, batches, tables) lies in device memory"""
    want, woff = expected(case, tables, **kw)
    move = dev if device else (lambda a: a)
    given = {k: (on_device(case[k]) if device else case[k]) for k in tables if case[k] is not None}
    batches = [None if b is None else (move(b[0]), move(b[1])) for b in (case["batch_a"], case["batch_b"])]
    got, off = fm.format_sam_mates(move(case["rec_a"]), batches[0], move(case["rec_b"]) if case["rec_b"] is not None else None, batches[1], pairs=move(case["pairs"]),
                                   interleaved=case["interleaved"], strands="dna5" if case["strands"] else None, want_line_offsets=True, **given, **kw)
    assert off.tolist() == woff
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError((len(got), len(want), at, got[max(at - 80, 0): at + 40], want[max(at - 80, 0): at + 40]))
    return got


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("interleaved", [False, True])
def test_read_lengths_around_pieces_waves_and_the_window(strand, interleaved):
    n = len(LENGTHS)
    lengths = [m for f in range(n) for m in (LENGTHS[f], LENGTHS[(f + 4) % n])]              # A and B of a fragment differ; every length on either side
    classes = [(PROPER, SAME_SEQ, OTHER_SEQ, ONLY_A, ONLY_B)[f % 5] for f in range(n)]
    slots, pairs = random_slots(classes, seed=1 + strand, strand=strand)
    case = build(slots, pairs, lengths, interleaved, seed=2)
    assert int(case["batch_a"][1][0]) == 3
    text = check(case)
    assert text.count(b"\n") == 2 * n and b"\t20000M\t" in text and b"N" in text
    flags = [int(ln.split(b"\t")[1]) for ln in text.splitlines()]
    assert all(bool(f & 16) == bool(strand) for f in flags if not f & 4) and any(f & 4 for f in flags)
    check(case, device=True)
    # the other strand for the mates of B: SEQ of either direction in one fragment
    for l in range(1, 2 * n, 2):
        slots[l] = [(1 - st, s, p, e) for st, s, p, e in slots[l]]
    check(build(slots, pairs, lengths, interleaved, seed=2), device=True)


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 2500])
def test_fragment_counts_around_the_workgroup(n):
    rng = np.random.default_rng(n)
    classes = rng.integers(1, 7, size=n).tolist()
    slots, pairs = random_slots(classes, seed=n + 1)
    interleaved = n % 2 == 1
    case = build(slots, pairs, rng.integers(0, 70, size=2 * n).tolist(), interleaved, seed=n, shuffle=True)
    check(case)
    check(case, tables=(), device=True)                                     # short lines: hundreds per window when the reads are short
    # the same fragments on empty reads: lines of about 30 bytes, several hundred of them in a window
    empty = build(slots, pairs, [0] * (2 * n), not interleaved, seed=n)
    text = check(empty, tables=(), cigar=False)
    assert n < 128 or len(text) / (2 * n) < WINDOW / 300


def raw_spec(case, tables=("read_names", "quals_a", "quals_b", "seq_names"), batch_a=None, batch_b=None, cigar=1, strip=1, **override):
    keep = []

    def table(t):
        if t is None:
            return None
        if len(t) == 3:                                                      # a table that states more bytes than it holds: device memory, used in place
            data, spans = DeviceBuffer.from_array(np.concatenate([t[0], np.zeros(8, dtype=np.uint8)])), DeviceBuffer.from_array(t[1])
            nt = capi.NameTable(data.ptr, t[2], spans.ptr, len(t[1]))
        else:
            data, spans = t
            nt = capi.NameTable(capi.ptr(data).value, data.nbytes if isinstance(data, np.ndarray) else data.nbytes - 8, capi.ptr(spans).value,
                                spans.nbytes // TEXT_SPAN_DTYPE.itemsize)
        keep.append((nt, data, spans))
        return C.pointer(nt)
    batch_a, batch_b = batch_a or case["batch_a"], batch_b or case["batch_b"] or (None, None)
    st = capi.Strands(DNA5.ctypes.data_as(capi.u8p), 5, 0)
    keep += [st, batch_a, batch_b]
    given = {k: override.get(k, case[k] if k in tables else None) for k in ("read_names", "quals_a", "quals_b", "seq_names")}
    spec = capi.SamMatesSpec(capi.ptr(batch_a[0]), capi.ptr(batch_a[1]), capi.ptr(batch_b[0]), capi.ptr(batch_b[1]), case["n"], CHAR_OF.ctypes.data,
                             C.pointer(st) if case["strands"] else None, table(given["read_names"]), table(given["quals_a"]), table(given["quals_b"]),
                             table(given["seq_names"]), 1 if case["interleaved"] else 0, cigar, strip, 60, 0, (C.c_uint8 * 3)(0, 0, 0))
    return spec, keep


def raw(rec_a, rec_b, pairs, spec, out, capacity, off=None):
    n = C.c_uint64(123)
    count = lambda a: 0 if a is None else a.nbytes // 32                      # noqa: E731  (records and pairs are 32 bytes each)
    ptr = lambda a: capi.ptr(a) if count(a) else None                        # noqa: E731
    rc = capi.lib().fmgpu_positions_sam_mates(ptr(rec_a), count(rec_a), ptr(rec_b), count(rec_b), ptr(pairs), count(pairs), C.byref(spec), capi.ptr(out), capacity,
                                              C.byref(n), capi.ptr(off), None)
    return rc, int(n.value)


def test_every_output_alignment_and_the_guard_bytes():
    n = 130
    classes = [1 + f % 6 for f in range(n)]
    slots, pairs = random_slots(classes, seed=5)
    case = build(slots, pairs, [(101, 0, 33, 64, 7, 150, 16, 1)[l % 8] for l in range(2 * n)], seed=6, prefix=(0, 1))
    want, woff = expected(case)
    assert len(want) > 2 * WINDOW
    da, db, dp = dev(case["rec_a"]), dev(case["rec_b"]), dev(case["pairs"])
    spec, keep = raw_spec(case, batch_a=tuple(dev(x) for x in case["batch_a"]), batch_b=tuple(dev(x) for x in case["batch_b"]))
    guard = 64

    def at_alignment(spec, want, shift):
        fill = np.full(guard + 16 + len(want) + guard, 0xAA, dtype=np.uint8)
        buf = DeviceBuffer.from_array(fill)
        assert buf.ptr % 256 == 0
        rc, got = raw(da, db, dp, spec, buf.ptr + guard + shift, len(want))
        assert rc == 0 and got == len(want), capi.lib().fmgpu_last_error()
        back = buf.to_array(np.uint8, fill.size)
        assert back[guard + shift: guard + shift + got].tobytes() == want, shift
        assert (back[: guard + shift] == 0xAA).all() and (back[guard + shift + got:] == 0xAA).all(), shift
    for shift in range(16):
        at_alignment(spec, want, shift)
    # names of 100 .. 400 bytes on the same short reads: QNAME and RNAME are copied by their lane, the part inside the workgroup's window, and some lie across the edges
    # between windows.  That some do is asserted from the model's text alone, for an aligned and for an odd output address, before the device is asked.
    rng = np.random.default_rng(7)
    long_names = lambda count: fm.pack_names([bytes(rng.integers(33, 127, size=int(rng.integers(100, 401))).astype(np.uint8)) for _ in range(count)])  # noqa: E731
    named = dict(case, read_names=long_names(n), seq_names=long_names(4))
    long_want, long_off = expected(named)
    long_spec, long_keep = raw_spec(named, batch_a=tuple(dev(x) for x in case["batch_a"]), batch_b=tuple(dev(x) for x in case["batch_b"]))
    for shift in (0, 5):
        edges = range(WINDOW - shift, len(long_want), WINDOW)                # in bytes of the text: windows are cut from the 16-byte piece that holds its first byte
        crossing = {"QNAME": 0, "RNAME": 0}
        for l in range(len(long_off) - 1):
            f = long_want[long_off[l]: long_off[l + 1]].split(b"\t")
            for field, start, size in (("QNAME", long_off[l], len(f[0])), ("RNAME", long_off[l] + len(f[0]) + len(f[1]) + 2, len(f[2]))):
                crossing[field] += any(start < e < start + size for e in edges)
        assert len(edges) >= 4 and crossing["QNAME"] >= 1 and crossing["RNAME"] >= 1, (shift, crossing)
        at_alignment(long_spec, long_want, shift)
    # records at an odd multiple of 8 bytes: no 16-byte loads there
    pad = DeviceBuffer.from_array(np.concatenate([np.zeros(8, dtype=np.uint8), case["rec_a"].view(np.uint8)]))
    out = np.zeros(len(want), dtype=np.uint8)
    n_bytes = C.c_uint64()
    rc = capi.lib().fmgpu_positions_sam_mates(pad.ptr + 8, len(case["rec_a"]), capi.ptr(db), len(case["rec_b"]), capi.ptr(dp), len(case["pairs"]), C.byref(spec),
                                              capi.ptr(out), len(want), C.byref(n_bytes), None, None)
    assert rc == 0 and out.tobytes() == want


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("strands", [False, True])
def test_the_six_situations_first_last_and_across_the_windows(interleaved, strands):
    for rot in range(6):                                                     # every situation is the first fragment once and the last one once
        classes = [(rot + i) % 6 + 1 for i in range(12)]
        slots, pairs = random_slots(classes, seed=20 + rot, strand=None if strands else 0)
        case = build(slots, pairs, [(40 + 7 * l) % 90 for l in range(24)], interleaved, strands, seed=30 + rot)
        text = check(case, device=bool(rot % 2))
        want_flags = {PROPER: 3, SAME_SEQ: 1, OTHER_SEQ: 1, ONLY_A: 9, ONLY_B: 5, NEITHER: 13}
        lines = text.splitlines()
        assert [int(lines[2 * f].split(b"\t")[1]) & 15 for f in range(12)] == [want_flags[c] for c in classes]
    # each situation with a line across an edge between two windows: asserted from the model's text before the device is asked (a staged `out` starts a window)
    n = 420                                                                  # runs of 70 fragments of one situation: 140 lines of 150 bytes and more are longer than a window
    classes = [1 + f // 70 for f in range(n)]
    slots, pairs = random_slots(classes, seed=40, strand=None if strands else 0)
    case = build(slots, pairs, [60 + (37 * l) % 50 for l in range(2 * n)], interleaved, strands, seed=41)
    want, woff = expected(case)
    crossing = set()
    for edge in range(WINDOW, len(want), WINDOW):
        line = int(np.searchsorted(woff, edge, side="right")) - 1
        if woff[line] < edge:
            crossing.add(classes[line >> 1])
    assert crossing == {1, 2, 3, 4, 5, 6}, crossing
    check(case)
    check(case, device=True)


def test_pairs_in_any_order_with_ties_and_by_the_thousand():
    # ties in the error sum: the lowest index in `pairs` wins, wherever the pair stands
    slots = [[(0, 0, 100, 1), (0, 0, 300, 0), (0, 0, 500, 1)], [(1, 0, 150, 0), (1, 0, 350, 1), (1, 0, 550, 0)],          # fragment 0: sums 1, 1, 1, and one of 2
             [(0, 1, 10, 2)], [(1, 1, 60, 2)],                                                                              # fragment 1: one pair
             [(1, 2, 900, 0), (1, 2, 100, 0)], [(0, 2, 800, 0), (0, 2, 50, 0)]]                                              # fragment 2: two pairs without an error
    pairs = [(2, 1, 1), (0, 2, 2), (1, 0, 0), (0, 0, 1), (0, 1, 1), (2, 0, 0), (0, 0, 0)]
    case = build(slots, pairs, [30, 31, 32, 33, 34, 35], seed=50)
    lines = [ln.split(b"\t") for ln in check(case, mapq=(42, 7)).splitlines()]
    assert [int(ln[3]) for ln in lines] == [501, 551, 11, 61, 101, 51] and [int(ln[4]) for ln in lines] == [7, 7, 42, 42, 7, 7]
    assert [int(ln[8]) for ln in lines] == [81, -81, 83, -83, -84, 84]
    again = dict(case, pairs=case["pairs"][::-1].copy())                     # the other order: other pairs come first among equals
    lines = [ln.split(b"\t") for ln in check(again, device=True).splitlines()]
    assert [int(ln[3]) for ln in lines] == [101, 151, 11, 61, 901, 801]
    # one fragment with 3000 records per mate and 5000 pairs among small ones, the pairs shuffled; fragments whose mates both have records but no pair
    rng = np.random.default_rng(51)
    classes = [PROPER, SAME_SEQ, PROPER, OTHER_SEQ, PROPER, SAME_SEQ, ONLY_B, PROPER]
    slots, pairs = random_slots(classes, seed=52)
    many = lambda: [(int(rng.integers(0, 2)), 2, int(rng.integers(0, 1 << 30)), int(rng.integers(0, 4))) for _ in range(3000)]          # noqa: E731
    slots[4], slots[5] = many(), many()
    slots[10], slots[11] = many()[:700], many()[:900]                        # (no pairs here: each mate takes its primary record)
    pairs = [p for p in pairs if p[0] != 2] + [(2, int(a), int(b)) for a, b in zip(rng.integers(0, 3000, size=5000), rng.integers(0, 3000, size=5000))]
    for interleaved in (False, True):
        case = build(slots, pairs, [50, 101, 75, 40] * 4, interleaved, seed=53, shuffle=True)
        text = check(case, device=interleaved)
        assert text.count(b"NH:i:3000\n") == 2 and text.count(b"NH:i:700\n") == 1 and text.count(b"NH:i:900\n") == 1


def test_every_optional_table_given_and_missing_and_the_switches():
    classes = [1, 2, 3, 4, 5, 6, 1, 1]
    slots, pairs = random_slots(classes, seed=60)
    case = build(slots, pairs, [20, 0, 64, 101, 17, 3, 0, 0, 33, 12, 5, 5, 80, 81, 16, 48], seed=61)
    names = ("read_names", "quals_a", "quals_b", "seq_names")
    for mask in range(16):
        check(case, tables=tuple(k for bit, k in enumerate(names) if mask >> bit & 1), device=bool(mask & 1))
    plain = check(case, strip_mate_suffix=False, cigar=False, mapq=(40, 3))
    stripped = check(case)
    assert b"/1\t" in plain and b"frag_1\t" in stripped and b"frag_1/1\t" in plain and b"f0\t" in stripped and b"f0/2\t" in plain
    one = build(slots, pairs, [20, 0, 64, 101, 17, 3, 0, 0, 33, 12, 5, 5, 80, 81, 16, 48], interleaved=True, strands=False, seed=62)
    for mask in range(8):
        check(one, tables=tuple(k for bit, k in enumerate(("read_names", "quals_a", "seq_names")) if mask >> bit & 1), device=bool(mask & 1))


def test_the_counting_call_and_a_capacity_one_byte_short():
    n = 150
    slots, pairs = random_slots([1 + f % 6 for f in range(n)], seed=70)
    case = build(slots, pairs, [101] * (2 * n), seed=71)
    want, woff = expected(case)
    spec, keep = raw_spec(case)
    for device in (False, True):
        fill = np.full(len(want) + 32, 0xAA, dtype=np.uint8)
        out = DeviceBuffer.from_array(fill) if device else fill
        off = np.full(len(woff), 9, dtype=np.uint64)
        assert raw(case["rec_a"], case["rec_b"], case["pairs"], spec, out, len(want) - 1, off) == (capi.FMGPU_ERR_CAPACITY, len(want)) and off.tolist() == woff
        assert ((out.to_array(np.uint8, fill.size) if device else out) == 0xAA).all()
        assert raw(case["rec_a"], case["rec_b"], case["pairs"], spec, None, 0) == (0, len(want))          # the counting call
        doff = DeviceBuffer.from_array(np.full(len(woff), 9, dtype=np.uint64))                              # the offsets in device memory
        assert raw(case["rec_a"], case["rec_b"], case["pairs"], spec, out, len(want), doff) == (0, len(want))
        assert (out.to_array(np.uint8, fill.size) if device else out)[:len(want)].tobytes() == want and doff.to_array(np.uint64, len(woff)).tolist() == woff


def refused(case, **kw):
    """the call and the model refuse the same offender with the same code and message, and nothing is written"""
    tables = tuple(k for k in ("read_names", "quals_a", "quals_b", "seq_names") if k in kw) or ()
    full = dict(case, **kw)
    with pytest.raises(model.SamMatesError) as want:
        expected(full, tables)
    out = np.full(4096, 0xAA, dtype=np.uint8)
    off = np.full(2 * case["n"] + 1, 9, dtype=np.uint64)
    spec, keep = raw_spec(full, tables)
    rc, n = raw(full["rec_a"], full["rec_b"], full["pairs"], spec, out, out.size, off)
    message = capi.lib().fmgpu_last_error().decode()
    assert rc == CODES[want.value.code] and want.value.names in message, (message, str(want.value))
    assert (out == 0xAA).all() and (off == 9).all() and n == 0
    return want.value.who, want.value.index, want.value.what, want.value.mate


@pytest.mark.parametrize("interleaved", [False, True])
def test_device_checks_name_the_lowest_offender(interleaved):
    classes = [PROPER, SAME_SEQ, ONLY_A, PROPER, ONLY_B, NEITHER, PROPER, OTHER_SEQ]
    slots, pairs = random_slots(classes, seed=80, most=2)
    case = build(slots, pairs, [10, 20, 0, 30, 5, 12, 9, 9, 14, 3, 8, 8, 21, 22, 6, 7], interleaved, seed=81, prefix=(0, 0))
    check(case)
    A, B = "rec_a", "rec_a" if interleaved else "rec_b"
    arr_b, off_b = ("positions_a", "qoff_a") if interleaved else ("positions_b", "qoff_b")
    reads = 16 if interleaved else 8

    def edit(key, field, at, value):
        rec = case[key].copy()
        rec[field][at] = value
        return rec
    # 1: a read beyond the batch, A before B, before anything else
    bad = edit(A, "qidx", [2, 4], 2 * reads + 1)
    assert refused(case, rec_a=bad, pairs=edit("pairs", "fragment", 0, 99))[:3] == ("positions_a: record", 2, "range")
    if not interleaved:
        assert refused(case, rec_b=edit(B, "qidx", [1, 3], 2 * reads))[:3] == ("positions_b: record", 1, "range")
        assert refused(case, rec_a=bad, rec_b=edit(B, "qidx", 0, 2 * reads))[:3] == ("positions_a: record", 2, "range")
    # 2: a read below its predecessor's (the strand bit does not count)
    last = len(case[A]) - 1
    assert refused(case, rec_a=edit(A, "qidx", [last - 1, last], [2 * reads - 1, 0]))[:3] == ("positions_a: record", last, "order")
    if not interleaved:
        lb = len(case[B]) - 1
        assert refused(case, rec_b=edit(B, "qidx", lb, 0))[:3] == ("positions_b: record", lb, "order")
    # 3: offsets that decrease, before a bad pos and a bad pair
    down = case["batch_a"][1].copy(); down[2] += 6; down[5] -= 20
    assert refused(case, batch_a=(case["batch_a"][0], down), rec_a=edit(A, "pos", 0, 1 << 62))[:3] == ("qoff_a: read", 2, "qoff")
    if not interleaved:
        down = case["batch_b"][1].copy(); down[4] -= 11
        assert refused(case, batch_b=(case["batch_b"][0], down))[:3] == ("qoff_b: read", 3, "qoff")
    # 4: pos >= 2^62
    assert refused(case, rec_a=edit(A, "pos", [1, 3], [1 << 62, (1 << 64) - 1]), pairs=edit("pairs", "a", 0, 999))[:3] == ("positions_a: record", 1, "pos")
    if not interleaved:
        assert refused(case, rec_b=edit(B, "pos", 2, 1 << 63))[:3] == (arr_b + ": record", 2, "pos")
    # 5: a pair that names what does not exist, or a record of another fragment or of the wrong mate
    np_ = len(case["pairs"])
    first_of_3 = int(np.flatnonzero(case["pairs"]["fragment"] == 3)[0])
    for field, value in (("fragment", 8), ("a", len(case[A])), ("b", len(case[B])), ("fragment", 0), ("a", int(case["pairs"]["a"][0])), ("b", int(case["pairs"]["b"][0]))):
        bad = edit("pairs", field, [first_of_3, np_ - 1], value)
        assert refused(case, pairs=bad, read_names=(case["read_names"][0], case["read_names"][1][:1]))[:3] == ("pairs: pair", first_of_3, "pair")
    if interleaved:                                                          # a and b swapped: records of the wrong mates
        bad = case["pairs"].copy(); bad["a"][1], bad["b"][1] = case["pairs"]["b"][1], case["pairs"]["a"][1]
        assert refused(case, pairs=bad)[:3] == ("pairs: pair", 1, "pair")
    # 6: per line, the rows, spans and quality lengths
    short = lambda t, k: (t[0], t[1][:k])                                    # noqa: E731
    beyond = lambda t, row: (t[0], np.array([(s["offset"], s["len"] + (t[0].size if i == row else 0)) for i, s in enumerate(t[1])], dtype=TEXT_SPAN_DTYPE))  # noqa: E731
    rows_a = 2 if interleaved else 1                                         # table rows per fragment on the A side
    assert refused(case, read_names=short(case["read_names"], 3 * rows_a)) == ("fragment", 3, "read_names row", "A")
    assert refused(case, read_names=beyond(case["read_names"], 1 * rows_a)) == ("fragment", 1, "read_names span", "A")
    assert refused(case, quals_a=short(case["quals_a"], 4 * rows_a), seq_names=short(SEQS, 0)) == ("fragment", 0, "seq_names row", "A")
    if interleaved:
        assert refused(case, quals_a=short(case["quals_a"], 9)) == ("fragment", 4, "quals row", "B")
        assert refused(case, quals_a=beyond(case["quals_a"], 5)) == ("fragment", 2, "quals span", "B")
    else:
        assert refused(case, quals_a=short(case["quals_a"], 4), quals_b=short(case["quals_b"], 2)) == ("fragment", 2, "quals row", "B")
        assert refused(case, quals_b=beyond(case["quals_b"], 2)) == ("fragment", 2, "quals span", "B")
    wrong = case["quals_a"][1].copy(); wrong["len"][2 * rows_a] -= 1; wrong["len"][5 * rows_a] += 1          # neither 0 nor m
    assert refused(case, quals_a=(case["quals_a"][0], wrong)) == ("fragment", 2, "quals len", "A")
    who = refused(case, seq_names=short(SEQS, 3))                            # the lowest line that names sequence 3, as RNAME or as RNEXT
    assert who[2] == "seq_names row"
    # a refused call leaves the library usable
    check(case, device=True)


def test_what_is_too_long_is_unsupported_and_an_invalid_line_goes_first():
    """Sizes of 2^31 and more are refused by what the offsets and the spans state, in the pass that measures the lines: no byte of such a read or span is read (the
    batches are staged behind the read-back only, a table that states more than it holds lies in device memory and is used in place)."""
    big, spans = 1 << 31, lambda *rows: np.array(list(rows), dtype=TEXT_SPAN_DTYPE)          # noqa: E731
    short = np.frombuffer(b"abcdefgh", dtype=np.uint8)
    slots, pairs = [[(0, 0, 7, 0)], [(1, 0, 9, 0)], [], [(0, 1, 5, 0)]], [(0, 0, 0)]
    case = build(slots, pairs, [4, 4, 4, 4], seed=90, prefix=(0, 0))
    qbuf = case["batch_a"][0]
    far = (qbuf, np.array([0, 4, 4 + big], dtype=np.uint64))
    assert refused(case, batch_a=far) == ("fragment", 1, "read", "A")
    assert "2^31" in capi.lib().fmgpu_last_error().decode()
    assert refused(case, batch_b=far) == ("fragment", 1, "read", "B")
    assert refused(case, read_names=(short, spans((0, 3), (0, big)), big + 5)) == ("fragment", 1, "name", "A")
    assert refused(case, quals_b=(short, spans((0, 4), (0, big)), big + 5)) == ("fragment", 1, "name", "B")
    assert refused(case, seq_names=(short, spans((0, 3), (1, big)), big + 5)) == ("fragment", 1, "name", "A")          # the unmapped mate A is placed at its mate
    # a line of 2^32 bytes: SEQ and QUAL of 2^31 - 1 bytes each
    wide = (qbuf, np.array([0, big - 1, big + 3], dtype=np.uint64))
    assert refused(case, batch_a=wide, quals_a=(short, spans((0, big - 1), (0, 4)), big + 5)) == ("fragment", 0, "line", "A")
    assert "2^32" in capi.lib().fmgpu_last_error().decode()
    # an invalid line anywhere goes first
    assert refused(case, batch_a=wide, seq_names=(short, spans((0, 3)))) == ("fragment", 1, "seq_names row", "A")
    check(case)


def test_two_fastq_files_to_paired_sam_end_to_end_against_the_indexed_text(tmp_path):
    """Does not lean on the model: two FASTQ texts -> parse_queries -> map_reads on both strands -> join_mates -> format_sam_mates; the lines of every proper fragment
    are held against the text that was indexed."""
    from tests.test_example_cli import load_fasta
    from tests.test_example_cli_mates import _pair_files
    rng = np.random.default_rng(41)
    _, (ref, t1, t2) = _pair_files(rng, tmp_path)
    texts = [np.array(s, dtype=np.uint8) for s in load_fasta(ref, False)]
    assert [t.size for t in texts] == [1800, 1200, 900]

    def fastq(fasta):
        recs = [r.split("\n") for r in fasta.split(">")[1:]]
        return "".join("@%s extra\n%s\n+\n%s\n" % (r[0], r[1], "".join(chr(33 + (7 * i + len(r[0])) % 90) for i in range(len(r[1])))) for r in recs).encode()
    raws = [fastq(t1), fastq(t2)]
    gx = fm.BiFMIndex.from_sequences(texts, 5, "IB16", 16)
    parsed = [fm.parse_queries(raw, "fastq", fm.symbol_table.dna5(), device=True, want_names=True, want_quals=True) for raw in raws]
    assert [p.reads for p in parsed] == [60, 60]
    pos = [fm.map_reads(gx, p.batch, errors=2, edit=False, strands="dna5") for p in parsed]
    qoffs = [p.batch[1] for p in parsed]
    joined = fm.join_mates(pos[0], qoffs[0], pos[1], qoffs[1], min_tlen=0, max_tlen=1000)
    text, off = fm.format_sam_mates(pos[0], parsed[0].batch, pos[1], parsed[1].batch, pairs=joined, strands="dna5", read_names=(raws[0], parsed[0].names),
                                    quals_a=(raws[0], parsed[0].quals), quals_b=(raws[1], parsed[1].quals), seq_names=[b"chr0", b"chr1", b"chr2"],
                                    want_line_offsets=True)
    lines = [ln.split(b"\t") for ln in text.splitlines()]
    assert len(lines) == 120 and off[-1] == len(text)
    value = {c: i for i, c in enumerate(b"$ACGT")}
    proper = 0
    for f in range(60):
        a, b = lines[2 * f], lines[2 * f + 1]
        assert a[0] == b[0] == b"frag%d" % f
        fa, fb = int(a[1]), int(b[1])
        assert fa & 65 == 65 and fb & 129 == 129 and bool(fa & 2) == bool(fb & 2) == (joined.cls[f] == 4)
        if not fa & 2:
            continue
        proper += 1
        mine = joined.pairs[joined.off[f]: joined.off[f + 1]]
        for ln in (a, b):
            t, p = texts[int(ln[2][3:])], int(ln[3]) - 1
            seq = np.array([value[c] for c in ln[9]], dtype=np.uint8)
            assert ln[5] == b"36M" and len(ln[10]) == 36 and ln[11].startswith(b"NM:i:")
            assert int((seq != t[p: p + 36]).sum()) == int(ln[11][5:]) <= 2
        assert bool(fa & 16) == bool(fb & 32) and bool(fb & 16) == bool(fa & 32) and bool(fa & 16) != bool(fb & 16)
        assert a[6] == b[6] == b"=" and a[7] == b[3] and b[7] == a[3]
        assert int(a[8]) + int(b[8]) == 0 and abs(int(a[8])) in set(int(t) for t in mine["tlen"])
        assert int(a[11][5:]) + int(b[11][5:]) == int(mine["errors"].min())
    assert proper >= 50
