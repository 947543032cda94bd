"""fmgpu_positions_sam_mates (include/fmgpu.h) on the host: the symbol and the struct, every argument check that comes before the first use of the device, and the
plain-Python model of tests/sam_mates_model.py against the header's worked example, hand-written lines for the six situations of a fragment, the model of
fmgpu_positions_sam for the fields both calls share, and the QNAME rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import MATE_PAIR_DTYPE, POSITION_DTYPE, TEXT_SPAN_DTYPE
from tests import sam_mates_model as model
from tests import sam_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAR_OF = fm.char_table("dna5")
COMP = np.array(fm.DNA5_COMPLEMENT, dtype=np.uint8)


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def last_error():
    return capi.lib().fmgpu_last_error()


def records(rows):
    return np.array([(q, s, p, e, 0) for q, s, p, e in rows], dtype=POSITION_DTYPE)


def pair_records(rows):
    return np.array([(f, 0, a, b, 0, 0) for f, a, b in rows], dtype=MATE_PAIR_DTYPE)


def test_the_symbol_exists_and_the_abi_version_stays():
    L = capi.lib()
    assert "fmgpu_positions_sam_mates" in capi.EXPORTS and hasattr(L, "fmgpu_positions_sam_mates")
    assert re.search(r"\bint\s+fmgpu_positions_sam_mates\s*\(", header())
    assert L.fmgpu_abi_version() == 6 and re.search(r"#define FMGPU_ABI_VERSION 6\b", header())
    assert "format_sam_mates" in fm.__all__


def test_the_struct_mirrors_the_header():
    body = re.search(r"typedef struct fmgpu_sam_mates_spec \{(.*?)\} fmgpu_sam_mates_spec;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            names += [re.sub(r"\[\d+\]", "", first.split()[-1]).lstrip("*")] + [re.sub(r"\[\d+\]", "", m.strip()).lstrip("*") for m in more]
    S = capi.SamMatesSpec
    assert C.sizeof(S) == 96 and "96 bytes" in re.search(r"typedef struct fmgpu_sam_mates_spec \{(.*)", header()).group(1)
    assert [f[0] for f in S._fields_] == names == ["qbuf_a", "qoff_a", "qbuf_b", "qoff_b", "n_fragments", "char_of", "strands", "read_names", "quals_a", "quals_b",
                                                    "seq_names", "interleaved", "cigar", "strip_mate_suffix", "mapq_unique", "mapq_multi", "reserved"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 89, 90, 91, 92, 93]


QBUF = np.array([1, 2, 3, 4], dtype=np.uint8)
QOFF = np.array([0, 2, 4], dtype=np.uint64)
KEEP = object()


def spec(qbuf_a=QBUF, qoff_a=QOFF, qbuf_b=KEEP, qoff_b=KEEP, n=2, char_of=CHAR_OF, strands=None, read_names=None, quals_a=None, quals_b=None, seq_names=None,
         interleaved=0, cigar=1, strip=1, reserved=(0, 0, 0)):
    """two fragments; separate mode takes the one batch for both sides unless told otherwise, interleaved mode (then n = 1 fits the batch) has no B side"""
    if qbuf_b is KEEP:
        qbuf_b = None if interleaved else QBUF
    if qoff_b is KEEP:
        qoff_b = None if interleaved else QOFF
    p = lambda a: a if a is None or isinstance(a, C.c_void_p) else capi.ptr(a)          # noqa: E731
    t = lambda a: None if a is None else C.pointer(a)                                   # noqa: E731
    return capi.SamMatesSpec(p(qbuf_a), p(qoff_a), p(qbuf_b), p(qoff_b), n, p(char_of), t(strands), t(read_names), t(quals_a), t(quals_b), t(seq_names), interleaved,
                             cigar, strip, 60, 0, (C.c_uint8 * 3)(*reserved))


def test_argument_checks_come_before_the_device():
    L = capi.lib()
    rec = np.zeros(2, dtype=POSITION_DTYPE)
    prs = np.zeros(1, dtype=MATE_PAIR_DTYPE)
    out = np.full(64, 0xAA, dtype=np.uint8)
    garbage = C.c_void_p(0x10)                                           # never read through: the checks come first
    nbytes = C.c_uint64(7)
    names = np.zeros(4, dtype=np.uint8)
    spans = np.zeros(1, dtype=TEXT_SPAN_DTYPE)
    A = capi.ptr(rec)

    def call(s, pa=A, ca=2, pb=A, cb=2, pairs=capi.ptr(prs), n_pairs=1, out_=capi.ptr(out), capacity=64, out_bytes=C.byref(nbytes)):
        return L.fmgpu_positions_sam_mates(pa, ca, pb, cb, pairs, n_pairs, None if s is None else C.byref(s), out_, capacity, out_bytes, None, None)

    def inter(**kw):
        return call(spec(interleaved=1, n=1, **kw), pb=None, cb=0)

    no_bytes = capi.NameTable(None, 4, capi.ptr(spans).value, 1)
    no_spans = capi.NameTable(capi.ptr(names).value, 4, None, 1)
    fine = capi.NameTable(capi.ptr(names).value, 4, capi.ptr(spans).value, 1)
    comp = COMP.ctypes.data_as(capi.u8p)
    cases = [
        (lambda: call(None), b"spec is null"),
        (lambda: call(spec(char_of=None)), b"char_of is null"),
        (lambda: call(spec(), out_bytes=None), b"out_bytes is null"),
        (lambda: call(spec(qbuf_a=None)), b"qbuf_a is null while n_fragments > 0"),
        (lambda: call(spec(qoff_a=None)), b"qoff_a is null while n_fragments > 0"),
        (lambda: call(spec(qbuf_b=None)), b"qbuf_b is null in separate mode"),
        (lambda: call(spec(qoff_b=None)), b"qoff_b is null in separate mode"),
        (lambda: call(spec(), pb=None), b"positions_b is null while count_b > 0"),
        (lambda: inter(qbuf_b=QBUF), b"qbuf_b and qoff_b must be null in interleaved mode"),
        (lambda: inter(qoff_b=QOFF), b"qbuf_b and qoff_b must be null in interleaved mode"),
        (lambda: inter(quals_b=fine), b"quals_b must be null in interleaved mode"),
        (lambda: call(spec(interleaved=1, n=1), pb=A, cb=0), b"positions_b must be null with count_b = 0 in interleaved mode"),
        (lambda: call(spec(interleaved=1, n=1), pb=None, cb=2), b"positions_b must be null with count_b = 0 in interleaved mode"),
        (lambda: call(spec(), pa=None), b"positions_a is null while count_a > 0"),
        (lambda: call(spec(), pairs=None), b"pairs is null while n_pairs > 0"),
        (lambda: call(spec(), out_=None), b"out is null while capacity > 0"),
        (lambda: call(spec(interleaved=2)), b"interleaved must be 0 or 1"),
        (lambda: call(spec(cigar=2)), b"cigar must be 0 or 1"),
        (lambda: call(spec(strip=255)), b"strip_mate_suffix must be 0 or 1"),
        (lambda: call(spec(reserved=(0, 0, 1))), b"reserved must be 0"),
        (lambda: call(spec(reserved=(1, 0, 0))), b"reserved must be 0"),
        (lambda: call(spec(strands=capi.Strands(None, 5, 0))), b"strands has a null complement"),
        (lambda: call(spec(strands=capi.Strands(comp, 0, 0))), b"strands->n must be in [1, 256]"),
        (lambda: call(spec(strands=capi.Strands(comp, 257, 0))), b"strands->n must be in [1, 256]"),
        (lambda: call(spec(read_names=no_bytes)), b"the read_names table has no bytes but n_bytes > 0"),
        (lambda: call(spec(read_names=no_spans)), b"the read_names table has no spans but count > 0"),
        (lambda: call(spec(quals_a=no_bytes)), b"the quals_a table has no bytes but n_bytes > 0"),
        (lambda: call(spec(quals_a=no_spans)), b"the quals_a table has no spans but count > 0"),
        (lambda: call(spec(quals_b=no_bytes)), b"the quals_b table has no bytes but n_bytes > 0"),
        (lambda: call(spec(quals_b=no_spans)), b"the quals_b table has no spans but count > 0"),
        (lambda: call(spec(seq_names=no_bytes)), b"the seq_names table has no bytes but n_bytes > 0"),
        (lambda: call(spec(seq_names=no_spans)), b"the seq_names table has no spans but count > 0"),
        # the same with no record, no pair and no fragment: the checks do not depend on them
        (lambda: call(spec(reserved=(0, 9, 0)), pa=None, ca=0, pb=None, cb=0, pairs=None, n_pairs=0), b"reserved must be 0"),
        (lambda: call(spec(qbuf_a=None, qoff_a=None, qbuf_b=None, qoff_b=None, n=0, cigar=3)), b"cigar must be 0 or 1"),
        (lambda: call(spec(char_of=None, qbuf_a=None, qoff_a=None, n=0), pa=None, ca=0), b"char_of is null"),
        # garbage pointers behind a bad spec are never looked at
        (lambda: call(spec(qbuf_a=garbage, qoff_a=garbage, qbuf_b=garbage, qoff_b=garbage, reserved=(0, 1, 0)), pa=garbage, pb=garbage, pairs=garbage, out_=garbage),
         b"reserved must be 0"),
    ]
    messages = set()
    for run, word in cases:
        nbytes.value = 7
        assert run() == capi.FMGPU_ERR_INVALID and word in last_error(), (word, last_error())
        messages.add(last_error())
    assert len(messages) == 28                                           # each check has a message of its own
    assert (out == 0xAA).all()
    # the size limits: refused before anything is staged
    big = (1 << 32) - 256
    g = spec(qbuf_a=garbage, qoff_a=garbage, qbuf_b=garbage, qoff_b=garbage)
    for kw in (dict(ca=big), dict(cb=big), dict(n_pairs=big)):
        assert call(g, **dict(dict(pa=garbage, pb=garbage, pairs=garbage, out_=None, capacity=0), **kw)) == capi.FMGPU_ERR_UNSUPPORTED and b"2^32 - 256" in last_error()
    g = spec(qbuf_a=garbage, qoff_a=garbage, qbuf_b=garbage, qoff_b=garbage, n=(1 << 31) - 1)
    assert call(g, pa=garbage, pb=garbage, pairs=garbage, out_=None, capacity=0) == capi.FMGPU_ERR_UNSUPPORTED and b"2^31 - 1" in last_error()


def test_no_fragment_returns_zero_behind_the_checks():
    L = capi.lib()
    nbytes = C.c_uint64(7)
    off = np.full(3, 9, dtype=np.uint64)
    none = spec(qbuf_a=None, qoff_a=None, qbuf_b=None, qoff_b=None, n=0)
    assert L.fmgpu_positions_sam_mates(None, 0, None, 0, None, 0, C.byref(none), None, 0, C.byref(nbytes), capi.ptr(off), None) == 0
    assert nbytes.value == 0 and off.tolist() == [0, 9, 9]
    empty = (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    no = np.zeros(0, dtype=POSITION_DTYPE)
    assert fm.format_sam_mates(no, empty, no, empty) == b""
    text, offsets = fm.format_sam_mates(no, empty, interleaved=True, want_line_offsets=True)
    assert text == b"" and offsets.tolist() == [0]
    assert model.format_sam_mates(no, empty, no, empty, char_of=CHAR_OF) == (b"", [0])
    for bad in (dict(positions_b=no), dict(queries_b=empty), dict(quals_b=[b"x"])):
        with pytest.raises(ValueError):
            fm.format_sam_mates(no, empty, interleaved=True, **bad)
    with pytest.raises(ValueError):
        fm.format_sam_mates(no, empty)


def test_the_model_writes_the_worked_example_of_the_header_text():
    """fragment 0, m = 4: mate A ACGT at seq 0, pos 10, strand 0, no error; mate B GGTA at seq 0, pos 50, strand 1, one error; one pair joins them"""
    ra, rb = records([(0, 0, 10, 0)]), records([(1, 0, 50, 1)])
    qa, qb = fm.flatten([[1, 2, 3, 4]]), fm.flatten([[3, 3, 4, 1]])
    text, off = model.format_sam_mates(ra, qa, rb, qb, pair_records([(0, 0, 0)]), CHAR_OF, fm.DNA5_COMPLEMENT)
    want = [b"0\t99\t0\t11\t60\t4M\t=\t51\t44\tACGT\t*\tNM:i:0\tNH:i:1\n", b"0\t147\t0\t51\t60\t4M\t=\t11\t-44\tTACC\t*\tNM:i:1\tNH:i:1\n"]
    assert text == b"".join(want) and off == [0, len(want[0]), len(want[0]) + len(want[1])]
    # the same two reads as one interleaved batch: pairs[].b indexes the one array
    rec = records([(0, 0, 10, 0), (3, 0, 50, 1)])
    both = model.format_sam_mates(rec, fm.flatten([[1, 2, 3, 4], [3, 3, 4, 1]]), pairs=pair_records([(0, 0, 1)]), char_of=CHAR_OF, complement=fm.DNA5_COMPLEMENT,
                                  interleaved=True)
    assert both == (text, off)


# six fragments, one per situation; reads of 3 .. 6 symbols, names with the mate suffix, qualities for both batches, named sequences
READS_A = [[1, 2, 3, 4], [1, 1, 2], [4, 4, 4, 1, 2], [2, 3, 2], [3, 3, 3, 1], [1, 4]]
READS_B = [[3, 3, 4, 1, 1], [2, 2, 2, 2], [1, 2, 1], [4, 1, 4, 1], [2, 2, 1], [4, 4, 4]]
NAMES = [b"f0/1 first", b"f1/1", b"f2/1", b"f3/1", b"f4/1\tx", b"f5/1"]
QUALS_A = [b"ABCD", b"EFG", b"HIJKL", b"MNO", b"PQRS", b"TU"]
QUALS_B = [b"abcde", b"fghi", b"jkl", b"mnop", b"qrs", b"tuv"]
SEQS = [b"chr1 one", b"chr2", b"chrM"]
# qidx = 2 read + strand.  Fragment 0: a proper pair (two pair records, the second with fewer errors wins); 1: both mapped on chr2, no pair; 2: chr1 and chrM; 3: only A
# (twice, equally good); 4: only B; 5: neither
REC_A = [(0, 0, 100, 1), (0, 0, 400, 0), (2, 1, 30, 0), (5, 0, 7, 2), (6, 2, 9, 0), (7, 2, 90, 0)]
REC_B = [(1, 0, 150, 1), (1, 0, 460, 0), (2, 1, 10, 1), (4, 2, 7, 0), (9, 1, 0, 3)]
PAIRS = [(0, 0, 0), (0, 1, 1)]
SIX = [b"f0\t99\tchr1\t401\t60\t4M\t=\t461\t65\tACGT\tABCD\tNM:i:0\tNH:i:2\n",
       b"f0\t147\tchr1\t461\t60\t5M\t=\t401\t-65\tTTACC\tedcba\tNM:i:0\tNH:i:2\n",
       b"f1\t65\tchr2\t31\t60\t3M\t=\t11\t-23\tAAC\tEFG\tNM:i:0\tNH:i:1\n",
       b"f1\t129\tchr2\t11\t60\t4M\t=\t31\t23\tCCCC\tfghi\tNM:i:1\tNH:i:1\n",
       b"f2\t81\tchr1\t8\t60\t5M\tchrM\t8\t0\tGTAAA\tLKJIH\tNM:i:2\tNH:i:1\n",
       b"f2\t161\tchrM\t8\t60\t3M\tchr1\t8\t0\tACA\tjkl\tNM:i:0\tNH:i:1\n",
       b"f3\t73\tchrM\t10\t0\t3M\t=\t10\t0\tCGC\tMNO\tNM:i:0\tNH:i:2\n",
       b"f3\t133\tchrM\t10\t0\t*\t=\t10\t0\tTATA\tmnop\n",
       b"f4\t101\tchr2\t1\t0\t*\t=\t1\t0\tGGGA\tPQRS\n",
       b"f4\t153\tchr2\t1\t60\t3M\t=\t1\t0\tTGG\tsrq\tNM:i:3\tNH:i:1\n",
       b"f5\t77\t*\t0\t0\t*\t*\t0\t0\tAT\tTU\n",
       b"f5\t141\t*\t0\t0\t*\t*\t0\t0\tTTT\ttuv\n"]


def six(**kw):
    args = dict(char_of=CHAR_OF, complement=fm.DNA5_COMPLEMENT, read_names=fm.pack_names(NAMES), quals_a=fm.pack_names(QUALS_A), quals_b=fm.pack_names(QUALS_B),
                seq_names=fm.pack_names(SEQS))
    pairs = kw.pop("pairs", PAIRS)
    args.update(kw)
    return model.format_sam_mates(records(REC_A), fm.flatten(READS_A), records(REC_B), fm.flatten(READS_B), pair_records(pairs), **args)


def test_the_model_writes_hand_written_lines_for_the_six_situations():
    text, off = six()
    got = text.split(b"\n")
    for k, want in enumerate(SIX):
        assert got[k] + b"\n" == want, (k, got[k], want)
    assert text == b"".join(SIX) and off == [sum(len(w) for w in SIX[:k]) for k in range(len(SIX) + 1)]
    # a tie in the error sum: the lowest pair index wins, and MAPQ says that the choice was not unique
    tie = records([(0, 0, 100, 0), (0, 0, 400, 0)] + REC_A[2:])
    text, _ = model.format_sam_mates(tie, fm.flatten(READS_A), records([(1, 0, 150, 0), (1, 0, 460, 0)] + REC_B[2:]), fm.flatten(READS_B), pair_records(PAIRS[::-1]),
                                     CHAR_OF, fm.DNA5_COMPLEMENT, mapq_unique=50, mapq_multi=3)
    assert text.split(b"\n")[0] == b"0\t99\t0\t401\t3\t4M\t=\t461\t65\tACGT\t*\tNM:i:0\tNH:i:2"
    assert text.split(b"\n")[1] == b"0\t147\t0\t461\t3\t5M\t=\t401\t-65\tTTACC\t*\tNM:i:0\tNH:i:2"
    # equal pos: A writes t, B writes -t; t = 0 is written as 0, never -0
    ra, rb = records([(0, 0, 5, 0)]), records([(0, 0, 5, 0)])
    text, _ = model.format_sam_mates(ra, fm.flatten([[1, 2]]), rb, fm.flatten([[1, 2, 3]]), char_of=CHAR_OF)
    assert [ln.split(b"\t")[8] for ln in text.split(b"\n")[:2]] == [b"3", b"-3"]
    text, _ = model.format_sam_mates(ra, fm.flatten([[]]), rb, fm.flatten([[]]), char_of=CHAR_OF, cigar=1)
    assert text == b"0\t65\t0\t6\t60\t*\t=\t6\t0\t*\t*\tNM:i:0\tNH:i:1\n0\t129\t0\t6\t60\t*\t=\t6\t0\t*\t*\tNM:i:0\tNH:i:1\n"


def test_a_fragment_without_a_pair_writes_the_fields_of_the_primary_lines_of_format_sam():
    """QNAME, RNAME, POS, MAPQ, CIGAR, SEQ, QUAL, NM and NH of each mate's line equal those of the primary line the model of fmgpu_positions_sam writes for that read"""
    text, _ = six(pairs=[], strip_mate_suffix=0)
    paired = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
    shared = (0, 2, 3, 4, 5, 9, 10, 11, 12)
    seen = 0
    for side, (rec, reads, quals) in enumerate(((REC_A, READS_A, QUALS_A), (REC_B, READS_B, QUALS_B))):
        single, _ = sam_model.format_sam(records(rec), *fm.flatten(reads), CHAR_OF, fm.DNA5_COMPLEMENT, fm.pack_names(NAMES), fm.pack_names(quals), fm.pack_names(SEQS))
        primary = {}
        for ln in single.split(b"\n")[:-1]:
            f = ln.split(b"\t")
            if not int(f[1]) & 256:
                primary[f[0]] = f
        for frag in range(6):
            mine, other = paired[2 * frag + side], paired[2 * frag + 1 - side]
            want = primary[mine[0]]
            if int(want[1]) & 4:                                 # no record: placed at its mate if that one has a record
                assert int(mine[1]) & 4 and mine[9:] == want[9:] and mine[5] == b"*" and mine[4] == b"0"
                assert mine[2:4] == (other[2:4] if not int(other[1]) & 4 else [b"*", b"0"])
            else:
                assert [mine[k] for k in shared] == [want[k] for k in shared], (side, frag)
                assert bool(int(mine[1]) & 16) == bool(int(want[1]) & 16)
                seen += 1
    assert seen == 8


@pytest.mark.parametrize("name, want", [(b"x/1", b"x"), (b"/1", b"/1"), (b"x/3", b"x/3"), (b"x/2 second mate", b"x"), (b"ab/2/1", b"ab/2"), (b"", b"*"), (b" x", b"*"),
                                        (b"r/1/", b"r/1/")])
def test_strip_mate_suffix(name, want):
    ra, rb = records([]), records([])
    for strip in (1, 0):
        text, _ = model.format_sam_mates(ra, fm.flatten([[1]]), rb, fm.flatten([[2]]), char_of=CHAR_OF, read_names=fm.pack_names([name]), strip_mate_suffix=strip)
        cut = name.split(b" ")[0].split(b"\t")[0]
        assert [ln.split(b"\t")[0] for ln in text.split(b"\n")[:2]] == [want if strip else (cut or b"*")] * 2


def test_the_model_refuses_in_the_order_of_the_header_text():
    qa, qb = fm.flatten(READS_A), fm.flatten(READS_B)

    def refused(ra=REC_A, rb=REC_B, pairs=PAIRS, qa_=qa, qb_=qb, **kw):
        with pytest.raises(model.SamMatesError) as e:
            model.format_sam_mates(records(ra), qa_, records(rb), qb_, pair_records(pairs), CHAR_OF, fm.DNA5_COMPLEMENT, **kw)
        return e.value.code, e.value.who, e.value.index, e.value.what, e.value.mate

    down = (qa[0], np.array([0, 4, 3, 12, 15, 19, 21], dtype=np.uint64))
    assert refused(ra=REC_A + [(12, 0, 0, 0)], rb=[(99, 0, 0, 0)]) == (model.INVALID, "positions_a: record", 6, "range", None)
    assert refused(rb=[(99, 0, 0, 0)] + REC_B, ra=REC_A[::-1]) == (model.INVALID, "positions_b: record", 0, "range", None)
    assert refused(ra=REC_A[::-1], rb=REC_B[::-1]) == (model.INVALID, "positions_a: record", 2, "order", None)
    assert refused(rb=REC_B[::-1], qa_=down) == (model.INVALID, "positions_b: record", 1, "order", None)
    assert refused(qa_=down, ra=[(0, 0, 1 << 62, 0)]) == (model.INVALID, "qoff_a: read", 1, "qoff", None)
    assert refused(ra=[(0, 0, 1 << 62, 0)], rb=[(0, 0, 1 << 63, 0)], pairs=[(9, 0, 0)]) == (model.INVALID, "positions_a: record", 0, "pos", None)
    for bad in ((6, 0, 0), (0, 6, 0), (0, 0, 5), (0, 2, 0), (0, 0, 2), (1, 0, 0)):
        assert refused(pairs=[(0, 0, 0), bad, (7, 0, 0)], read_names=(b"", [])) == (model.INVALID, "pairs: pair", 1, "pair", None)
    assert refused(read_names=fm.pack_names(NAMES[:4]), quals_a=(b"ABCD", [(0, 4)] * 6)) == (model.INVALID, "fragment", 1, "quals len", "A")
    assert refused(read_names=fm.pack_names(NAMES[:4]), quals_b=(b"ABCD", [(0, 4)] * 6)) == (model.INVALID, "fragment", 0, "quals len", "B")
    assert refused(seq_names=fm.pack_names(SEQS[:2])) == (model.INVALID, "fragment", 2, "seq_names row", "A")
    big = 1 << 31
    far = (qa[0], np.array([0, 4, 7, 12, 15, 19, 19 + big], dtype=np.uint64))
    assert refused(qa_=far) == (model.UNSUPPORTED, "fragment", 5, "read", "A")
    assert refused(qa_=far, seq_names=fm.pack_names(SEQS[:2])) == (model.INVALID, "fragment", 2, "seq_names row", "A")
    e = model.SamMatesError(model.INVALID, "fragment", 2, "seq_names row", "A")
    assert e.names == "fragment 2 mate A names a row beyond the seq_names table"
