"""fmgpu_positions_mates on the device (include/fmgpu.h): synthetic position records joined and compared record for record, with out_off, out_class and *out_count,
against the plain-Python model of tests/mates_model.py.  The shapes are the smallest at which the kernels can go wrong: runs of records that straddle the 256 lanes of
a workgroup, empty mates at every place, one fragment of 3 000 x 3 000 records in a tandem layout, positions above 2^32 and below max_tlen, several sequences inside a
run, both modes, every switch, host and device memory.  One end-to-end test maps two batches of mates cut from an indexed text and finds every fragment's true pair.
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import MATE_PAIR_DTYPE, POSITION_DTYPE, DeviceBuffer
from tests import mates_model as model

pytestmark = pytest.mark.gpu
KINDS = {"fr": model.FR, "any": model.ANY}


def make_side(per_read, seed, strands=True, nseq=3, base=0, span=2500, errors=3):
    """per_read[r] records for read r, in read order: random strand, seq_id below nseq, pos in [base, base + span), errors below `errors` (ties are common)"""
    rng = np.random.default_rng(seed)
    reads = np.repeat(np.arange(len(per_read), dtype=np.uint64), per_read)
    rec = np.zeros(reads.size, dtype=POSITION_DTYPE)
    st = rng.integers(0, 2, size=reads.size).astype(np.uint64)
    rec["qidx"] = 2 * reads + st if strands else reads
    rec["seq_id"] = rng.integers(0, nseq, size=reads.size)
    rec["pos"] = np.uint64(base) + rng.integers(0, span, size=reads.size).astype(np.uint64)
    rec["errors"] = rng.integers(0, errors, size=reads.size)
    rec["hit"] = np.arange(reads.size)
    return rec


def make_qoff(n, seed, first=7):
    rng = np.random.default_rng(seed)
    return (first + np.concatenate([[0], np.cumsum(rng.integers(30, 151, size=n))])).astype(np.uint64)


def dev(a):
    return DeviceBuffer.from_array(a) if a is not None and a.size else a


def check(ra, qa, rb, qb, device=(), strands=True, **kw):
    """join_mates against the model: pairs, off, cls; `device`: which of "a", "b", "qoff" lie in device memory"""
    mkw = dict(kw)
    mkw["orientation"] = KINDS[kw.get("orientation", "fr")]
    want = model.join(ra, qa, rb, qb, strand_shift=1 if strands else 0, **mkw)
    got = fm.join_mates(dev(ra) if "a" in device else ra, dev(qa) if "qoff" in device else qa, dev(rb) if "b" in device else rb,
                        dev(qb) if "qoff" in device and qb is not None else qb, strands=strands, **kw)
    assert got.off.tolist() == want[1] and got.cls.tolist() == want[2]
    assert got.pairs.tobytes() == model.as_array(want[0], MATE_PAIR_DTYPE).tobytes()
    return got


def test_runs_that_straddle_the_workgroup_edge_and_empty_mates_everywhere():
    # A: records 0 .. 2, 3 .. 252, 253 .. 262 (across lane 256), none, 263 .. 562 (across 512), ...; B the same shifted; the first and the last fragment are empty
    per_a = [0, 3, 250, 10, 0, 300, 1, 0, 5, 190, 7, 0]
    per_b = [0, 250, 3, 0, 9, 260, 0, 1, 5, 7, 250, 0]
    n = len(per_a)
    ra, rb = make_side(per_a, 1), make_side(per_b, 2)
    qa, qb = make_qoff(n, 3), make_qoff(n, 4, first=0)
    got = check(ra, qa, rb, qb)
    assert got.cls[[0, 3, 4, 6, 7, 11]].tolist() == [0, 1, 2, 1, 2, 0] and got.cls[5] == 4 and len(got) > 1000
    check(ra, qa, rb, qb, device=("a", "b", "qoff"))
    check(ra, qa, rb, qb, device=("a",), orientation="any", min_tlen=200, max_tlen=700)
    check(ra, qa, rb, qb, device=("b", "qoff"), best=True)
    # no record on one side, on the other, on both: classes only
    none = np.zeros(0, dtype=POSITION_DTYPE)
    assert check(none, qa, rb, qb).cls.tolist() == [2 if c else 0 for c in per_b]
    assert check(ra, qa, none, qb, device=("a",)).cls.tolist() == [1 if c else 0 for c in per_a]
    assert check(none, qa, none, qb).cls.tolist() == [0] * n
    # one fragment, one record each
    check(make_side([1], 5, nseq=1, span=300), make_qoff(1, 5), make_side([1], 6, nseq=1, span=300), make_qoff(1, 6), orientation="any")
    # 257 fragments: the highest read number is 2^8, one key bit more in the last sort than 256 fragments take; the last fragment has records on both sides
    many = check(make_side([2] * 257, 7, nseq=1, span=300), make_qoff(257, 7), make_side([2] * 257, 8, nseq=1, span=300), make_qoff(257, 8), orientation="any")
    assert many.cls[256] == 4 and many.cls[255] == 4


@pytest.mark.parametrize("strands", [True, False])
def test_every_switch_against_the_model(strands):
    rng = np.random.default_rng(11)
    n = 60
    per_a, per_b = rng.integers(0, 9, size=n).tolist(), rng.integers(0, 9, size=n).tolist()
    per_a[:4], per_b[:4] = [0, 0, 3, 2], [0, 2, 0, 3]
    ra, rb = make_side(per_a, 12, strands=strands, span=1500), make_side(per_b, 13, strands=strands, span=1500)
    qa, qb = make_qoff(n, 14), make_qoff(n, 15)
    seen = set()
    for orientation in ("fr", "any"):
        for best in (False, True):
            for max_records in (0, 1, 5):
                got = check(ra, qa, rb, qb, strands=strands, orientation=orientation, best=best, max_records=max_records, min_tlen=60, max_tlen=900)
                seen |= set(got.cls.tolist())
                if orientation == "fr" and not strands:
                    assert len(got) == 0                                 # every strand is 0: FR finds nothing, and that is no error
    assert seen == {0, 1, 2, 3, 4, 5}


def test_a_tandem_run_of_3000_by_3000_records():
    """one fragment whose mates each have 3 000 records 7 apart, every tenth position twice: a window of +- 1000 holds hundreds of candidates; a light fragment on each side"""
    def tandem(read, seed):
        rng = np.random.default_rng(seed)
        pos = 5000 + 7 * (np.arange(3000) - (np.arange(3000) % 10 == 9))         # record 10k + 9 repeats the position of record 10k + 8
        rec = np.zeros(3000, dtype=POSITION_DTYPE)
        rec["qidx"] = 2 * read + rng.integers(0, 2, size=3000)
        rec["seq_id"] = 1
        rec["pos"] = rng.permutation(pos)                                        # a run is in no order of its own
        rec["errors"] = rng.integers(0, 3, size=3000)
        return rec
    light_a, light_b = make_side([2, 0, 3], 21), make_side([2, 0, 3], 22)
    ra = np.concatenate([light_a[:2], tandem(1, 23), light_a[2:]])
    rb = np.concatenate([light_b[:2], tandem(1, 24), light_b[2:]])
    qa, qb = make_qoff(3, 25), make_qoff(3, 26)
    got = check(ra, qa, rb, qb, device=("a", "b", "qoff"), max_tlen=1000)
    assert got.cls[1] == 4
    assert int(got.off[2] - got.off[1]) > 3000 * 40                              # hundreds of candidates per record; a quarter of them are on the other strand and in FR order
    best = check(ra, qa, rb, qb, best=True, max_tlen=1000)
    assert 0 < int(best.off[2] - best.off[1]) < int(got.off[2] - got.off[1]) and (best.pairs["errors"][int(best.off[1]): int(best.off[2])] == 0).all()
    assert check(ra, qa, rb, qb, max_records=2999).cls[1] == 5


def test_positions_above_2_32_and_below_max_tlen():
    n = 30
    rng = np.random.default_rng(31)
    per_a, per_b = rng.integers(1, 6, size=n).tolist(), rng.integers(1, 6, size=n).tolist()
    far_a, far_b = make_side(per_a, 32, base=(1 << 40) + 5, span=800), make_side(per_b, 33, base=(1 << 40) + 5, span=800)
    qa, qb = make_qoff(n, 34), make_qoff(n, 35)
    got = check(far_a, qa, far_b, qb, device=("a", "b"), orientation="any", max_tlen=600)
    assert len(got) > 0 and (got.pairs["tlen"] <= 600).all()
    # seq_id of 2^32 and more, in the opposite order of their low 32 bits: an order of the B side by fewer than 64 bits would misplace every run
    wide = np.array([(1 << 33) + 1, (1 << 32) + 3, 5], dtype=np.uint64)
    wide_a, wide_b = far_a.copy(), far_b.copy()
    wide_a["seq_id"], wide_b["seq_id"] = wide[far_a["seq_id"]], wide[far_b["seq_id"]]
    for device in ((), ("b",), ("a", "b", "qoff")):
        assert len(check(wide_a, qa, wide_b, qb, device=device, orientation="any", max_tlen=600)) == len(got)
    assert len(check(wide_a, qa, wide_b, qb, best=True, max_tlen=600)) > 0             # FR and best: the walks' bisection on the 64-bit seq_id
    # the highest pos the call takes, and a window that reaches below 0: p(a) < max_tlen clamps to 0
    edge_a, edge_b = make_side(per_a, 36, span=300), make_side(per_b, 37, span=300)
    assert len(check(edge_a, qa, edge_b, qb, orientation="any", max_tlen=1000)) > 0
    edge_a["pos"][0], edge_b["pos"][0] = (1 << 62) - 1, (1 << 62) - 40
    edge_a["seq_id"][0] = edge_b["seq_id"][0] = 2
    got = check(edge_a, qa, edge_b, qb, orientation="any", max_tlen=(1 << 64) - 1)
    assert ((got.pairs["a"] == 0) & (got.pairs["b"] == 0)).any()


def interleave(ra, qa, rb, qb, n):
    """the two batches as one: reads 2f and 2f + 1; returns (records, qoff, new index of every A-record, of every B-record)"""
    la, lb = np.diff(qa.astype(np.int64)), np.diff(qb.astype(np.int64))
    lens = np.empty(2 * n, dtype=np.int64)
    lens[0::2], lens[1::2] = la, lb
    qoff = (3 + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    read_a, read_b = (ra["qidx"] >> np.uint64(1)).astype(np.int64), (rb["qidx"] >> np.uint64(1)).astype(np.int64)
    key = np.concatenate([2 * read_a, 2 * read_b + 1])
    order = np.argsort(key, kind="stable")
    rec = np.concatenate([ra, rb])[order]
    rec["qidx"] = 2 * key[order].astype(np.uint64) + (rec["qidx"] & np.uint64(1))
    where = np.empty(order.size, dtype=np.int64)
    where[order] = np.arange(order.size)
    return rec, qoff, where[:ra.size], where[ra.size:]


@pytest.mark.parametrize("device", [False, True])
def test_the_interleaved_batch_gives_the_separate_result_renamed(device):
    per_a = [0, 3, 250, 10, 0, 300, 1, 0, 5]
    per_b = [2, 250, 3, 0, 9, 260, 0, 0, 5]
    n = len(per_a)
    ra, rb = make_side(per_a, 41), make_side(per_b, 42)
    qa, qb = make_qoff(n, 43), make_qoff(n, 44)
    rec, qoff, new_a, new_b = interleave(ra, qa, rb, qb, n)
    for kw in (dict(), dict(orientation="any", best=True, max_records=255), dict(min_tlen=300, max_tlen=500)):
        sep = fm.join_mates(ra, qa, rb, qb, **kw)
        mkw = dict(kw, orientation=KINDS[kw.get("orientation", "fr")])
        want = model.join(rec, qoff, interleaved=True, **mkw)
        one = fm.join_mates(dev(rec) if device else rec, dev(qoff) if device else qoff, interleaved=True, **kw)
        assert one.off.tolist() == want[1] == sep.off.tolist() and one.cls.tolist() == want[2] == sep.cls.tolist()
        assert one.pairs.tobytes() == model.as_array(want[0], MATE_PAIR_DTYPE).tobytes()
        renamed = sep.pairs.copy()
        renamed["a"], renamed["b"] = new_a[sep.pairs["a"]], new_b[sep.pairs["b"]]
        assert renamed.tobytes() == one.pairs.tobytes() and len(one) > 0


def raw(pa, ca, pb, cb, qa, qb, n, out, capacity, off=None, cls=None, interleaved=0, **kw):
    """the C call itself: (rc, *out_count)"""
    fields = dict(min_tlen=0, max_tlen=1000, max_records=0, strand_shift=1, orientation=0, best=0)
    fields.update(kw)
    spec = capi.MatesSpec(capi.ptr(qa), capi.ptr(qb), n, fields["min_tlen"], fields["max_tlen"], fields["max_records"], fields["strand_shift"], interleaved,
                          fields["orientation"], fields["best"], (C.c_uint8 * 4)(0, 0, 0, 0))
    total = C.c_uint64(12345)
    rc = capi.lib().fmgpu_positions_mates(capi.ptr(pa), ca, capi.ptr(pb), cb, C.byref(spec), capi.ptr(out), capacity, C.byref(total), capi.ptr(off), capi.ptr(cls), None)
    return rc, total.value


def fixture():
    per_a, per_b = [2, 0, 130, 4, 1, 200], [3, 1, 140, 0, 2, 190]
    n = len(per_a)
    ra, rb = make_side(per_a, 51), make_side(per_b, 52)
    return n, ra, rb, make_qoff(n, 53), make_qoff(n, 54)


def test_host_and_device_memory_for_every_array_and_an_unaligned_out_off():
    n, ra, rb, qa, qb = fixture()
    pairs, off, cls = model.join(ra, qa, rb, qb)
    want = model.as_array(pairs, MATE_PAIR_DTYPE)
    dra, drb, dqa, dqb = dev(ra), dev(rb), dev(qa), dev(qb)
    for k in range(1 << 7):                                              # bit j: argument j lies in device memory
        on = [bool(k >> j & 1) for j in range(7)]
        if k not in (0, 127) and bin(k).count("1") not in (1, 6):
            continue                                                     # all host, all device, each one alone, each one alone on the host
        out = np.zeros(len(want) + 1, dtype=MATE_PAIR_DTYPE)
        out = DeviceBuffer.from_array(out) if on[4] else out
        # a device out_off 8 bytes into its allocation: aligned to its element and to nothing more
        pad = DeviceBuffer.from_array(np.full(n + 3, 77, dtype=np.uint64)) if on[5] else None
        goff = pad.ptr + 8 if on[5] else np.zeros(n + 1, dtype=np.uint64)
        gcls = DeviceBuffer(n + 8) if on[6] else np.zeros(n, dtype=np.uint8)
        rc, total = raw(dra if on[0] else ra, len(ra), drb if on[1] else rb, len(rb), dqa if on[2] else qa, dqb if on[3] else qb, n, out, len(want) + 1, goff, gcls)
        assert (rc, total) == (0, len(want)), capi.lib().fmgpu_last_error()
        got = out.to_array(MATE_PAIR_DTYPE, len(want) + 1) if on[4] else out
        assert got[:len(want)].tobytes() == want.tobytes() and got[len(want):].tobytes() == bytes(32)
        if on[5]:
            whole = pad.to_array(np.uint64, n + 3)
            assert whole[1: n + 2].tolist() == off and whole[0] == 77 and whole[n + 2] == 77
        else:
            assert goff.tolist() == off
        assert (gcls.to_array(np.uint8, n) if on[6] else gcls).tolist() == cls


def test_the_counting_call_and_a_capacity_too_small():
    n, ra, rb, qa, qb = fixture()
    pairs, off, cls = model.join(ra, qa, rb, qb)
    assert len(pairs) > 100
    assert raw(ra, len(ra), rb, len(rb), qa, qb, n, None, 0) == (0, len(pairs))
    goff, gcls = np.full(n + 1, 99, dtype=np.uint64), np.full(n, 99, dtype=np.uint8)
    assert raw(dev(ra), len(ra), dev(rb), len(rb), dev(qa), dev(qb), n, None, 0, goff, gcls) == (0, len(pairs)) and goff.tolist() == off and gcls.tolist() == cls
    # one record short: the exact count, nothing written to out, out_off and out_class written
    for device in (False, True):
        fill = np.full(len(pairs) * 32, 0xAA, dtype=np.uint8)
        out = DeviceBuffer.from_array(fill) if device else fill.copy()
        goff, gcls = np.full(n + 1, 99, dtype=np.uint64), np.full(n, 99, dtype=np.uint8)
        rc, total = raw(ra, len(ra), rb, len(rb), qa, qb, n, out, len(pairs) - 1, goff, gcls)
        assert (rc, total) == (capi.FMGPU_ERR_CAPACITY, len(pairs)) and b"more than `capacity`" in capi.lib().fmgpu_last_error()
        assert ((out.to_array(np.uint8, fill.size) if device else out) == 0xAA).all()
        assert goff.tolist() == off and gcls.tolist() == cls
        rc, total = raw(ra, len(ra), rb, len(rb), qa, qb, n, out, len(pairs), goff, gcls)
        assert (rc, total) == (0, len(pairs))
        assert (out.to_array(np.uint8, fill.size) if device else out).tobytes() == model.as_array(pairs, MATE_PAIR_DTYPE).tobytes()


def test_what_the_device_refuses_names_the_array_and_the_lowest_offender():
    n, ra, rb, qa, qb = fixture()
    words = {"range": b"names a read beyond the batch", "order": b"names a read below its predecessor's", "qoff": b"has an offset above its successor's",
             "pos": b"has a pos of 2^62 or more"}

    def spoil(rec, at, **fields):
        rec = rec.copy()
        for k, v in fields.items():
            rec[k][at] = v
        return rec

    bad_q = qb.copy()
    bad_q[3], bad_q[5] = bad_q[2] - 1, bad_q[4] - 1
    cases = [
        (spoil(spoil(ra, 300, qidx=2 * n), 40, qidx=2 * n + 1), rb, qa, qb),                 # two records beyond the batch: the lower one is named
        (ra, spoil(spoil(rb, 7, qidx=0), 200, qidx=2), qa, qb),                              # read 0 behind read 2
        (ra, rb, qa, bad_q),
        (spoil(ra, 5, pos=1 << 62), spoil(rb, 1, pos=(1 << 64) - 1), qa, qb),                # both arrays: A is named
        (spoil(ra, 5, pos=1 << 62), spoil(rb, 7, qidx=0), bad_q, qb),                        # pos in A, order in B, qoff_a: the kinds in the header's order
        (ra, spoil(rb, len(rb) - 1, qidx=1 << 40), qa, qb),
        (ra, spoil(rb, 3, pos=1 << 62), qa, qb),                                             # array B alone: its own word
        (spoil(ra, 9, qidx=2 * n), spoil(rb, 2, qidx=2 * n), qa, qb),                        # beyond the batch in both arrays: A is named
    ]
    for a, b, q1, q2 in cases:
        with pytest.raises(model.MatesError) as e:
            model.join(a, q1, b, q2)
        for device in (False, True):
            goff, gcls = np.full(n + 1, 99, dtype=np.uint64), np.full(n, 99, dtype=np.uint8)
            out = np.full(4096, 0xAA, dtype=np.uint8).view(MATE_PAIR_DTYPE)
            rc, total = raw(dev(a) if device else a, len(a), dev(b) if device else b, len(b), dev(q1) if device else q1, q2, n, out, len(out), goff, gcls)
            message = capi.lib().fmgpu_last_error()
            assert rc == capi.FMGPU_ERR_INVALID and total == 0
            noun = b"read" if e.value.what == "qoff" else b"record"
            assert b"%s: %s %d %s" % (e.value.array.encode(), noun, e.value.index, words[e.value.what]) in message, (message, str(e.value))
            assert (out.view(np.uint8) == 0xAA).all() and (goff == 99).all() and (gcls == 99).all()
    # the interleaved batch is array A
    rec, qoff, _, _ = interleave(ra, qa, rb, qb, n)
    rec["qidx"][100] = 4 * n
    rc, total = raw(rec, len(rec), None, 0, qoff, None, n, None, 0, interleaved=1)
    assert rc == capi.FMGPU_ERR_INVALID and b"positions_a: record 100 names a read beyond the batch" in capi.lib().fmgpu_last_error()


def test_mates_cut_from_an_indexed_text_end_to_end():
    """3 sequences of 2 000 uniform symbols; 96 fragments of 120 .. 400 symbols; mate A = the first 50 symbols, mate B = the first 50 of the reverse complement; the mates
    of every second fragment swapped, one substitution in every second read.  Mapped with the both-strand pair ladder of Hamming schemes k = 0, 1 and joined FR with
    [100, 500]: every fragment is class 4, its true pair is among its pair records, and the whole output is the model's on the library's positions."""
    rng = np.random.default_rng(2024)
    texts = [rng.integers(1, 5, size=2000).astype(np.uint8) for _ in range(3)]
    comp = np.array(fm.DNA5_COMPLEMENT, dtype=np.uint8)
    mates, truth = ([], []), []
    for f in range(96):
        t, length = int(rng.integers(0, 3)), int(rng.integers(120, 401))
        at = int(rng.integers(0, 2000 - length + 1))
        frag = texts[t][at: at + length]
        first, second = frag[:50].copy(), comp[frag[::-1]][:50].copy()             # forward at `at`; the reverse strand of [at + length - 50, at + length)
        where = [(at, 0), (at + length - 50, 1)]
        reads = [first, second]
        if f % 2:
            reads, where = reads[::-1], where[::-1]
        for k in range(2):
            if (2 * f + k) % 4 in (1, 2):                                          # half of the reads, of either mate
                j = int(rng.integers(0, 50))
                reads[k][j] = (reads[k][j] - 1 + int(rng.integers(1, 4))) % 4 + 1
            mates[k].append(reads[k])
        truth.append((t, where, length))
    gx = fm.BiFMIndex.from_sequences(texts, 5, "IB16", 4)
    batches = [fm.flatten(m) for m in mates]
    pos = [fm.map_reads(gx, b, errors=1, edit=False, strands="dna5", pair=True) for b in batches]
    got = fm.join_mates(pos[0], batches[0][1], pos[1], batches[1][1], orientation="fr", min_tlen=100, max_tlen=500)
    want = model.join(pos[0], batches[0][1], pos[1], batches[1][1], min_tlen=100, max_tlen=500)
    assert got.off.tolist() == want[1] and got.cls.tolist() == want[2] and got.pairs.tobytes() == model.as_array(want[0], MATE_PAIR_DTYPE).tobytes()
    assert got.cls.tolist() == [4] * 96                                            # no fragment is left out
    for f, (t, where, length) in enumerate(truth):
        mine = got.pairs[int(got.off[f]): int(got.off[f + 1])]
        a, b = pos[0][mine["a"]], pos[1][mine["b"]]
        true = ((a["seq_id"] == t) & (b["seq_id"] == t) & (a["pos"] == where[0][0]) & (b["pos"] == where[1][0]) & ((a["qidx"] & 1) == where[0][1]) &
                ((b["qidx"] & 1) == where[1][1]) & (a["qidx"] >> 1 == f) & (b["qidx"] >> 1 == f) & (mine["tlen"] == length) & (mine["fragment"] == f))
        assert true.sum() == 1, (f, t, where, length, mine)
        assert bool(mine["flags"][true][0] & 1) == (where[0][0] <= where[1][0])
