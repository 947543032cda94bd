"""Exact search along the sample chain (k_exact_p parks a one-row read, k_exact_chain seeks the next sampled row and jumps `rate` symbols per entry, k_exact_p
resumes): intervals, miss rows and the step count equal the oracle's one-symbol search and the same call with FMGPU_SEL_NO_SAMPLE_CHAIN — sampling rates 1, 4
and 16, handles made from reference arrays and by the device construction, reads that straddle the park threshold and the 127-symbol window, substitutions in
every stage, sequence starts and boundaries, delimiters and foreign bytes inside a jumped window, reads from a repeat that never reach one row."""
import contextlib
import functools

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests.util import make_text, oracle_arrays

pytestmark = pytest.mark.gpu

SEQ_LENS = (100_003, 37, 4096)            # + the rest; 4096 is a multiple of every rate: the sequence's delimiter is a sampled position
STAT_FIELDS = ("lf_steps", "hits", "table_bytes", "table_accesses", "table_steps")


@functools.lru_cache(maxsize=None)
def sequences():
    rng = np.random.default_rng(17)
    base = make_text(200_000, 5, seed=23)
    block = rng.integers(1, 5, size=20_000, dtype=np.uint8)
    text = np.concatenate([base[:60_000], block, base[60_000:130_000], block, base[130_000:], block])      # 260 000 symbols, the block three times
    cuts = np.cumsum((0,) + SEQ_LENS)
    return tuple(text[a:b].copy() for a, b in zip(cuts, list(cuts[1:]) + [len(text)]))


@functools.lru_cache(maxsize=None)
def reads():
    seqs = sequences()
    rng = np.random.default_rng(29)
    joined = np.concatenate([np.concatenate([s, [0]]) for s in seqs]).astype(np.uint8)      # the text with its delimiters
    big = (0, 3)
    out = []

    def copy_of(m, s=None):
        s = seqs[big[int(rng.integers(0, 2))]] if s is None else s
        p = int(rng.integers(0, len(s) - m + 1))
        return s[p: p + m].copy()

    def subst(r, j):                    # the symbol consumed as the j-th (backward search starts at the read's end)
        r = r.copy()
        r[len(r) - 1 - j] = r[len(r) - 1 - j] % 4 + 1
        return r

    lengths = [30, 47, 48, 49, 63, 64, 65, 79, 80, 81, 101, 126, 127, 128, 129, 145, 160, 300]
    for m in lengths:
        for _ in range(6):
            out.append(copy_of(m))
        q = copy_of(m)
        # one substitution before the one-row point (~9 symbols), inside the seek, inside every jump window, in the tail
        for j in sorted(set([0, 3, 7, 10, 12, 14, 17, 19, 22, 25, 28] + list(range(31, m, 5)) + [m - 1, m - 2, m - 3])):
            if j < m:
                out.append(subst(q, j))
        # a delimiter inside the jumped region
        for j in (24, 33, 47, 62, 90):
            if j < m:
                r = q.copy(); r[m - 1 - j] = 0; out.append(r)
    # reads that start within a window of a sequence's start, and reads that end at its end
    for s in (seqs[0], seqs[2], seqs[3]):
        for p in (0, 1, 3, 4, 5, 15, 16, 17, 31, 32):
            for m in (64, 101, 160):
                out.append(s[p: p + m].copy())
        for m in (64, 101):
            out.append(s[len(s) - m:].copy())
    # reads that run across a sequence boundary (they hold the delimiter)
    ends = np.cumsum([len(s) + 1 for s in seqs])
    for e in ends[:3]:
        for back in (1, 5, 16, 40, 70, 100):
            out.append(joined[e - back: e - back + 101].copy())
    out.append(seqs[1].copy())          # the 37-symbol sequence itself
    # reads from the repeated block: three rows to the end, or one row only after the block's edge
    block_at = 60_000
    for m in (64, 101, 160, 300):
        for _ in range(8):
            p = block_at + int(rng.integers(0, 20_000 - m))
            out.append(seqs[0][p: p + m].copy())
        for over in (3, 20, 50):
            out.append(seqs[0][block_at + 20_000 - m + over: block_at + 20_000 + over].copy())
    # bulk: a few thousand copies with 0 or 1 substitution, shuffled with the rest (ragged waves)
    for i in range(2500):
        m = lengths[i % len(lengths)]
        r = copy_of(m)
        out.append(subst(r, int(rng.integers(0, m))) if i % 3 == 0 else r)
    order = rng.permutation(len(out))
    return fm.flatten([out[i] for i in order])


@functools.lru_cache(maxsize=None)
def foreign_reads():
    """bytes outside the alphabet inside the seek and the jumped region (an empty interval here, undefined in the reference: compared with the pair-table and one-symbol kernels)"""
    seqs = sequences()
    rng = np.random.default_rng(31)
    out = []
    for m in (64, 80, 101, 128, 160, 300):
        for _ in range(4):
            p = int(rng.integers(0, len(seqs[0]) - m + 1))
            q = seqs[0][p: p + m].copy()
            for j in (12, 20, 24, 33, 47, 62, 90, m - 1):
                if j < m:
                    for byte in (5, 200, 255):
                        r = q.copy(); r[m - 1 - j] = byte; out.append(r)
            out.append(q)
    return fm.flatten([out[i] for i in rng.permutation(len(out))])


@functools.lru_cache(maxsize=None)
def oracle(rate):
    return fo.OraIndex.build("IB16", 5, list(sequences()), rate, False)


@functools.lru_cache(maxsize=None)
def expected():
    qbuf, qoff = reads()
    return oracle(16).search_exact(qbuf, qoff, want_steps=True)


def make(rate, how, **opts):
    with fm.options(**opts) if opts else contextlib.nullcontext():
        if how == "arrays":
            return fm.FMIndex.from_reference_arrays(**oracle_arrays(oracle(rate)))
        return fm.FMIndex.from_sequences(list(sequences()), 5, "IB16", rate)


def stats_of(st):
    return tuple(int(getattr(st, f)) for f in STAT_FIELDS)


def samples(rate):
    return sum(len(s) // rate + 1 for s in sequences())


@pytest.mark.parametrize("how", ["arrays", "built"])
@pytest.mark.parametrize("rate", [1, 4, 16])
def test_chain_search_equals_oracle(rate, how):
    gx = make(rate, how)
    assert gx.formats & capi.FMT_CHAIN and gx.formats & capi.FMT_PAIRS
    qbuf, qoff = reads()
    olb, oln, ost = expected()
    assert (oln > 1).sum() > 20 and (oln == 0).sum() > 200 and (olb[oln == 0] > 0).any()      # (repeat reads, misses, misses that end on a row)
    lb, ln, st = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
    print("rate", rate, how, "lf_steps", st.lf_steps, "oracle", int(ost.sum()), "table_steps", st.table_steps, "wrong lb", int((lb != olb).sum()), "wrong len", int((ln != oln).sum()))
    assert np.array_equal(ln, oln) and np.array_equal(lb, olb)
    assert st.lf_steps == int(ost.sum())
    assert st.table_steps > 0 and st.table_steps % rate == 0
    # the same call on the pair table alone
    with fm.options(kernel_select=capi.SEL_NO_SAMPLE_CHAIN):
        lb0, ln0, st0 = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
    assert np.array_equal(lb0, lb) and np.array_equal(ln0, ln) and st0.lf_steps == st.lf_steps and st0.table_steps == 0
    # the 4-bit form: every field of the stats
    pq = fm.pack_queries((qbuf, qoff), 5)
    lb4, ln4, st4 = fm.search_no_errors.search(gx, pq, want_stats=True)
    ub = fm.unpack_queries(pq)          # (a byte >= 5 comes back as 255: the byte batch the packed one stands for)
    lbu, lnu, stu = fm.search_no_errors.search(gx, ub, want_stats=True)
    assert np.array_equal(lb4, lb) and np.array_equal(ln4, ln) and np.array_equal(lbu, lb) and np.array_equal(lnu, ln)
    assert stats_of(st4) == stats_of(stu) == stats_of(st)
    # bytes outside the alphabet: the rows and steps of the pair-table kernel and of the one-symbol kernel
    fq = foreign_reads()
    a = fm.search_no_errors.search(gx, fq, want_stats=True)
    with fm.options(kernel_select=capi.SEL_NO_SAMPLE_CHAIN):
        b = fm.search_no_errors.search(gx, fq, want_stats=True)
    with fm.options(kernel_select=capi.SEL_EXACT_ONE_SYMBOL):
        c = fm.search_no_errors.search(gx, fq, want_stats=True)
    a4 = fm.search_no_errors.search(gx, fm.pack_queries(fq, 5), want_stats=True)
    for other in (b, c, a4):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2].lf_steps == other[2].lf_steps
    assert a[2].table_steps > 0 and b[2].table_steps == 0 and stats_of(a4[2]) == stats_of(a[2]) and (a[1] > 0).sum() == 24
    # one result word per read
    word, stp = fm.search_no_errors.search_packed(gx, (qbuf, qoff), want_stats=True)
    assert np.array_equal(word, (lb << np.uint64(32)) | ln) and stats_of(stp) == stats_of(st)
    # a batch of one read: a wave of one lane
    for i in range(0, len(qoff) - 1, 211):
        one = (qbuf[qoff[i]: qoff[i + 1]], np.array([0, qoff[i + 1] - qoff[i]], dtype=np.uint64))
        a, b, s1 = fm.search_no_errors.search(gx, one, want_stats=True)
        assert (a[0], b[0], s1.lf_steps) == (olb[i], oln[i], int(ost[i])), i


def test_short_batches_stay_on_the_pair_table():
    """a batch whose longest read is below the park threshold + one window (32 + 16 symbols) takes the pair-table kernel alone"""
    gx = make(16, "arrays")
    qbuf, qoff = reads()
    olb, oln, ost = expected()
    keep = [i for i in range(len(qoff) - 1) if qoff[i + 1] - qoff[i] < 48]
    batch = fm.flatten([qbuf[qoff[i]: qoff[i + 1]] for i in keep])
    lb, ln, st = fm.search_no_errors.search(gx, batch, want_stats=True)
    assert np.array_equal(lb, olb[keep]) and np.array_equal(ln, oln[keep]) and st.lf_steps == int(ost[keep].sum()) and st.table_steps == 0


@pytest.mark.parametrize("case", ["wide", "rate32", "option"])
def test_no_chain_where_it_does_not_apply(case):
    """64-bit rows, a sampling rate above 16 and option 0 leave the format bit clear; the results are the same"""
    rate = 32 if case == "rate32" else 16
    opts = {"force_wide": 1} if case == "wide" else ({"sample_chain": 0} if case == "option" else {})
    gx = make(rate, "arrays", **opts)
    assert not gx.formats & capi.FMT_CHAIN and gx.formats & capi.FMT_PAIRS
    qbuf, qoff = reads()
    olb, oln, ost = expected()
    lb, ln, st = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
    assert np.array_equal(lb, olb) and np.array_equal(ln, oln) and st.lf_steps == int(ost.sum()) and st.table_steps == 0
    if case == "option":
        full = make(rate, "arrays")
        grown = full.device_bytes - gx.device_bytes
        print("chain bytes", grown, "12 x samples", 12 * samples(rate))
        assert full.formats & capi.FMT_CHAIN and 0 <= grown - 12 * samples(rate) <= 8192      # (+ the list of 512 entries and the allocations' alignment)


def test_file_round_trip_and_clone_keep_the_chain(tmp_path):
    gx = make(16, "built")
    qbuf, qoff = reads()
    olb, oln, ost = expected()
    path = str(tmp_path / "chain.fmgpu")
    gx.save(path, tables=True)
    for other in (fm.FMIndex.load(path), gx.clone()):
        assert other.formats == gx.formats and other.formats & capi.FMT_CHAIN and abs(other.device_bytes - gx.device_bytes) < 4096
        lb, ln, st = fm.search_no_errors.search(other, (qbuf, qoff), want_stats=True)
        assert np.array_equal(lb, olb) and np.array_equal(ln, oln) and st.lf_steps == int(ost.sum()) and st.table_steps > 0
        other.close()
