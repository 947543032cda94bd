"""fmgpu_stats.table_bytes / table_accesses / table_steps of the exact-search family against the CPU model of tests/exact_traffic_model.py, which is written from the
rule beside fmgpu_stats in include/fmgpu.h: integers, compared exactly.  Every case first pins lb, len and lf_steps to the oracle (and to the model's own walk for the
reads that hold a byte >= sigma, which the reference does not define), so the trace the model prices is the one the kernel walked."""
import contextlib
import functools

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from tests import exact_traffic_model as tm
from tests import smem_brute
from tests.util import oracle_arrays

pytestmark = pytest.mark.gpu

RATE = 16


@functools.lru_cache(maxsize=None)
def sequences(sigma, many=False):
    if many:                                # more than 512 delimiter pairs: 300 sequences of 40 symbols
        rng = np.random.default_rng(77)
        return tuple(rng.integers(1, sigma, size=40, dtype=np.uint8) for _ in range(300))
    return tuple(tm.small_sequences(sigma))


@functools.lru_cache(maxsize=None)
def oracle(layout, sigma, many=False, rate=RATE):
    return fo.OraIndex.build(layout, sigma, list(sequences(sigma, many)), rate, False)


@functools.lru_cache(maxsize=None)
def model_index(sigma, many=False):
    return tm.Index.from_oracle(oracle("IB16", sigma, many))        # (the BWT does not depend on the layout)


@functools.lru_cache(maxsize=None)
def batch(sigma, many=False):
    seqs = sequences(sigma, many)
    if many:
        joined = [np.concatenate(seqs[:150]), np.concatenate(seqs[150:])]      # reads that run across sequences miss at the delimiter
        return tm.small_batch(joined, sigma, count=600, longest=60)
    return tm.small_batch(list(seqs), sigma)


@functools.lru_cache(maxsize=None)
def trace(sigma, many=False):
    qbuf, qoff = batch(sigma, many)
    tr = tm.Trace(model_index(sigma, many), qbuf, qoff)
    shared, split = tm.shared_split(tr)
    assert 10 * shared >= shared + split and 10 * split >= shared + split, ("the batch does not weigh both branches of the rule", sigma, shared, split)
    return tr


def handle(layout, sigma, many=False, **opts):
    with fm.options(**opts) if opts else contextlib.nullcontext():
        gx = fm.FMIndex.from_reference_arrays(**oracle_arrays(oracle(layout, sigma, many)))
    assert gx.row_bits == (64 if opts.get("force_wide") else 32)
    return gx


def counters(st):
    return int(st.table_bytes), int(st.table_accesses), int(st.table_steps)


def check(gx, ox, tr, queries, want, what, select=0):
    """the kernel's cursors and step count equal the oracle's (the model's, for reads with a foreign byte), then its three counters equal `want`"""
    qbuf, qoff = queries
    with fm.options(kernel_select=select):
        lb, ln, st = fm.search_no_errors.search(gx, (qbuf, qoff), want_stats=True)
    what = "%s, %d-bit rows, formats 0x%x, kernel_select 0x%x" % (what, gx.row_bits, gx.formats, select)
    valid = tm.valid_reads(qbuf, qoff, ox.sigma)
    olb, oln, ost = ox.search_exact(*tm.take_reads(qbuf, qoff, valid), want_steps=True)
    assert np.array_equal(lb[valid], olb) and np.array_equal(ln[valid], oln), what
    assert np.array_equal(lb.astype(np.int64), tr.lb) and np.array_equal(ln.astype(np.int64), tr.ln), what
    assert np.array_equal(tr.steps[valid], ost.astype(np.int64)) and st.lf_steps == int(tr.steps.sum()), what
    got = counters(st)
    print(what, "(bytes, accesses, steps): kernel", got, "model", tuple(want))
    assert got == tuple(want), "%s: (table_bytes, table_accesses, table_steps) = %s, the model gives %s" % (what, got, tuple(want))
    return st


# ---------------------------------------------------------------------------------------------------------------- one-symbol blocks
@pytest.mark.parametrize("fused", [1, 0])
def test_one_symbol_blocks_dna(fused):
    gx = handle("IB16", 5, fused_locate=fused)
    assert bool(gx.formats & capi.FMT_FUSED) == bool(fused) and gx.formats & capi.FMT_PAIRS
    tr = trace(5)
    assert (tr.ex & (tr.sym == 0)).sum() > 0
    check(gx, oracle("IB16", 5), tr, batch(5), tm.cost_blocks(tr, fused=bool(fused)), "k_exact_a<5> IB16 sigma 5 fused %d" % fused, capi.SEL_EXACT_ONE_SYMBOL)


@pytest.mark.parametrize("sigma", [4, 6, 28, 256])
def test_one_symbol_blocks_any_sigma(sigma):
    gx = handle("IB16", sigma)
    tr = trace(sigma)
    nbytes, acc, steps = tm.cost_blocks(tr, fused=bool(gx.formats & capi.FMT_FUSED))
    assert nbytes == 12 * acc and int(tr.steps.sum()) >= acc // 2
    check(gx, oracle("IB16", sigma), tr, batch(sigma), (nbytes, acc, steps), "k_exact_a<0> IB16 sigma %d" % sigma)


# ---------------------------------------------------------------------------------------------------------------- pair table
@pytest.mark.parametrize("lut_len", [None, 3, 12])
def test_pair_table(lut_len):
    gx = handle("IB16", 5)
    fused = bool(gx.formats & capi.FMT_FUSED)
    if lut_len:
        gx.accelerate(1, lut_len=lut_len)
        assert gx.formats & capi.FMT_INTERVALS
    assert gx.formats & capi.FMT_PAIRS
    tr = trace(5)
    check(gx, oracle("IB16", 5), tr, batch(5), tm.cost_pairs(tr, lut_len, fused=fused), "k_exact_p IB16 sigma 5 interval table %s" % lut_len, capi.SEL_NO_SAMPLE_CHAIN)
    if lut_len:       # the same handle taken off the pair-table kernel: the table-driven kernel serves it, from the entry and then in single steps
        check(gx, oracle("IB16", 5), tr, batch(5), tm.cost_kstep(tr, 1, lut_len, 0, fused=fused), "k_exact_kstep IB16 sigma 5 NO_EXACT_LUT on interval table %d" % lut_len,
              capi.SEL_NO_SAMPLE_CHAIN | capi.SEL_NO_EXACT_LUT)


def test_pair_table_not_built_for_many_sequences():
    gx = handle("IB16", 5, many=True)
    assert not gx.formats & capi.FMT_PAIRS
    tr = trace(5, True)
    check(gx, oracle("IB16", 5, True), tr, batch(5, True), tm.cost_blocks(tr, fused=bool(gx.formats & capi.FMT_FUSED)), "k_exact_a<5> IB16 sigma 5, 300 sequences")


# ---------------------------------------------------------------------------------------------------------------- symbol planes, tree, reference blocks
@pytest.mark.parametrize("layout", ["WAVELET", "EPR16"])
@pytest.mark.parametrize("sigma", [6, 21, 28])
def test_symbol_planes(layout, sigma):
    gx = handle(layout, sigma)
    assert gx.formats & capi.FMT_PLANES and not gx.formats & capi.FMT_BLOCKS
    tr = trace(sigma)
    check(gx, oracle(layout, sigma), tr, batch(sigma), tm.cost_planes(tr), "k_exact_s %s sigma %d" % (layout, sigma))
    gx.accelerate(0, lut_len=3)                  # (kstep 0: no expansion into one-symbol blocks, the interval table sits in front of the planes)
    assert gx.formats & capi.FMT_INTERVALS and not gx.formats & capi.FMT_BLOCKS
    want, name = tm.cost_planes(tr, 3), "k_exact_s"
    check(gx, oracle(layout, sigma), tr, batch(sigma), want, "%s %s sigma %d interval table 3" % (name, layout, sigma))


@pytest.mark.parametrize("sigma,opts,select", [(28, {}, capi.SEL_EXACT_ON_TREE), (256, {}, capi.SEL_EXACT_ON_TREE), (5, {"expand_dna": 0}, 0)])
def test_tree(sigma, opts, select):
    gx = handle("WAVELET", sigma, **opts)
    assert gx.formats & capi.FMT_TREE and not gx.formats & capi.FMT_BLOCKS
    tr = trace(sigma)
    check(gx, oracle("WAVELET", sigma), tr, batch(sigma), tm.cost_tree(tr), "k_exact_m WAVELET sigma %d digits %s" % (sigma, tm.tree_digits(sigma)), select)


@pytest.mark.parametrize("layout,sigma,opts", [("EPR16", 5, {"expand_dna": 0}), ("EPRV2_16", 40, {})])
def test_reference_blocks_count_nothing(layout, sigma, opts):
    gx = handle(layout, sigma, **opts)
    assert gx.formats & capi.FMT_REFERENCE and not gx.formats & (capi.FMT_BLOCKS | capi.FMT_PLANES)
    tr = trace(sigma)
    check(gx, oracle(layout, sigma), tr, batch(sigma), (0, 0, 0), "k_exact %s sigma %d in place" % (layout, sigma))


# ---------------------------------------------------------------------------------------------------------------- k-step, interval and walk tables
@pytest.mark.parametrize("sigma", [5, 6, 256])
def test_kstep_tables(sigma):
    gx = handle("IB16", sigma)
    fused = bool(gx.formats & capi.FMT_FUSED)
    tr = trace(sigma)
    ksteps = (2, 3) if sigma <= 6 else ()           # ((sigma - 1)^kstep <= 255 contexts)
    combos = [(k, 0, 0) for k in ksteps] + [(1, 4 if sigma <= 6 else 1, 0), (1, 0, 1), (1, 0, 2), (ksteps[-1] if ksteps else 1, 5 if sigma <= 6 else 1, 2)]
    assert tm.walk_len(sigma) == {5: 16, 6: 10, 256: 4}[sigma]
    for kstep, lut_len, walk in combos:
        gx.accelerate(kstep, lut_len=lut_len, walk=walk)
        if sigma == 5 and kstep == 1 and lut_len and not walk:
            want, name = tm.cost_pairs(tr, lut_len, fused=fused), "k_exact_p"         # (the interval table alone sits in front of the pair table)
        else:
            want, name = tm.cost_kstep(tr, kstep, lut_len, walk, fused=fused), "k_exact_kstep"
        check(gx, oracle("IB16", sigma), tr, batch(sigma), want, "%s IB16 sigma %d J %d k-step %d interval table %d walk %d" % (name, sigma, tm.walk_len(sigma), kstep, lut_len, walk),
              capi.SEL_NO_SAMPLE_CHAIN)


# ---------------------------------------------------------------------------------------------------------------- 64-bit rows
def test_wide_rows():
    ox, tr, q = oracle("IB16", 5), trace(5), batch(5)
    gx = handle("IB16", 5, force_wide=1)
    fused = bool(gx.formats & capi.FMT_FUSED)
    assert gx.formats & capi.FMT_PAIRS and not gx.formats & capi.FMT_CHAIN
    check(gx, ox, tr, q, tm.cost_blocks(tr, fused), "k_exact_a<5> IB16 sigma 5", capi.SEL_EXACT_ONE_SYMBOL)
    check(gx, ox, tr, q, tm.cost_pairs(tr, None, True, fused), "k_exact_p IB16 sigma 5 no interval table")
    gx.accelerate(1, lut_len=5)
    check(gx, ox, tr, q, tm.cost_pairs(tr, 5, True, fused), "k_exact_p IB16 sigma 5 interval table 5 (16-byte entries)")
    for lut_len, walk in ((0, 1), (4, 2)):
        gx.accelerate(1, lut_len=lut_len, walk=walk)
        check(gx, ox, tr, q, tm.cost_kstep(tr, 1, lut_len, walk, True, fused), "k_exact_kstep IB16 sigma 5 interval table %d walk %d (16-byte entries)" % (lut_len, walk))
    px = handle("WAVELET", 28, force_wide=1)
    check(px, oracle("WAVELET", 28), trace(28), batch(28), tm.cost_tree(trace(28)), "k_exact_m WAVELET sigma 28", capi.SEL_EXACT_ON_TREE)


# ---------------------------------------------------------------------------------------------------------------- additivity, waves without steps
def test_counters_add_up_over_split_batches():
    gx, ox, tr = handle("IB16", 5), oracle("IB16", 5), trace(5)
    fused = bool(gx.formats & capi.FMT_FUSED)
    qbuf, qoff = batch(5)
    cut = 611                                            # (not a multiple of 64: the counters are per read, not per wave)
    for select, cost, name in ((capi.SEL_NO_SAMPLE_CHAIN, lambda t: tm.cost_pairs(t, None, False, fused), "k_exact_p"),
                               (capi.SEL_EXACT_ONE_SYMBOL, lambda t: tm.cost_blocks(t, fused), "k_exact_a<5>")):
        parts = []
        for keep in (range(0, cut), range(cut, tr.nq)):
            sub = tm.take_reads(qbuf, qoff, keep)
            st = check(gx, ox, tm.Trace(tr.ix, *sub), sub, cost(tm.Trace(tr.ix, *sub)), "%s IB16 sigma 5 reads %d..%d" % (name, keep[0], keep[-1]), select)
            parts.append(counters(st))
        assert tm.total(parts) == tuple(cost(tr)), name


def test_waves_without_steps():
    gx, ox = handle("IB16", 5), oracle("IB16", 5)
    fused = bool(gx.formats & capi.FMT_FUSED)
    qbuf, qoff = batch(5)
    lens = np.diff(qoff.astype(np.int64))
    one = int(np.nonzero(lens == 65)[0][0])
    sub = (qbuf[int(qoff[one]): int(qoff[one + 1])].copy(), np.concatenate([np.zeros(65, dtype=np.uint64), [np.uint64(65)]]))
    tr = tm.Trace(model_index(5), *sub)
    assert tr.nq == 65 and int(tr.steps[:64].sum()) == 0
    check(gx, ox, tr, sub, tm.cost_pairs(tr, None, False, fused), "k_exact_p IB16 sigma 5, 64 empty reads + 1", capi.SEL_NO_SAMPLE_CHAIN)
    check(gx, ox, tr, sub, tm.cost_blocks(tr, fused), "k_exact_a<5> IB16 sigma 5, 64 empty reads + 1", capi.SEL_EXACT_ONE_SYMBOL)
    gx.accelerate(2, lut_len=3, walk=1)
    check(gx, ox, tr, sub, tm.cost_kstep(tr, 2, 3, 1, False, fused), "k_exact_kstep IB16 sigma 5 k-step 2 interval table 3 walk 1, 64 empty reads + 1")


# ---------------------------------------------------------------------------------------------------------------- sample chain
@functools.lru_cache(maxsize=None)
def chain_sequences():
    rng = np.random.default_rng(17)
    base = rng.integers(1, 5, size=26_000, dtype=np.uint8)
    block = rng.integers(1, 5, size=2_000, dtype=np.uint8)
    text = np.concatenate([base[:9_000], block, base[9_000:], block])           # 30 000 symbols, the block twice
    cuts = [0, 20_003, 20_040, 24_136, len(text)]                             # (4096 is a multiple of every rate: that sequence's delimiter is a sampled position)
    return tuple(text[a:b].copy() for a, b in zip(cuts, cuts[1:]))


@functools.lru_cache(maxsize=None)
def chain_reads():
    """reads of 30 .. 300 symbols in the manner of tests/test_gpu_sample_chain.py's generator: copies, one substitution before the one-row point, inside the seek, inside
    every jump window and in the tail, delimiters and foreign bytes inside the jumped region, reads at sequence starts, ends and across boundaries, reads from the repeat"""
    seqs = chain_sequences()
    rng = np.random.default_rng(29)
    joined = np.concatenate([np.concatenate([s, [0]]) for s in seqs]).astype(np.uint8)
    out = []

    def copy_of(m, s=None):
        s = seqs[(0, 3)[int(rng.integers(0, 2))]] if s is None else s
        p = int(rng.integers(0, len(s) - m + 1))
        return s[p: p + m].copy()

    def put(r, j, c):                   # the symbol consumed as the j-th
        r = r.copy()
        r[len(r) - 1 - j] = r[len(r) - 1 - j] % 4 + 1 if c is None else c
        return r

    lengths = [30, 47, 48, 49, 63, 64, 65, 79, 80, 81, 101, 126, 127, 128, 129, 145, 160, 300]
    for m in lengths:
        out += [copy_of(m) for _ in range(4)]
        q = copy_of(m)
        for j in sorted(set([0, 3, 7, 10, 12, 14, 17, 19, 22, 25, 28] + list(range(31, m, 7)) + [m - 1, m - 2, m - 3])):
            if j < m:
                out.append(put(q, j, None))
        for j in (12, 24, 33, 47, 62, 90):
            if j < m:
                out += [put(q, j, 0), put(q, j, 200)]
    for s in (seqs[0], seqs[2], seqs[3]):
        for p in (0, 1, 3, 4, 5, 15, 16, 17, 31, 32):
            out += [s[p: p + m].copy() for m in (64, 101, 160)]
        out += [s[len(s) - m:].copy() for m in (64, 101)]
    ends = np.cumsum([len(s) + 1 for s in seqs])
    for e in ends[:3]:
        out += [joined[e - back: e - back + 101].copy() for back in (1, 5, 16, 40, 70, 100)]
    out.append(seqs[1].copy())
    for m in (64, 101, 160, 300):
        out += [seqs[0][9_000 + p: 9_000 + p + m].copy() for p in rng.integers(0, 2_000 - m, size=6)]
        out += [seqs[0][11_000 - m + over: 11_000 + over].copy() for over in (3, 20, 50)]
    for i in range(800):
        r = copy_of(lengths[i % len(lengths)])
        out.append(put(r, int(rng.integers(0, len(r))), None) if i % 3 == 0 else r)
    out.append(np.zeros(0, dtype=np.uint8))
    return fm.flatten([out[i] for i in rng.permutation(len(out))])


@functools.lru_cache(maxsize=None)
def chain_oracle(rate):
    return fo.OraIndex.build("IB16", 5, list(chain_sequences()), rate, False)


@functools.lru_cache(maxsize=None)
def chain_text():
    """(model index, joined text, sa, sequence starts)"""
    ox = chain_oracle(16)
    seqs = chain_sequences()
    starts = np.concatenate([[0], np.cumsum([len(s) + 1 for s in seqs])])[:-1]
    sa = np.zeros(ox.n, dtype=np.int64)
    for row in range(ox.n):
        seq, pos, steps = ox.locate(row)                    # (the sampled position in front of the row's, and the LF steps to it)
        sa[row] = starts[seq] + pos + steps
    joined = np.concatenate([np.concatenate([s, [0]]) for s in seqs]).astype(np.uint8)
    ix = tm.Index.from_oracle(ox)
    assert np.array_equal(ix.bwt, joined[sa - 1].astype(np.int64)) and sorted(sa) == list(range(ox.n))
    return ix, joined, sa, starts


@pytest.mark.parametrize("rate", [4, 16])
def test_sample_chain(rate):
    ix, joined, sa, starts = chain_text()
    ox = chain_oracle(rate)
    gx = fm.FMIndex.from_reference_arrays(**oracle_arrays(ox))
    assert gx.formats & capi.FMT_CHAIN and gx.formats & capi.FMT_PAIRS and gx.formats & capi.FMT_FUSED
    qbuf, qoff = chain_reads()
    tr = tm.Trace(ix, qbuf, qoff)
    parts = tm.cost_chain(tr, joined, sa, starts, rate, fused=True)
    want = tm.total(parts[k] for k in ("park", "seek", "jump", "resume"))
    print("rate", rate, parts)
    assert want[2] == rate * parts["jumped_entries"] and parts["jumped_entries"] > 500 and parts["seek"][1] > 500
    st = check(gx, ox, tr, (qbuf, qoff), want, "k_exact_p / k_exact_chain IB16 sigma 5 sampling rate %d, byte form" % rate)
    pq = fm.pack_queries((qbuf, qoff), 5)
    lb4, ln4, st4 = fm.search_no_errors.search(gx, pq, want_stats=True)
    assert np.array_equal(lb4.astype(np.int64), tr.lb) and np.array_equal(ln4.astype(np.int64), tr.ln) and st4.lf_steps == st.lf_steps
    assert counters(st4) == want, "k_exact_p / k_exact_chain IB16 sigma 5 sampling rate %d, _q4 form: %s, the model gives %s" % (rate, counters(st4), want)


# ---------------------------------------------------------------------------------------------------------------- SMEM walk
@functools.lru_cache(maxsize=None)
def smem_reads(sigma):
    qbuf, qoff = batch(sigma)
    qoff = qoff.astype(np.int64)
    return [qbuf[qoff[i]: qoff[i + 1]] for i in range(0, len(qoff) - 1, 8)]


@pytest.mark.parametrize("layout,sigma", [("IB16", 5), ("IB16", 28), ("WAVELET", 28), ("EPR16", 6)])
def test_smem_walk(layout, sigma):
    gx = handle(layout, sigma)
    reads = smem_reads(sigma)
    walks = [w for r in reads for w in smem_brute.walk_reads(r, sigma)]
    tr = tm.Trace(model_index(sigma), *fm.flatten(walks))
    on_blocks = bool(gx.formats & capi.FMT_BLOCKS)
    want = tm.cost_blocks(tr) if on_blocks else (0, 0, 0)
    if on_blocks:
        shared, split = tm.shared_split(tr)
        assert 10 * shared >= shared + split and 10 * split >= shared + split
    hits, spans, lengths, st = fm.search_smems(gx, fm.flatten(reads), want_lengths=True, want_stats=True)
    what = "k_smem_walk %s sigma %d, %d-bit rows" % (layout, sigma, gx.row_bits)
    matched = np.where(tr.ln != 0, tr.steps, tr.steps - 1)          # (the extension that came out empty is a step and no match)
    assert np.array_equal(lengths.astype(np.int64), np.maximum(matched, 0)) and st.lf_steps == int(tr.steps.sum()), what
    print(what, "kernel", counters(st), "model", want)
    assert counters(st) == want, "%s: (table_bytes, table_accesses, table_steps) = %s, the model gives %s" % (what, counters(st), want)
