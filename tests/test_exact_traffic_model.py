"""tests/exact_traffic_model.py against itself and the oracle, on texts of a few hundred rows: every vectorised cost function equals a literal per-read, per-step loop
written from the rule beside fmgpu_stats (include/fmgpu.h), the identities of Format A hold, a read of foreign bytes costs steps and no access, and the model's walk ends
where the oracle's search_exact ends.  No GPU."""
import functools

import numpy as np
import pytest

import fmoracle as fo
from tests import exact_traffic_model as tm
from tests import smem_brute


@functools.lru_cache(maxsize=None)
def sequences(sigma):
    base = np.random.default_rng(sigma + 100).integers(1, sigma, size=420, dtype=np.uint8)
    return [np.concatenate([base[:300], base[40:140]]), base[300:].copy(), np.array([1, 1, 2], dtype=np.uint8)]


@functools.lru_cache(maxsize=None)
def setup(sigma):
    rng = np.random.default_rng(sigma)
    seqs = sequences(sigma)
    ox = fo.OraIndex.build("IB16", sigma, seqs, 4, False)
    reads = []
    for i in range(260):
        s = seqs[i % 2]
        m = int(rng.integers(1, 40))
        p = int(rng.integers(0, len(s) - m + 1))
        r = s[p: p + m].copy()
        if i % 3 == 0:
            r[int(rng.integers(0, m))] = rng.integers(1, sigma)
        if i % 23 == 1:
            r[int(rng.integers(0, m))] = 0
        if i % 19 == 2 and sigma < 256:
            r[int(rng.integers(0, m))] = 255
        reads.append(r)
    reads += [np.zeros(0, dtype=np.uint8), np.array([1], dtype=np.uint8), np.array([0], dtype=np.uint8), np.array([0, 1, 1], dtype=np.uint8), np.array([1, 1, 0], dtype=np.uint8)]
    qbuf = np.concatenate(reads).astype(np.uint8)
    qoff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    ix = tm.Index.from_oracle(ox)
    return ox, ix, reads, qbuf, qoff, tm.Trace(ix, qbuf, qoff)


class Literal:
    """the rule, read by read and step by step, on the BWT as a plain list"""

    def __init__(self, bwt, sigma):
        self.bwt, self.sigma, self.n = [int(c) for c in bwt], sigma, len(bwt)
        self.C = [sum(1 for s in self.bwt if s < c) for c in range(sigma + 1)]

    def rank(self, i, c):
        return sum(1 for s in self.bwt[:i] if s == c)

    def walk(self, read):
        """([(a, b, c) per executed step], (lb, len))"""
        lb, ln, out = 0, self.n, []
        for c in [int(x) for x in read[::-1]]:
            out.append((lb, lb + ln, c))
            if c >= self.sigma:
                lb, ln = 0, 0
                break
            ra, rb = self.C[c] + self.rank(lb, c), self.C[c] + self.rank(lb + ln, c)
            lb, ln = ra, rb - ra
            if ln == 0:
                break
        return out, (lb, ln)

    def single(self, step, fused):
        a, b, c = step
        if c >= self.sigma:
            return 0
        if c == 0 and fused:
            return 2
        return 1 if a >> 6 == b >> 6 else 2

    def reaches(self, steps, end, j):
        return j < len(steps) or (j == len(steps) and end[1] != 0)

    def entry(self, read, steps, end, lut_len):
        """(reads its entry, starts from it)"""
        tail = [int(c) for c in read[::-1][:lut_len]]
        reads = bool(lut_len) and self.n > 1 and len(read) >= lut_len and all(1 <= c < self.sigma for c in tail)
        return reads, reads and self.reaches(steps, end, lut_len)

    def blocks(self, read, fused=False):
        steps, _ = self.walk(read)
        acc = sum(self.single(s, fused) for s in steps)
        return 12 * acc, acc, 0

    def planes(self, read, lut_len=0):
        steps, end = self.walk(read)
        reads, used = self.entry(read, steps, end, lut_len)
        acc = sum((1 if a >> 6 == b >> 6 else 2) for a, b, c in steps[lut_len if used else 0:] if c < self.sigma)
        return 44 * acc + 8 * reads, acc + reads, lut_len * used

    def tree(self, read):
        steps, _ = self.walk(read)
        digits = tm.tree_digits(self.sigma)
        nbytes = acc = 0
        for a, b, c in steps:
            if c >= self.sigma:
                continue
            low = sum(digits)
            for d in digits:
                pa = sum(1 for s in self.bwt[:a] if s >> low == c >> low)
                pb = sum(1 for s in self.bwt[:b] if s >> low == c >> low)
                k = 1 if pa >> 6 == pb >> 6 else 2
                acc += k
                nbytes += (4 + 8 * d) * k
                low -= d
        return nbytes, acc, 0

    def pairs(self, read, lut_len=None, fused=False):
        steps, end = self.walk(read)
        sym = [int(c) for c in read[::-1]]
        m, done, lines, singles, reads, used = len(read), 0, 0, 0, False, False
        if lut_len is None:
            if m & 1:
                if not 1 <= sym[0] <= 4:
                    singles += self.single(steps[0], fused)
                done = 1
        else:
            reads, used = self.entry(read, steps, end, lut_len)
            done = lut_len if used else 0
        while done < m and done < len(steps):
            two = done + 2 <= m
            if two and 1 <= sym[done] <= 4 and 1 <= sym[done + 1] <= 4:
                a, b, _ = steps[done]
                lines += 1 if a >> 7 == b >> 7 else 2
                if self.reaches(steps, end, done + 2):
                    done += 2
                    continue
            singles += self.single(steps[done], fused)
            if two and done + 1 < len(steps):
                singles += self.single(steps[done + 1], fused)
            done += 2
        return 68 * lines + 12 * singles + 8 * reads, lines + singles + reads, (lut_len or 0) * used


def summed(fn, reads):
    return tm.total(fn(r) for r in reads)


@pytest.mark.parametrize("sigma", [4, 5, 28, 256])
def test_walk_ends_where_the_oracle_ends(sigma):
    ox, ix, reads, qbuf, qoff, tr = setup(sigma)
    valid = tm.valid_reads(qbuf, qoff, sigma)
    assert len(valid) < tr.nq or sigma == 256
    olb, oln, ost = ox.search_exact(*tm.take_reads(qbuf, qoff, valid), want_steps=True)
    assert np.array_equal(tr.lb[valid], olb.astype(np.int64)) and np.array_equal(tr.ln[valid], oln.astype(np.int64)) and np.array_equal(tr.steps[valid], ost.astype(np.int64))
    lit = Literal(ix.bwt, sigma)
    for q, r in enumerate(reads):
        steps, end = lit.walk(r)
        assert len(steps) == tr.steps[q] and end == (tr.lb[q], tr.ln[q])
        assert [(int(tr.a[q, j]), int(tr.b[q, j]), int(tr.sym[q, j])) for j in range(len(steps))] == steps
    assert np.array_equal(ix.C, ox.C.astype(np.int64))


@pytest.mark.parametrize("sigma", [4, 5, 28, 256])
def test_one_symbol_blocks(sigma):
    ox, ix, reads, qbuf, qoff, tr = setup(sigma)
    lit = Literal(ix.bwt, sigma)
    for fused in (False, True):
        nbytes, acc, steps = tm.cost_blocks(tr, fused)
        assert (nbytes, acc, steps) == summed(lambda r: lit.blocks(r, fused), reads)
        assert nbytes == 12 * acc and steps == 0
        known = int((tr.ex & (tr.sym < sigma)).sum())       # (a foreign byte is a step without an access)
        assert known <= acc <= 2 * known and acc <= 2 * int(tr.steps.sum())
        assert sum(tm.shared_split(tr, fused)) == acc
        vt = tm.Trace(ix, *tm.take_reads(qbuf, qoff, tm.valid_reads(qbuf, qoff, sigma)))       # without foreign bytes: steps <= accesses <= 2 steps
        assert int(vt.steps.sum()) <= tm.cost_blocks(vt, fused)[1] <= 2 * int(vt.steps.sum())
    assert tm.cost_blocks(tr, True)[1] > tm.cost_blocks(tr, False)[1]      # (the batch holds delimiters whose ends share a block)


def test_foreign_reads_cost_steps_and_no_access():
    ox, ix, reads, qbuf, qoff, tr = setup(5)
    foreign = [np.array([200], dtype=np.uint8), np.array([5, 9, 255], dtype=np.uint8), np.array([7] * 40, dtype=np.uint8)]
    qb = np.concatenate(foreign)
    qo = np.concatenate([[0], np.cumsum([len(r) for r in foreign])])
    ft = tm.Trace(ix, qb, qo)
    assert list(ft.steps) == [1, 1, 1] and list(ft.ln) == [0, 0, 0] and list(ft.lb) == [0, 0, 0]
    for cost in (tm.cost_blocks(ft), tm.cost_blocks(ft, True), tm.cost_pairs(ft), tm.cost_pairs(ft, 3), tm.cost_planes(ft), tm.cost_planes(ft, 2), tm.cost_tree(ft),
                 tm.cost_kstep(ft, 2, 3, 2)):
        assert cost == (0, 0, 0)


@pytest.mark.parametrize("lut_len", [None, 1, 3, 6])
def test_pair_table(lut_len):
    ox, ix, reads, qbuf, qoff, tr = setup(5)
    lit = Literal(ix.bwt, 5)
    for fused in (False, True):
        got = tm.cost_pairs(tr, lut_len, False, fused)
        assert got == summed(lambda r: lit.pairs(r, lut_len, fused), reads)
    if lut_len:
        wide = tm.cost_pairs(tr, lut_len, True, False)
        narrow = tm.cost_pairs(tr, lut_len, False, False)
        entries = sum(1 for r in reads if lit.entry(r, *lit.walk(r), lut_len)[0])
        assert wide[1:] == narrow[1:] and wide[0] - narrow[0] == 8 * entries and entries >= narrow[2] // lut_len > 0      # (16-byte entries; an entry may be empty)


@pytest.mark.parametrize("sigma", [6, 28])
@pytest.mark.parametrize("lut_len", [0, 2])
def test_symbol_planes(sigma, lut_len):
    ox, ix, reads, qbuf, qoff, tr = setup(sigma)
    lit = Literal(ix.bwt, sigma)
    assert tm.cost_planes(tr, lut_len) == summed(lambda r: lit.planes(r, lut_len), reads)
    if not lut_len:
        assert tm.cost_planes(tr)[1] == tm.cost_blocks(tr)[1]


@pytest.mark.parametrize("sigma", [5, 28, 256])
def test_tree(sigma):
    ox, ix, reads, qbuf, qoff, tr = setup(sigma)
    lit = Literal(ix.bwt, sigma)
    assert tm.tree_digits(256) == (3, 3, 2) and tm.tree_digits(28) == (3, 2) and tm.tree_digits(5) == (3,)
    sub = list(range(0, len(reads), 3))
    st = tm.Trace(ix, *tm.take_reads(qbuf, qoff, sub))
    assert tm.cost_tree(st) == summed(lit.tree, [reads[i] for i in sub])


def test_kstep_phases_without_tables_are_single_steps():
    """with no table at all every step is one single step, and the step that comes out empty is issued twice (main phase, then tail)"""
    ox, ix, reads, qbuf, qoff, tr = setup(5)
    single = tm.single_accesses(tr, True)
    last = np.maximum(tr.steps - 1, 0)
    twice = np.where((tr.steps > 0) & (tr.ln == 0), single[np.arange(tr.nq), last], 0)
    acc = int(single.sum() + twice.sum())
    assert tm.cost_kstep(tr, 1, 0, 0, fused=True) == (12 * acc, acc, 0)
    # a walk table saves accesses, a k-step table too
    assert tm.cost_kstep(tr, 1, 0, 1, fused=True)[1] < acc and tm.cost_kstep(tr, 3, 0, 0, fused=True)[1] < acc


def test_smem_walk_reads():
    ox, ix, reads, qbuf, qoff, tr = setup(5)
    brute = smem_brute.Batch(sequences(5), reads[:40], 5)
    walks = [w for r in reads[:40] for w in smem_brute.walk_reads(r, 5)]
    wt = tm.Trace(ix, np.concatenate(walks), np.concatenate([[0], np.cumsum([len(w) for w in walks])]))
    assert int(wt.steps.sum()) == brute.steps and list(np.where(wt.ln != 0, wt.steps, wt.steps - 1).clip(0)) == brute.lengths
    assert tm.cost_smems(ix, walks) == tm.cost_blocks(wt) and tm.cost_smems(ix, walks, counts=False) == (0, 0, 0)
    for r in reads[:40]:
        pieces = smem_brute.walk_reads(r, 5)
        assert len(pieces) == len(r)
        for e, p in enumerate(pieces):
            assert all(1 <= c < 5 for c in p) and bytes(p) == bytes(r[e + 1 - len(p): e + 1])
            assert len(p) == e + 1 or smem_brute.is_break(r[e - len(p)], 5)
