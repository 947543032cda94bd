"""CPU model of fmgpu_stats.table_bytes / table_accesses / table_steps for the exact-search family, written from the rule beside fmgpu_stats in
include/fmgpu.h (not from the kernels).  Plain numpy and Python integers.

Index    the BWT as a cumulative-count table: rank, LF, C
trace    the one-symbol backward search of every read of a batch (the reference's search_no_errors walk), vectorised over the reads: per executed step the
         interval ends (a, b) it started from and the symbol it consumed
cost_*   one function per row of the rule's table: a trace -> (table_bytes, table_accesses, table_steps)
The k-step / walk-table phases and the sample chain are state machines per read: plain loops over the reads (cost_kstep, cost_chain).
tests/test_exact_traffic_model.py keeps every vectorised function equal to a literal per-read, per-step loop."""
import numpy as np


class Index:
    """occ[i, c] = rows < i that hold symbol c;  C[c] = rows that hold a smaller symbol;  below[i, c] = rows < i that hold a symbol < c"""

    def __init__(self, bwt, sigma):
        bwt = np.asarray(bwt, dtype=np.int64)
        self.bwt, self.sigma, self.n = bwt, int(sigma), len(bwt)
        self.occ = np.zeros((self.n + 1, self.sigma), dtype=np.int32)
        self.occ[np.arange(1, self.n + 1), bwt] = 1
        np.cumsum(self.occ, axis=0, out=self.occ)
        self.C = np.concatenate([[0], np.cumsum(self.occ[self.n])]).astype(np.int64)
        self._below = None

    @classmethod
    def from_oracle(cls, ox):
        s = ox.bwt_string()
        return cls([s.symbol(i) for i in range(ox.n)], ox.sigma)

    @property
    def below(self):
        if self._below is None:
            self._below = np.zeros((self.n + 1, self.sigma + 1), dtype=np.int32)
            np.cumsum(self.occ, axis=1, out=self._below[:, 1:])
        return self._below

    def lf(self, i, c):
        return int(self.C[c]) + int(self.occ[i, c])


class Trace:
    """of a batch of nq reads, the longest of M symbols.  Column j is the j-th symbol consumed (the read's symbol m - 1 - j).
    sym[q, j]   that symbol (-1 beyond the read)
    ex[q, j]    step j was executed
    a, b[q, j]  the interval [a, b) step j started from (valid where ex)
    m, steps    the read's length, its executed steps;  lb, ln: the cursor after the last executed step (the root [0, n) for an empty read)"""

    def __init__(self, ix, qbuf, qoff):
        qbuf = np.asarray(qbuf, dtype=np.int64)
        qoff = np.asarray(qoff, dtype=np.int64)
        nq = len(qoff) - 1
        self.ix, self.nq = ix, nq
        self.m = m = qoff[1:] - qoff[:-1]
        M = int(m.max()) if nq else 0
        self.M = M
        col = np.arange(M)[None, :]
        inside = col < m[:, None]
        at = np.where(inside, qoff[1:, None] - 1 - col, 0)
        self.sym = np.where(inside, qbuf[at] if len(qbuf) else 0, -1)
        self.ex = np.zeros((nq, M), dtype=bool)
        self.a = np.zeros((nq, M), dtype=np.int64)
        self.b = np.zeros((nq, M), dtype=np.int64)
        lb = np.zeros(nq, dtype=np.int64)
        ln = np.full(nq, ix.n, dtype=np.int64)
        alive = m > 0
        for j in range(M):
            alive = alive & (j < m)
            if not alive.any():
                break
            c = self.sym[:, j]
            self.ex[:, j] = alive
            self.a[:, j] = lb
            self.b[:, j] = lb + ln
            ok = alive & (c < ix.sigma)
            cc = np.where(ok, c, 0)
            ra = ix.C[cc] + ix.occ[lb, cc]
            rb = ix.C[cc] + ix.occ[lb + ln, cc]
            foreign = alive & ~ok                               # a symbol >= sigma: a step, the cursor empties to (0, 0)
            lb = np.where(ok, ra, np.where(foreign, 0, lb))
            ln = np.where(ok, rb - ra, np.where(foreign, 0, ln))
            alive = alive & (ln != 0)
        self.steps = self.ex.sum(axis=1)
        self.lb, self.ln = lb, ln

    def reaches(self, j):
        """[q, len(j)] or [q]: the cursor after j consumed symbols exists and is not empty (j = 0: the root)"""
        j = np.asarray(j)
        s = self.steps if j.ndim == 1 else self.steps[:, None]
        e = self.ln if j.ndim == 1 else self.ln[:, None]
        return (j < s) | ((j == s) & (e != 0))


def total(parts):
    """sum of (bytes, accesses, steps) triples"""
    parts = list(parts)
    return tuple(int(sum(p[k] for p in parts)) for k in range(3))


# ---------------------------------------------------------------------------------------------------------------- one access per block / line
def ends_accesses(tr, shift):
    """[q, j]: 1 where both ends of step j's interval lie in the same block of 2^shift rows, else 2"""
    return 1 + ((tr.a >> shift) != (tr.b >> shift)).astype(np.int64)


def single_accesses(tr, fused=False):
    """[q, j]: accesses of step j taken as ONE one-symbol step on Format A (12 bytes each): none for a symbol >= sigma, always 2 for a delimiter on a table with fused
    presence bits, else one per end, one if both ends share a 64-row block"""
    acc = ends_accesses(tr, 6)
    if fused:
        acc = np.where(tr.sym == 0, 2, acc)
    return np.where(tr.ex & (tr.sym < tr.ix.sigma), acc, 0)


def cost_blocks(tr, fused=False):
    """one-symbol blocks (Format A): k_exact_a"""
    acc = int(single_accesses(tr, fused).sum())
    return 12 * acc, acc, 0


def shared_split(tr, fused=False):
    """accesses of cost_blocks that come from steps whose ends share a block / lie in two"""
    acc = single_accesses(tr, fused)
    return int(acc[acc == 1].sum()), int(acc[acc == 2].sum())


def lut_start(tr, lut_len, entry_bytes):
    """the interval table in front of a kernel: (start[q], bytes, accesses, table_steps).  A read of at least lut_len symbols (on a text of more than one row) whose last
    lut_len symbols are all in 1 .. sigma - 1 reads its entry; where the entry is not empty the read starts behind those symbols (start = lut_len, they cost nothing
    else), otherwise at 0"""
    start = np.zeros(tr.nq, dtype=np.int64)
    if not lut_len or tr.ix.n <= 1 or tr.M < lut_len:
        return start, 0, 0, 0
    head = tr.sym[:, :lut_len]
    reads = (tr.m >= lut_len) & ((head >= 1) & (head < tr.ix.sigma)).all(axis=1)
    used = reads & tr.reaches(np.full(tr.nq, lut_len))
    start[used] = lut_len
    return start, entry_bytes * int(reads.sum()), int(reads.sum()), lut_len * int(used.sum())


def cost_planes(tr, lut_len=0, wide=False):
    """symbol planes (Format S): one 64-row line of 44 bytes per end, one if shared; optionally behind an interval table"""
    start, lb, la, ls = lut_start(tr, lut_len, 16 if wide else 8)
    col = np.arange(tr.M)[None, :]
    acc = np.where(tr.ex & (tr.sym < tr.ix.sigma) & (col >= start[:, None]), ends_accesses(tr, 6), 0)
    acc = int(acc.sum())
    return 44 * acc + lb, acc + la, ls


def tree_digits(sigma):
    """digit bits of the multi-ary tree's levels from the top, for symbols of bit_width(sigma - 1) bits"""
    return {1: (1,), 2: (2,), 3: (3,), 4: (2, 2), 5: (3, 2), 6: (3, 3), 7: (3, 2, 2), 8: (3, 3, 2)}[max(1, int(sigma - 1).bit_length())]


def cost_tree(tr):
    """multi-ary tree (Format M): per level and end one node block of 64 node-local positions, 4 + 8 d bytes for a level of d digit bits; one if both ends share it.
    The node-local position of row i at a level = the rows < i whose higher digits equal the node's."""
    ix = tr.ix
    digits = tree_digits(ix.sigma)
    valid = tr.ex & (tr.sym < ix.sigma)
    c = np.where(valid, tr.sym, 0)
    low = sum(digits)
    nbytes = acc = 0
    for d in digits:
        # the node of this level: symbols that share c's bits above `low`
        first = (c >> low) << low
        last = np.minimum(first + (1 << low), ix.sigma)
        pa = ix.below[tr.a, last] - ix.below[tr.a, first]
        pb = ix.below[tr.b, last] - ix.below[tr.b, first]
        k = np.where(valid, 1 + ((pa >> 6) != (pb >> 6)), 0)
        acc += int(k.sum())
        nbytes += (4 + 8 * d) * int(k.sum())
        low -= d
    return nbytes, acc, 0


# ---------------------------------------------------------------------------------------------------------------- pair table
def pair_walk(tr, start, stop, odd_first=None, fused=False):
    """the pair-table walk of every read over its consumed symbols start[q] .. stop[q] - 1 (stop <= m), as (lines, singles): accesses to 128-row pair lines (68 bytes) and
    to block entries (12 bytes).
      odd_first[q]  the symbol at `start` is the read's odd one: taken from C where it is in 1 .. 4 (no access), else a single step; the pairs begin behind it
      pairs         two symbols (y, then x), both in 1 .. 4: one line per end of the interval, one if both ends share a line — counted also where the pair comes out empty
      singles       a pair that holds a delimiter or a foreign byte, or that came out empty, is taken as two single steps (the second only if the first left rows);
                    so is a symbol left over at the end of the stretch"""
    col = np.arange(tr.M)[None, :]
    start = np.asarray(start, dtype=np.int64)[:, None]
    stop = np.asarray(stop, dtype=np.int64)[:, None]
    odd = np.zeros((tr.nq, 1), dtype=bool) if odd_first is None else np.asarray(odd_first, dtype=bool)[:, None]
    single = single_accesses(tr, fused)
    inside = tr.ex & (col >= start) & (col < stop)
    free = inside & odd & (col == start) & (tr.sym >= 1) & (tr.sym <= 4)
    first = start + odd
    is_first = inside & (col >= first) & (((col - first) & 1) == 0)           # the first symbol of a pass of the pair loop
    nxt = np.concatenate([tr.sym[:, 1:], np.full((tr.nq, 1), -1)], axis=1)
    pairable = is_first & (col + 2 <= stop) & (tr.sym >= 1) & (tr.sym <= 4) & (nxt >= 1) & (nxt <= 4)
    lines = int(np.where(pairable, ends_accesses(tr, 7), 0).sum())
    stepped = pairable & tr.reaches(col + 2)
    covered = stepped | np.concatenate([np.zeros((tr.nq, 1), dtype=bool), stepped[:, :-1]], axis=1) | free
    singles = int(np.where(inside & ~covered, single, 0).sum())
    return lines, singles


def cost_pairs(tr, lut_len=None, wide=False, fused=False):
    """pair table (Format P): k_exact_p.  lut_len None: no interval table, the odd symbol first and from C.  lut_len = L: behind an interval table; a read that does
    not start from its entry is walked from the root in pairs; either way a symbol left over is the LAST one and a single step"""
    if lut_len is None:
        lines, singles = pair_walk(tr, np.zeros(tr.nq, dtype=np.int64), tr.m, (tr.m & 1) == 1, fused)
        return 68 * lines + 12 * singles, lines + singles, 0
    start, lb, la, ls = lut_start(tr, lut_len, 16 if wide else 8)
    lines, singles = pair_walk(tr, start, tr.m, None, fused)
    return 68 * lines + 12 * singles + lb, lines + singles + la, ls


# ---------------------------------------------------------------------------------------------------------------- k-step / walk tables
def walk_len(sigma):
    """J: symbols of one walk entry = 32 / bit_width(sigma - 2)"""
    return 32 // int(sigma - 2).bit_length()


def cursor_at(tr, q, done):
    """(lb, len) of read q after `done` consumed symbols, or None where the walk does not get there with rows left"""
    if done < tr.steps[q]:
        return int(tr.a[q, done]), int(tr.b[q, done] - tr.a[q, done])
    if done == tr.steps[q] and tr.ln[q] != 0:
        return int(tr.lb[q]), int(tr.ln[q])
    return None


def cost_kstep(tr, kstep=1, lut_len=0, walk=0, wide=False, fused=False):
    """k_exact_kstep, read by read.  Phases:
      interval entry   as lut_start (table_steps stays 0 behind this kernel)
      main             one row left and 2J symbols remain (walk >= 2), or J (walk >= 1): one walk entry (LF^2J: 12 bytes, LF^J: 8; 16 with 64-bit rows); else, with a
                       k-step table, one 12-byte context entry per end (one if same 64-row block) for the next K symbols; else one single step.
                       The phase ends at a stretch that is short or holds a symbol outside 1 .. sigma - 1 (nothing read), at a walk entry that met a delimiter, and at a
                       context or single step that comes out empty (these were read, and count).  A walk entry whose symbols differ from the read's: the symbols
                       before the first differing one still go K at a time through the context table, then the phase ends.
      tail             single steps to the read's end or the empty interval (a step that came out empty above is issued again here, and counts again)"""
    ix = tr.ix
    K = kstep if kstep >= 2 else 0
    J = walk_len(ix.sigma)
    w1, w2 = (16, 16) if wide else (8, 12)
    start, nbytes, acc, _ = lut_start(tr, lut_len, 16 if wide else 8)
    single = single_accesses(tr, fused)
    for q in range(tr.nq):
        m, done = int(tr.m[q]), int(start[q])
        sym = tr.sym[q]

        def plain(frm, cnt):
            return m - frm >= cnt and all(1 <= sym[frm + t] < ix.sigma for t in range(cnt))

        def met(row, cnt):                                  # the symbols a walk of cnt LF steps from `row` meets; None if a delimiter is among them
            out = []
            for _ in range(cnt):
                c = int(ix.bwt[row])
                if c == 0:
                    return None
                out.append(c)
                row = ix.lf(row, c)
            return out

        def context():                                      # K symbols through the context table: False ends the phase
            nonlocal acc, nbytes, done
            if not plain(done, K):
                return False
            k = 1 + int((tr.a[q, done] >> 6) != (tr.b[q, done] >> 6))
            acc += k; nbytes += 12 * k
            if cursor_at(tr, q, done + K) is None:
                return False
            done += K
            return True

        walks, limit = True, 0
        while True:
            lb, ln = cursor_at(tr, q, done)
            if not walks:
                if not K or done + K > limit or not context():
                    break
            elif walk >= 2 and ln == 1 and m - done >= 2 * J or walk >= 1 and ln == 1 and m - done >= J:
                span = 2 * J if walk >= 2 and m - done >= 2 * J else J
                if not plain(done, span):
                    break
                acc += 1; nbytes += w2 if span == 2 * J else w1
                got = met(lb, span)
                if got is None:
                    break
                want = [int(sym[done + t]) for t in range(span)]
                if got != want:
                    walks, limit = False, done + next(t for t in range(span) if got[t] != want[t])
                    continue
                done += span
            elif K:
                if not context():
                    break
            else:
                if done >= m or sym[done] >= ix.sigma:
                    break
                acc += int(single[q, done]); nbytes += 12 * int(single[q, done])
                if cursor_at(tr, q, done + 1) is None:
                    break
                done += 1
        tail = int(single[q, done:].sum())
        acc += tail; nbytes += 12 * tail
    return int(nbytes), int(acc), 0


# ---------------------------------------------------------------------------------------------------------------- sample chain
PARK_MIN = 32           # a one-row read is parked while at least this many symbols remain
CHAIN_MIN_LONGEST = 48  # ... in a batch whose longest read has at least this many


def cost_chain(tr, text, sa, seq_starts, rate, fused=True):
    """exact search along the sample chain.  text: the sequences joined, each followed by its delimiter; sa[row] = the text position of row's suffix; seq_starts: the text
    position of every sequence's first symbol; the sampled positions are those at a multiple of `rate` from their sequence's start.
    Returns {"park", "seek", "jump", "resume"} -> (bytes, accesses, steps) and "jumped_entries":
      park    the pair-table walk up to the park point: the first pass of the pair loop (pair granularity: behind the odd symbol, then every second symbol) at which
              the interval is one row and at least PARK_MIN symbols remain
      seek    at most rate - 1 single steps to a sampled row: the 64-byte block of every row looked at (the sampled row's included); ends without a sampled row where
              the next symbol is not in 1 .. 4 or the step would empty the interval
      jump    on a sampled row: the 4-byte rank -> position word and the row's own 8-byte entry; then, while `rate` symbols remain and the entry can be used (not the
              first sample of a sequence, no delimiter in its window), the 8-byte entry in front of it is read and the window compared: equal moves on and stands for
              `rate` steps (table_steps), unequal ends the jump
      resume  the pair-table walk of the rest, from where the read stands (a symbol left over is the last one and a single step)
    A batch whose longest read is below CHAIN_MIN_LONGEST does not park at all."""
    text = np.asarray(text, dtype=np.int64)
    starts = np.asarray(sorted(int(s) for s in seq_starts), dtype=np.int64)
    nq, m = tr.nq, tr.m
    odd = (m & 1) == 1
    zero = np.zeros(nq, dtype=np.int64)
    nothing = (0, 0, 0)
    if tr.M < CHAIN_MIN_LONGEST:
        return {"park": cost_pairs(tr, None, False, fused), "seek": nothing, "jump": nothing, "resume": nothing, "jumped_entries": 0}
    col = np.arange(tr.M)[None, :]
    first = odd[:, None].astype(np.int64)
    can = tr.ex & (col >= first) & (((col - first) & 1) == 0) & ((tr.b - tr.a) == 1) & (m[:, None] - col >= PARK_MIN)
    parked = can.any(axis=1)
    park = np.where(parked, can.argmax(axis=1), m)
    lines, singles = pair_walk(tr, zero, park, odd, fused)
    out = {"park": (68 * lines + 12 * singles, lines + singles, 0)}
    resume = m.copy()
    blocks = words = entries = jumped = 0

    def seq_first(pos):
        return int(starts[np.searchsorted(starts, pos, side="right") - 1])

    for q in np.nonzero(parked)[0]:
        done, row, walked, found = int(park[q]), int(tr.a[q, park[q]]), 0, False
        sym, mq = tr.sym[q], int(m[q])
        while True:
            blocks += 1
            pos = int(sa[row])
            if (pos - seq_first(pos)) % rate == 0:
                found = True
                break
            cur = int(sym[done]) if done < mq else -1
            if walked + 1 >= rate or not 1 <= cur <= 4 or int(tr.ix.bwt[row]) != cur:
                break
            row = tr.ix.lf(row, cur)
            done += 1; walked += 1
        if found:
            words += 1; entries += 1
            while mq - done >= rate:
                window = text[pos - rate: pos][::-1] if pos > seq_first(pos) else None      # the symbols in front of the position, the nearest first
                if window is None or not ((window >= 1) & (window <= 4)).all():
                    break
                entries += 1
                if not np.array_equal(window, sym[done: done + rate]):
                    break
                pos -= rate; done += rate; jumped += 1
        resume[q] = done
    out["seek"] = (64 * blocks, blocks, 0)
    out["jump"] = (4 * words + 8 * entries, words + entries, rate * jumped)
    lines, singles = pair_walk(tr, resume, m, None, fused)
    out["resume"] = (68 * lines + 12 * singles, lines + singles, 0)
    out["jumped_entries"] = jumped
    return out


# ---------------------------------------------------------------------------------------------------------------- SMEM walk
def cost_smems(ix, walk_reads, counts=True):
    """fmgpu_search_smems' walk: one one-symbol walk per batch symbol (tests/smem_brute.walk_reads gives the symbols each of them may consume); the one-symbol
    rule on Format A, nothing on every other layout"""
    if not counts:
        return 0, 0, 0
    qbuf = np.concatenate([np.asarray(r, dtype=np.uint8) for r in walk_reads] + [np.zeros(0, dtype=np.uint8)])
    qoff = np.concatenate([[0], np.cumsum([len(r) for r in walk_reads])])
    return cost_blocks(Trace(ix, qbuf, qoff))


# ---------------------------------------------------------------------------------------------------------------- the small batch of the GPU tests
FIXED_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128, 129)


def small_sequences(sigma, rows=12_000, seed=1):
    """three sequences of `rows` symbols in all; the first holds a block of 700 symbols twice, so that reads from it never reach one row"""
    rng = np.random.default_rng(1000 * sigma + seed)
    base = rng.integers(1, sigma, size=rows - 700 - 37, dtype=np.uint8)
    block = base[1000:1700]
    cut = (rows * 2) // 3
    return [np.concatenate([base[:cut], block]), base[cut:].copy(), rng.integers(1, sigma, size=37, dtype=np.uint8)]


def small_batch(seqs, sigma, count=1500, seed=2, longest=150):
    """about `count` reads of 1 .. `longest` symbols copied from the sequences, every length of FIXED_LENGTHS among them; every third with one substitution, a few with a
    delimiter, a few with a byte >= sigma (where a byte can be), a few from the repeated block, one empty"""
    rng = np.random.default_rng(1000 * sigma + seed)
    reads = []
    for i in range(count):
        s = seqs[i % 2]
        m = FIXED_LENGTHS[i % len(FIXED_LENGTHS)] if i < 4 * len(FIXED_LENGTHS) else int(rng.integers(1, (longest if i % 2 else 40) + 1))     # (half of them short: the first steps of a read are the ones with two blocks)
        if i % 50 == 7:                                          # ends inside the second copy of the repeated block
            s, m = seqs[0], min(m, 600)
            p = len(s) - int(rng.integers(0, 100)) - m
        else:
            p = int(rng.integers(0, len(s) - m + 1))
        r = s[p: p + m].copy()
        if i % 3 == 0:
            j = int(rng.integers(0, m))
            r[j] = (int(r[j]) - 1 + int(rng.integers(1, sigma - 1))) % (sigma - 1) + 1
        if i % 97 == 5:
            r[int(rng.integers(0, m))] = 0
        if i % 89 == 11 and sigma < 256:
            r[int(rng.integers(0, m))] = (sigma, 255, sigma + 1)[i % 3] if sigma < 255 else 255
        reads.append(r)
    reads.append(np.zeros(0, dtype=np.uint8))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    qbuf = np.concatenate(reads).astype(np.uint8)
    qoff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return qbuf, qoff


def valid_reads(qbuf, qoff, sigma):
    """the reads the reference's walk is defined for: every symbol below sigma"""
    bad = np.concatenate([[0], np.cumsum(np.asarray(qbuf) >= sigma)])
    qoff = np.asarray(qoff, dtype=np.int64)
    return np.nonzero(bad[qoff[1:]] == bad[qoff[:-1]])[0]


def take_reads(qbuf, qoff, keep):
    qoff = np.asarray(qoff, dtype=np.int64)
    parts = [qbuf[qoff[i]: qoff[i + 1]] for i in keep]
    return (np.concatenate(parts + [np.zeros(0, dtype=np.uint8)]).astype(np.uint8),
            np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64))
