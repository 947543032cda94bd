"""The delimiter-row lists of Formats P and D (the head of csrc/fmgpu_common.h) restated in NumPy: what the device builds from a sigma = 5 BWT and what the kernels
compute on it.  Both formats write a row that holds a delimiter as code 0 ('A' / "AA"), leave it out of the counts and list it; a rank of 'A' / "AA" subtracts the
listed rows between the start of the end's line (128 rows, Format P) or block (64 rows, Format D) and the end.  `corrections=False` drops the lists: the model of a
kernel whose correction is broken.  Every "AA" / 'A' interval end a search passes is recorded (events_p / events_d) with what the correction was and whether the
kernels' filter of `bits` entries (line or block number mod bits) sends the end to the list at all."""
import numpy as np

LINE, BLOCK = 128, 64


class _String:
    """one BWT: block counts and symbols, enough for rank, LF and its inverse"""

    def __init__(self, s):
        self.s = np.ascontiguousarray(s, dtype=np.uint8)
        self.n = len(self.s)
        assert self.s.max(initial=0) < 5
        self.C = np.concatenate([[0], np.cumsum(np.bincount(self.s, minlength=5))]).astype(np.int64)      # C[c] = rows with a smaller symbol; C[5] = n
        nb = self.n // BLOCK + 1
        pad = np.full(nb * BLOCK, 255, dtype=np.uint8)
        pad[: self.n] = self.s
        per = np.stack([(pad.reshape(nb, BLOCK) == c).sum(axis=1) for c in range(5)], axis=1)
        self.before = np.concatenate([np.zeros((1, 5), dtype=np.int64), np.cumsum(per, axis=0)])           # before[B][c] = #{ j < 64 B : s[j] == c }
        self.pad = pad

    def rank(self, i, c):
        B = i >> 6
        return int(self.before[B, c]) + int(np.count_nonzero(self.pad[B * BLOCK: i] == c))

    def lf(self, i, c):
        return int(self.C[c]) + self.rank(i, c)

    def lf_rows(self):
        """LF of every row by its own symbol"""
        out = np.empty(self.n, dtype=np.int64)
        for c in range(5):
            rows = np.nonzero(self.s == c)[0]
            out[rows] = self.C[c] + np.arange(len(rows))
        return out

    def first_symbol(self, r):
        """the symbol suffix r starts with"""
        return int(np.searchsorted(self.C, r, side="right")) - 1

    def psi(self, r):
        """the row of suffix r without its first symbol (the inverse of LF)"""
        c = self.first_symbol(r)
        k = r - int(self.C[c])                                       # the k-th row (from 0) that holds c
        B = int(np.searchsorted(self.before[:, c], k, side="right")) - 1
        hits = np.nonzero(self.pad[B * BLOCK: (B + 1) * BLOCK] == c)[0]
        return B * BLOCK + int(hits[k - int(self.before[B, c])])

    def text_at(self, r, m):
        """the m symbols suffix r starts with (None if a delimiter is among them)"""
        out = []
        for _ in range(m):
            c = self.first_symbol(r)
            if c == 0:
                return None
            out.append(c)
            r = self.psi(r)
        return np.array(out, dtype=np.uint8)


def plain_search(string, read):
    """search/SearchNoErrors.h:12-26 on a _String: (lb, len, steps); a miss ends on the row and at the step of the symbol that emptied the interval"""
    lb, ln, steps = 0, string.n, 0
    for c in read[::-1]:
        c = int(c)
        a, b = string.lf(lb, c), string.lf(lb + ln, c)
        lb, ln, steps = a, b - a, steps + 1
        if ln == 0:
            break
    return lb, ln, steps


class ListedRows:
    def __init__(self, bwt, bwt_rev=None, corrections=True, bits=32768):
        self.corrections, self.bits = corrections, bits
        self.fw = _String(bwt)
        self.n = self.fw.n
        self.C = self.fw.C
        self._build_pairs()
        self.dense = [self._build_dense(self.fw)]
        if bwt_rev is not None:
            self.rv = _String(bwt_rev)
            assert self.rv.n == self.n and np.array_equal(self.rv.C, self.C)
            self.dense.append(self._build_dense(self.rv))
        self.events_p = []                    # (row i, listed rows in [first row of i's line, i)) per end of an "AA" step
        self.events_d = [[], []]              # per direction: (row i, delimiter rows in [first row of i's block, i)) per end of an 'A' step

    # ------------------------------------------------------------------ Format P
    def _build_pairs(self):
        s, n = self.fw.s, self.n
        y = s.astype(np.int64)
        x = s[self.fw.lf_rows()].astype(np.int64)                    # (x, y) = (s[LF(i)], s[i]): the two symbols in front of suffix i
        listed = (y == 0) | (x == 0)
        self.pair_code = np.where(listed, 0, (x - 1) * 4 + (y - 1)).astype(np.uint8)      # what the planes spell: a listed row reads as "AA"
        self.pairs_ex = np.nonzero(listed)[0].astype(np.int64)       # ascending
        nlines = n // LINE + 1
        pad = np.full(nlines * LINE, 255, dtype=np.uint8)
        pad[:n] = np.where(listed, 255, self.pair_code)              # listed rows are in no count
        per = np.stack([(pad.reshape(nlines, LINE) == pc).sum(axis=1) for pc in range(16)], axis=1)
        start = np.array([self.fw.lf(self.fw.lf(0, (pc & 3) + 1), (pc >> 2) + 1) for pc in range(16)], dtype=np.int64)       # first row of "xy": y first, then x
        self.pair_count = start[None, :] + np.concatenate([np.zeros((1, 16), dtype=np.int64), np.cumsum(per, axis=0)])[:nlines]
        self.pair_plane = np.zeros(nlines * LINE, dtype=np.uint8)
        self.pair_plane[:n] = self.pair_code                         # rows behind the last one: code 0, never below an end
        self.pair_flag = np.zeros(self.bits, dtype=bool)
        self.pair_flag[(self.pairs_ex >> 7) % self.bits] = True
        self.pair_line_listed = np.zeros(nlines, dtype=bool)
        self.pair_line_listed[self.pairs_ex >> 7] = True

    def listed_before(self, i):
        first = i & ~(LINE - 1)
        return int(np.searchsorted(self.pairs_ex, i) - np.searchsorted(self.pairs_ex, first))

    def pair_rank(self, i, pc):
        """the line's count + matching plane rows below i - (pc == 0) the listed rows among them"""
        L = i >> 7
        r = int(self.pair_count[L, pc]) + int(np.count_nonzero(self.pair_plane[L * LINE: i] == pc))
        if pc == 0:
            corr = self.listed_before(i)
            self.events_p.append((i, corr))
            if self.corrections:
                r -= corr
        return r

    def search_pairs(self, read):
        """k_exact_p (csrc/fmgpu_exact.hip), the whole search: a read of odd length takes its last symbol first, as the step from [0, n) to [C[c], C[c + 1]); then two
        symbols per step; a pair that comes out empty, holds a delimiter or a byte outside the alphabet, and a last single symbol, are taken in one-symbol steps.
        (lb, len, steps)"""
        q = [int(v) for v in read]
        m, n = len(q), self.n
        st = {"lb": 0, "len": n, "steps": 0}

        def single(c):
            st["steps"] += 1
            if c >= 5:
                st["lb"], st["len"] = 0, 0
                return False
            a, b = min(st["lb"], n), min(st["lb"] + st["len"], n)    # (without the corrections a rank may overshoot the table)
            ra, rb = self.fw.lf(a, c), self.fw.lf(b, c)
            st["lb"], st["len"] = ra, rb - ra
            return st["len"] != 0

        alive, done = m != 0, 0
        if m & 1:
            c = q[m - 1]
            if 1 <= c <= 4:
                st["steps"] += 1
                st["lb"], st["len"] = int(self.C[c]), int(self.C[c + 1] - self.C[c])
                alive = st["len"] != 0
            else:
                alive = single(c)
            done = 1
        while alive and done < m:
            y = q[m - 1 - done]
            two = done + 2 <= m
            x = q[m - 2 - done] if two else 0
            done += 2
            stepped = False
            if two and 1 <= y <= 4 and 1 <= x <= 4:
                pc = (x - 1) * 4 + (y - 1)
                a, b = min(st["lb"], n), min(st["lb"] + st["len"], n)
                ra, rb = self.pair_rank(a, pc), self.pair_rank(b, pc)
                if rb > ra:
                    st["lb"], st["len"] = ra, rb - ra
                    st["steps"] += 2
                    stepped = True
            if not stepped:
                alive = single(y)
                if alive and two:
                    alive = single(x)
        return st["lb"], st["len"], st["steps"]

    def pair_events(self):
        """the recorded "AA" ends as arrays: row, correction, on_listed (the end's own row is listed), flagged (the filter sends the end to the list),
        alias (flagged, though the end's own line holds no listed row)"""
        ev = np.array(self.events_p, dtype=np.int64).reshape(-1, 2)
        row, corr = ev[:, 0], ev[:, 1]
        line = row >> 7
        flagged = self.pair_flag[line % self.bits]
        return {"row": row, "correction": corr, "on_listed": np.isin(row, self.pairs_ex), "flagged": flagged, "alias": flagged & ~self.pair_line_listed[line]}

    # ------------------------------------------------------------------ Format D
    def _build_dense(self, string):
        s, n = string.s, string.n
        code = np.where(s == 0, 0, s.astype(np.int64) - 1).astype(np.uint8)           # a delimiter row reads as 'A'
        nb = n // BLOCK + 1
        plane = np.full(nb * BLOCK, 255, dtype=np.uint8)                             # (the device pads with code 0; a pad row is never below an end)
        plane[:n] = code
        ex = np.nonzero(s == 0)[0].astype(np.int64)
        flag = np.zeros(self.bits, dtype=bool)
        flag[(ex >> 6) % self.bits] = True
        has = np.zeros(nb, dtype=bool)
        has[ex >> 6] = True
        return {"string": string, "p0": plane & 1, "p1": (plane >> 1) & 1, "plane": plane, "occ": string.C[None, 1:5] + string.before[:nb, 1:5], "ex": ex, "flag": flag,
                "block_listed": has}

    def delims_before(self, i, rev=False):
        ex = self.dense[int(rev)]["ex"]
        return int(np.searchsorted(ex, i) - np.searchsorted(ex, i & ~(BLOCK - 1)))

    def dense_rank(self, i, c, rev=False):
        """c in 1..4: the block's count (C folded in) + rows of the block below i whose planes spell c - 1, - (c == 1) the delimiter rows among them"""
        d = self.dense[int(rev)]
        B = i >> 6
        r = int(d["occ"][B, c - 1]) + int(np.count_nonzero(d["plane"][B * BLOCK: i] == c - 1))
        if c == 1:
            corr = self.delims_before(i, rev)
            self.events_d[int(rev)].append((i, corr))
            if self.corrections:
                r -= corr
        return r

    def row_symbol(self, i, rev=False):
        """the symbol the planes give for row i; 0 on a listed row (without the list: 'A')"""
        d = self.dense[int(rev)]
        if self.corrections and np.searchsorted(d["ex"], i, side="right") - np.searchsorted(d["ex"], i) == 1:
            return 0
        return int(d["p0"][i]) + 2 * int(d["p1"][i]) + 1

    def search_dense(self, read, rev=False):
        """an exact search in one-symbol steps on Format D: backward on bwt; on bwtRev the read is taken from its front (extending right).  Symbols 1..4 only.
        (lb in that string, len, steps)"""
        lb, ln, steps = 0, self.n, 0
        for c in (read if rev else read[::-1]):
            a, b = min(lb, self.n), min(lb + ln, self.n)
            ra, rb = self.dense_rank(a, int(c), rev), self.dense_rank(b, int(c), rev)
            lb, ln, steps = ra, rb - ra, steps + 1
            if ln <= 0:
                return lb, 0, steps
        return lb, ln, steps

    def dense_events(self, rev=False):
        d = self.dense[int(rev)]
        ev = np.array(self.events_d[int(rev)], dtype=np.int64).reshape(-1, 2)
        row, corr = ev[:, 0], ev[:, 1]
        blk = row >> 6
        flagged = d["flag"][blk % self.bits]
        return {"row": row, "correction": corr, "on_listed": np.isin(row, d["ex"]), "flagged": flagged, "alias": flagged & ~d["block_listed"][blk]}

    def clear_events(self):
        self.events_p = []
        self.events_d = [[], []]
