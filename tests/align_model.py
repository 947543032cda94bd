"""fmgpu_chains_align (include/fmgpu.h) in plain Python loops: the rule as the header states it, nothing shared with the library.  align() takes the arrays the call takes
and returns (records, ops): records[c] = (first_op, n_ops, status, n_match, n_mismatch, n_ins, n_del), ops = the operations of all chains as len << 4 | code."""

I, D, S, EQ, X = 1, 2, 4, 7, 8
INVALID, UNSUPPORTED = -1, -2
LETTER = {I: "I", D: "D", S: "S", EQ: "=", X: "X"}
KINDS = ("anchors", "index", "hit", "query", "order", "ends", "qend", "window", "long", "piece")      # the order the device reports them in
LONG = 1 << 28


class AlignError(Exception):
    def __init__(self, what, chain, anchor=None):
        Exception.__init__(self, "%s: chain %d" % (what, chain))
        self.what, self.chain, self.anchor = what, chain, anchor
        self.code = UNSUPPORTED if what == "long" else INVALID


def band_of(gq, gt, w):
    d = gt - gq
    return min(0, d) - w, max(0, d) + w


def gap_ops(Q, T, w):
    """the global alignment of Q against T with unit costs on the band of width w around the two corner diagonals -> (cost, [(len, code), ...]).  rows[a] holds
    D(a, b) for the b that the band leaves row a, the first of them at first[a]; a cell outside has no value"""
    gq, gt = len(Q), len(T)
    lo, hi = band_of(gq, gt, w)
    none = 1 << 60
    rows, first = [], []
    for a in range(gq + 1):
        b0, b1 = max(0, a + lo), min(gt, a + hi)
        row = [none] * (b1 - b0 + 1)
        if a:
            up, u0 = rows[a - 1], first[a - 1]
            un = len(up)
            qs = Q[a - 1]
        for b in range(b0, b1 + 1):
            if a == 0 and b == 0:
                row[0] = 0
                continue
            best = none
            if a and b and 0 <= b - 1 - u0 < un:
                best = up[b - 1 - u0] + (qs != T[b - 1])
            if b > b0 and row[b - 1 - b0] + 1 < best:
                best = row[b - 1 - b0] + 1
            if a and 0 <= b - u0 < un and up[b - u0] + 1 < best:
                best = up[b - u0] + 1
            row[b - b0] = best
        rows.append(row)
        first.append(b0)

    def value(a, b):
        return rows[a][b - first[a]] if a >= 0 and 0 <= b - first[a] < len(rows[a]) else None

    a, b, back = gq, gt, []
    while a or b:
        v = value(a, b)
        if a > 0 and b > 0 and value(a - 1, b - 1) + (0 if Q[a - 1] == T[b - 1] else 1) == v:
            back.append(EQ if Q[a - 1] == T[b - 1] else X)
            a, b = a - 1, b - 1
        elif b > 0 and value(a, b - 1) is not None and value(a, b - 1) + 1 == v:
            back.append(D)
            b -= 1
        else:
            assert a > 0 and value(a - 1, b) + 1 == v
            back.append(I)
            a -= 1
    return rows[gq][gt - first[gq]], canonical([(1, c) for c in reversed(back)])


def canonical(ops):
    out = []
    for n, c in ops:
        if n == 0:
            continue
        if out and out[-1][1] == c:
            out[-1] = (out[-1][0] + n, c)
        else:
            out.append((n, c))
    return out


def cells(gq, gt, w):
    lo, hi = band_of(gq, gt, w)
    return (gq + 1) * (hi - lo + 1)


def chain_anchors(ch, anchors, positions, spans):
    """the anchors of a chain as (q, l, t, qidx, seq_id)"""
    out = []
    for k in range(int(ch[7])):
        p = positions[int(anchors[int(ch[8]) + k])]
        s = spans[int(p[4])]
        out.append((int(s[0]), int(s[1]), int(p[2]), int(p[0]), int(p[1])))
    return out


def check(chains, anchors, positions, spans, qoff, toff):
    """the device-side checks, kind by kind in the header's order; within a kind the lowest chain (and anchor)"""
    nq, n_anchor, count, n_spans = len(qoff) - 1, len(anchors), len(positions), len(spans)
    total = 0
    for c, ch in enumerate(chains):
        total += int(ch[7])
        if int(ch[7]) == 0 or int(ch[8]) + int(ch[7]) > n_anchor or total > n_anchor:
            raise AlignError("anchors", c)
    for c, ch in enumerate(chains):
        if any(int(anchors[int(ch[8]) + k]) >= count for k in range(int(ch[7]))):
            raise AlignError("index", c)
    for c, ch in enumerate(chains):
        for k in range(int(ch[7])):
            hit = int(positions[int(anchors[int(ch[8]) + k])][4])
            if hit >= n_spans or int(spans[hit][1]) == 0:
                raise AlignError("hit", c)
    for c, ch in enumerate(chains):
        if int(ch[0]) >= nq or any((x[3], x[4]) != (int(ch[0]), int(ch[1])) for x in chain_anchors(ch, anchors, positions, spans)):
            raise AlignError("query", c)
    for c, ch in enumerate(chains):
        xs = chain_anchors(ch, anchors, positions, spans)
        if any(not (xs[k + 1][0] > xs[k][0] and xs[k + 1][2] > xs[k][2]) for k in range(len(xs) - 1)):
            raise AlignError("order", c)
    for c, ch in enumerate(chains):
        xs = chain_anchors(ch, anchors, positions, spans)
        if (int(ch[2]), int(ch[4])) != (xs[0][2], xs[0][0]) or (int(ch[3]), int(ch[5])) != (xs[-1][2] + xs[-1][1], xs[-1][0] + xs[-1][1]):
            raise AlignError("ends", c)
    for c, ch in enumerate(chains):
        if int(ch[5]) > int(qoff[int(ch[0]) + 1]) - int(qoff[int(ch[0])]):
            raise AlignError("qend", c)
    for c, ch in enumerate(chains):
        if int(toff[c + 1]) - int(toff[c]) != int(ch[3]) - int(ch[2]):
            raise AlignError("window", c)
    for c, ch in enumerate(chains):
        if int(toff[c + 1]) - int(toff[c]) >= LONG or int(qoff[int(ch[0]) + 1]) - int(qoff[int(ch[0])]) >= LONG:
            raise AlignError("long", c)


def pieces_and_gaps(xs):
    """[(q, t, l')], [(gq, gt)] of a chain's anchors"""
    n = len(xs)
    pieces, gaps = [], []
    for k in range(n):
        q, l, t = xs[k][:3]
        lp = l if k == n - 1 else min(l, xs[k + 1][0] - q, xs[k + 1][2] - t)
        pieces.append((q, t, lp))
        if k < n - 1:
            gaps.append((xs[k + 1][0] - q - lp, xs[k + 1][2] - t - lp))
    return pieces, gaps


def align(chains, anchors, positions, spans, qbuf, qoff, tbuf, toff, band=64, max_gap_len=5000, max_cells=1 << 24, want_gaps=None):
    """want_gaps: a list that receives (chain, k, Q, T, cost) of every gap that went through the matrix"""
    check(chains, anchors, positions, spans, qoff, toff)
    lines = []
    for c, ch in enumerate(chains):
        xs = chain_anchors(ch, anchors, positions, spans)
        Q = [int(v) for v in qbuf[int(qoff[int(ch[0])]): int(qoff[int(ch[0]) + 1])]]
        T = [int(v) for v in tbuf[int(toff[c]): int(toff[c + 1])]]
        tbeg = int(ch[2])
        pieces, gaps = pieces_and_gaps(xs)
        for k, (q, t, lp) in enumerate(pieces):
            if Q[q: q + lp] != T[t - tbeg: t - tbeg + lp]:
                raise AlignError("piece", c, k)
        lines.append((ch, Q, T, pieces, gaps))
    records, ops = [], []
    for c, (ch, Q, T, pieces, gaps) in enumerate(lines):
        tbeg = int(ch[2])
        out = any(gq > 0 and gt > 0 and (max(gq, gt) > max_gap_len or cells(gq, gt, band) > max_cells) for gq, gt in gaps)
        if out:
            records.append((len(ops), 0, 1, 0, 0, 0, 0))
            continue
        line = [(int(ch[4]), S)]
        for k, (q, t, lp) in enumerate(pieces):
            line.append((lp, EQ))
            if k < len(gaps):
                gq, gt = gaps[k]
                if gq == 0 or gt == 0:
                    line += [(gt, D), (gq, I)]
                else:
                    Qg, Tg = Q[q + lp: q + lp + gq], T[t - tbeg + lp: t - tbeg + lp + gt]
                    cost, g = gap_ops(Qg, Tg, band)
                    if want_gaps is not None:
                        want_gaps.append((c, k, Qg, Tg, cost))
                    line += g
        line.append((len(Q) - int(ch[5]), S))
        line = canonical(line)
        count = {code: sum(n for n, c_ in line if c_ == code) for code in (EQ, X, I, D)}
        records.append((len(ops), len(line), 0, count[EQ], count[X], count[I], count[D]))
        ops += [n << 4 | code for n, code in line]
    return records, ops


def cigar(ops):
    return "".join("%d%s" % (int(w) >> 4, LETTER[int(w) & 15]) for w in ops)


# ---- two statements that share nothing with the rule above
def replay(ops, Q, T):
    """walks a chain's operations over the read Q and the window T -> (read symbols consumed, text symbols consumed, {code: bases}); asserts equality under every `=` and
    inequality under every X, that no operation is empty and that no two neighbours are the same"""
    a = b = 0
    count = {EQ: 0, X: 0, I: 0, D: 0, S: 0}
    before = None
    for w in ops:
        n, code = int(w) >> 4, int(w) & 15
        assert n > 0 and code != before and code in count
        before = code
        count[code] += n
        if code in (EQ, X):
            for j in range(n):
                assert (Q[a + j] == T[b + j]) == (code == EQ), (a + j, b + j)
            a, b = a + n, b + n
        elif code == D:
            b += n
        else:
            a += n
    return a, b, count


def levenshtein(x, y):
    """the edit distance of two sequences, two rows, no band"""
    row = list(range(len(y) + 1))
    for i in range(1, len(x) + 1):
        new = [i] + [0] * len(y)
        for j in range(1, len(y) + 1):
            new[j] = min(row[j - 1] + (x[i - 1] != y[j - 1]), row[j] + 1, new[j - 1] + 1)
        row = new
    return row[len(y)]
