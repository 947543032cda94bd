"""fmgpu_seeds_chain (include/fmgpu.h) in plain Python: dictionaries and loops over sorted tuples, nothing shared with the library.

chain(...) is the rule as the header states it (links, then heirs).  backtrack_chains(...) is a second, independent statement of the chain extraction, the way minimap2
does it: anchors by descending f, each unused one backtracked to the first used anchor.  Without ties in f the two give the same chains (tests/test_chain_host.py)."""

INVALID, UNSUPPORTED, CAPACITY = -1, -2, -5
POS_LIMIT, SPAN_LIMIT, RECORD_LIMIT = 1 << 62, 1 << 31, (1 << 32) - 256
CLS_NONE, CLS_CHAINED, CLS_FILTERED, CLS_SKIPPED = 0, 1, 2, 3


class ChainError(Exception):
    def __init__(self, code, index, what):
        super().__init__("record %s: %s" % (index, what))
        self.code, self.index, self.what = code, index, what


def _rows(positions):
    """[(qidx, seq_id, pos, hit)] of a structured array or of (qidx, seq_id, pos, errors, hit) tuples"""
    if hasattr(positions, "dtype") and positions.dtype.names:
        return [(int(r["qidx"]), int(r["seq_id"]), int(r["pos"]), int(r["hit"])) for r in positions]
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[4])) for r in positions]


def _spans(spans):
    if hasattr(spans, "dtype") and spans.dtype.names:
        return [(int(s["qbeg"]), int(s["qlen"])) for s in spans]
    return [(int(s[0]), int(s[1])) for s in spans]


def check(rows, spans, nq):
    """what the device refuses: the kinds in the header's order, of each kind the lowest record"""
    kinds = {"range": [], "order": [], "hit": [], "pos": [], "span": []}
    for i, (q, _, pos, hit) in enumerate(rows):
        if q >= nq:
            kinds["range"].append(i)
            continue                                                   # (a record beyond the batch is not looked at further)
        if i and rows[i - 1][0] > q:
            kinds["order"].append(i)
        if hit >= len(spans):
            kinds["hit"].append(i)
        elif spans[hit][1] == 0 or spans[hit][0] + spans[hit][1] >= SPAN_LIMIT:
            kinds["span"].append(i)
        if pos >= POS_LIMIT:
            kinds["pos"].append(i)
    for what in ("range", "order", "hit", "pos", "span"):
        if kinds[what]:
            raise ChainError(INVALID, kinds[what][0], what)


def gain_of(ti, qi, li, tj, qj, max_gap, max_skew, gap_cost_q8):
    """the gain of linking anchor i behind candidate j, or None"""
    dt, dq = ti - tj, qi - qj
    if dt < 1 or dq < 1 or dt > max_gap or dq > max_gap or abs(dt - dq) > max_skew:
        return None
    gain = min(li, dq, dt) - ((gap_cost_q8 * abs(dt - dq)) >> 8)
    return gain if gain >= 1 else None


def links(run, max_gap, max_skew, gap_cost_q8, max_lookback):
    """f and p over one run: run = [(t, q, l, index)] in the order; p holds places in the run or None"""
    f, p = [], []
    for i, (ti, qi, li, _) in enumerate(run):
        best, source = li, None
        for j in range(i - 1, max(i - max_lookback, 0) - 1, -1):      # nearest first
            g = gain_of(ti, qi, li, run[j][0], run[j][1], max_gap, max_skew, gap_cost_q8)
            if g is not None and f[j] + g > best:                      # an equal value further away does not replace a nearer one; a value of l_i does not link
                best, source = f[j] + g, j
        f.append(best)
        p.append(source)
    return f, p


def heir_chains(f, p):
    """the chains of one run by the header's rule: [(score, [places], branch)] in the order of their first places"""
    n = len(f)
    children = {j: [] for j in range(n)}
    for i in range(n):
        if p[i] is not None:
            children[p[i]].append(i)
    t = list(f)
    for j in range(n - 1, -1, -1):                                     # children lie behind their parent
        for c in children[j]:
            t[j] = max(t[j], t[c])
    heir = {}
    for j in range(n):
        for c in children[j]:                                          # ascending places: the earliest of the largest t
            if j not in heir or t[c] > t[heir[j]]:
                heir[j] = c
    out = []
    for s in range(n):
        if p[s] is not None and heir[p[s]] == s:
            continue
        places = [s]
        while places[-1] in heir:
            places.append(heir[places[-1]])
        score = f[places[-1]] - (f[p[s]] if p[s] is not None else 0)
        out.append((score, places, p[s] is not None))
    return out


def backtrack_chains(f, p):
    """the second statement: anchors by descending f; each unused one is an end, backtracked through p until a used anchor"""
    used = set()
    out = []
    for end in sorted(range(len(f)), key=lambda i: (-f[i], i)):
        if end in used:
            continue
        places, at = [], end
        while at is not None and at not in used:
            places.append(at)
            used.add(at)
            at = p[at]
        places.reverse()
        out.append((f[end] - (f[at] if at is not None else 0), places, at is not None))
    return sorted(out, key=lambda c: c[1][0])


def chain(positions, spans, nq, max_gap=5000, max_skew=500, gap_cost_q8=128, max_lookback=64, min_score=0, min_anchors=1, max_chains=0, max_anchors=0,
          extract=heir_chains):
    """-> (chains, off, cls, anchors): chains = [(qidx, seq_id, tbeg, tend, qbeg, qend, score, n_anchors, first, flags)] in output order"""
    rows, spans = _rows(positions), _spans(spans)
    if len(rows) >= RECORD_LIMIT or len(spans) >= RECORD_LIMIT:
        raise ChainError(UNSUPPORTED, None, "count")
    if nq == 0 or not rows:
        return [], [0] * (nq + 1), [0] * nq, []
    check(rows, spans, nq)
    per_query = {}
    for i, (q, seq, pos, hit) in enumerate(rows):
        per_query.setdefault(q, []).append((seq, pos, spans[hit][0], i, spans[hit][1]))
    chains, off, cls, anchors = [], [0], [], []
    for q in range(nq):
        mine = sorted(per_query.get(q, []))                            # (seq_id, t, q, index): the order
        if not mine:
            cls.append(CLS_NONE)
        elif max_anchors and len(mine) > max_anchors:
            cls.append(CLS_SKIPPED)
        else:
            found = []
            base = 0
            while base < len(mine):
                end = base
                while end < len(mine) and mine[end][0] == mine[base][0]:
                    end += 1
                run = [(t, qb, l, i) for _, t, qb, i, l in mine[base:end]]
                f, p = links(run, max_gap, max_skew, gap_cost_q8, max_lookback)
                for score, places, branch in extract(f, p):
                    if score >= min_score and len(places) >= max(min_anchors, 1):
                        first, last = run[places[0]], run[places[-1]]
                        found.append((-score, base + places[0], (q, mine[base][0], first[0], last[0] + last[2], first[1], last[1] + last[2], score, len(places)),
                                      1 if branch else 0, [run[k][3] for k in places]))
                base = end
            found.sort(key=lambda c: (c[0], c[1]))
            if max_chains:
                found = found[:max_chains]
            for _, _, head, flags, idx in found:
                chains.append(head + (len(anchors), flags))
                anchors += idx
            cls.append(CLS_CHAINED if found else CLS_FILTERED)
        off.append(len(chains))
    return chains, off, cls, anchors
