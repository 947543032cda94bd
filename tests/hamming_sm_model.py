"""A plain-Python restatement of the walk of fmgpu_search_hamming_sm (include/fmgpu.h), written from that text, on the cursor steps of fmoracle.OraIndex, and a
brute-force scorer over the delimiter-joined text.  There is no live reference for this search: the two keep each other honest (tests/test_hamming_sm_host.py) and
are the oracle of tests/test_gpu_hamming_sm.py."""
import numpy as np

UINT64_MAX = (1 << 64) - 1


def members(mask):
    """the text symbols of a mask word, ascending"""
    return [r for r in range(32) if (int(mask) >> r) & 1]


def part_lengths(P, m, partition=None):
    """createUniformPartition(P, m), or the explicit partition if it covers the read exactly (else None: the read is skipped)"""
    if partition is not None:
        part = [int(x) for x in partition]
        return part if sum(part) == m else None
    return [m // P + (1 if p < m % P else 0) for p in range(P)]


class _Done(Exception):
    pass


def walk_read(ox, read, scheme, free_mask, cost_mask, partition=None, n=UINT64_MAX):
    """one read: ([(lb, lb_rev, len, errors)] in callback order, with the clipping of search_n; the extensions the reference executes)"""
    pi, l, u = (np.asarray(x).astype(np.int64).tolist() for x in scheme)
    S, P = len(pi), len(pi[0]) if len(pi) else 0
    m = len(read)
    recs, steps = [], [0]
    if n == 0 or S == 0 or m < P or ox.n == 0:
        return recs, 0
    lens = part_lengths(P, m, partition)
    if lens is None:
        return recs, 0
    starts = [sum(lens[:p]) for p in range(P)]
    qsig = len(free_mask)
    F = [members(x) for x in free_mask]
    K = [members(x) for x in cost_mask]
    left = [n]

    def report(cur, e):
        ln = min(int(cur.len), left[0])
        left[0] -= ln
        recs.append((int(cur.lb), int(cur.lb_rev), ln, e))
        if left[0] == 0:
            raise _Done

    def enter(s, cur, e, p):
        if p == P:
            if l[s][P - 1] <= e <= u[s][P - 1]:
                report(cur, e)
            return
        if e > u[s][p]:
            return
        lo = starts[pi[s][p]]
        step(s, cur, e, p, lo, lo + lens[pi[s][p]], p == 0 or pi[s][p - 1] < pi[s][p])

    def step(s, cur, e, p, lo, hi, right):
        if lo == hi:
            if l[s][p] <= e:
                enter(s, cur, e, p + 1)
            return
        c = int(read[lo] if right else read[hi - 1])
        f, k = (F[c], K[c]) if c < qsig else ([], [])
        nlo, nhi = (lo + 1, hi) if right else (lo, hi - 1)
        if e + 1 <= u[s][p]:
            steps[0] += 1
            kids = ox.extend_right_all(cur) if right else ox.extend_left_all(cur)
            for r in f:
                if kids[r].len:
                    step(s, kids[r], e, p, nlo, nhi, right)
            for r in k:
                if kids[r].len:
                    step(s, kids[r], e + 1, p, nlo, nhi, right)
        else:
            steps[0] += len(f)
            for r in f:
                kid = ox.extend_right(cur, r) if right else ox.extend_left(cur, r)
                if kid.len:
                    step(s, kid, e, p, nlo, nhi, right)

    try:
        for s in range(S):
            enter(s, ox.cursor(), 0, 0)
    except _Done:
        pass
    return recs, steps[0]


def walk(ox, reads, scheme, free_mask, cost_mask, partition=None, n=UINT64_MAX):
    """a batch: ([(qidx, lb, lb_rev, len, errors, seq)] in callback order, the step count)"""
    out, steps = [], 0
    for q, read in enumerate(reads):
        recs, st = walk_read(ox, read, scheme, free_mask, cost_mask, partition, n)
        steps += st
        out += [(q, lb, lr, ln, e, seq) for seq, (lb, lr, ln, e) in enumerate(recs)]
    return out, steps


def joined(seqs):
    """the text the index is built over: every sequence followed by one delimiter 0; and per text position its (seq_id, pos)"""
    text = np.concatenate([np.concatenate([np.asarray(s, dtype=np.uint8), np.zeros(1, dtype=np.uint8)]) for s in seqs])
    sid = np.concatenate([np.full(len(s) + 1, i, dtype=np.int64) for i, s in enumerate(seqs)])
    pos = np.concatenate([np.arange(len(s) + 1, dtype=np.int64) for s in seqs])
    return text, sid, pos


def brute(seqs, reads, free_mask, cost_mask, min_errors, max_errors):
    """{(qidx, seq_id, pos, errors)}: every window of the joined text that the masks pair with the read at min_errors .. max_errors errors"""
    text, sid, pos = joined(seqs)
    big = 1 << 20
    score = np.full((256, 32), big, dtype=np.int64)
    for c in range(len(free_mask)):
        for r in members(free_mask[c]):
            score[c, r] = 0
        for r in members(cost_mask[c]):
            score[c, r] = 1
    out = set()
    for q, read in enumerate(reads):
        m = len(read)
        if m == 0 or m > len(text):
            continue
        tot = np.zeros(len(text) - m + 1, dtype=np.int64)
        for j in range(m):
            tot += score[int(read[j])][text[j: len(text) - m + 1 + j]]
        for at in np.nonzero((tot >= min_errors) & (tot <= max_errors))[0]:
            out.add((q, int(sid[at]), int(pos[at]), int(tot[at])))
    return out


def located(ox, recs):
    """{(qidx, seq_id, pos, errors)} of model records, through the oracle's locate"""
    out = set()
    for q, lb, _, ln, e, _ in recs:
        for row in range(lb, lb + ln):
            s, p, st = ox.locate(row)
            out.add((q, s, p + st, e))
    return out
