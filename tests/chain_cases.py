"""inputs of the fmgpu_seeds_chain tests: synthetic anchor batches, and the reads of the end-to-end test with the places they were cut from"""
import numpy as np

from fmindex_collection_amd.capi import POSITION_DTYPE, SEED_SPAN_DTYPE


def run_anchors(rng, n, qidx, seq_id, base=1000):
    """n anchors of one (query, sequence) on three noisy diagonals: (qidx, seq_id, t, q, l)"""
    q = np.sort(rng.integers(0, max(8 * n, 40), n))
    d = rng.integers(0, 3, n) * 7 + rng.integers(0, 3, n)
    ln = rng.integers(12, 30, n)
    return [(qidx, seq_id, base + int(q[k]) + int(d[k]), int(q[k]), int(ln[k])) for k in range(n)]


def tandem_anchors(qidx, seq_id, seeds=20, copies=1000, period=50, length=25):
    """a read of `seeds` seeds one period apart on a tandem repeat of `copies` periods: every seed lies at every copy, ties everywhere"""
    return [(qidx, seq_id, c * period + s * period, s * period, length) for s in range(seeds) for c in range(copies)]


def pack(rows, rng=None):
    """(qidx, seq_id, t, q, l) rows -> (positions, spans): the rows of a query in a shuffled order, the spans shuffled behind `hit`"""
    rows = list(rows)
    if rng is not None:
        keys = rng.permutation(len(rows))
        rows = [rows[k] for k in sorted(range(len(rows)), key=lambda k: (rows[k][0], keys[k]))]
        where = rng.permutation(len(rows))
    else:
        where = np.arange(len(rows))
    pos, spans = np.zeros(len(rows), dtype=POSITION_DTYPE), np.zeros(len(rows), dtype=SEED_SPAN_DTYPE)
    for i, (q, s, t, qb, ln) in enumerate(rows):
        pos[i] = (q, s, t, 7, where[i])
        spans[where[i]] = (qb, ln)
    return pos, spans


COMPLEMENT = np.array([0, 4, 3, 2, 1], dtype=np.uint8)          # dna5: A C G T = 1 2 3 4
E2E_SEED = 1


def end_to_end(seed=E2E_SEED):
    """three random sequences (sigma 5, 20 000 symbols), 200 reads of 150 symbols cut from known places, each with substitutions at offsets 37, 75 and 112 and a
    deletion of two bases at offset 90, every second one reverse-complemented -> (seqs, reads, truth): truth[r] = (seq_id, start, reversed)"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, n).astype(np.uint8) for n in (8000, 7000, 5000)]
    reads, truth = [], []
    for r in range(200):
        s = int(rng.integers(0, 3))
        start = int(rng.integers(0, len(seqs[s]) - 152))
        piece = seqs[s][start: start + 152]
        read = np.concatenate([piece[:90], piece[92:]])
        for at in (37, 75, 112):
            read[at] = (read[at] - 1 + int(rng.integers(1, 4))) % 4 + 1
        rev = r % 2 == 1
        if rev:
            read = COMPLEMENT[read[::-1]]
        reads.append(read.astype(np.uint8))
        truth.append((s, start, rev))
    return seqs, reads, truth


def check_top_chains(chains, off, truth):
    """for EVERY read the top chain of its true strand lies on the true sequence, tbeg - qbeg within 2 of the true start, with at least 3 anchors; chains: rows with
    (qidx, seq_id, tbeg, tend, qbeg, qend, score, n_anchors, ...) in output order"""
    for r, (s, start, rev) in enumerate(truth):
        q = 2 * r + (1 if rev else 0)
        assert off[q + 1] > off[q], ("read %d has no chain on its true strand" % r)
        top = chains[int(off[q])]
        assert int(top[0]) == q and int(top[1]) == s and abs(int(top[2]) - int(top[4]) - start) <= 2 and int(top[7]) >= 3, (r, tuple(int(x) for x in top), s, start)
