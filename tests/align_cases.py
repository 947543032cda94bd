"""inputs of the fmgpu_chains_align tests: chains written out symbol by symbol, so that every piece is a true match and every gap is what the test asks for"""
import numpy as np

from fmindex_collection_amd.capi import CHAIN_DTYPE, POSITION_DTYPE, SEED_SPAN_DTYPE


def chain_spec(pieces, gaps, head=0, tail=0, extra=None, noise=0.2):
    """pieces: l' of every piece; gaps: (gq, gt) behind every piece but the last; head / tail: clipped read symbols; extra[k]: what anchor k's stated length exceeds
    l' by (only where its gap has gq == 0 or gt == 0, else l' would grow); noise: the share of a gap's read symbols that differ from the text's"""
    assert len(gaps) == len(pieces) - 1
    return dict(pieces=list(pieces), gaps=list(gaps), head=head, tail=tail, extra=extra or {}, noise=noise)


def build(rng, specs, sigma=4, shuffle=True, text_pad=5, empty_reads=(0,)):
    """-> dict(chains, anchors, positions, spans, qbuf, qoff, tbuf, toff, nq): one read per chain (reads without symbols in front of the chains listed in empty_reads),
    positions and spans in a shuffled order, the text windows behind text_pad unused bytes"""
    reads, windows, rows, chains = [], [], [], []
    for c, sp in enumerate(specs):
        if c in empty_reads:
            reads.append([])
        qidx, seq_id, tbeg = len(reads), int(rng.integers(0, 4)), int(rng.integers(0, 1 << 20)) + (1 << 33 if c % 3 == 2 else 0)
        Q, T, anc = [int(v) for v in rng.integers(1, sigma + 1, sp["head"])], [], []
        for k, lp in enumerate(sp["pieces"]):
            piece = [int(v) for v in rng.integers(1, sigma + 1, lp)]
            anc.append((len(Q), len(T), lp + sp["extra"].get(k, 0)))
            Q += piece
            T += piece
            if k < len(sp["gaps"]):
                gq, gt = sp["gaps"][k]
                tg = [int(v) for v in rng.integers(1, sigma + 1, gt)]
                qg = (tg + [int(v) for v in rng.integers(1, sigma + 1, max(gq - gt, 0))])[:gq]
                if gq > gt and gt:                                   # the surplus somewhere inside, not at the end
                    at = int(rng.integers(0, gt))
                    qg = qg[:at] + qg[gt:] + qg[at:gt]
                elif gt > gq and gq:
                    at = int(rng.integers(0, gq))
                    qg = tg[:at] + tg[at + gt - gq:]
                qg = [int(rng.integers(1, sigma + 1)) if rng.random() < sp["noise"] else v for v in qg]
                Q += qg
                T += tg
        qend = len(Q)
        Q += [int(v) for v in rng.integers(1, sigma + 1, sp["tail"])]
        chains.append((qidx, seq_id, tbeg, tbeg + len(T), sp["head"], qend, 0, len(anc), len(rows), 0))
        rows += [(qidx, seq_id, tbeg + t, q, l) for q, t, l in anc]
        reads.append(Q)
        windows.append(T)
    reads.append([])
    n = len(rows)
    where = rng.permutation(n) if shuffle else np.arange(n)      # anchors[i] = where[i]: the record of anchor i
    hit = rng.permutation(n) if shuffle else np.arange(n)
    positions, spans = np.zeros(n, dtype=POSITION_DTYPE), np.zeros(n, dtype=SEED_SPAN_DTYPE)
    for i, (q, s, t, qb, ln) in enumerate(rows):
        positions[where[i]] = (q, s, t, 3, hit[i])
        spans[hit[i]] = (qb, ln)
    qoff = np.zeros(len(reads) + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    toff = np.zeros(len(windows) + 1, dtype=np.uint64)
    toff[0] = text_pad
    toff[1:] = text_pad + np.cumsum([len(w) for w in windows])
    flat = lambda seqs, pad: np.array([0] * pad + [v for s in seqs for v in s] + [0], dtype=np.uint8)      # noqa: E731
    return dict(chains=np.array(chains, dtype=CHAIN_DTYPE), anchors=where.astype(np.uint32), positions=positions, spans=spans, qbuf=flat(reads, 0), qoff=qoff,
                tbuf=flat(windows, text_pad), toff=toff, nq=len(reads))


def random_specs(rng, n, max_piece=30, max_gap=12):
    """n chains of 1 .. 6 anchors with every kind of gap: none, pure I, pure D, 1 x 1, and matrices of both skews"""
    specs = []
    for _ in range(n):
        k = int(rng.integers(1, 7))
        gaps, extra = [], {}
        for j in range(k - 1):
            kind = int(rng.integers(0, 6))
            g = (0, 0) if kind == 0 else (int(rng.integers(1, max_gap)), 0) if kind == 1 else (0, int(rng.integers(1, max_gap))) if kind == 2 else (1, 1) if kind == 3 else \
                (int(rng.integers(1, max_gap)), int(rng.integers(1, max_gap)))
            gaps.append(g)
            if (g[0] == 0) != (g[1] == 0) and rng.random() < 0.5:
                extra[j] = int(rng.integers(1, 9))
        specs.append(chain_spec([int(v) for v in rng.integers(1, max_piece, k)], gaps, head=int(rng.integers(0, 3)) * 4, tail=int(rng.integers(0, 3)) * 5, extra=extra,
                                noise=float(rng.choice([0.0, 0.1, 0.5]))))
    return specs


def model_args(case):
    return (case["chains"], case["anchors"], case["positions"], case["spans"], case["qbuf"], case["qoff"], case["tbuf"], case["toff"])
