"""Models of the both-strand calls (include/fmgpu.h: fmgpu_queries_strands, fmgpu_search_best_pairs): the doubled batch as a plain Python double loop, the example's
reverse-complement rule, and the pair ladder composed from per-stratum record sets.  Pure NumPy / Python: no device, no library call."""
import numpy as np

from fmindex_collection_amd.capi import HIT_DTYPE


def both_strands_loops(reads, complement):
    """the doubled batch of a list of reads, symbol by symbol: read 2q = read q, read 2q + 1 = read q reversed, a byte c < len(complement) as complement[c], any other
    byte as it is -> (qbuf, qoff)"""
    out, off = [], [0]
    for r in reads:
        for c in r:
            out.append(int(c))
        off.append(len(out))
        for k in range(len(r) - 1, -1, -1):
            c = int(r[k])
            out.append(int(complement[c]) if c < len(complement) else c)
        off.append(len(out))
    return np.array(out, dtype=np.uint8), np.array(off, dtype=np.uint64)


def example_reverse_complement(read):
    """the example's host rule for the rank alphabet $ A C G T N (0 .. 5): A <-> T, C <-> G, every other rank stays"""
    swap = {1: 4, 2: 3, 3: 2, 4: 1}
    return [swap.get(int(c), int(c)) for c in reversed(list(read))]


def pair_ladder(nq, n_strata, search):
    """The pair ladder over a batch of nq reads (nq even; reads 2j and 2j + 1 are a pair).  search(i, reads) -> the HIT_DTYPE records stratum i's single-scheme call
    produces for the sub-batch `reads` (an ascending array of read numbers), qidx numbering that sub-batch.  Stratum i searches the reads of the pairs no earlier
    stratum found, in batch order; a pair is found when either of its reads has a record with len > 0.  -> (records in stratum order, qidx in the batch; stratum per
    read, both entries of a found pair alike, 255 = unfound; the number of reads every stratum searched)"""
    assert nq % 2 == 0
    alive = list(range(nq // 2))
    stratum = np.full(nq, 255, dtype=np.uint8)
    out, searched = [], []
    for i in range(n_strata):
        reads = np.array([r for j in alive for r in (2 * j, 2 * j + 1)], dtype=np.int64)
        if reads.size == 0:
            break
        searched.append(int(reads.size))
        rec = np.array(search(i, reads), dtype=HIT_DTYPE).copy()
        rec["qidx"] = reads[rec["qidx"].astype(np.int64)]
        out.append(rec)
        found = {int(q) >> 1 for q in rec["qidx"][rec["len"] > 0]}
        for j in found:
            stratum[2 * j] = stratum[2 * j + 1] = i
        alive = [j for j in alive if j not in found]
    return (np.concatenate(out) if out else np.zeros(0, dtype=HIT_DTYPE)), stratum, searched


def independent_ladder(nq, n_strata, search):
    """fmgpu_search_best's rule with the same `search`: every read on its own -> (records, stratum, reads searched per stratum)"""
    alive = list(range(nq))
    stratum = np.full(nq, 255, dtype=np.uint8)
    out, searched = [], []
    for i in range(n_strata):
        reads = np.array(alive, dtype=np.int64)
        if reads.size == 0:
            break
        searched.append(int(reads.size))
        rec = np.array(search(i, reads), dtype=HIT_DTYPE).copy()
        rec["qidx"] = reads[rec["qidx"].astype(np.int64)]
        out.append(rec)
        found = {int(q) for q in rec["qidx"][rec["len"] > 0]}
        for q in found:
            stratum[q] = i
        alive = [q for q in alive if q not in found]
    return (np.concatenate(out) if out else np.zeros(0, dtype=HIT_DTYPE)), stratum, searched


def callback_order(records):
    """records whose reads each come from one stratum, in fmgpu_hits_sort's order: ascending qidx, inside a read the order the stratum reported (seq)"""
    return records[np.lexsort((records["seq"], records["qidx"]))]


def table_search(per_stratum):
    """a `search` from hand-made tables: per_stratum[i][read] = the list of (lb, len, errors) that stratum i reports for that read of the batch"""
    def search(i, reads):
        rows = []
        for sub, q in enumerate(reads.tolist()):
            for seq, (lb, ln, err) in enumerate(per_stratum[i].get(q, [])):
                rows.append((sub, lb, 0, ln, err, seq))
        return np.array(rows, dtype=HIT_DTYPE)
    return search
