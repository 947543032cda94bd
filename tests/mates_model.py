"""fmgpu_positions_mates (include/fmgpu.h) as a plain double loop over a fragment's records: the rules of the header in Python integers, no library call.  Where a
mate has hundreds of records the inner loop is the same rules over a NumPy row (_row_numpy; tests/test_mates_host.py holds the two forms against each other).
join(...) returns (pairs, off, cls): pairs as a list of (fragment, tlen, a, b, errors, flags) tuples in the call's output order."""
import numpy as np

INVALID = -1
FR, ANY = 0, 1


class MatesError(Exception):
    """what the device refuses: the array's name, the lowest offender and the kind (range, order, qoff, pos)"""

    def __init__(self, array, index, what):
        super().__init__("%s: %d: %s" % (array, index, what))
        self.code, self.array, self.index, self.what = INVALID, array, index, what


def _runs(positions, shift, reads, name, errors):
    """(first, end) per read of one array; what is out of range, out of order or too far right goes to `errors`"""
    first, end = {}, {}
    before = None
    for i, rec in enumerate(positions):
        read = int(rec["qidx"]) >> shift
        if read >= reads:
            errors.setdefault(("range", name), i)
            before = read
            continue
        if before is not None and before > read:
            errors.setdefault(("order", name), i)
        if int(rec["pos"]) >= 1 << 62:
            errors.setdefault(("pos", name), i)
        first.setdefault(read, i)
        end[read] = i + 1
        before = read
    return first, end


def concordant(pa, ma, sa, seq_a, pb, mb, sb, seq_b, orientation, min_tlen, max_tlen):
    """the template length of the pair, or None if it is not concordant"""
    ea, eb = pa + ma, pb + mb
    tlen = max(ea, eb) - min(pa, pb)
    if seq_a != seq_b or not min_tlen <= tlen <= max_tlen:
        return None
    if orientation == FR:
        if sa == sb:
            return None
        (pf, ef), (pr, er) = ((pa, ea), (pb, eb)) if sa == 0 else ((pb, eb), (pa, ea))
        if pf > pr or ef > er:
            return None
    return tlen


VECTOR_FROM = 256          # a mate B with this many records is compared by the NumPy form of the same rules (_row_numpy), a record of A at a time


def _row_numpy(f, i, pa, ma, sa, seq_a, err_a, nb, ib, mb, shift, orientation, min_tlen, max_tlen):
    """the pairs of record i of mate A with records ib of mate B: `concordant` over the whole row at once (positions below 2^62 and read lengths that fit int64)"""
    js = np.arange(ib.start, ib.stop)
    pb, seq_b = nb["pos"][js], nb["seq_id"][js]
    sb = (nb["qidx"][js] & 1) if shift else np.zeros(len(js), dtype=np.int64)
    ea, eb = pa + ma, pb + mb
    tlen = np.maximum(ea, eb) - np.minimum(pa, pb)
    ok = (seq_b == seq_a) & (tlen >= min(min_tlen, (1 << 63) - 1)) & (tlen <= min(max_tlen, (1 << 63) - 1))
    if orientation == FR:
        pf, ef, pr, er = (pa, ea, pb, eb) if sa == 0 else (pb, eb, pa, ea)
        ok &= (sb != sa) & (pf <= pr) & (ef <= er)
    js, pb, tlen = js[ok], pb[ok], tlen[ok]
    order = np.lexsort((js, pb))
    return [(f, int(tlen[k]), i, int(js[k]), (err_a + int(nb["errors"][js[k]])) & 0xffffffff, 1 if pa <= int(pb[k]) else 0) for k in order]


def join(positions_a, qoff_a, positions_b=None, qoff_b=None, n_fragments=None, strand_shift=1, interleaved=False, orientation=FR, min_tlen=0, max_tlen=1000,
         best=False, max_records=0):
    qoff_a = [int(x) for x in qoff_a]
    qoff_b = qoff_a if interleaved else [int(x) for x in qoff_b]
    if interleaved:
        positions_b = positions_a
    n = n_fragments if n_fragments is not None else (len(qoff_a) - 1) // (2 if interleaved else 1)
    reads = 2 * n if interleaved else n
    errors = {}
    first_a, end_a = _runs(positions_a, strand_shift, reads, "positions_a", errors)
    first_b, end_b = (first_a, end_a) if interleaved else _runs(positions_b, strand_shift, reads, "positions_b", errors)
    for name, q in (("qoff_a", qoff_a),) + (() if interleaved else (("qoff_b", qoff_b),)):
        for r in range(reads):
            if q[r + 1] < q[r]:
                errors.setdefault(("qoff", name), r)
                break
    for what in ("range", "order", "qoff", "pos"):
        for name in ("qoff_a", "qoff_b") if what == "qoff" else ("positions_a", "positions_b"):
            if (what, name) in errors:
                raise MatesError(name, errors[(what, name)], what)
    ca = {k: positions_a[k].tolist() for k in ("qidx", "seq_id", "pos", "errors")}                # Python integers: nothing wraps
    cb = ca if interleaved else {k: positions_b[k].tolist() for k in ("qidx", "seq_id", "pos", "errors")}
    nb = {k: np.asarray(positions_b[k]).astype(np.int64 if k != "errors" else np.uint32) for k in ("qidx", "seq_id", "pos", "errors")} if len(positions_b) else None
    pairs, off, cls = [], [], []
    for f in range(n):
        off.append(len(pairs))
        ra, rb = (2 * f, 2 * f + 1) if interleaved else (f, f)
        ia = range(first_a[ra], end_a[ra]) if ra in first_a else range(0)
        ib = range(first_b[rb], end_b[rb]) if rb in first_b else range(0)
        if not ia or not ib:
            cls.append(0 if not ia and not ib else 1 if not ib else 2)
            continue
        if max_records and (len(ia) > max_records or len(ib) > max_records):
            cls.append(5)
            continue
        found = []
        mb = qoff_b[rb + 1] - qoff_b[rb]
        for i in ia:
            pa, ma, sa = ca["pos"][i], qoff_a[ra + 1] - qoff_a[ra], ca["qidx"][i] & 1 if strand_shift else 0
            if len(ib) >= VECTOR_FROM:
                found += _row_numpy(f, i, pa, ma, sa, ca["seq_id"][i], ca["errors"][i], nb, ib, mb, strand_shift, orientation, min_tlen, max_tlen)
                continue
            mine = []
            for j in ib:
                pb, sb = cb["pos"][j], cb["qidx"][j] & 1 if strand_shift else 0
                tlen = concordant(pa, ma, sa, ca["seq_id"][i], pb, mb, sb, cb["seq_id"][j], orientation, min_tlen, max_tlen)
                if tlen is not None:
                    mine.append((pb, j, (f, tlen, i, j, (ca["errors"][i] + cb["errors"][j]) & 0xffffffff, 1 if pa <= pb else 0)))
            found += [m[2] for m in sorted(mine)]
        if best and found:
            least = min(p[4] for p in found)
            found = [p for p in found if p[4] == least]
        cls.append(4 if found else 3)
        pairs += found
    off.append(len(pairs))
    return pairs, off, cls


def as_array(pairs, dtype):
    return np.array(pairs, dtype=dtype) if pairs else np.zeros(0, dtype=dtype)
