"""Collections and read sets that stand on the delimiter-row lists of Formats P, D and C (tests/listed_rows_model.py): many sequences, their delimiter rows next to
each other in one line or block, the lists filled to their last slot and one past it.  Shared by tests/test_listed_rows_host.py (which shows on the CPU that these
inputs tell a broken correction from a working one) and tests/test_gpu_listed_rows.py.  Everything is seeded; nothing here touches a device."""
import functools

import numpy as np

import fmoracle as fo
from tests.listed_rows_model import ListedRows

RATE = 4                                  # sampling rate of the small indices: a parked read jumps 4 symbols per chain entry
SMALL = ("clustered", "cap", "cap+1", "mixed")
OVERHANGS = ((1,), (1, 1), (1, 1, 1), (2, 1), (1, 2))          # "A", "AA", "AAA", "CA", "AC"
OVERHANG_NAMES = ("A", "AA", "AAA", "CA", "AC")
FAMILIES = ("windows", "thresholds", "a_runs", "whole") + tuple("overhang_front:" + o for o in OVERHANG_NAMES) + tuple("overhang_behind:" + o for o in OVERHANG_NAMES) + ("cluster",)


def _u8(v):
    return np.asarray(v, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def sequences(name):
    if name == "clustered":
        # copies of one 85 %-'A' sequence (all their whole-sequence suffixes on adjacent rows: a line with > 100 listed rows, a block of 64 delimiter rows), truncated
        # copies, empty sequences (delimiters on rows 0, 1, 2 ...), one-symbol ones, and unique sequences whose long reads reach one row and park
        rng = np.random.default_rng(101)
        base = np.where(rng.random(300) < 0.85, 1, rng.integers(2, 5, size=300)).astype(np.uint8)
        seqs = [base.copy() for _ in range(190)]
        for _ in range(30):
            a, b = sorted(int(v) for v in rng.integers(0, 301, size=2))
            seqs.append(base[a: max(b, a + 1)].copy())
        seqs += [_u8([]) for _ in range(20)] + [_u8([c]) for c in (1, 1, 1, 2, 3, 4)]
        seqs += [rng.integers(1, 5, size=2000, dtype=np.uint8) for _ in range(10)]
        assert len(seqs) == 256
        return tuple(seqs[i] for i in rng.permutation(len(seqs)))
    if name in ("cap", "cap+1"):
        rng = np.random.default_rng(103)
        lens = [1, 1, 1, 2, 2, 3, 5, 7, 11, 15, 16, 32, 48, 64, 160, 320, 592, 600] + [int(v) for v in rng.integers(17, 600, size=256 - 18)]
        seqs = [rng.integers(1, 5, size=m, dtype=np.uint8) for m in lens]
        seqs = [seqs[i] for i in rng.permutation(256)]
        if name == "cap+1":
            seqs.append(rng.integers(1, 5, size=77, dtype=np.uint8))
        return tuple(seqs)
    if name == "mixed":
        rng = np.random.default_rng(107)
        seqs = [rng.integers(1, 5, size=int(rng.integers(1, 500)), dtype=np.uint8) for _ in range(200)] + [_u8([]) for _ in range(57)]
        return tuple(seqs[i] for i in rng.permutation(len(seqs)))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle(name, bidirectional=False):
    return fo.OraIndex.build("IB16", 5, list(sequences(name)), RATE, bidirectional)


def bwt_of(string):
    """the symbols of an oracle string, from its ranks"""
    n = string.size()
    rs, _ = string.all_ranks_rows(np.arange(n + 1, dtype=np.uint64))
    return np.argmax(rs[1:] != rs[:-1], axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model(name, corrections=True):
    ox = oracle(name, True)
    return ListedRows(bwt_of(ox.bwt_string()), bwt_of(ox.bwt_string(rev=True)), corrections=corrections)


def _subst(r, rng):
    r = r.copy()
    j = int(rng.integers(0, len(r)))
    r[j] = r[j] % 4 + 1
    return r


def exact_families(seqs, seed, windows=600):
    """{family: [reads]} of section (a): symbols 1..4 only, but for the delimiter inside the reads of the family `cluster`"""
    rng = np.random.default_rng(seed)
    long_ = [s for s in seqs if len(s) >= 140]
    longest = sorted(seqs, key=len)[-10:]
    fam = {f: [] for f in FAMILIES}

    def window(m, pool):
        s = pool[int(rng.integers(0, len(pool)))]
        p = int(rng.integers(0, len(s) - m + 1))
        return s[p: p + m].copy()

    for i in range(windows):
        r = window(int(rng.integers(8, 141)), long_)
        fam["windows"].append(_subst(r, rng) if i % 3 == 0 else r)
    for m in (46, 47, 48, 49, 50, 126, 127, 128, 129, 130):      # the park threshold (32 + 16 symbols) and the 127-symbol query window
        for i in range(12):
            r = window(m, longest if i % 2 else long_)
            fam["thresholds"].append(_subst(r, rng) if i % 4 == 3 else r)
    fam["a_runs"] = [np.ones(k, dtype=np.uint8) for k in range(1, 41)]
    fam["whole"] = [s.copy() for s in seqs if len(s)]
    able = [s for s in seqs if len(s) >= 20]
    texts = set(s.tobytes() for s in seqs)
    for i in range(60):
        for over, oname in zip(OVERHANGS, OVERHANG_NAMES):
            for front in (True, False):
                while True:                                          # (on a text of 85 % 'A' some overhangs spell what another sequence holds: those are no overhang reads)
                    s = able[int(rng.integers(0, len(able)))]
                    m = min(len(s), int(rng.integers(20, 101)))
                    r = np.concatenate([_u8(over), s[:m]]) if front else np.concatenate([s[len(s) - m:], _u8(over)])
                    if not any(r.tobytes() in t for t in texts):
                        break
                fam[("overhang_front:" if front else "overhang_behind:") + oname].append(r)
    # "AA" in front of a whole sequence (or of all but its first symbol), its delimiter and the first symbols of the sequence behind it: among the copies of one
    # sequence these intervals end INSIDE the run of adjacent listed rows, where an end has dozens of them below it in its line
    top = max(set(s.tobytes() for s in seqs if len(s) >= 100), key=lambda b: sum(1 for s in seqs if s.tobytes() == b))
    at = [i for i, s in enumerate(seqs) if s.tobytes() == top and i + 1 < len(seqs)]
    if len(at) >= 50:
        for i in at[:: max(1, len(at) // 24)]:
            behind = [seqs[j] for j in range(i + 1, min(i + 4, len(seqs)))]
            text = np.concatenate([np.concatenate([s, _u8([0])]) for s in behind])
            ends = np.cumsum([len(s) + 1 for s in behind])
            cuts = sorted(set([0, 1, 2, 3, 5] + [int(e) + d for e in ends[:2] for d in (0, 1, 2, 4)]))
            for t in (0, 1):
                for j in cuts:
                    fam["cluster"].append(np.concatenate([_u8([1, 1]), seqs[i][t:], _u8([0]), text[:j]]))
    return fam


@functools.lru_cache(maxsize=None)
def exact_reads(name):
    """(reads in one shuffled batch, the family of each)"""
    fam = exact_families(sequences(name), seed=211 + SMALL.index(name))
    reads = [r for f in FAMILIES for r in fam[f]]
    label = [f for f in FAMILIES for _ in fam[f]]
    order = np.random.default_rng(223).permutation(len(reads))
    return tuple(reads[i] for i in order), tuple(label[i] for i in order)


@functools.lru_cache(maxsize=None)
def foreign_reads(name):
    """reads with a delimiter or a byte >= 5 inside: no reference value for the latter, compared between kernels"""
    rng = np.random.default_rng(227)
    reads, _ = exact_reads(name)
    out = []
    for r in reads[:: max(1, len(reads) // 120)]:
        if len(r) >= 4:
            for byte in (0, 5, 255):
                q = r.copy()
                q[int(rng.integers(0, len(q)))] = byte
                out.append(q)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def lean_reads(name, length, k):
    """section (b): an equal-length batch with 0 .. k + 1 substitutions, the overhang family with 'A's in both directions among them"""
    rng = np.random.default_rng(229 + length + k)
    seqs = sequences(name)
    pool = [s for s in seqs if len(s) >= length]
    out = []
    for i in range(120 if name == "clustered" else 300):
        s = pool[int(rng.integers(0, len(pool)))] if i % 2 else pool[-1 - i % min(10, len(pool))]
        p = int(rng.integers(0, len(s) - length + 1))
        r = s[p: p + length].copy()
        for _ in range(i % (k + 2)):
            r = _subst(r, rng)
        out.append(r)
    for i in range(60):
        s = pool[int(rng.integers(0, len(pool)))]
        a = 1 + i % 3
        out.append(np.concatenate([np.ones(a, dtype=np.uint8), s[: length - a]]))
        out.append(np.concatenate([s[len(s) - (length - a):], np.ones(a, dtype=np.uint8)]))
    return tuple(out[i] for i in rng.permutation(len(out)))


@functools.lru_cache(maxsize=None)
def walk(name):
    """the model over the exact reads of a collection, with and without the corrections: per read (lb, len, steps) in pair steps, and in one-symbol steps on Format D
    in both directions (the reads of symbols 1..4 only); the events of the walk WITH corrections"""
    mo, mb = model(name), model(name, False)
    mo.clear_events()
    reads, label = exact_reads(name)
    clean = [i for i, r in enumerate(reads) if len(r) and 1 <= int(r.min()) and int(r.max()) <= 4]
    out = {"reads": reads, "label": label, "clean": clean}
    for tag, m in (("fixed", mo), ("broken", mb)):
        out[tag] = {"pairs": [m.search_pairs(r) for r in reads], "dense": {rev: {i: m.search_dense(reads[i], rev) for i in clean} for rev in (False, True)}}
    out["events_p"] = mo.pair_events()
    out["events_d"] = {rev: mo.dense_events(rev) for rev in (False, True)}
    return out


SHOWN_OVERHANGS = ("overhang_front:A", "overhang_front:AA", "overhang_behind:A", "overhang_behind:AA", "overhang_behind:AAA")


def overhang_hits_without_corrections(name):
    """(overhang reads of the kinds that can show it, those of them that are a hit without the lists).  A front overhang is prepended across the delimiter row of bwt — "AA"
    by a pair step on Format P, "A" by a one-symbol step on Format D — and an overhang behind is appended across the delimiter row of bwtRev: Format D in the other
    direction.  "CA" and "AC" take a step with another symbol from the wrong row the uncorrected step gave, and so does the third 'A' in front: they miss either way."""
    w = walk(name)
    total = hit = 0
    for i, f in enumerate(w["label"]):
        if f in SHOWN_OVERHANGS:
            total += 1
            b = w["broken"]
            hit += (b["pairs"][i][1] > 0 or b["dense"][False][i][1] > 0) if f.startswith("overhang_front") else b["dense"][True][i][1] > 0
    return total, hit


@functools.lru_cache(maxsize=None)
def check_coverage(name):
    """the conditions on the inputs (on the model's counters, no device involved): what makes a pass of the device tests mean something"""
    w, mo = walk(name), model(name)
    ev = w["events_p"]
    over = [i for i, f in enumerate(w["label"]) if f.startswith("overhang")]
    assert len(over) >= 500 and all(w["fixed"]["pairs"][i][1] == 0 for i in over)                      # every overhang read is a miss
    if name == "clustered":
        # (on the other collections a fifth of the blocks holds a delimiter: the walk without the lists goes wrong before it reaches the overhang)
        total, hit = overhang_hits_without_corrections(name)
        assert total >= 300 and hit >= 0.9 * total, (name, total, hit)
        c = ev["correction"]
        assert (c >= 1).sum() >= 1000 and (c >= 8).sum() >= 100 and (c >= 64).sum() >= 10, (name, (c >= 1).sum(), (c >= 8).sum(), (c >= 64).sum())
        assert ev["on_listed"].sum() >= 20 and ((ev["row"] & 127 == 0) & ev["flagged"]).sum() >= 20
        for rev in (False, True):
            c = w["events_d"][rev]["correction"]
            assert (c >= 1).sum() >= 500 and (c >= 8).sum() >= 50, (name, rev, (c >= 1).sum(), (c >= 8).sum())
    if name == "cap":
        assert len(mo.pairs_ex) == 512 and len(mo.dense[0]["ex"]) == 256 and len(mo.dense[1]["ex"]) == 256
        last = mo.pairs_ex[-1]
        assert ((ev["row"] > last) & (ev["row"] >> 7 == last >> 7)).any()                               # a correction scan runs to the list's last slot
        for rev in (False, True):
            e, last = w["events_d"][rev], mo.dense[int(rev)]["ex"][-1]
            assert ((e["row"] > last) & (e["row"] >> 6 == last >> 6)).any()


# ---------------------------------------------------------------------------------------------------------------- more lines / blocks than the filters have bits
# The kernels' filters hold 32 768 bits: line number mod 32 768 (Format P: it wraps at 4 194 304 rows), block number mod 32 768 (Format D: 2 097 152 rows).  On these two
# collections a line or block is flagged through the listed rows of ANOTHER one, 32 768 lines or blocks away, and the scan of the list must then find nothing.  The index
# is built on the device; the model stands on the BWT it built, and the reads are aimed with it: the text behind row r, read off the BWT (psi), is a read whose walk
# arrives at the one-row interval [r, r + 1) — with 'A's in front of it the next step is an "AA" / 'A' step with both ends in r's line or block.
ALIASED = {"aliased_p": (256, 17_200), "aliased_d": (256, 9_000)}       # sequences x symbols: 4 403 456 and 2 304 256 rows


@functools.lru_cache(maxsize=None)
def aliased_sequences(name):
    count, length = ALIASED[name]
    rng = np.random.default_rng(307 + len(name))
    return tuple(rng.integers(1, 5, size=length, dtype=np.uint8) for _ in range(count))


def _aimed_rows(flag, has, ex, shift, per_unit, rng):
    """(rows in lines / blocks that are flagged only through an alias, rows right above a listed row in its own line / block)"""
    size = 1 << shift
    units = np.nonzero(flag[np.arange(len(has)) % len(flag)] & ~has)[0]
    alias = [int(u) * size + int(o) for u in units for o in rng.choice(size - 1, size=per_unit, replace=False)]      # (not the last row: r + 1 stays in the line)
    true = [int(e) + d for e in ex for d in (1, 2) if (int(e) & (size - 1)) + d < size - 1]
    return alias, true


def _bulk(seqs, count, lengths, rng, every=3):
    out = []
    for i in range(count):
        s = seqs[int(rng.integers(0, len(seqs)))]
        m = int(lengths[i % len(lengths)])
        p = int(rng.integers(0, len(s) - m + 1))
        out.append(_subst(s[p: p + m], rng) if i % every == 0 else s[p: p + m].copy())
    return out


def aliased_p_reads(mo, seqs):
    """(the exact batch: at most 5 000 reads, shuffled; the indices of the aimed ones).  n rows from a device-built BWT"""
    rng = np.random.default_rng(311)
    alias, true = _aimed_rows(mo.pair_flag, mo.pair_line_listed, mo.pairs_ex, 7, 16, rng)
    aimed = []
    for r in alias + true[:200]:
        if r < mo.n:
            tail = mo.fw.text_at(r, int(rng.integers(20, 101)))
            if tail is not None:
                aimed.append(np.concatenate([_u8([1, 1]), tail]))
    bulk = _bulk(seqs, 2400, list(range(8, 141)), rng) + _bulk(seqs, 240, [46, 47, 48, 49, 50, 126, 127, 128, 129, 130], rng, every=4)
    bulk += [np.ones(k, dtype=np.uint8) for k in range(1, 41)]
    reads = aimed + bulk
    assert len(reads) <= 5000
    order = rng.permutation(len(reads))
    where = np.argsort(order)
    return [reads[i] for i in order], [int(where[i]) for i in range(len(aimed))]


def check_aliased_p(mo, reads, aimed):
    """the coverage conditions of the wrapped Format P filter, on the walk of the aimed reads"""
    assert mo.n > 4_194_304 + 128 * 1000 and len(mo.pairs_ex) == 2 * ALIASED["aliased_p"][0]
    mo.clear_events()
    for i in aimed:
        mo.search_pairs(reads[i])
    ev = mo.pair_events()
    figures = (int(ev["alias"].sum()), int(((ev["correction"] >= 1)).sum()), int(ev["flagged"].sum()), len(ev["row"]))
    assert figures[0] >= 100 and figures[1] >= 20, figures
    assert not (ev["alias"] & (ev["correction"] > 0)).any()
    return figures


def aliased_d_reads(mo, seqs, length):
    """an equal-length batch of at most 250 reads: aimed at the aliased blocks of bwt ('A' in front) and of bwtRev ('A' behind), and windows with 0 .. 2 substitutions"""
    rng = np.random.default_rng(313 + length)
    out, aimed = [], []
    for rev in (False, True):
        d = mo.dense[int(rev)]
        alias, true = _aimed_rows(d["flag"], d["block_listed"], d["ex"], 6, 2, rng)
        rows = [alias[i] for i in rng.permutation(len(alias))[:60]] + true[:10]
        for r in rows:
            tail = d["string"].text_at(r, length - 1) if r < mo.n else None
            if tail is not None:
                aimed.append((len(out), rev))
                out.append(np.concatenate([tail[::-1], _u8([1])]) if rev else np.concatenate([_u8([1]), tail]))
    for i, r in enumerate(_bulk(seqs, 100, [length], rng, every=1)):
        out.append(r if i % 3 == 0 else (_subst(r, rng) if i % 3 == 2 else _bulk(seqs, 1, [length], rng, every=2)[0]))
    assert len(out) <= 250 and all(len(r) == length for r in out)
    return out, aimed


def check_aliased_d(mo, batches):
    """batches: [(reads, aimed)] — the coverage conditions of the wrapped Format D filter, per direction, on the exact walk of the aimed reads"""
    assert mo.n > 2_097_152 + 64 * 1000 and len(mo.dense[0]["ex"]) == len(mo.dense[1]["ex"]) == ALIASED["aliased_d"][0]
    mo.clear_events()
    for reads, aimed in batches:
        for i, rev in aimed:
            mo.search_dense(reads[i], rev)
    figures = []
    for rev in (False, True):
        ev = mo.dense_events(rev)
        figures.append((int(ev["alias"].sum()), int((ev["correction"] >= 1).sum()), len(ev["row"])))
        assert figures[-1][0] >= 100, (rev, figures)
        assert not (ev["alias"] & (ev["correction"] > 0)).any()
    return figures
