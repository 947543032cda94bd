"""fmgpu_search_best / _ng21 / _q4: a ladder of schemes walked over one batch on the device, against the CPU oracle composed per stratum (search the reads still
unfound, drop those with a len > 0 record, map qidx back).  The library's own single-scheme calls are never the ground truth.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import fmoracle as fo
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import HIT_DTYPE
from tests.util import make_text, sample_reads, oracle_arrays

pytestmark = pytest.mark.gpu
HIT_KEYS = ("qidx", "lb", "lb_rev", "len", "errors")
UNLIMITED = fm.UINT64_MAX
SIGMA = 5

# FOREIGN READS.  The batch holds a read of 24 x symbol 7 on a sigma = 5 index.  The CPU oracle indexes its rank tables and its extend-all array by the query symbol, so what
# it returns for that read depends on what lies behind those arrays: its node count for the same one-read call was measured as 1 in one process and 2 in another.  The
# ground truth for such a read is therefore reasoned, not taken from the oracle: no row of the text holds the symbol, so it has no record and stays unfound; every search
# of every scheme used here begins with a step whose upper bound is 0 (asserted), so each search extends the empty pattern once by the foreign symbol, gets the empty
# interval and ends: n_searches nodes per stratum (what the oracle counts whenever its out-of-range reads return zeros).  Every other read goes to the oracle.


def gpu_index(ox):
    return fm.BiFMIndex.from_reference_arrays(**oracle_arrays(ox))


@pytest.fixture(scope="module")
def world():
    """135 reads: the count is no multiple of 64, the lengths fall below, at and above one 16-byte gather chunk"""
    base = make_text(1200, 5, seed=7)
    seqs = [np.concatenate([base, base[200:500]]), make_text(300, 5, seed=8)]
    ox = fo.OraIndex.build("IB16", 5, seqs, 4, True)
    reads = list(sample_reads(seqs[0], 131, 24, seed=11, mutate=3))
    reads += [np.zeros(0, dtype=np.uint8), np.array([1, 2, 3, 4, 1], dtype=np.uint8), make_text(40, 5, seed=99), np.full(24, 7, dtype=np.uint8)]
    assert len(reads) == 135
    return {"ox": ox, "gx": gpu_index(ox), "reads": reads, "oracle": {}}


def ladder_of(kind):
    if kind == "ng21":
        return [fm.search_scheme.expand(fm.search_scheme.pigeon_opt(k, k), 24) for k in range(3)]
    return [fm.search_scheme.h2(k + 2, 0, k) for k in range(3)]


def oracle_ladder(w, kind, max_hits, reads=None, ladder=None):
    """the oracle stratum by stratum -> (blocks of records with batch read numbers, node count per stratum, found-stratum per read); computed once per case"""
    key = (kind, max_hits) if reads is None and ladder is None else None
    if key in w["oracle"]:
        return w["oracle"][key]
    ox, reads = w["ox"], w["reads"] if reads is None else reads
    ladder = ladder_of(kind) if ladder is None else ladder
    todo = np.arange(len(reads))
    blocks, nodes, stratum = [], [], np.full(len(reads), 255, dtype=np.uint8)
    foreign = np.array([len(r) > 0 and bool((np.asarray(r) >= SIGMA).any()) for r in reads])
    assert all((np.asarray(reads[j]) >= SIGMA).all() and len(reads[j]) == 24 for j in np.nonzero(foreign)[0])
    for i, sch in enumerate(ladder):
        if todo.size == 0:
            break
        inside = todo[~foreign[todo]]                                 # a read of symbols >= sigma is withheld from the oracle, see FOREIGN READS above
        qb, qo = fm.flatten([reads[j] for j in inside])
        if kind == "ng21":
            h, _, nd = ox.search_ng21(qb, qo, sch, max_hits) if inside.size else (np.zeros(0, dtype=HIT_DTYPE), None, 0)
        else:
            h, _, nd = ox.search_ng26(qb, qo, sch, None, max_hits, edit=(kind == "edit")) if inside.size else (np.zeros(0, dtype=HIT_DTYPE), None, 0)
        h = h.copy()
        assert (h["len"] > 0).all()                                  # the oracle emits no empty record on this input: "any record" and "a row" agree
        found = np.zeros(len(reads), dtype=bool)
        found[inside[np.unique(h["qidx"].astype(np.int64))]] = True
        h["qidx"] = inside.astype(np.uint64)[h["qidx"].astype(np.int64)]
        stratum[found] = i
        blocks.append(h)
        u = np.asarray(sch[2])
        assert (u[:, 0] == 0).all()                                  # every search begins with an exact step: the one extension a foreign read costs
        nodes.append(nd + int(foreign[todo].sum()) * u.shape[0] if max_hits else 0)
        todo = todo[~found[todo]]
    res = (blocks, nodes, stratum)
    if key is not None:
        w["oracle"][key] = res
    return res


def callback_order(blocks):
    h = np.concatenate(blocks) if blocks else np.zeros(0, dtype=HIT_DTYPE)
    return h[np.argsort(h["qidx"], kind="stable")]                   # the oracle emits in callback order inside a read, and a read's records sit in one block


def same_hits(g, o):
    return len(g) == len(o) and all(np.array_equal(g[k].astype(np.uint64), o[k].astype(np.uint64)) for k in HIT_KEYS)


def record_set(h):
    return sorted(zip(h["qidx"].tolist(), h["lb"].tolist(), h["lb_rev"].tolist(), h["len"].tolist(), (h["errors"] & 0xff).tolist()))


def scheme_array(kind, ladder):
    keep = [tuple(np.ascontiguousarray(np.asarray(x, dtype=np.uint64)) for x in sch) for sch in ladder]
    arr = ((capi.ExpandedScheme if kind == "ng21" else capi.Scheme) * len(keep))()
    for sc, (pi, l, u) in zip(arr, keep):
        if kind == "ng21":
            sc.n_searches, sc.length = pi.shape
        else:
            sc.n_searches, sc.n_parts = pi.shape
            sc.partition, sc.edit = None, 1 if kind == "edit" else 0
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    return arr, keep


def call_best(gx, qbuf, qoff, nq, kind, ladder, max_hits, capacity, q4=False, out=None, stratum=None):
    """the raw C call -> (rc, records as written, out_count, out_stratum, stats list)"""
    arr, keep = scheme_array(kind, ladder)
    L = capi.lib()
    name = "fmgpu_search_best" + ("_ng21" if kind == "ng21" else "") + ("_q4" if q4 else "")
    rec = np.zeros(max(capacity, 1), dtype=HIT_DTYPE) if out is None else out
    strat = np.full(max(nq, 1), 77, dtype=np.uint8) if stratum is None else stratum
    stats = (capi.Stats * len(keep))()
    cnt = C.c_uint64(12345)
    rc = getattr(L, name)(gx._h, capi.ptr(qbuf), capi.ptr(qoff), nq, arr, len(keep), max_hits, capi.ptr(rec), capacity, C.byref(cnt), capi.ptr(strat), stats, None)
    return rc, rec, int(cnt.value), strat, [stats[i] for i in range(len(keep))]


def sorted_on_device(rec, count):
    h = np.ascontiguousarray(rec[:count])
    capi.check(capi.lib().fmgpu_hits_sort(capi.ptr(h), count, None))
    return h


def check_against_oracle(w, gx, kind, max_hits, got):
    rc, rec, count, strat, stats = got
    blocks, nodes, want_stratum = oracle_ladder(w, kind, max_hits)
    assert rc == 0 and count == sum(len(b) for b in blocks)
    assert np.array_equal(strat[: len(w["reads"])], want_stratum)
    at = 0
    for i, b in enumerate(blocks):                                    # the records of stratum 0 come first, then stratum 1's ...
        assert stats[i].hits == len(b), (i, stats[i].hits, len(b))
        assert record_set(rec[at: at + len(b)]) == record_set(b), i
        assert stats[i].lf_steps == nodes[i], (i, stats[i].lf_steps, nodes[i])
        at += len(b)
    assert same_hits(sorted_on_device(rec, count), callback_order(blocks))
    return blocks, want_stratum


def conditions(blocks, stratum, many_writers):
    """what makes the input a test of the ladder: every stratum finds a read, a read stays unfound, and (edit distance, ng21) a read has several records in one stratum"""
    assert len(blocks) == 3 and all(int((stratum == i).sum()) > 0 for i in range(3)) and int((stratum == 255).sum()) > 0
    if many_writers:
        assert max(int(np.bincount(b["qidx"].astype(np.int64)).max()) for b in blocks) >= 2


# ------------------------------------------------------------------------------------------------ 1. search_ng26 ladders
@pytest.mark.parametrize("kind,max_hits", [("hamming", UNLIMITED), ("edit", UNLIMITED), ("hamming", 2), ("edit", 2)])
def test_ng26_ladder(world, kind, max_hits):
    qbuf, qoff = fm.flatten(world["reads"])
    got = call_best(world["gx"], qbuf, qoff, 135, kind, ladder_of(kind), max_hits, 4096)
    blocks, stratum = check_against_oracle(world, world["gx"], kind, max_hits, got)
    conditions(blocks, stratum, many_writers=(kind == "edit"))
    # the Python mirror: the same records in callback order, and out_stratum through the new keyword
    hits, strat = fm.search_best(world["gx"], (qbuf, qoff), 0, n=max_hits, edit=(kind == "edit"), schemes=[(s, None) for s in ladder_of(kind)], want_stratum=True)
    assert same_hits(hits, callback_order(blocks)) and np.array_equal(strat, stratum)


# ------------------------------------------------------------------------------------------------ 2. search_ng21 ladders
@pytest.mark.parametrize("max_hits", [UNLIMITED, 3])
def test_ng21_ladder(world, max_hits):
    qbuf, qoff = fm.flatten(world["reads"])
    got = call_best(world["gx"], qbuf, qoff, 135, "ng21", ladder_of("ng21"), max_hits, 8192)
    blocks, stratum = check_against_oracle(world, world["gx"], "ng21", max_hits, got)
    conditions(blocks, stratum, many_writers=True)
    inb, ino = fm.flatten(world["reads"][:134])                      # the oracle's own search_best / search_best_n (the foreign read is the last one: the numbers stay)
    want, _ = world["ox"].search_ng21_best(inb, ino, ladder_of("ng21"), max_hits)
    assert same_hits(callback_order(blocks), want)
    if max_hits == UNLIMITED:
        hits = fm.search_ng21.search_best(world["gx"], (qbuf, qoff), ladder_of("ng21"))
    else:
        hits = fm.search_ng21.search_best_n(world["gx"], (qbuf, qoff), ladder_of("ng21"), 3)
    assert same_hits(hits, want)


# ------------------------------------------------------------------------------------------------ 3. the same batch three ways
@pytest.mark.parametrize("kind", ["edit", "ng21"])
def test_same_batch_three_ways(world, kind):
    gx, reads = world["gx"], world["reads"]
    qbuf, qoff = fm.flatten(reads)
    total = int(qoff[-1])
    blocks, _, stratum = oracle_ladder(world, kind, UNLIMITED)
    want = callback_order(blocks)
    # behind a lead of 3 foreign bytes
    sbuf, soff = np.concatenate([np.full(3, 2, dtype=np.uint8), qbuf[:total]]), qoff + np.uint64(3)
    rc, rec, count, strat, _ = call_best(gx, sbuf, soff, 135, kind, ladder_of(kind), UNLIMITED, 8192)
    assert rc == 0 and same_hits(sorted_on_device(rec, count), want) and np.array_equal(strat[:135], stratum)
    # as device buffers: queries, offsets, records and out_stratum all in HBM
    dq, do = capi.DeviceBuffer.from_array(sbuf), capi.DeviceBuffer.from_array(soff)
    dout, dstrat = capi.DeviceBuffer(8192 * HIT_DTYPE.itemsize), capi.DeviceBuffer(135)
    rc, _, count, _, _ = call_best(gx, dq, do, 135, kind, ladder_of(kind), UNLIMITED, 8192, out=dout, stratum=dstrat)
    assert rc == 0 and count == len(want)
    assert same_hits(sorted_on_device(dout.to_array(HIT_DTYPE, count), count), want) and np.array_equal(dstrat.to_array(np.uint8, 135), stratum)
    # as a 4-bit packed batch whose first symbol is an odd nibble (the nibble before it belongs to someone else); symbol 7 travels as nibble 15
    nib = np.concatenate([np.full(1, 3, dtype=np.uint8), np.where(qbuf[:total] >= 5, 15, qbuf[:total]).astype(np.uint8)])
    nib = np.concatenate([nib, np.zeros(nib.size & 1, dtype=np.uint8)])
    packed, poff = (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8), qoff + np.uint64(1)
    rc, rec, count, strat, _ = call_best(gx, packed, poff, 135, kind, ladder_of(kind), UNLIMITED, 8192, q4=True)
    assert rc == 0 and same_hits(sorted_on_device(rec, count), want) and np.array_equal(strat[:135], stratum)
    pq = fm.PackedQueries(capi.DeviceBuffer.from_array(packed), capi.DeviceBuffer.from_array(poff), 135)    # the mirrors take it without a host copy
    if kind == "ng21":
        assert same_hits(fm.search_ng21.search_best(gx, pq, ladder_of(kind)), want)
    else:
        assert same_hits(fm.search_best(gx, pq, 0, edit=True, schemes=[(s, None) for s in ladder_of(kind)]), want)


# ------------------------------------------------------------------------------------------------ 4. a ladder that ends early
def test_stratum_zero_finds_every_read(world):
    reads = world["reads"][0:131:4]                                   # read i carries i % 4 substitutions: these are copies of the text
    qbuf, qoff = fm.flatten(reads)
    blocks, nodes, stratum = oracle_ladder(world, "hamming", UNLIMITED, reads=reads)
    assert len(blocks) == 1 and (stratum == 0).all()
    rc, rec, count, strat, stats = call_best(world["gx"], qbuf, qoff, len(reads), "hamming", ladder_of("hamming"), UNLIMITED, 1024)
    assert rc == 0 and same_hits(sorted_on_device(rec, count), callback_order(blocks)) and (strat[: len(reads)] == 0).all()
    assert stats[0].hits == count and stats[0].lf_steps == nodes[0]
    for st in stats[1:]:                                              # the later strata did not run
        assert (st.lf_steps, st.hits, st.kernel_ms, st.prepass_ms, st.table_bytes, st.table_accesses, st.table_steps) == (0, 0, 0.0, 0.0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ 5. a ladder that finds nothing
def test_nothing_found(world):
    reads = [np.full(24, 7, dtype=np.uint8)] * 3
    qbuf, qoff = fm.flatten(reads)
    for kind in ("edit", "ng21"):
        blocks, _, stratum = oracle_ladder(world, kind, UNLIMITED, reads=reads)
        assert sum(len(b) for b in blocks) == 0 and (stratum == 255).all()
        rc, _, count, strat, stats = call_best(world["gx"], qbuf, qoff, 3, kind, ladder_of(kind), UNLIMITED, 64)
        assert rc == 0 and count == 0 and (strat[:3] == 255).all() and all(st.hits == 0 for st in stats)
    # no scheme, no read: 0 records, out_stratum all 255
    L = capi.lib()
    cnt, strat = C.c_uint64(9), np.zeros(3, dtype=np.uint8)
    assert L.fmgpu_search_best(world["gx"]._h, capi.ptr(qbuf), capi.ptr(qoff), 3, None, 0, UNLIMITED, None, 0, C.byref(cnt), capi.ptr(strat), None, None) == 0
    assert cnt.value == 0 and (strat == 255).all()


# ------------------------------------------------------------------------------------------------ 6. capacity
def test_capacity(world):
    gx = world["gx"]
    qbuf, qoff = fm.flatten(world["reads"])
    blocks, _, stratum = oracle_ladder(world, "hamming", UNLIMITED)
    sizes = [len(b) for b in blocks]
    assert sizes[1] > 1
    cap = sizes[0] + 1
    rc, _, count, _, _ = call_best(gx, qbuf, qoff, 135, "hamming", ladder_of("hamming"), UNLIMITED, cap)
    assert rc == capi.FMGPU_ERR_CAPACITY and count == sizes[0] + sizes[1] and count > cap
    for rounds in range(1, 4):                                        # growing to max(count, 2 x capacity) ends within n_schemes rounds
        cap = max(count, 2 * cap)
        rc, rec, count, strat, _ = call_best(gx, qbuf, qoff, 135, "hamming", ladder_of("hamming"), UNLIMITED, cap)
        if rc != capi.FMGPU_ERR_CAPACITY:
            break
        assert count > cap
    assert rc == 0 and rounds <= 3 and count == sum(sizes)
    assert same_hits(sorted_on_device(rec, count), callback_order(blocks)) and np.array_equal(strat[:135], stratum)
    hits = fm.search_best(gx, (qbuf, qoff), 0, edit=False, schemes=[(s, None) for s in ladder_of("hamming")], capacity=sizes[0] + 1)
    assert same_hits(hits, callback_order(blocks))
    # argument errors on a real handle: the single-scheme calls' codes
    arr, keep = scheme_array("hamming", ladder_of("hamming"))
    L, cnt = capi.lib(), C.c_uint64()
    rec = np.zeros(8, dtype=HIT_DTYPE)
    assert L.fmgpu_search_best(gx._h, None, capi.ptr(qoff), 135, arr, 3, UNLIMITED, capi.ptr(rec), 8, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_search_best(gx._h, capi.ptr(qbuf), capi.ptr(qoff), 135, arr, 255, UNLIMITED, capi.ptr(rec), 8, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID
    keep[2][0][0, 0] = 99                                             # a bad entry in the LAST scheme: nothing runs, nothing is written
    rec.view(np.uint8)[:] = 0x5A
    assert L.fmgpu_search_best(gx._h, capi.ptr(qbuf), capi.ptr(qoff), 135, arr, 3, UNLIMITED, capi.ptr(rec), 8, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID
    assert (rec.view(np.uint8) == 0x5A).all() and cnt.value == 0
    uni = fm.FMIndex.from_reference_arrays(**{k: v for k, v in oracle_arrays(world["ox"]).items() if k != "bwt_rev"})
    arr, keep = scheme_array("hamming", ladder_of("hamming"))
    assert L.fmgpu_search_best(uni._h, capi.ptr(qbuf), capi.ptr(qoff), 135, arr, 3, UNLIMITED, capi.ptr(rec), 8, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID
    assert b"BiFMIndex" in L.fmgpu_last_error()


# ------------------------------------------------------------------------------------------------ 7. 64-bit rows
def test_wide_rows(world):
    with fm.options(force_wide=1):
        gx = gpu_index(world["ox"])
    assert gx.row_bits == 64
    qbuf, qoff = fm.flatten(world["reads"])
    got = call_best(gx, qbuf, qoff, 135, "edit", ladder_of("edit"), UNLIMITED, 4096)
    check_against_oracle(world, gx, "edit", UNLIMITED, got)


# ------------------------------------------------------------------------------------------------ 8. chained into fmgpu_locate_hits
def test_chained_into_locate_hits(world):
    gx, ox = world["gx"], world["ox"]
    qbuf, qoff = fm.flatten(world["reads"])
    want_hits = callback_order(oracle_ladder(world, "edit", UNLIMITED)[0])
    want = []                                                         # search_locate of the oracle ladder: every row of every cursor, in report order
    for h in want_hits:
        for row in range(int(h["lb"]), int(h["lb"] + h["len"])):
            s, p, k = ox.locate(row)
            want.append((int(h["qidx"]), int(s), int(p + k), int(h["errors"]) & 0xff))
    dout = capi.DeviceBuffer(4096 * HIT_DTYPE.itemsize)
    rc, _, count, _, _ = call_best(gx, qbuf, qoff, 135, "edit", ladder_of("edit"), UNLIMITED, 4096, out=dout)
    assert rc == 0 and count == len(want_hits)
    capi.check(capi.lib().fmgpu_hits_sort(capi.ptr(dout), count, None))
    pos = np.zeros(len(want) + 8, dtype=capi.POSITION_DTYPE)
    cnt = C.c_uint64()
    capi.check(capi.lib().fmgpu_locate_hits(gx._h, capi.ptr(dout), count, capi.ptr(pos), len(pos), C.byref(cnt), None, None))
    got = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(pos["qidx"][: cnt.value], pos["seq_id"][: cnt.value], pos["pos"][: cnt.value], pos["errors"][: cnt.value])]
    assert got == want and len(want) > len(want_hits)
