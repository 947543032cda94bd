"""dev probe: reads in, located positions out — fmgpu_map and fmgpu_feed_map (include/fmgpu.h) against the composition of the calls they chain, with the method of
tools/feed_probe.py.  The genome stand-in (datasets.genome_like_text with bench.GRCH38_LENGTHS scaled by --scale) as a BiFMIndex<5, IB16> at sampling
rate 16, --nq reads of --length symbols with 0 / 1 / 2 substitutions in ratio 1:1:1, the Hamming ladder h2(k + 2, 0, k), k = 0, 1, 2.  Every figure is the wall time of
one call sequence, host clock, ending when its results have landed.
  legs, alternated --rounds times, --reps calls each:
    A     the composition fmc::Search and search_locate perform without fmgpu_map, from the library given with --parent-lib (the build of the commit before fmgpu_map; it gets
          an index of its own, built from the same text) — without --parent-lib, from this library (those calls are the same code): fmgpu_search_best with host pointers,
          the hit records on the host, fmgpu_hits_sort on them, fmgpu_locate_hits from host records into host positions; buffers sized exactly (no retry round)
    Adev  the device-side part of A: the same three calls on device pointers, the hit records staying in HBM
    B     fmgpu_map, every buffer in device memory
    C     fmgpu_map with host pointers (pageable)
    D     fmgpu_feed_map, pageable in and out;   E  fmgpu_feed_map, pinned in and out
  requirement: B not slower than Adev by more than the spread (max - min) of Adev's own round medians.
  --max-hits N: at most N rows per read (the n of search_n), what a mapper sets; the stand-in's runs of one symbol give reads of ~10^8 rows each, which no buffer holds.
  memory: the lowest free device memory (hipMemGetInfo, sampled every millisecond by a host thread) during one call of C and of D, against the idle level before it,
  and what fmgpu_feed_info reports for D.
Writes profiles/map_probe.log (or --log)."""
import argparse
import ctypes as C
import os
import sys
import threading
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi, datasets
from fmindex_collection_amd.capi import HIT_DTYPE, POSITION_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--nq", type=int, default=1_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--chunk-reads", type=int, default=0)
ap.add_argument("--max-hits", type=int, default=0, help="rows per read at most (n of search_n); 0 = unlimited")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "map_probe.log"))
args = ap.parse_args()
assert args.rounds >= 3

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


def wall(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


dev = torch.device("cuda", 0)
c = types.SimpleNamespace(torch=torch, np=np, datasets=datasets, dev=dev, rank=0, args=types.SimpleNamespace(scale=args.scale))
L = capi.lib()
shown = [a for i, a in enumerate(sys.argv[1:]) if not a.startswith("/") and not (i + 2 < len(sys.argv) and sys.argv[i + 2].startswith("/"))]      # (absolute paths and their flags are left out)
say("# python tools/map_probe.py " + " ".join(shown) + (" --parent-lib <the parent commit's libfmgpu.so>" if args.parent_lib else ""))
props = torch.cuda.get_device_properties(0)
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; clock_rate {getattr(props, 'clock_rate', 0) / 1e3:.0f} MHz; "
    f"memory_clock_rate {getattr(props, 'memory_clock_rate', 0) / 1e3:.0f} MHz; {props.total_memory / 2**30:.0f} GiB")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
qbuf, qoff = bench.sample_reads(c, text, lengths, args.length, args.nq, 1000, "k2")
torch.cuda.synchronize()
t0 = time.time()
index = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
nq, total = args.nq, args.nq * args.length
say(f"# genome stand-in, {int(text.numel())} symbols, {len(lengths)} sequences; BiFMIndex (formats {index.formats:#x}, {index.device_bytes / 1e9:.2f} GB) built in {time.time() - t0:.1f} s; "
    f"{nq} reads x {args.length} symbols, 0 / 1 / 2 substitutions 1:1:1; ladder h2(k + 2, 0, k), k = 0, 1, 2, Hamming distance")

ladder = [fm.search_scheme.h2(k + 2, 0, k) for k in range(3)]
MAX_HITS = args.max_hits if args.max_hits else fm.UINT64_MAX
what, alive = fm._map_query(None, ladder, False, False, MAX_HITS, True, 0)
schemes = C.cast(C.c_void_p(what.schemes), C.POINTER(capi.Scheme))

# leg A's library and its own index
P, parent_index = L, index._h
if args.parent_lib:
    P = C.CDLL(args.parent_lib)
    P.fmgpu_last_error.restype = C.c_char_p
    for name in ("fmgpu_build_index", "fmgpu_search_best", "fmgpu_hits_sort", "fmgpu_locate_hits"):
        getattr(P, name).argtypes = getattr(L, name).argtypes
    assert not hasattr(P, "fmgpu_map"), "--parent-lib is a build without fmgpu_map"
    ph = C.c_void_p()
    rc = P.fmgpu_build_index(C.c_void_p(text.data_ptr()), C.c_void_p(seq_off.data_ptr()), len(lengths), 5, capi.LAYOUTS["IB16"], 16, 1, 0, C.byref(ph), None)
    assert rc == 0, P.fmgpu_last_error()
    parent_index = ph
    say("# legs A and Adev run in the parent commit's library, on its own index of the same text")
else:
    say("# legs A and Adev run in THIS library (no --parent-lib): the calls they make are unchanged code")

ptr = lambda t: C.c_void_p(t.data_ptr())
hq, ho = qbuf.cpu().numpy(), qoff.cpu().numpy().astype(np.uint64)           # pageable


def run_map(call, target, a, b, pos, cap, hits, hcap, stratum, stream=True):
    cnt, hcnt = C.c_uint64(), C.c_uint64()
    rc = call(target, a, b, nq, C.byref(what), pos, cap, C.byref(cnt), hits, hcap, C.byref(hcnt), stratum, None, None, *((None,) if stream else ()))
    return rc, int(cnt.value), int(hcnt.value)


# the sizes, from one call that only counts
rc, npos, nhits = run_map(L.fmgpu_map, index._h, ptr(qbuf), ptr(qoff), None, 0, None, 0, None)
assert rc in (0, capi.FMGPU_ERR_CAPACITY), L.fmgpu_last_error()      # (the stand-in's runs of one symbol give reads of ~10^8 rows: bound them with --max-hits)
say(f"# {nhits} hit records, {npos} positions: {nhits * 40 / 1e6:.0f} MB + {npos * 32 / 1e6:.0f} MB" + (f" (at most {args.max_hits} rows per read)" if args.max_hits else ""))
assert npos * 32 <= 8 << 30, "more than 8 GiB of positions: the probe keeps several host copies of them — bound the rows per read with --max-hits"

dpos, dhits, dstr = (torch.empty(max(n, 1), dtype=torch.uint8, device=dev) for n in (npos * 32, nhits * 40, nq))
hpos, hhits, hstr = np.zeros(npos, dtype=POSITION_DTYPE), np.zeros(nhits, dtype=HIT_DTYPE), np.zeros(nq, dtype=np.uint8)
apos, ahits, astr = np.zeros(npos, dtype=POSITION_DTYPE), np.zeros(nhits, dtype=HIT_DTYPE), np.zeros(nq, dtype=np.uint8)
adpos, adhits, adstr = (torch.empty(max(n, 1), dtype=torch.uint8, device=dev) for n in (npos * 32, nhits * 40, nq))
pins = [capi.PinnedBuffer.from_array(hq), capi.PinnedBuffer.from_array(ho), capi.PinnedBuffer(max(npos, 1) * 32), capi.PinnedBuffer(max(nhits, 1) * 40), capi.PinnedBuffer(nq)]
pq, po = pins[0].array(np.uint8, hq.size), pins[1].array(np.uint64, ho.size)
ppos, phits, pstr = pins[2].array(POSITION_DTYPE, npos), pins[3].array(HIT_DTYPE, nhits), pins[4].array(np.uint8, nq)
feed_cfg = dict(chunk_reads=args.chunk_reads) if args.chunk_reads else {}
feeds = {"D": fm.Feed(index, **feed_cfg), "E": fm.Feed(index, **feed_cfg)}


def composition(lib, handle, q, o, hits, pos, stratum):
    cnt, pcnt = C.c_uint64(), C.c_uint64()
    rc = lib.fmgpu_search_best(handle, q, o, nq, schemes, 3, MAX_HITS, hits, nhits, C.byref(cnt), stratum, None, None)
    assert rc == 0 and cnt.value == nhits, lib.fmgpu_last_error()
    assert lib.fmgpu_hits_sort(hits, nhits, None) == 0
    rc = lib.fmgpu_locate_hits(handle, hits, nhits, pos, npos, C.byref(pcnt), None, None)
    assert rc == 0 and pcnt.value == npos, lib.fmgpu_last_error()


def expect(rc_counts):
    assert rc_counts == (0, npos, nhits), (rc_counts, L.fmgpu_last_error())


LEGS = {
    "A": lambda: composition(P, parent_index, capi.ptr(hq), capi.ptr(ho), capi.ptr(ahits), capi.ptr(apos), capi.ptr(astr)),
    "Adev": lambda: composition(P, parent_index, ptr(qbuf), ptr(qoff), ptr(adhits), ptr(adpos), ptr(adstr)),
    "B": lambda: expect(run_map(L.fmgpu_map, index._h, ptr(qbuf), ptr(qoff), ptr(dpos), npos, ptr(dhits), nhits, ptr(dstr))),
    "C": lambda: expect(run_map(L.fmgpu_map, index._h, capi.ptr(hq), capi.ptr(ho), capi.ptr(hpos), npos, capi.ptr(hhits), nhits, capi.ptr(hstr))),
    "D": lambda: expect(run_map(L.fmgpu_feed_map, feeds["D"]._f, capi.ptr(hq), capi.ptr(ho), capi.ptr(hpos), npos, capi.ptr(hhits), nhits, capi.ptr(hstr), stream=False)),
    "E": lambda: expect(run_map(L.fmgpu_feed_map, feeds["E"]._f, capi.ptr(pq), capi.ptr(po), capi.ptr(ppos), npos, capi.ptr(phits), nhits, capi.ptr(pstr), stream=False)),
}
NAMES = {"A": "A composition, host hits", "Adev": "Adev composition, device", "B": "B fmgpu_map, device-resident", "C": "C fmgpu_map, host pointers",
         "D": "D fmgpu_feed_map, pageable", "E": "E fmgpu_feed_map, pinned"}


def low_water(f):
    """(idle free bytes before the call, lowest free bytes seen during it)"""
    torch.cuda.synchronize()
    idle = torch.cuda.mem_get_info(0)[0]
    low, stop = [idle], threading.Event()

    def watch():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
            time.sleep(0.001)

    t = threading.Thread(target=watch)
    t.start()
    f()
    torch.cuda.synchronize()
    stop.set()
    t.join()
    return idle, low[0]


for k, f in LEGS.items():                                                    # warm-up, and the results of every leg against leg A's
    f()
    torch.cuda.synchronize()
want = (apos.tobytes(), ahits.tobytes(), astr.tobytes())
for k, got in (("Adev", (adpos, adhits, adstr)), ("B", (dpos, dhits, dstr))):
    g = tuple(t.cpu().numpy()[: n].tobytes() for t, n in zip(got, (npos * 32, nhits * 40, nq)))
    assert g == want, k + ": results differ from leg A's"
assert (hpos.tobytes(), hhits.tobytes(), hstr.tobytes()) == want, "C / D: results differ from leg A's"
assert (ppos.tobytes(), phits.tobytes(), pstr.tobytes()) == want, "E: results differ from leg A's"
say("# every leg returns leg A's positions, hit records and strata, byte for byte")
for k in "DE":
    i = feeds[k].info()
    say(f"# feed {k}: {i['chunks']} chunks, staged {i['staged_bytes'] / 1e6:.0f} MB, uploaded {i['uploaded_bytes'] / 1e6:.0f} MB, holds {i['pinned_bytes'] / 1e6:.0f} MB pinned and {i['device_bytes'] / 1e6:.0f} MB of device memory")

say(f"# legs, wall ms of one call sequence: round, leg, the {args.reps} calls, their median")
med = {k: [] for k in LEGS}
for r in range(args.rounds):
    for k, f in LEGS.items():
        t = [wall(f) for _ in range(args.reps)]
        med[k].append(float(np.median(t)))
        say(f"round {r + 1}  {NAMES[k]:<32s} " + " ".join(f"{x:9.2f}" for x in t) + f"   median {med[k][-1]:9.2f}")
spread = {k: max(med[k]) - min(med[k]) for k in med}
say(f"# spread over the rounds (max - min of the round medians): A {spread['A']:.2f} ms, Adev {spread['Adev']:.2f} ms")
for k in LEGS:
    m = float(np.median(med[k]))
    say(f"# {NAMES[k]:<32s} median of the rounds {m:9.2f} ms, {nq / m / 1e3:7.2f} M reads/s" + ("" if k == "A" else f", A / {k} = {float(np.median(med['A'])) / m:.3f}"))
over = [med["B"][r] - med["Adev"][r] for r in range(args.rounds)]
ok = float(np.median(med["B"])) - float(np.median(med["Adev"])) <= spread["Adev"]
say("# B - Adev per round: " + ", ".join(f"{w:.2f}" for w in over) + f" ms; medians of the rounds: {float(np.median(med['B'])) - float(np.median(med['Adev'])):.2f} ms -> "
    f"B is {'NOT slower' if ok else 'SLOWER'} than the device-side part of A by more than Adev's own spread")
for k in "CDE":
    wins = [med["A"][r] - med[k][r] for r in range(args.rounds)]
    say(f"# A - {k} per round: " + ", ".join(f"{w:.2f}" for w in wins) + f" ms -> {k} is {'faster' if all(w > spread['A'] for w in wins) else 'NOT faster'} than A in every round by more than A's spread")

# peak device memory of the one-shot call against the feed, chunked
say("# device memory during one call (hipMemGetInfo sampled every ms; other processes on the card would show too):")
for tag, f in (("C fmgpu_map, host pointers", LEGS["C"]),):
    idle, low = low_water(f)
    say(f"mem  {tag:<40s} idle free {idle / 1e6:10.0f} MB, lowest free {low / 1e6:10.0f} MB: the call held up to {(idle - low) / 1e6:8.0f} MB")
for cr in sorted({max(1, nq // 16), max(1, nq // 4), nq}):
    with fm.Feed(index, chunk_reads=cr) as f:
        leg = lambda: expect(run_map(L.fmgpu_feed_map, f._f, capi.ptr(hq), capi.ptr(ho), capi.ptr(hpos), npos, capi.ptr(hhits), nhits, capi.ptr(hstr), stream=False))
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info(0)[0]
        leg()                                                                # the slots grow to their size
        idle, low = low_water(leg)
        t = min(wall(leg) for _ in range(2))
        i = f.info()
        say(f"mem  D feed, chunk_reads {cr:8d} ({i['chunks']:3d} chunks)  slots hold {i['device_bytes'] / 1e6:8.0f} MB (fmgpu_feed_info), free before the feed's first call {before / 1e6:10.0f} MB, "
            f"lowest free during a call {low / 1e6:10.0f} MB: feed + call held up to {(before - low) / 1e6:8.0f} MB; wall {t:9.2f} ms")
sys.exit(0 if ok else 1)
