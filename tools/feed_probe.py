"""dev probe: a host batch end to end — the one-shot call against a feed (include/fmgpu.h: fmgpu_feed_*) on the genome stand-in (datasets.genome_like_text with
bench.GRCH38_LENGTHS scaled by --scale; FMIndex<5, IB16>, plain index), --nq reads of --length symbols in PAGEABLE host memory, results into pageable host memory.
Every figure is the wall time of one call, host clock, the call returns after its results have landed.
  legs, alternated --rounds times, --reps calls each:
    A  one-shot fmgpu_search_exact with host pointers, from the library given with --parent-lib (the build of the commit before feeds; it gets an index of its own,
       built from the same text) — without --parent-lib, from this library (the one-shot path is the same code);
    B  feed, bytes;   C  feed, pack4 = 1;   D  feed from pinned memory into pinned memory;   E  the device-resident call (kernel floor, wall)
    and one plain pinned host-to-device copy of the batch's symbols (PCIe floor).
  verdict: B below A in every round, by more than the spread (max - min) of A's own round medians.  B, C, D over max(E, PCIe floor) are printed beside them.
  sweep: chunk_reads 64 k / 256 k / 1 M x host_threads 1 / 4 / 16, bytes, the best of two calls each; and from pinned memory, chunk_reads 256 k / 1 M x slots 2 / 4.
  --k2-nq N (0 = skip): one k = 2 Hamming leg (h2(4, 0, 2), BiFMIndex of the same text), one-shot against feed, N reads.
Writes profiles/feed_probe.log (or --log)."""
import argparse
import ctypes as C
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi, datasets

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--nq", type=int, default=10_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--k2-nq", type=int, default=0)
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "feed_probe.log"))
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
say("# python tools/feed_probe.py " + " ".join(a for a in sys.argv[1:] if not a.startswith("/")))
say(f"# device: {torch.cuda.get_device_name(0)}; {torch.cuda.get_device_properties(0).multi_processor_count} CUs; clock_rate {getattr(torch.cuda.get_device_properties(0), 'clock_rate', 0) / 1e3:.0f} MHz")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
qbuf, qoff = bench.sample_reads(c, text, lengths, args.length, args.nq, 1000, "exact")
torch.cuda.synchronize()
fm.options["lf_table"] = 0
t0 = time.time()
index = fm.FMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
nq, total = args.nq, args.nq * args.length
say(f"# genome stand-in, {int(text.numel())} symbols, {len(lengths)} sequences; plain index (formats {index.formats:#x}, {index.device_bytes / 1e9:.2f} GB) built in {time.time() - t0:.1f} s; "
    f"{nq} reads x {args.length} symbols: {total / 1e6:.0f} MB of symbols and {8 * (nq + 1) / 1e6:.0f} MB of offsets in, {16 * nq / 1e6:.0f} MB out")

# leg A's library and its own index
P, parent_index = L, index._h
if args.parent_lib:
    P = C.CDLL(args.parent_lib)
    P.fmgpu_last_error.restype = C.c_char_p
    P.fmgpu_set_option.argtypes = [C.c_int32, C.c_int64]
    P.fmgpu_build_index.argtypes = L.fmgpu_build_index.argtypes
    P.fmgpu_search_exact.argtypes = L.fmgpu_search_exact.argtypes
    P.fmgpu_index_destroy.argtypes = [C.c_void_p]
    assert not hasattr(P, "fmgpu_feed_create"), "--parent-lib is a build without feeds"
    assert P.fmgpu_set_option(capi.OPTIONS["lf_table"], 0) == 0
    ph = C.c_void_p()
    rc = P.fmgpu_build_index(C.c_void_p(text.data_ptr()), C.c_void_p(seq_off.data_ptr()), len(lengths), 5, capi.LAYOUTS["IB16"], 16, 0, 0, C.byref(ph), None)
    assert rc == 0, P.fmgpu_last_error()
    parent_index = ph
    say("# leg A runs in the parent commit's library, on its own index of the same text")
else:
    say("# leg A runs in THIS library (no --parent-lib): the one-shot path is unchanged code")

hq, ho = qbuf.cpu().numpy(), qoff.cpu().numpy().astype(np.uint64)           # pageable
lb, ln = np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint64)
pin_q, pin_lb, pin_ln = capi.PinnedBuffer.from_array(hq), capi.PinnedBuffer(8 * nq), capi.PinnedBuffer(8 * nq)
pq, plb, pln = pin_q.array(np.uint8, hq.size), pin_lb.array(np.uint64, nq), pin_ln.array(np.uint64, nq)
dlb, dln = torch.empty(nq, dtype=torch.int64, device=dev), torch.empty(nq, dtype=torch.int64, device=dev)
ptr = lambda t: C.c_void_p(t.data_ptr())

capi.check(L.fmgpu_search_exact(index._h, ptr(qbuf), ptr(qoff), nq, ptr(dlb), ptr(dln), None, None))
torch.cuda.synchronize()
want = (dlb.cpu().numpy().astype(np.uint64), dln.cpu().numpy().astype(np.uint64))
say(f"# {int((want[1] > 0).sum())} reads with occurrences")

feeds = {"B": fm.Feed(index), "C": fm.Feed(index, pack4=True), "D": fm.Feed(index)}


def check(tag, got):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag + ": results differ from the device-resident call"


def leg_a():
    rc = P.fmgpu_search_exact(parent_index, capi.ptr(hq), capi.ptr(ho), nq, capi.ptr(lb), capi.ptr(ln), None, None)
    assert rc == 0, P.fmgpu_last_error()


LEGS = {
    "A": leg_a,
    "B": lambda: feeds["B"].search_exact((hq, ho), out=(lb, ln)),
    "C": lambda: feeds["C"].search_exact((hq, ho), out=(lb, ln)),
    "D": lambda: feeds["D"].search_exact((pq, ho), out=(plb, pln)),
    "E": lambda: capi.check(L.fmgpu_search_exact(index._h, ptr(qbuf), ptr(qoff), nq, ptr(dlb), ptr(dln), None, None)),
}
NAMES = {"A": "A one-shot, host pointers", "B": "B feed, bytes", "C": "C feed, pack4", "D": "D feed, pinned in and out", "E": "E device-resident call"}

for k, f in LEGS.items():                                                    # warm-up, and the results of every leg
    lb[:] = 0; ln[:] = 0; plb[:] = 0; pln[:] = 0
    f()
    torch.cuda.synchronize()
    if k != "E":
        check(k, (plb, pln) if k == "D" else (lb, ln))
for k in "BCD":
    i = feeds[k].info()
    say(f"# feed {k}: {i['chunks']} chunks, staged {i['staged_bytes'] / 1e6:.0f} MB, uploaded {i['uploaded_bytes'] / 1e6:.0f} MB, holds {i['pinned_bytes'] / 1e6:.0f} MB pinned and {i['device_bytes'] / 1e6:.0f} MB of device memory")

dq = torch.empty(total, dtype=torch.uint8, device=dev)
pcie = min(wall(lambda: capi.check(L.fmgpu_memcpy_h2d(ptr(dq), C.c_void_p(pin_q.ptr), total))) for _ in range(4))
say(f"# PCIe floor: one pinned host-to-device copy of the {total / 1e6:.0f} MB of symbols: {pcie:.2f} ms ({total / pcie / 1e6:.1f} GB/s), the best of 4")
del dq

say(f"# legs, wall ms of one call: round, leg, the {args.reps} calls, their median")
med = {k: [] for k in LEGS}
for r in range(args.rounds):
    for k, f in LEGS.items():
        t = [wall(f) for _ in range(args.reps)]
        med[k].append(float(np.median(t)))
        say(f"round {r + 1}  {NAMES[k]:<28s} " + " ".join(f"{x:8.2f}" for x in t) + f"   median {med[k][-1]:8.2f}")
floor = max(float(np.median(med["E"])), pcie)
spread_a = max(med["A"]) - min(med["A"])
say(f"# floor = max(E, PCIe) = {floor:.2f} ms; A's own spread over the rounds (max - min of its medians) = {spread_a:.2f} ms")
for k in "ABCD":
    m = float(np.median(med[k]))
    say(f"# {NAMES[k]:<28s} median of the rounds {m:8.2f} ms = {m / floor:5.2f} x floor, {nq / m / 1e3:7.1f} M reads/s" + ("" if k == "A" else f", A / {k} = {float(np.median(med['A'])) / m:.3f}"))
wins = [med["A"][r] - med["B"][r] for r in range(args.rounds)]
ok = all(w > spread_a for w in wins)
say("# A - B per round: " + ", ".join(f"{w:.2f}" for w in wins) + f" ms -> B is {'faster than A in every round by more than' if ok else 'NOT faster than A in every round by more than'} A's spread")

if not args.no_sweep:
    say("# sweep (bytes, pageable): chunk_reads, host_threads, wall ms (the better of two calls after one warm-up)")
    for cr in (64 * 1024, 256 * 1024, 1024 * 1024):
        for ht in (1, 4, 16):
            with fm.Feed(index, chunk_reads=cr, host_threads=ht) as f:
                f.search_exact((hq, ho), out=(lb, ln))
                t = min(wall(lambda: f.search_exact((hq, ho), out=(lb, ln))) for _ in range(2))
                check("sweep", (lb, ln))
                say(f"sweep  chunk_reads {cr:8d}  host_threads {ht:2d}  {t:8.2f}")

    say("# sweep (bytes, pinned in and out: no staging): chunk_reads, slots, wall ms (the better of two calls after one warm-up)")
    for cr in (256 * 1024, 1024 * 1024):
        for slots in (2, 4):
            with fm.Feed(index, chunk_reads=cr, slots=slots) as f:
                f.search_exact((pq, ho), out=(plb, pln))
                t = min(wall(lambda: f.search_exact((pq, ho), out=(plb, pln))) for _ in range(2))
                check("sweep pinned", (plb, pln))
                say(f"sweep  pinned  chunk_reads {cr:8d}  slots {slots}  {t:8.2f}")

if args.k2_nq:
    for f in feeds.values():
        f.close()
    del index
    n2 = args.k2_nq
    t0 = time.time()
    bi = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
    say(f"# k = 2 Hamming, h2(4, 0, 2): BiFMIndex built in {time.time() - t0:.1f} s; {n2} reads x {args.length} symbols from pageable memory")
    sch = fm.search_scheme.h2(4, 0, 2)
    kq, ko = hq[: n2 * args.length], ho[: n2 + 1]
    one = fm.search_ng26.search(bi, (kq, ko), sch)
    with fm.Feed(bi) as f:
        fed = f.search_scheme((kq, ko), sch)
        assert fed.tobytes() == one.tobytes(), "k = 2: the feed's records differ"
        for r in range(args.rounds):
            a = wall(lambda: fm.search_ng26.search(bi, (kq, ko), sch, capacity=len(one) + 1))
            b = wall(lambda: f.search_scheme((kq, ko), sch, capacity=len(one) + 1))
            say(f"k2 round {r + 1}  one-shot {a:9.2f} ms   feed {b:9.2f} ms   ({len(one)} records, sorted on the device in both)")
sys.exit(0 if ok else 1)
