"""dev probe: 4-bit packed query batches on the genome stand-in (datasets.genome_like_text with bench.GRCH38_LENGTHS scaled by --scale; FMIndex<5, IB16>, plain
index: pair table, no interval / k-step / walk table), --nq reads of --length symbols (bench.sample_reads, mode "exact").
  (a) kernel_ms of fmgpu_search_exact_q4 against fmgpu_search_exact, both on device-resident queries, alternated --rounds times (each figure the mean of --steps
      launches after --warmup); the outputs must be byte-equal.  The byte path of the same job is the yardstick: the packed mean may exceed the byte mean by at most
      the byte path's own (max - min) / mean over the rounds — the probe prints the verdict and exits 1 if it is missed.
  (b) host to host, wall time of one call each: the byte form; the packed form, packed on the host beforehand; device bytes -> fmgpu_queries_pack4 with the
      complement table -> fmgpu_search_exact_q4 on both strands (reported only, with the bytes that crossed PCIe and the rate they crossed at).
Writes profiles/packed_queries_probe.log (or --log)."""
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
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "packed_queries_probe.log"))
args = ap.parse_args()
assert args.rounds >= 3

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


dev = torch.device("cuda", 0)
c = types.SimpleNamespace(torch=torch, np=np, datasets=datasets, dev=dev, rank=0, args=types.SimpleNamespace(scale=args.scale))
L = capi.lib()
say(f"# python tools/packed_queries_probe.py --scale {args.scale} --nq {args.nq} --length {args.length} --rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
qbuf, qoff = bench.sample_reads(c, text, lengths, args.length, args.nq, 1000, "exact")
torch.cuda.synchronize()
fm.options["lf_table"] = 0
t0 = time.time()
index = fm.FMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
say(f"# genome stand-in, {int(text.numel())} symbols, {len(lengths)} sequences; plain index (formats {index.formats:#x}, {index.device_bytes / 1e9:.2f} GB) built in {time.time() - t0:.1f} s; "
    f"{args.nq} reads x {args.length} symbols")
del text
nq, total = args.nq, args.nq * args.length
ptr = lambda t: C.c_void_p(t.data_ptr())

# the packed batch, made on the device from the device bytes (one strand)
packed = torch.empty((total + 1) // 2 + 16, dtype=torch.uint8, device=dev)
poff = torch.empty(nq + 1, dtype=torch.int64, device=dev)
capi.check(L.fmgpu_queries_pack4(ptr(qbuf), ptr(qoff), nq, 5, None, ptr(packed), ptr(poff), None))
torch.cuda.synchronize()
outs = {k: torch.empty(2 * nq, dtype=torch.int64, device=dev) for k in ("byte", "q4")}
stats = capi.Stats()


def launch(kind):
    if kind == "byte":
        capi.check(L.fmgpu_search_exact(index._h, ptr(qbuf), ptr(qoff), nq, ptr(outs[kind][:nq]), ptr(outs[kind][nq:]), C.byref(stats), None))
    else:
        capi.check(L.fmgpu_search_exact_q4(index._h, ptr(packed), ptr(poff), nq, ptr(outs[kind][:nq]), ptr(outs[kind][nq:]), C.byref(stats), None))
    return stats.kernel_ms, stats.lf_steps


say("# (a) device-resident queries: run, kernel_ms (HIP events, mean of the launches), lf_steps per launch")
means = {"byte": [], "q4": []}
for r in range(args.rounds):
    for kind in ("byte", "q4"):
        for _ in range(args.warmup):
            launch(kind)
        got = [launch(kind) for _ in range(args.steps)]
        means[kind].append(float(np.mean([g[0] for g in got])))
        say(f"{kind}_{r + 1:<3d} {means[kind][-1]:8.3f}  {got[-1][1]}")
torch.cuda.synchronize()
equal = bool(torch.equal(outs["byte"], outs["q4"]))
hits = int((outs["byte"][nq:] > 0).sum())
mb, mq = float(np.mean(means["byte"])), float(np.mean(means["q4"]))
noise = (max(means["byte"]) - min(means["byte"])) / mb
ok = equal and mq <= mb * (1 + noise)
say(f"# outputs byte-equal: {equal} ({hits} reads with occurrences)")
say(f"# means: byte {mb:.3f}, q4 {mq:.3f} -> q4 / byte = {mq / mb:.4f}; the byte path's own (max - min) / mean = {noise:.4f}: q4 is {'within' if ok else 'NOT within'} it")

say("# (b) host to host, one call each, wall ms (queries and results in pageable host memory)")
hq, ho = qbuf.cpu().numpy(), qoff.cpu().numpy().astype(np.uint64)
hp, hpo = packed[: (total + 1) // 2].cpu().numpy(), poff.cpu().numpy().astype(np.uint64)
lb, ln = np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint64)


def wall(f):
    torch.cuda.synchronize()
    t = time.time()
    f()
    torch.cuda.synchronize()
    return (time.time() - t) * 1e3


def report(name, ms, up_bytes, down_bytes, reads):
    say(f"{name:<34s} {ms:9.1f} ms  up {up_bytes / 1e6:8.1f} MB  down {down_bytes / 1e6:7.1f} MB  {(up_bytes + down_bytes) / ms / 1e6:6.2f} GB/s over the whole call  {reads / ms / 1e3:7.2f} M reads/s")


for rep in range(2):
    ms = wall(lambda: capi.check(L.fmgpu_search_exact(index._h, capi.ptr(hq), capi.ptr(ho), nq, capi.ptr(lb), capi.ptr(ln), None, None)))
    report("byte form, host -> host", ms, hq.nbytes + ho.nbytes, 16 * nq, nq)
    keep = (lb.copy(), ln.copy())
    ms = wall(lambda: capi.check(L.fmgpu_search_exact_q4(index._h, capi.ptr(hp), capi.ptr(hpo), nq, capi.ptr(lb), capi.ptr(ln), None, None)))
    report("packed on the host, host -> host", ms, hp.nbytes + hpo.nbytes, 16 * nq, nq)
    assert np.array_equal(lb, keep[0]) and np.array_equal(ln, keep[1])
comp = np.array([0, 4, 3, 2, 1], dtype=np.uint8)
lb2, ln2 = np.empty(2 * nq, dtype=np.uint64), np.empty(2 * nq, dtype=np.uint64)
both = torch.empty(total + 16, dtype=torch.uint8, device=dev)
both_off = torch.empty(2 * nq + 1, dtype=torch.int64, device=dev)


def both_strands():
    capi.check(L.fmgpu_queries_pack4(ptr(qbuf), ptr(qoff), nq, 5, capi.ptr(comp), ptr(both), ptr(both_off), None))
    capi.check(L.fmgpu_search_exact_q4(index._h, ptr(both), ptr(both_off), 2 * nq, capi.ptr(lb2), capi.ptr(ln2), None, None))


for rep in range(2):
    ms = wall(both_strands)
    report("device bytes -> pack4 + rc -> q4", ms, 0, 32 * nq, 2 * nq)
assert np.array_equal(lb2[0::2], keep[0]) and np.array_equal(ln2[0::2], keep[1])
say(f"# both strands: forward reads equal the one-strand result; {int((ln2[1::2] > 0).sum())} reverse complements with occurrences")
sys.exit(0 if ok else 1)
