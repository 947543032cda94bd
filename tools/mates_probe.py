"""dev probe: fmgpu_positions_mates on the device-resident positions of --fragments paired-end fragments (separate batches, both strands, reads of 100 symbols, FR,
template lengths 0 .. 1000).  The mix: of every 8 fragments one has a mate without a record and one has 2 - 3 records per mate (the first ones the true pair, the others
elsewhere); every other fragment has one record per mate, the true pair (insert 200 .. 600, half of them with mate A on the reverse strand); one fragment in
--heavy-every has --heavy-min .. --heavy-max records per mate in a tandem layout, 7 apart, strands at random.  (Heavy fragments of 10^3 .. 10^4 records at one in 1000
of 8 x 10^6 fragments would alone be 4 x 10^7 records per side and about 2 x 10^9 pairs; the default keeps 10^7 + 10^7 records: one in 40 000.)  One job on one card; the
legs are alternated --rounds times, each figure the mean of --steps runs after --warmup:
  (a) the baseline: one hipMemcpy of both record arrays into pinned host memory, then tools/mates_probe_host.cpp (g++ -O2, ONE host thread: std::sort of mate B's
      records per fragment, a bisection and a walk per record of mate A) writing the pairs into a host array; wall clock, once per round;
  (b) fmgpu_positions_mates device to device (out, out_off and out_class in device memory): the whole call between two events;
  (b0) its counting call alone: every pass but the write walk;
  (c) one device-to-device copy of the bytes of both record arrays.
The pairs and offsets of (a) and (b) are compared first.  --heavy-every 0 leaves the heavy fragments out (what they cost is the difference).  --only-mates runs leg (b)
alone, --steps times, for `rocprofv3 --kernel-trace --stats -- python tools/mates_probe.py --only-mates` (the passes kernel by kernel: this probe times whole calls
only, and the record of such a run is kept by hand as profiles/mates_probe_kernels.log).  Writes profiles/mates_probe.log (or --log)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from fmindex_collection_amd import capi
from fmindex_collection_amd.capi import MATE_PAIR_DTYPE, POSITION_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--fragments", type=int, default=8_000_000)
ap.add_argument("--heavy-every", type=int, default=40_000)
ap.add_argument("--heavy-min", type=int, default=1000)
ap.add_argument("--heavy-max", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--only-mates", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mates_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    if not args.only_mates:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if not torch.cuda.is_available():
    raise SystemExit("mates_probe needs a GPU: nothing is measured without one")
dev = torch.device("cuda", 0)
L = capi.lib()
props = torch.cuda.get_device_properties(0)
say(f"# python tools/mates_probe.py --fragments {args.fragments} --heavy-every {args.heavy_every} --heavy-min {args.heavy_min} --heavy-max {args.heavy_max} "
    f"--rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}")
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; clock_rate {getattr(props, 'clock_rate', 0) / 1e3:.0f} MHz; "
    f"memory_clock_rate {getattr(props, 'memory_clock_rate', 0) / 1e3:.0f} MHz; {props.total_memory / 2**30:.0f} GiB")

# ---- the records of both mates, made on the host and uploaded
M, n = 100, args.fragments
rng = np.random.default_rng(17)
f_all = np.arange(n)
kind = f_all % 8
heavy = (f_all % args.heavy_every) == args.heavy_every - 1 if args.heavy_every else np.zeros(n, dtype=bool)
start = rng.integers(0, 250_000_000, size=n)
insert = rng.integers(200, 601, size=n)
seq = rng.integers(0, 25, size=n)
flipped = rng.integers(0, 2, size=n).astype(bool)                        # mate A is the reverse one, downstream
heavy_count = rng.integers(args.heavy_min, args.heavy_max + 1, size=n)


def side(mate):
    per = np.ones(n, dtype=np.int64)
    per[kind == 3] = 2 + (f_all[kind == 3] // 8 + mate) % 2
    per[(kind == 5) & ((f_all // 8) % 2 == mate)] = 0
    per[heavy] = heavy_count[heavy] if mate == 0 else heavy_count[heavy][::-1]
    read = np.repeat(f_all, per)
    first = np.cumsum(per) - per
    k = np.arange(read.size) - first[read]                              # the record's number inside its run
    reverse = flipped[read] != bool(mate)                                # the true pair: one forward mate upstream, one reverse mate downstream
    rec = np.zeros(read.size, dtype=POSITION_DTYPE)
    true = (k == 0) & ~heavy[read]
    extra = ~true & ~heavy[read]
    strand = np.where(true, reverse, rng.integers(0, 2, size=read.size).astype(bool))
    rec["qidx"] = 2 * read + strand
    rec["seq_id"] = np.where(extra, rng.integers(0, 25, size=read.size), seq[read])
    pos = np.where(reverse, start[read] + insert[read] - M, start[read])
    pos = np.where(extra, rng.integers(0, 250_000_000, size=read.size), pos)
    rec["pos"] = np.where(heavy[read], start[read] + 7 * k, pos)
    rec["errors"] = rng.integers(0, 3, size=read.size)
    rec["hit"] = np.arange(read.size) & 0xffffffff
    return rec


host_a, host_b = side(0), side(1)
qoff_host = (np.arange(n + 1, dtype=np.uint64) * M)
rec_a = torch.from_numpy(host_a.view(np.int64).reshape(-1, 4).copy()).to(dev)
rec_b = torch.from_numpy(host_b.view(np.int64).reshape(-1, 4).copy()).to(dev)
qoff = torch.from_numpy(qoff_host.astype(np.int64)).to(dev)
ca, cb = len(host_a), len(host_b)
in_bytes = (ca + cb) * 32
spec = capi.MatesSpec(qoff.data_ptr(), qoff.data_ptr(), n, 0, 1000, 0, 1, 0, capi.MATES_FR, 0, (C.c_uint8 * 4)(0, 0, 0, 0))
d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
d_cls = torch.empty(n, dtype=torch.uint8, device=dev)


def join(out, capacity, off=None, cls=None):
    total = C.c_uint64()
    capi.check(L.fmgpu_positions_mates(C.c_void_p(rec_a.data_ptr()), ca, C.c_void_p(rec_b.data_ptr()), cb, C.byref(spec), None if out is None else C.c_void_p(out.data_ptr()),
                                       capacity, C.byref(total), None if off is None else C.c_void_p(off.data_ptr()), None if cls is None else C.c_void_p(cls.data_ptr()), None))
    return int(total.value)


pairs = join(None, 0, d_off, d_cls)
cls_count = np.bincount(d_cls.cpu().numpy(), minlength=6)
say(f"# {n} fragments ({int(heavy.sum())} heavy, {int(heavy_count[heavy].sum())} records per side in them); {ca} + {cb} records = {in_bytes} bytes; {pairs} pairs = {pairs * 32} bytes; "
    f"classes 0 .. 5: {cls_count.tolist()}")
d_out = torch.empty((max(pairs, 1), 4), dtype=torch.int64, device=dev)


def timed(run, events=True, steps=None, warmup=None):
    """mean ms per run: between two events on the stream the call uses, or by the host clock around work that ends in a synchronise"""
    for _ in range(args.warmup if warmup is None else warmup):
        run()
    torch.cuda.synchronize()
    steps = args.steps if steps is None else steps
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        run()
    b.record()
    torch.cuda.synchronize()
    return (a.elapsed_time(b) if events else (time.perf_counter() - t0) * 1e3) / steps


if args.only_mates:
    say(f"mates, device to device {timed(lambda: join(d_out, pairs, d_off, d_cls)):.2f} ms (under a profiler: not a figure)")
    raise SystemExit(0)

# ---- the baseline's helper, and the two results against each other
tmp = tempfile.TemporaryDirectory()
so = os.path.join(tmp.name, "mates_probe_host.so")
subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "mates_probe_host.cpp"), "-o", so], check=True)
H = C.CDLL(so)
H.mates_join.restype = C.c_uint64
H.mates_join.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
pinned_a, pinned_b = torch.empty((ca, 4), dtype=torch.int64).pin_memory(), torch.empty((cb, 4), dtype=torch.int64).pin_memory()
host_out = np.zeros(max(pairs, 1), dtype=MATE_PAIR_DTYPE)
host_off = np.zeros(n + 1, dtype=np.uint64)
parts = {"copy": [], "join": []}


def baseline():
    t0 = time.perf_counter()
    pinned_a.copy_(rec_a)
    pinned_b.copy_(rec_b)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = H.mates_join(pinned_a.data_ptr(), ca, pinned_b.data_ptr(), cb, qoff_host.ctypes.data, qoff_host.ctypes.data, n, 0, 1000, host_out.ctypes.data, host_out.size,
                       host_off.ctypes.data)
    t2 = time.perf_counter()
    assert got == pairs, (got, pairs)
    parts["copy"].append((t1 - t0) * 1e3)
    parts["join"].append((t2 - t1) * 1e3)


baseline()
assert join(d_out, pairs, d_off, d_cls) == pairs
assert np.array_equal(d_out.cpu().numpy().reshape(-1)[: pairs * 4], host_out.view(np.int64).reshape(-1)[: pairs * 4]), "the device pairs differ from the host join's"
assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), host_off), "the device offsets differ from the host join's"
say("# the device pairs and offsets equal the host join's, record for record")
parts = {"copy": [], "join": []}

src = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
landing = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
legs = {
    "a  baseline: both arrays to pinned host + std::sort join, one host thread": (baseline, dict(events=False, steps=1, warmup=0)),
    "b  mates, device to device": (lambda: join(d_out, pairs, d_off, d_cls), {}),
    "b0 mates, the counting call alone (every pass but the write walk)": (lambda: join(None, 0), {}),
    "c  device -> device copy of the input bytes": (lambda: landing.copy_(src), {}),
}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for k, (run, kw) in legs.items():
        times[k].append(timed(run, **kw))
    say(f"round {r}: " + "; ".join(f"{k.split()[0]} {times[k][-1]:.2f} ms" for k in legs))
mean = {k: float(np.mean(v)) for k, v in times.items()}
for k, v in times.items():
    say(f"({k}): mean {mean[k]:9.2f} ms, min {min(v):9.2f}, max {max(v):9.2f}  = {(ca + cb) / mean[k] / 1e3:9.1f} M records/s, {in_bytes / mean[k] / 1e6:8.2f} GB/s of input")
say(f"(a  parts): hipMemcpy of {in_bytes} bytes to pinned host mean {np.mean(parts['copy']):.2f} ms; the join mean {np.mean(parts['join']):.2f} ms")
ka, kb, kb0, kc = (next(k for k in legs if k.split()[0] == tag) for tag in ("a", "b", "b0", "c"))
say(f"write walk (b - b0) = {mean[kb] - mean[kb0]:.2f} ms for {pairs * 32} bytes of pairs; ratios: baseline / device-to-device = {mean[ka] / mean[kb]:.1f}x; "
    f"device-to-device / copy (c) = {mean[kb] / mean[kc]:.1f}x")
