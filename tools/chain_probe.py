"""dev probe: fmgpu_seeds_chain on device-resident synthetic anchors of --queries queries.  The mix: a light query has 1 .. 20 seeds (25 apart in the read, 20 long);
about 70 % of them lie on the read's true diagonal, with an indel of 0 .. 2 bases between neighbours, the others anywhere on any of 25 sequences (runs of one anchor);
one query in --heavy-every is heavy: --heavy-anchors anchors of 20 seeds on a tandem repeat (period 50), one run, ties everywhere.  The default is 10^6 queries with one
heavy query in 10 000: 100 heavy queries of 10^4 anchors beside about 1.05 x 10^7 light anchors.  One job on one card; the legs are alternated --rounds times, each
figure the mean of --steps runs after --warmup:
  (a) the baseline: one hipMemcpy of the records and spans into pinned host memory, then tools/chain_probe_host.cpp (g++ -O2, ONE host thread) writing chains and
      anchors into host arrays; wall clock, once per round;
  (b) fmgpu_seeds_chain device to device (out, out_anchor, out_off and out_class in device memory): the whole call between two events;
  (b0) its counting call alone: every pass up to the read-back;
  (c) one device-to-device copy of the bytes of the records.
The chains, anchors and offsets of (a) and (b) are compared first.  --heavy-every 0 leaves the heavy queries out (what long runs cost is the difference).  --only-chain
runs leg (b) alone, --steps times, for `rocprofv3 --kernel-trace --stats -- python tools/chain_probe.py --only-chain` (the passes kernel by kernel; the record of such a
run is kept by hand as profiles/chain_probe_kernels.log).  Writes profiles/chain_probe.log (or --log)."""
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
from fmindex_collection_amd.capi import CHAIN_DTYPE, POSITION_DTYPE, SEED_SPAN_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--heavy-every", type=int, default=10_000)
ap.add_argument("--heavy-anchors", type=int, default=10_000)
ap.add_argument("--max-lookback", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--only-chain", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "chain_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    if not args.only_chain:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if not torch.cuda.is_available():
    raise SystemExit("chain_probe needs a GPU: nothing is measured without one")
dev = torch.device("cuda", 0)
L = capi.lib()
props = torch.cuda.get_device_properties(0)
say(f"# python tools/chain_probe.py --queries {args.queries} --heavy-every {args.heavy_every} --heavy-anchors {args.heavy_anchors} --max-lookback {args.max_lookback} "
    f"--rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}")
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; {props.total_memory / 2**30:.0f} GiB")

# ---- the anchors, made on the host and uploaded: anchor i has span i
nq = args.queries
rng = np.random.default_rng(29)
q_all = np.arange(nq)
heavy = (q_all % args.heavy_every) == args.heavy_every - 1 if args.heavy_every else np.zeros(nq, dtype=bool)
per = rng.integers(1, 21, size=nq)
per[heavy] = args.heavy_anchors
count = int(per.sum())
query = np.repeat(q_all, per)
first = np.cumsum(per) - per
k = np.arange(count) - first[query]                                      # the anchor's number inside its query
is_heavy = heavy[query]
start = rng.integers(0, 250_000_000, size=nq)
seq = rng.integers(0, 25, size=nq)
true = rng.random(count) < 0.7
shift = np.cumsum(rng.integers(0, 3, size=count)) % 7                    # a slowly drifting diagonal: indels of a few bases
copies = max(args.heavy_anchors // 20, 1)
rec = np.zeros(count, dtype=POSITION_DTYPE)
spans = np.zeros(count, dtype=SEED_SPAN_DTYPE)
rec["qidx"] = query
rec["seq_id"] = np.where(is_heavy | true, seq[query], rng.integers(0, 25, size=count))
light_q = 25 * k
rec["pos"] = np.where(is_heavy, start[query] + 50 * (k // copies + k % copies),
                      np.where(true, start[query] + light_q + shift, rng.integers(0, 250_000_000, size=count)))
rec["hit"] = np.arange(count) & 0xffffffff
spans["qbeg"] = np.where(is_heavy, 50 * (k // copies), light_q)
spans["qlen"] = np.where(is_heavy, 25, 20)
d_rec = torch.from_numpy(rec.view(np.int64).reshape(-1, 4).copy()).to(dev)
d_spans = torch.from_numpy(spans.view(np.int64).copy()).to(dev)
in_bytes = count * 40
spec = capi.ChainSpec(nq, 5000, 500, 128, args.max_lookback, 0, 1, 0, 0, (C.c_uint8 * 8)())
d_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
d_cls = torch.empty(nq, dtype=torch.uint8, device=dev)
d_anchor = torch.empty(count, dtype=torch.int32, device=dev)


def chain(out, capacity, anchors=None, off=None, cls=None):
    total = C.c_uint64()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
    capi.check(L.fmgpu_seeds_chain(ptr(d_rec), count, ptr(d_spans), count, C.byref(spec), ptr(out), capacity, C.byref(total), ptr(anchors), ptr(off), ptr(cls), None))
    return int(total.value)


chains = chain(None, 0, None, d_off, d_cls)
cls_count = np.bincount(d_cls.cpu().numpy(), minlength=4)
say(f"# {nq} queries ({int(heavy.sum())} heavy = {heavy.mean():.6f} of them, {int(per[heavy].sum())} anchors in them); {count} anchors = {in_bytes} bytes of records and spans; "
    f"{chains} chains = {chains * 56} bytes; classes 0 .. 3: {cls_count.tolist()}")
d_out = torch.empty((max(chains, 1), 7), dtype=torch.int64, device=dev)


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


if args.only_chain:
    say(f"chain, device to device {timed(lambda: chain(d_out, chains, d_anchor, d_off, d_cls)):.2f} ms (under a profiler: not a figure)")
    raise SystemExit(0)

# ---- the baseline's helper, and the two results against each other
tmp = tempfile.TemporaryDirectory()
so = os.path.join(tmp.name, "chain_probe_host.so")
subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "chain_probe_host.cpp"), "-o", so], check=True)
H = C.CDLL(so)
H.chain_host.restype = C.c_uint64
H.chain_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_uint32] * 8 + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
pinned_rec, pinned_spans = torch.empty((count, 4), dtype=torch.int64).pin_memory(), torch.empty(count, dtype=torch.int64).pin_memory()
host_out = np.zeros(max(chains, 1), dtype=CHAIN_DTYPE)
host_anchor = np.zeros(count, dtype=np.uint32)
host_off = np.zeros(nq + 1, dtype=np.uint64)
parts = {"copy": [], "chain": []}


def baseline():
    t0 = time.perf_counter()
    pinned_rec.copy_(d_rec)
    pinned_spans.copy_(d_spans)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = H.chain_host(pinned_rec.data_ptr(), count, pinned_spans.data_ptr(), nq, 5000, 500, 128, args.max_lookback, 0, 1, 0, 0, host_out.ctypes.data, host_out.size,
                       host_anchor.ctypes.data, host_off.ctypes.data)
    t2 = time.perf_counter()
    assert got == chains, (got, chains)
    parts["copy"].append((t1 - t0) * 1e3)
    parts["chain"].append((t2 - t1) * 1e3)


baseline()
assert chain(d_out, chains, d_anchor, d_off, d_cls) == chains
assert np.array_equal(d_out.cpu().numpy().reshape(-1)[: chains * 7], host_out.view(np.int64).reshape(-1)[: chains * 7]), "the device chains differ from the host's"
used = int(host_out["n_anchors"][:chains].sum())
assert np.array_equal(d_anchor.cpu().numpy().view(np.uint32)[:used], host_anchor[:used]), "the device anchors differ from the host's"
assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), host_off), "the device offsets differ from the host's"
say(f"# the device chains, anchors ({used}) and offsets equal the host's, record for record; the longest chain has {int(host_out['n_anchors'].max())} anchors")
parts = {"copy": [], "chain": []}

src = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
landing = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
legs = {
    "a  baseline: records and spans to pinned host + the rule on one host thread": (baseline, dict(events=False, steps=1, warmup=0)),
    "b  chain, device to device": (lambda: chain(d_out, chains, d_anchor, d_off, d_cls), {}),
    "b0 chain, the counting call alone (every pass up to the read-back)": (lambda: chain(None, 0), {}),
    "c  device -> device copy of the input bytes": (lambda: landing.copy_(src), {}),
}
times = {name: [] for name in legs}
for r in range(args.rounds):
    for name, (run, kw) in legs.items():
        times[name].append(timed(run, **kw))
    say(f"round {r}: " + "; ".join(f"{name.split()[0]} {times[name][-1]:.2f} ms" for name in legs))
mean = {name: float(np.mean(v)) for name, v in times.items()}
for name, v in times.items():
    say(f"({name}): mean {mean[name]:9.2f} ms, min {min(v):9.2f}, max {max(v):9.2f}  = {count / mean[name] / 1e3:9.1f} M anchors/s")
say(f"(a  parts): hipMemcpy of {in_bytes} bytes to pinned host mean {np.mean(parts['copy']):.2f} ms; the host rule mean {np.mean(parts['chain']):.2f} ms")
ka, kb, kb0, kc = (next(name for name in legs if name.split()[0] == tag) for tag in ("a", "b", "b0", "c"))
say(f"order, records and scatter (b - b0) = {mean[kb] - mean[kb0]:.2f} ms for {chains} chains; ratios: baseline / device-to-device = {mean[ka] / mean[kb]:.1f}x; "
    f"device-to-device / copy (c) = {mean[kb] / mean[kc]:.1f}x")
