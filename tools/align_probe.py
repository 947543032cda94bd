"""dev probe: fmgpu_chains_align on device-resident input.  The batch is tools/chain_probe.py's (a light query has 1 .. 20 seeds, 25 apart in the read and 20 long, about
70 % of them on the read's diagonal with an indel of 0 .. 2 bases between neighbours; one query in --heavy-every is heavy: --heavy-anchors anchors of 20 seeds on a tandem
repeat), passed through fmgpu_seeds_chain.  Reads are random; the text window of every chain is written from its read: the pieces copied, each gap's text the read's gap
symbols (cut or continued with random ones to the gap's text length) with a share of --divergence of them replaced: every piece is a true match and every gap has planted
differences.  One job on one card; the legs are alternated --rounds times, each figure the mean of --steps runs after --warmup:
  (a) the baseline: one hipMemcpy of all input arrays into pinned host memory, then tools/align_probe_host.cpp (g++ -O2, ONE host thread); wall clock, once per round;
  (b) fmgpu_chains_align device to device: the whole call between two events;
  (b0) its counting call alone: every pass up to the read-back, every matrix once;
  (c) one device-to-device copy of the input bytes.
The records and operations of (a) and (b) are compared first.  --heavy-every 0 leaves the heavy queries out.  --only-align runs leg (b) alone, --steps times, for
`rocprofv3 --kernel-trace --stats -- python tools/align_probe.py --only-align` (the split by kernel).  Writes profiles/align_probe.log (or --log)."""
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
from fmindex_collection_amd.capi import CHAIN_ALIGNMENT_DTYPE, CHAIN_DTYPE, POSITION_DTYPE, SEED_SPAN_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=200_000)
ap.add_argument("--heavy-every", type=int, default=10_000)
ap.add_argument("--heavy-anchors", type=int, default=10_000)
ap.add_argument("--divergence", type=float, default=0.08)
ap.add_argument("--band", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--only-align", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "align_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    if not args.only_align:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if not torch.cuda.is_available():
    raise SystemExit("align_probe needs a GPU: nothing is measured without one")
dev = torch.device("cuda", 0)
L = capi.lib()
props = torch.cuda.get_device_properties(0)
say(f"# python tools/align_probe.py --queries {args.queries} --heavy-every {args.heavy_every} --heavy-anchors {args.heavy_anchors} --divergence {args.divergence} --band {args.band} "
    f"--rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}")
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; {props.total_memory / 2**30:.0f} GiB")

# ---- the anchors of tools/chain_probe.py: anchor i has span i
nq = args.queries
rng = np.random.default_rng(29)
q_all = np.arange(nq)
heavy = (q_all % args.heavy_every) == args.heavy_every - 1 if args.heavy_every else np.zeros(nq, dtype=bool)
per = rng.integers(1, 21, size=nq)
per[heavy] = args.heavy_anchors
count = int(per.sum())
query = np.repeat(q_all, per)
k = np.arange(count) - (np.cumsum(per) - per)[query]
is_heavy = heavy[query]
start = rng.integers(0, 250_000_000, size=nq)
seq = rng.integers(0, 25, size=nq)
true = rng.random(count) < 0.7
shift = np.cumsum(rng.integers(0, 3, size=count)) % 7
copies = max(args.heavy_anchors // 20, 1)
rec = np.zeros(count, dtype=POSITION_DTYPE)
spans = np.zeros(count, dtype=SEED_SPAN_DTYPE)
rec["qidx"] = query
rec["seq_id"] = np.where(is_heavy | true, seq[query], rng.integers(0, 25, size=count))
rec["pos"] = np.where(is_heavy, start[query] + 50 * (k // copies + k % copies), np.where(true, start[query] + 25 * k + shift, rng.integers(0, 250_000_000, size=count)))
rec["hit"] = np.arange(count) & 0xffffffff
spans["qbeg"] = np.where(is_heavy, 50 * (k // copies), 25 * k)
spans["qlen"] = np.where(is_heavy, 25, 20)

# ---- the chains, from the library
chain_spec = capi.ChainSpec(nq, 5000, 500, 128, 64, 0, 1, 0, 0, (C.c_uint8 * 8)())
total = C.c_uint64()
capi.check(L.fmgpu_seeds_chain(capi.ptr(rec), count, capi.ptr(spans), count, C.byref(chain_spec), None, 0, C.byref(total), None, None, None, None))
n_chains = int(total.value)
chains, anchors = np.zeros(n_chains, dtype=CHAIN_DTYPE), np.zeros(count, dtype=np.uint32)
capi.check(L.fmgpu_seeds_chain(capi.ptr(rec), count, capi.ptr(spans), count, C.byref(chain_spec), capi.ptr(chains), n_chains, C.byref(total), capi.ptr(anchors), None, None, None))
n_anchor = int(chains["n_anchors"].sum())
anchors = anchors[:n_anchor].copy()

# ---- reads, and every chain's window written from its read
qlen = np.where(heavy, 50 * 20 + 40, 25 * 20 + 40).astype(np.uint64)
qoff = np.zeros(nq + 1, dtype=np.uint64)
qoff[1:] = np.cumsum(qlen)
qbuf = rng.integers(1, 5, size=int(qoff[-1]) + 1).astype(np.uint8)
e_chain = np.repeat(np.arange(n_chains), chains["n_anchors"])
e_k = np.arange(n_anchor) - chains["first"][e_chain]
a_rec = rec[anchors]
e_q, e_l, e_t = spans["qbeg"][a_rec["hit"]].astype(np.int64), spans["qlen"][a_rec["hit"]].astype(np.int64), a_rec["pos"].astype(np.int64)
last = e_k == chains["n_anchors"][e_chain] - 1
nxt = np.minimum(np.arange(n_anchor) + 1, n_anchor - 1)
dq, dt = np.where(last, 0, e_q[nxt] - e_q), np.where(last, 0, e_t[nxt] - e_t)
lp = np.where(last, e_l, np.minimum(e_l, np.minimum(dq, dt)))
gq, gt = np.where(last, 0, dq - lp), np.where(last, 0, dt - lp)
seg = lp + gt                                                            # the text symbols an element writes: its piece and the gap behind it
seg_start = np.cumsum(seg) - seg
n_text = int(seg.sum())
elem = np.repeat(np.arange(n_anchor), seg)
within = np.arange(n_text) - seg_start[elem]
src = qoff[a_rec["qidx"]].astype(np.int64)[elem] + e_q[elem] + within
from_read = within < (lp + gq)[elem]
tbuf = np.where(from_read, qbuf[np.minimum(src, qbuf.size - 1)], rng.integers(1, 5, size=n_text)).astype(np.uint8)
planted = (within >= lp[elem]) & (rng.random(n_text) < args.divergence)
tbuf[planted] = (tbuf[planted] - 1 + rng.integers(1, 4, size=int(planted.sum()))) % 4 + 1
tbuf = np.concatenate([tbuf, np.zeros(1, dtype=np.uint8)])
toff = np.zeros(n_chains + 1, dtype=np.uint64)
toff[1:] = np.cumsum(chains["tend"] - chains["tbeg"])
assert int(toff[-1]) == n_text
dp = (gq > 0) & (gt > 0)
say(f"# {nq} queries ({int(heavy.sum())} heavy), {count} anchors -> {n_chains} chains of {n_anchor} anchors; {int(qoff[-1])} read symbols, {n_text} text symbols; "
    f"{int(dp.sum())} gaps through a matrix ({int((dp & (gq <= 15) & (gt <= 15)).sum())} of up to 15 x 15), the largest {int(gq[dp].max()) if dp.any() else 0} x {int(gt[dp].max()) if dp.any() else 0}, "
    f"{int(((gq > 0) != (gt > 0)).sum())} pure insertions or deletions")

host = dict(chains=chains, anchors=anchors, positions=rec, spans=spans, qbuf=qbuf, qoff=qoff, tbuf=tbuf, toff=toff)
NAMES = ("chains", "anchors", "positions", "spans", "qbuf", "qoff", "tbuf", "toff")
d = {name: torch.from_numpy(host[name].view(np.uint8).reshape(-1).copy()).to(dev) for name in NAMES}
in_bytes = sum(int(t.numel()) for t in d.values())
spec = capi.AlignSpec(nq, 1 << 24, args.band, 5000, (C.c_uint8 * 8)())
d_out = torch.empty(n_chains * 32, dtype=torch.uint8, device=dev)


def align(ops, capacity):
    n = C.c_uint64()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
    capi.check(L.fmgpu_chains_align(p(d["chains"]), n_chains, p(d["anchors"]), n_anchor, p(d["positions"]), count, p(d["spans"]), count, p(d["qbuf"]), p(d["qoff"]),
                                    p(d["tbuf"]), p(d["toff"]), C.byref(spec), p(d_out), p(ops), capacity, C.byref(n), None))
    return int(n.value)


n_ops = align(None, 0)
d_ops = torch.empty(max(n_ops, 1), dtype=torch.int32, device=dev)
say(f"# {n_ops} operations = {n_ops * 4} bytes; {in_bytes} bytes of input")


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


if args.only_align:
    say(f"align, device to device {timed(lambda: align(d_ops, n_ops)):.2f} ms (under a profiler: not a figure)")
    raise SystemExit(0)

# ---- the baseline's helper, and the two results against each other
tmp = tempfile.TemporaryDirectory()
so = os.path.join(tmp.name, "align_probe_host.so")
subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "align_probe_host.cpp"), "-o", so], check=True)
H = C.CDLL(so)
H.align_host.restype = C.c_uint64
H.align_host.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
pinned = {name: torch.empty(d[name].numel(), dtype=torch.uint8).pin_memory() for name in NAMES}
host_out = np.zeros(n_chains, dtype=CHAIN_ALIGNMENT_DTYPE)
host_ops = np.zeros(max(n_ops, 1), dtype=np.uint32)
cells = C.c_uint64()
parts = {"copy": [], "align": []}


def baseline():
    t0 = time.perf_counter()
    for name in NAMES:
        pinned[name].copy_(d[name])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = H.align_host(pinned["chains"].data_ptr(), n_chains, *(pinned[name].data_ptr() for name in NAMES[1:]), args.band, 5000, 1 << 24, host_out.ctypes.data,
                       host_ops.ctypes.data, C.byref(cells))
    t2 = time.perf_counter()
    assert got == n_ops, (got, n_ops)
    parts["copy"].append((t1 - t0) * 1e3)
    parts["align"].append((t2 - t1) * 1e3)


baseline()
assert align(d_ops, n_ops) == n_ops
assert d_out.cpu().numpy().tobytes() == host_out.tobytes(), "the device records differ from the host's"
assert np.array_equal(d_ops.cpu().numpy().view(np.uint32)[:n_ops], host_ops[:n_ops]), "the device operations differ from the host's"
say(f"# the device records and operations equal the host's; {int(cells.value)} cells in the matrices; bases under = X I D: "
    f"{[int(host_out[f].sum(dtype=np.uint64)) for f in ('n_match', 'n_mismatch', 'n_ins', 'n_del')]}; {int((host_out['status'] == 1).sum())} chains left out")
parts = {"copy": [], "align": []}

src_, landing = torch.empty(in_bytes, dtype=torch.uint8, device=dev), torch.empty(in_bytes, dtype=torch.uint8, device=dev)
legs = {
    "a  baseline: the input to pinned host + the rule on one host thread": (baseline, dict(events=False, steps=1, warmup=0)),
    "b  align, device to device": (lambda: align(d_ops, n_ops), {}),
    "b0 align, the counting call alone (every pass up to the read-back)": (lambda: align(None, 0), {}),
    "c  device -> device copy of the input bytes": (lambda: landing.copy_(src_), {}),
}
times = {name: [] for name in legs}
for r in range(args.rounds):
    for name, (run, kw) in legs.items():
        times[name].append(timed(run, **kw))
    say(f"round {r}: " + "; ".join(f"{name.split()[0]} {times[name][-1]:.2f} ms" for name in legs))
mean = {name: float(np.mean(v)) for name, v in times.items()}
for name, v in times.items():
    say(f"({name}): mean {mean[name]:9.2f} ms, min {min(v):9.2f}, max {max(v):9.2f}  = {n_anchor / mean[name] / 1e3:9.1f} M anchors/s")
say(f"(a  parts): hipMemcpy of {in_bytes} bytes to pinned host mean {np.mean(parts['copy']):.2f} ms; the host rule mean {np.mean(parts['align']):.2f} ms "
    f"= {cells.value / np.mean(parts['align']) / 1e6:.2f} G cells/s")
ka, kb, kb0, kc = (next(name for name in legs if name.split()[0] == tag) for tag in ("a", "b", "b0", "c"))
say(f"cells: the counting call fills every matrix once = {cells.value / mean[kb0] / 1e6:.2f} G cells/s; the writing call twice = {2 * cells.value / mean[kb] / 1e6:.2f} G cells/s; "
    f"ratios: baseline / device-to-device = {mean[ka] / mean[kb]:.1f}x; device-to-device / copy (c) = {mean[kb] / mean[kc]:.1f}x")
