"""dev probe: best-stratum search on the genome stand-in (datasets.genome_like_text with bench.GRCH38_LENGTHS scaled by --scale; BiFMIndex<5, IB16>, plain index),
--nq reads of --length symbols, read i with i % 4 substitutions, ladder h2(k + 2, 0, k) for k = 0 .. 2 (Hamming distance), the batch resident in HBM.
  (a) end to end, wall ms, alternated --rounds times: fmgpu_search_best through the Python mirror (search_best(schemes=...)) against the host loop that mirror was
      before — kept in this file only (host_loop below: pull the batch to the host, per scheme re-flatten the reads that found nothing, upload, search, download,
      mark and rename on the host).  The records must be equal.
  (b) the share of one raw fmgpu_search_best call (records left in HBM) spent outside the strata's search kernels: wall time minus the sum of stats[i].kernel_ms
      — the hand-out prepass of the strata (stats[i].prepass_ms, reported beside it), mark, select, gather, the read-backs and the calls' own set-up.
Both figures are reported with the card's id and clocks; nothing is asserted on them.  Writes profiles/search_best_probe.log (or --log)."""
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
from fmindex_collection_amd.capi import HIT_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--nq", type=int, default=2_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "search_best_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


def host_loop(index, queries, schemes, n=fm.UINT64_MAX, edit=False):
    """search_best(schemes=[(scheme, partition), ...]) as it was before fmgpu_search_best: a host loop around the single-scheme call"""
    qbuf, qoff, nq = fm._queries(queries)
    if not isinstance(qoff, np.ndarray):
        qoff = qoff.to_array(np.uint64, nq + 1)
    if not isinstance(qbuf, np.ndarray):
        qbuf = qbuf.to_array(np.uint8, int(qoff[-1]))
    todo = np.arange(nq)
    parts = []
    for sch, part in schemes:
        if todo.size == 0:
            break
        qb, qo = fm.flatten([qbuf[int(qoff[i]): int(qoff[i + 1])] for i in todo])
        hits = fm.search_ng26.search(index, (qb, qo), sch, part, n, edit=edit).copy()
        found = np.unique(hits["qidx"].astype(np.int64))
        hits["qidx"] = todo.astype(np.uint64)[hits["qidx"].astype(np.int64)]
        parts.append(hits)
        todo = np.delete(todo, found)
    if not parts:
        return np.zeros(0, dtype=HIT_DTYPE)
    hits = np.concatenate(parts)
    return hits[np.lexsort((hits["seq"], hits["qidx"]))]


dev = torch.device("cuda", 0)
c = types.SimpleNamespace(torch=torch, np=np, datasets=datasets, dev=dev, rank=0, args=types.SimpleNamespace(scale=args.scale))
L = capi.lib()
say(f"# python tools/search_best_probe.py --scale {args.scale} --nq {args.nq} --length {args.length} --rounds {args.rounds}")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
nq, m = args.nq, args.length
gq = torch.Generator(device=dev)
gq.manual_seed(1000)
starts = torch.randint(0, text.numel() - m, (nq,), generator=gq, device=dev, dtype=torch.int64)
reads = torch.empty((nq, m), dtype=torch.uint8, device=dev)
ar = torch.arange(m, device=dev, dtype=torch.int64)
for lo in range(0, nq, 1 << 20):
    hi = min(nq, lo + (1 << 20))
    reads[lo:hi] = text[starts[lo:hi, None] + ar[None, :]]
rows = torch.arange(nq, device=dev)
for k in range(3):                                                   # read i: i % 4 substitutions
    sel = rows[rows % 4 > k]
    pos = torch.randint(0, m, (sel.numel(),), generator=gq, device=dev)
    shift = torch.randint(1, 4, (sel.numel(),), generator=gq, device=dev, dtype=torch.uint8)
    reads[sel, pos] = (reads[sel, pos] - 1 + shift) % 4 + 1
qbuf = reads.reshape(-1)
qoff = torch.arange(nq + 1, device=dev, dtype=torch.int64) * m
torch.cuda.synchronize()
fm.options["lf_table"] = 0
t0 = time.time()
index = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
torch.cuda.synchronize()
say(f"# genome stand-in, {int(text.numel())} symbols, {len(lengths)} sequences; plain BiFMIndex (formats {index.formats:#x}, {index.device_bytes / 1e9:.2f} GB) built in "
    f"{time.time() - t0:.1f} s; {nq} reads x {m} symbols, read i with i % 4 substitutions, in HBM")
del text
ladder = [(fm.search_scheme.h2(k + 2, 0, k), None) for k in range(3)]
batch = (capi.DeviceBuffer.from_array(qbuf.cpu().numpy()), capi.DeviceBuffer.from_array(qoff.cpu().numpy().astype(np.uint64)))     # the same batch as DeviceBuffers: what the host loop pulls back
smi = bench.Smi(0)
smi.start()


def wall(f):
    torch.cuda.synchronize()
    t = time.time()
    out = f()
    torch.cuda.synchronize()
    return (time.time() - t) * 1e3, out


say("# (a) end to end, device-resident batch -> host records in callback order, wall ms")
ms_new, ms_old = [], []
for r in range(args.rounds):
    t, new = wall(lambda: fm.search_best(index, batch, 0, edit=False, schemes=ladder))
    ms_new.append(t)
    say(f"device_{r + 1:<3d} {t:10.1f}  {len(new)} records")
    t, old = wall(lambda: host_loop(index, batch, ladder))
    ms_old.append(t)
    say(f"host_{r + 1:<5d} {t:10.1f}  {len(old)} records")
equal = len(new) == len(old) and all(np.array_equal(new[k], old[k]) for k in ("qidx", "lb", "lb_rev", "len", "errors", "seq"))
say(f"# records equal: {equal}")
say(f"# best of {args.rounds}: device call {min(ms_new):.1f} ms, host loop {min(ms_old):.1f} ms -> device / host = {min(ms_new) / min(ms_old):.4f}; "
    f"means {np.mean(ms_new):.1f} / {np.mean(ms_old):.1f} ms")

say("# (b) one raw fmgpu_search_best call, records left in HBM: wall ms, the strata's kernel_ms, prepass_ms and hits")
pi_keep = [tuple(np.ascontiguousarray(np.asarray(x, dtype=np.uint64)) for x in sch) for sch, _ in ladder]
arr = (capi.Scheme * 3)()
for sc, (pi, l, u) in zip(arr, pi_keep):
    sc.n_searches, sc.n_parts = pi.shape
    sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    sc.partition, sc.edit = None, 0
cap = max(len(new) + 1024, 4 * nq)
out = torch.empty(cap * HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
strat = torch.empty(nq, dtype=torch.uint8, device=dev)
stats = (capi.Stats * 3)()
cnt = C.c_uint64()
ptr = lambda t: C.c_void_p(t.data_ptr())
shares = []
for r in range(args.rounds):
    t, rc = wall(lambda: L.fmgpu_search_best(index._h, ptr(qbuf), ptr(qoff), nq, arr, 3, fm.UINT64_MAX, ptr(out), cap, C.byref(cnt), ptr(strat), stats, None))
    capi.check(rc)
    kern, pre = sum(stats[i].kernel_ms for i in range(3)), sum(stats[i].prepass_ms for i in range(3))
    shares.append(((t - kern) / t, (t - kern - pre) / t))
    say(f"raw_{r + 1:<6d} {t:10.1f}  kernel_ms {' '.join('%.1f' % stats[i].kernel_ms for i in range(3))}  prepass_ms {' '.join('%.1f' % stats[i].prepass_ms for i in range(3))}  "
        f"hits {' '.join(str(stats[i].hits) for i in range(3))}  outside the search kernels {100 * shares[-1][0]:.1f} %  (without the hand-out prepass {100 * shares[-1][1]:.1f} %)")
one = capi.Stats()
for r in range(args.rounds):                                         # what one single-scheme call costs around its kernel: the ladder pays that once per stratum
    t, rc = wall(lambda: L.fmgpu_search_scheme(index._h, ptr(qbuf), ptr(qoff), nq, arr, fm.UINT64_MAX, ptr(out), cap, C.byref(cnt), C.byref(one), None))
    capi.check(rc)
    say(f"single_{r + 1:<3d} {t:10.1f}  fmgpu_search_scheme with scheme 0 over the whole batch: kernel_ms {one.kernel_ms:.1f}, prepass_ms {one.prepass_ms:.1f}, {t - one.kernel_ms:.1f} ms outside the kernel")
capi.check(L.fmgpu_search_best(index._h, ptr(qbuf), ptr(qoff), nq, arr, 3, fm.UINT64_MAX, ptr(out), cap, C.byref(cnt), ptr(strat), stats, None))
found = [int((strat == i).sum()) for i in range(3)] + [int((strat == 255).sum())]
say(f"# reads found in strata 0 / 1 / 2 / none: {found}; {cnt.value} records")
say(f"# share outside the strata's search kernels, best of {args.rounds}: {100 * min(s[0] for s in shares):.1f} % of the call ({100 * min(s[1] for s in shares):.1f} % without the hand-out prepass)")
ck = smi.stop()
say(f"# card {ck.get('card') if ck else None}; clocks during the run: {ck}")
