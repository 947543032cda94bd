"""dev probe: fmgpu_search_smems on the genome stand-in (datasets.genome_like_text with bench.GRCH38_LENGTHS scaled by --scale; FMIndex<5, IB16>, plain index),
--nq reads of --length symbols in HBM: one third exact copies of text windows, one third with 3 - 6 substitutions, one third chimeras of two windows.
  (a) the walk kernel: kernel_ms, lf_steps, steps/s, seeds per read, and its lane utilisation computed from out_match_len: sum of L over, per wave of 64
      consecutive batch symbols, 64 x the wave's largest L (a wave runs until its longest walk is done);
  (b) the yardstick, same run, same handle, same reads: fmgpu_search_exact under FMGPU_SEL_EXACT_ONE_SYMBOL (k_exact_a) — the same unit of work: one-symbol LF steps,
      two interval ends, one load where both ends share a block.
The figure: the walk's steps/s divided by its lane utilisation, over k_exact_a's steps/s.  Alternated --rounds times; the best and the mean of each are reported with
the card's id and clocks; nothing is asserted.  Writes profiles/smems_probe.log (or --log)."""
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
ap.add_argument("--nq", type=int, default=1_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--min-len", type=int, default=1)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "smems_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


dev = torch.device("cuda", 0)
c = types.SimpleNamespace(torch=torch, np=np, datasets=datasets, dev=dev, rank=0, args=types.SimpleNamespace(scale=args.scale))
L = capi.lib()
say(f"# python tools/smems_probe.py --scale {args.scale} --nq {args.nq} --length {args.length} --rounds {args.rounds} --min-len {args.min_len}")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
nq, m = args.nq, args.length
gq = torch.Generator(device=dev)
gq.manual_seed(1000)
ar = torch.arange(m, device=dev, dtype=torch.int64)


def windows(count):
    starts = torch.randint(0, text.numel() - m, (count,), generator=gq, device=dev, dtype=torch.int64)
    out = torch.empty((count, m), dtype=torch.uint8, device=dev)
    for lo in range(0, count, 1 << 20):
        hi = min(count, lo + (1 << 20))
        out[lo:hi] = text[starts[lo:hi, None] + ar[None, :]]
    return out


reads = windows(nq)
rows = torch.arange(nq, device=dev)
for k in range(6):                                                   # reads 1 mod 3: 3 + (i // 3) % 4 substitutions
    sel = rows[(rows % 3 == 1) & (3 + (rows // 3) % 4 > k)]
    pos = torch.randint(0, m, (sel.numel(),), generator=gq, device=dev)
    shift = torch.randint(1, 4, (sel.numel(),), generator=gq, device=dev, dtype=torch.uint8)
    reads[sel, pos] = (reads[sel, pos] - 1 + shift) % 4 + 1
sel = rows[rows % 3 == 2]                                            # reads 2 mod 3: the head of one window, the tail of another, the joint at 30 .. 70 % of the read
other = windows(sel.numel())
cut = torch.randint(int(0.3 * m), int(0.7 * m) + 1, (sel.numel(),), generator=gq, device=dev)
reads[sel] = torch.where(ar[None, :] < cut[:, None], reads[sel], other)
del other
qbuf = reads.reshape(-1)
qoff = torch.arange(nq + 1, device=dev, dtype=torch.int64) * m
total = nq * m
torch.cuda.synchronize()
fm.options["lf_table"] = 0
t0 = time.time()
index = fm.FMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
torch.cuda.synchronize()
say(f"# genome stand-in, {int(text.numel())} symbols, {len(lengths)} sequences; plain FMIndex (formats {index.formats:#x}, {index.device_bytes / 1e9:.2f} GB, {index.row_bits}-bit rows) built in "
    f"{time.time() - t0:.1f} s; {nq} reads x {m} symbols in HBM: exact copies / 3 - 6 substitutions / chimeras, one third each")
del text
ptr = lambda t: C.c_void_p(t.data_ptr())
cap = 16 * nq
out = torch.empty(cap * HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
span = torch.empty(cap * 8, dtype=torch.uint8, device=dev)
mlen = torch.empty(total, dtype=torch.int32, device=dev)
lb, ln = torch.empty(nq, dtype=torch.int64, device=dev), torch.empty(nq, dtype=torch.int64, device=dev)
cnt, st, xst = C.c_uint64(), capi.Stats(), capi.Stats()
smi = bench.Smi(0)
smi.start()


def walk():
    global cap, out, span
    rc = L.fmgpu_search_smems(index._h, ptr(qbuf), ptr(qoff), nq, args.min_len, 0, ptr(out), ptr(span), cap, C.byref(cnt), ptr(mlen), C.byref(st), None)
    if rc == capi.FMGPU_ERR_CAPACITY:                                # once more with the size the call reported
        cap = int(cnt.value)
        out = torch.empty(cap * HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        span = torch.empty(cap * 8, dtype=torch.uint8, device=dev)
        rc = L.fmgpu_search_smems(index._h, ptr(qbuf), ptr(qoff), nq, args.min_len, 0, ptr(out), ptr(span), cap, C.byref(cnt), ptr(mlen), C.byref(st), None)
    capi.check(rc)


def yardstick():
    with fm.options(kernel_select=capi.SEL_EXACT_ONE_SYMBOL):
        capi.check(L.fmgpu_search_exact(index._h, ptr(qbuf), ptr(qoff), nq, ptr(lb), ptr(ln), C.byref(xst), None))


walk()
yardstick()                                                          # (one of each before anything is timed)
pad = (-total) % 64
lens = torch.cat([mlen.to(torch.int64), torch.zeros(pad, dtype=torch.int64, device=dev)]).reshape(-1, 64)
util = float(lens.sum()) / float(64 * lens.max(dim=1).values.sum())
say(f"# walk: {st.lf_steps} LF steps, sum of L {int(lens.sum())}, {cnt.value} seeds = {cnt.value / nq:.2f} per read (min_len {args.min_len}), lane utilisation {util:.4f}; "
    f"table accesses per step {st.table_accesses / max(st.lf_steps, 1):.3f}")
say(f"# yardstick: {xst.lf_steps} LF steps, {int((ln > 0).sum())} reads found; table accesses per step {xst.table_accesses / max(xst.lf_steps, 1):.3f}")
say("# kernel ms and G steps/s, alternated")
w_ms, y_ms = [], []
for r in range(args.rounds):
    walk()
    w_ms.append(st.kernel_ms)
    say(f"smem_walk_{r + 1:<3d} {st.kernel_ms:10.3f} ms  {st.lf_steps / st.kernel_ms / 1e6:8.2f} G steps/s")
    yardstick()
    y_ms.append(xst.kernel_ms)
    say(f"k_exact_a_{r + 1:<3d} {xst.kernel_ms:10.3f} ms  {xst.lf_steps / xst.kernel_ms / 1e6:8.2f} G steps/s")
for name, pick in (("best", min), ("mean", lambda v: float(np.mean(v)))):
    w, y = st.lf_steps / pick(w_ms) / 1e6, xst.lf_steps / pick(y_ms) / 1e6
    say(f"# {name} of {args.rounds}: walk {w:.2f} G steps/s, / utilisation {util:.4f} = {w / util:.2f}; k_exact_a {y:.2f} G steps/s; ratio {w / util / y:.3f} (wanted: >= 0.75)")
t = time.time()
walk()
torch.cuda.synchronize()
say(f"# one whole call, wall: {(time.time() - t) * 1e3:.1f} ms (walk kernel {st.kernel_ms:.1f} ms; select, scan, count read-back, emit and the scratch of {16 * total / 1e9:.2f} GB around it)")
ck = smi.stop()
say(f"# card {ck.get('card') if ck else None}; clocks during the run: {ck}")
