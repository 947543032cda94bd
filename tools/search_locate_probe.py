"""dev probe: search -> positions on the genome stand-in (datasets.genome_like_text with bench.GRCH38_LENGTHS, scaled by --scale).
  (a) 10 M x 101 bp exact reads: fmgpu_locate_hits over ALL rows of every hit (up to --max-rows rows per hit, --max-total in all), against fmgpu_locate on the same rows pre-expanded into a device array
  (b) 1 M reads at k = 2 (Hamming): search_locate end to end, against search_ng26.search + Python LocateLinear
  (c) 10 k reads through C++ fmc::Search (one fmgpu_locate_hits call) against the per-cursor LocateLinear loop it replaced (tests/cpp/test_locate_hits.cpp)"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

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
ap.add_argument("--exact-reads", type=int, default=10_000_000)
ap.add_argument("--k2-reads", type=int, default=1_000_000)
ap.add_argument("--cpp-reads", type=int, default=10_000)
ap.add_argument("--max-rows", type=int, default=100_000, help="(a): hits of more rows are left out")
ap.add_argument("--max-total", type=int, default=600_000_000, help="(a): rows located at most")
args = ap.parse_args()

dev = torch.device("cuda", 0)
lengths = [max(1000, int(l * args.scale)) for l in bench.GRCH38_LENGTHS]
text, _ = datasets.genome_like_text(lengths, seed=42, device=dev)
n = int(text.numel())
seq_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])).to(dev)
t0 = time.time()
index = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
print(f"genome stand-in: {n / 1e6:.1f} Mbp, index built in {time.time() - t0:.1f} s", flush=True)
g = torch.Generator(device=dev); g.manual_seed(7)
L = 101


def windows(count):
    starts = torch.randint(0, n - L, (count,), generator=g, device=dev, dtype=torch.int64)
    reads = text[starts[:, None] + torch.arange(L, device=dev)[None, :]].contiguous()
    return reads, torch.arange(count + 1, device=dev, dtype=torch.int64) * L


# ---- (a)
nq = args.exact_reads
reads, qoff = windows(nq)
lbln = torch.empty(2 * nq, dtype=torch.int64, device=dev)
fm.search_no_errors.search(index, (bench._Dev(reads), bench._Dev(qoff)), out=(bench._Dev(lbln[:nq]), bench._Dev(lbln[nq:])))
torch.cuda.synchronize()
lb, ln = lbln[:nq], lbln[nq:]
# the stand-in's runs of one symbol give reads of ~10^8 rows (7 x 10^13 rows over 10 M reads): hits of more than --max-rows rows are left out, and
# the batch is cut where the rows reach --max-total (64 bytes per row of device memory for the two runs)
found = torch.nonzero(ln > 0).flatten()
keep = found[ln[found] <= args.max_rows]
keep = keep[: int(torch.searchsorted(torch.cumsum(ln[keep], 0), args.max_total, right=True))]
hits = torch.zeros((keep.numel(), 5), dtype=torch.int64, device=dev)          # fmgpu_hit: qidx, lb, lb_rev, len, errors | seq
hits[:, 0], hits[:, 1], hits[:, 3] = keep, lb[keep], ln[keep]
total = int(ln[keep].sum())
lens = ln[keep]
print(f"(a) {nq} exact reads, {found.numel()} with hits ({int((ln[found] > args.max_rows).sum())} of more than {args.max_rows} rows left out); "
      f"located: the first {keep.numel()} hits, {total} rows (median {int(lens.median())}, mean {total / keep.numel():.2f}, max {int(lens.max())} rows per hit)", flush=True)
out = torch.empty(total * 32, dtype=torch.uint8, device=dev)
st, cnt = capi.Stats(), C.c_uint64()
t_hits = []
for _ in range(4):
    capi.check(capi.lib().fmgpu_locate_hits(index._h, C.c_void_p(hits.data_ptr()), keep.numel(), C.c_void_p(out.data_ptr()), total, C.byref(cnt), C.byref(st), None))
    t_hits.append(st.kernel_ms)
starts = torch.repeat_interleave(lb[keep] - torch.cumsum(lens, 0) + lens, lens)
rows = (starts + torch.arange(total, device=dev, dtype=torch.int64)).contiguous()
del starts
seq, pos, steps = (torch.empty_like(rows) for _ in range(3))
t_rows = []
for _ in range(4):
    capi.check(capi.lib().fmgpu_locate(index._h, C.c_void_p(rows.data_ptr()), total, C.c_void_p(seq.data_ptr()), C.c_void_p(pos.data_ptr()),
                                       C.c_void_p(steps.data_ptr()), C.byref(st), None))
    t_rows.append(st.kernel_ms)
torch.cuda.synchronize()
rec = out.view(torch.int64).view(total, 4)
same = bool(torch.equal(rec[:, 1], seq) and torch.equal(rec[:, 2], pos + steps))
th, tr = min(t_hits[1:]), min(t_rows[1:])
print(f"(a) fmgpu_locate_hits kernel {th:.3f} ms ({total / th / 1e6:.3f} G positions/s) | fmgpu_locate on the pre-expanded rows {tr:.3f} ms "
      f"({total / tr / 1e6:.3f} G rows/s) | ratio {th / tr:.3f} | identical {same} | all runs hits {['%.3f' % x for x in t_hits]} rows {['%.3f' % x for x in t_rows]}", flush=True)
torch.cuda.synchronize()
del reads, qoff, lbln, hits, out, rows, seq, pos, steps, rec
torch.cuda.empty_cache()

# ---- (b)
nq = args.k2_reads
reads, qoff = windows(2 * nq)                                                      # reads whose exact interval holds 1 .. --max-rows / 100 rows (see (a))
lbln = torch.empty(4 * nq, dtype=torch.int64, device=dev)
fm.search_no_errors.search(index, (bench._Dev(reads), bench._Dev(qoff)), out=(bench._Dev(lbln[: 2 * nq]), bench._Dev(lbln[2 * nq:])))
ok = torch.nonzero((lbln[2 * nq:] > 0) & (lbln[2 * nq:] <= args.max_rows // 100)).flatten()[:nq]
nq = ok.numel()
reads, qoff = reads[ok].contiguous(), qoff[: nq + 1].contiguous()
mut = torch.randint(0, L, (nq, 2), generator=g, device=dev)
sym = torch.randint(1, 5, (nq, 2), generator=g, device=dev, dtype=torch.uint8)
reads.scatter_(1, mut, sym)
qb, qo = reads.flatten().cpu().numpy(), qoff.cpu().numpy().astype(np.uint64)
torch.cuda.synchronize()
fm.search_locate(index, (qb[: 101 * 1000], qo[:1001]), 2, edit=False)          # warm-up
t0 = time.perf_counter()
new = fm.search_locate(index, (qb, qo), 2, edit=False)
t_new = time.perf_counter() - t0
t0 = time.perf_counter()
h = fm.search(index, (qb, qo), 2, edit=False)
owner, s, p, k = fm.LocateLinear(index, h["lb"], h["len"])()
t_old = time.perf_counter() - t0
same = bool(np.array_equal(new["qidx"], h["qidx"][owner.astype(np.int64)]) and np.array_equal(new["seq_id"], s) and np.array_equal(new["pos"], p + k))
print(f"(b) {nq} reads k=2 Hamming, {len(h)} hits, {len(new)} positions: search_locate {t_new:.3f} s | search + LocateLinear {t_old:.3f} s | "
      f"speed-up {t_old / t_new:.2f} x | identical {same}", flush=True)

# ---- (c)
exe = os.path.join(ROOT, "tests", "cpp", "test_locate_hits")
pkg = os.path.join(ROOT, "fmindex-collection_amd")
subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_locate_hits.cpp"), "-o", exe, "-L" + pkg, "-lfmgpu", "-Wl,-rpath," + pkg,
                "-Wl,--wrap=fmgpu_locate,--wrap=fmgpu_locate_hits"], check=True)
r = subprocess.run([exe, "time", str(args.cpp_reads)], capture_output=True, text=True, timeout=1800)
for line in r.stdout.splitlines():
    print("(c) C++", line, flush=True)
