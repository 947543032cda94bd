"""exact search along the sample chain: one build of the headline index, then the headline batch (10 M x 101 bp) under the development build's knobs —
the pair table alone, the five launches on one stream (FMGPU_DEV_EXACT_SERIAL: the side leg behind instead of beside the jump over all reads), the hand-over threshold
(FMGPU_DEV_EXACT_HAND), the park threshold (FMGPU_DEV_EXACT_PARK_MIN), park + resume without the jump (FMGPU_DEV_EXACT_NO_JUMP) — two rounds, every result compared with the first.
usage: python tools/exact_chain_sweep.py [launches per setting] [legs]   (needs make DEV=1; legs: only off / shipped / serial; FMGPU_LIBRARY = another development build of
the same ABI, e.g. the parent commit's, whose rows then stand beside this build's in one job)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FMGPU_LIBRARY", os.path.join(ROOT, "fmindex-collection_amd", "libfmgpu_dev.so"))
import numpy as np
import torch
import bench
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi, datasets

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
legs_only = len(sys.argv) > 2 and sys.argv[2] == "legs"
print("library", os.environ["FMGPU_LIBRARY"], flush=True)
c = bench.Ctx()
c.args = type("Args", (), {"scale": 1.0})()
c.rank, c.world, c.np, c.torch, c.fm, c.capi, c.datasets = 0, 1, np, torch, fm, capi, datasets
c.dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
capi.check(capi.lib().fmgpu_set_device(0))
t0 = time.time()
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
nq, L = 10_000_000, 101
qbuf, qoff = bench.sample_reads(c, text, lengths, L, nq, 1000, "exact")
torch.cuda.synchronize()
fm.options["lf_table"] = 0
t1 = time.time()
index = fm.FMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
print("text %.1f s, build %.1f s, device_bytes %d, formats %#x" % (t1 - t0, time.time() - t1, index.device_bytes, index.formats), flush=True)
out = torch.empty(2 * nq, dtype=torch.int64, device=c.dev)
stats = capi.Stats()


def run(label, env, sel):
    for k in ("FMGPU_DEV_EXACT_PARK_MIN", "FMGPU_DEV_EXACT_NO_JUMP", "FMGPU_DEV_EXACT_HAND", "FMGPU_DEV_EXACT_SERIAL"):
        os.environ.pop(k, None)
    os.environ.update(env)
    fm.options["kernel_select"] = sel
    def step():
        capi.check(capi.lib().fmgpu_search_exact(index._h, C.c_void_p(qbuf.data_ptr()), C.c_void_p(qoff.data_ptr()), nq, C.c_void_p(out[:nq].data_ptr()),
                                                 C.c_void_p(out[nq:].data_ptr()), C.byref(stats), None))
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    kms = []
    t = time.perf_counter()
    for _ in range(steps):
        step(); kms.append(stats.kernel_ms)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) / steps * 1e3
    res = out.clone()
    print("%-22s ms_per_step %7.3f kernel_ms %7.3f (min %.3f max %.3f)  lf_steps %d table_steps %d table_accesses %d table_bytes %d hits %d"
          % (label, ms, sum(kms) / len(kms), min(kms), max(kms), stats.lf_steps, stats.table_steps, stats.table_accesses, stats.table_bytes, int((res[nq:] > 0).sum())), flush=True)
    return res, stats.lf_steps


def knobs(hand, park, nojump=False):
    env = {"FMGPU_DEV_EXACT_HAND": str(hand), "FMGPU_DEV_EXACT_PARK_MIN": str(park)}
    if nojump:
        env["FMGPU_DEV_EXACT_NO_JUMP"] = "1"
    return ("hand%d_park%d%s" % (hand, park, "_nojump" if nojump else ""), env, 0)


base = None
for rnd in range(2):
    rows = [("off", {}, capi.SEL_NO_SAMPLE_CHAIN), ("shipped", {}, 0), ("serial", {"FMGPU_DEV_EXACT_SERIAL": "1"}, 0)]
    if not legs_only:
        rows += [knobs(h, p) for h, p in ((10, 32), (10, 48), (0, 48), (3, 48), (6, 48), (16, 48), (6, 32), (6, 64), (16, 32))] + [knobs(10, 32, True)]
    for label, env, sel in rows:
        res, lf = run(label + "_%d" % rnd, env, sel)
        if base is None:
            base = (res, lf)
        else:
            print("   equal to off_0: lb/len %s lf_steps %s" % (bool(torch.equal(res, base[0])), lf == base[1]), flush=True)
