"""dev probe: fmgpu_search_hamming_sm against the general k-mismatch kernel on the genome stand-in (datasets.genome_like_text with bench.GRCH38_LENGTHS scaled to --symbols;
BiFMIndex<5, IB16>, plain index), --nq reads of --length symbols in HBM (text windows, read i with i % 3 substitutions), scheme h2(4, 0, 2):
  (a) fmgpu_search_scheme on the general kernel (k_scheme): FMGPU_SEL_GENERAL_DFS | FMGPU_SEL_NO_SHARING | FMGPU_SEL_NO_LF_GENERAL — one read per lane, no table, no sharing;
  (b) fmgpu_search_hamming_sm with the identity matrix on the same batch: the same memory work per node (one extend-all) plus two LDS mask reads and the child set;
  (c) fmgpu_search_hamming_sm with ScoringMatrix.iupac_dna() and 1 % of the symbols replaced by N: no existing call can answer it, so it has no baseline.
Alternated --rounds times; kernel_ms, lf_steps and steps/s of each, the ratio (b) / (a), the card's id and clocks.  Nothing is asserted.  One process; it ends itself after
--time-limit seconds.  Writes profiles/hamming_sm_probe.log (or --log)."""
import argparse
import ctypes as C
import os
import signal
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
ap.add_argument("--symbols", type=float, default=50e6)
ap.add_argument("--nq", type=int, default=1_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--time-limit", type=int, default=900)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "hamming_sm_probe.log"))
args = ap.parse_args()
signal.alarm(args.time_limit)

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


dev = torch.device("cuda", 0)
scale = args.symbols / float(sum(bench.GRCH38_LENGTHS))
c = types.SimpleNamespace(torch=torch, np=np, datasets=datasets, dev=dev, rank=0, args=types.SimpleNamespace(scale=scale))
L = capi.lib()
say(f"# python tools/hamming_sm_probe.py --symbols {args.symbols:g} --nq {args.nq} --length {args.length} --rounds {args.rounds}")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
nq, m = args.nq, args.length
gq = torch.Generator(device=dev)
gq.manual_seed(1000)
ar = torch.arange(m, device=dev, dtype=torch.int64)
starts = torch.randint(0, text.numel() - m, (nq,), generator=gq, device=dev, dtype=torch.int64)
reads = torch.empty((nq, m), dtype=torch.uint8, device=dev)
for lo in range(0, nq, 1 << 20):
    hi = min(nq, lo + (1 << 20))
    reads[lo:hi] = text[starts[lo:hi, None] + ar[None, :]]
rows = torch.arange(nq, device=dev)
for k in range(2):                                                   # read i: i % 3 substitutions
    sel = rows[rows % 3 > k]
    pos = torch.randint(0, m, (sel.numel(),), generator=gq, device=dev)
    shift = torch.randint(1, 4, (sel.numel(),), generator=gq, device=dev, dtype=torch.uint8)
    reads[sel, pos] = (reads[sel, pos] - 1 + shift) % 4 + 1
with_n = reads.clone()
with_n[torch.rand((nq, m), generator=gq, device=dev) < 0.01] = 15   # 1 % of the symbols: N
qbuf, qbuf_n = reads.reshape(-1), with_n.reshape(-1)
qoff = torch.arange(nq + 1, device=dev, dtype=torch.int64) * m
torch.cuda.synchronize()
fm.options["lf_table"] = 0
t0 = time.time()
index = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
torch.cuda.synchronize()
say(f"# genome stand-in, {int(text.numel())} symbols, {len(lengths)} sequences; plain BiFMIndex (formats {index.formats:#x}, {index.device_bytes / 1e9:.2f} GB, {index.row_bits}-bit rows) built in "
    f"{time.time() - t0:.1f} s; {nq} reads x {m} symbols in HBM, read i with i % 3 substitutions; (c): {int((with_n == 15).sum())} symbols replaced by N")
del text
ptr = lambda t: C.c_void_p(t.data_ptr())
state = {"cap": 8 * nq}
state["out"] = torch.empty(state["cap"] * HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
sc, keep = bench._scheme_struct(capi, fm.search_scheme.h2(4, 0, 2))
identity, iupac = fm.ScoringMatrix(5), fm.ScoringMatrix.iupac_dna()
cnt = C.c_uint64()
smi = bench.Smi(0)
smi.start()


def with_room(call):
    """the call, once more with the capacity it reported if the buffer was too small"""
    rc = call()
    if rc == capi.FMGPU_ERR_CAPACITY:
        state["cap"] = int(cnt.value)
        state["out"] = torch.empty(state["cap"] * HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        rc = call()
    capi.check(rc)


def general(st):
    with fm.options(kernel_select=capi.SEL_GENERAL_DFS | capi.SEL_NO_SHARING | capi.SEL_NO_LF_GENERAL):
        with_room(lambda: L.fmgpu_search_scheme(index._h, ptr(qbuf), ptr(qoff), nq, C.byref(sc), capi.UINT64_MAX, ptr(state["out"]), state["cap"], C.byref(cnt), C.byref(st), None))


def matrix(st, q, sm):
    ms = sm._struct()
    with_room(lambda: L.fmgpu_search_hamming_sm(index._h, ptr(q), ptr(qoff), nq, C.byref(sc), C.byref(ms), capi.UINT64_MAX, ptr(state["out"]), state["cap"], C.byref(cnt), C.byref(st), None))


cases = (("(a) k_scheme, general kernel      ", lambda st: general(st)),
         ("(b) k_scheme_sm, identity matrix  ", lambda st: matrix(st, qbuf, identity)),
         ("(c) k_scheme_sm, IUPAC, 1 % N     ", lambda st: matrix(st, qbuf_n, iupac)))
ms_of = {name: [] for name, _ in cases}
last = {}
for name, call in cases:                                             # (one of each before anything is timed)
    st = capi.Stats()
    call(st)
    say(f"# {name}: {st.lf_steps} LF steps, {cnt.value} records, table accesses per step {st.table_accesses / max(st.lf_steps, 1):.3f}, hand-out pass {st.prepass_ms:.2f} ms")
say("# kernel ms and G steps/s, alternated")
for r in range(args.rounds):
    for name, call in cases:
        st = capi.Stats()
        call(st)
        ms_of[name].append(st.kernel_ms)
        last[name] = st.lf_steps
        say(f"{name} round {r + 1}: {st.kernel_ms:10.3f} ms  {st.lf_steps / st.kernel_ms / 1e6:8.3f} G steps/s")
for label, pick in (("best", min), ("mean", lambda v: float(np.mean(v)))):
    a, b, cc = (pick(ms_of[name]) for name, _ in cases)
    say(f"# {label} of {args.rounds}: (a) {a:.3f} ms, (b) {b:.3f} ms, (c) {cc:.3f} ms; (b) / (a) = {b / a:.3f} (expected: <= 1.2)")
ck = smi.stop()
say(f"# card {ck.get('card') if ck else None}; clocks during the run: {ck}")
