"""dev probe: text extraction (fmgpu_index_accelerate_extract + fmgpu_extract) on the genome stand-in (datasets.genome_like_text with bench.GRCH38_LENGTHS,
scaled by --scale; BiFMIndex<5, IB16>, sampling rate 16) and on a protein text (FMIndex<28, Wavelet>, --protein-seqs x 500 residues):
  table build time and bytes; whole-text reconstruction (kernel ms, LF steps/s, checked against the text); --windows random 200-symbol windows;
  fmgpu_locate's LF steps/s on --locate-rows random rows of the same index, for comparison.  The genome index is measured with its explicit LF table
  (one 4-byte load per step) and without it (the fused Format A blocks: one 64-byte line per step)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import fmindex_collection_amd as fm
from fmindex_collection_amd import capi, datasets
from fmindex_collection_amd.capi import TEXT_RANGE_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--windows", type=int, default=10_000_000)
ap.add_argument("--window-len", type=int, default=200)
ap.add_argument("--locate-rows", type=int, default=9_000_000)
ap.add_argument("--protein-seqs", type=int, default=1_000_000)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)


def best(f):
    """the fastest of --runs runs (kernel ms), with the stats of that run"""
    out = [f() for _ in range(args.runs)]
    return min(out, key=lambda s: s.kernel_ms), [round(s.kernel_ms, 2) for s in out]


def measure(name, index, text, seq_off, wl):
    n_text = int(text.numel())
    torch.cuda.synchronize()
    b0 = index.device_bytes
    t0 = time.time()
    index.accelerate_extract()
    build_s = time.time() - t0
    ids, lens = index.sequence_lengths()
    nsamp_bytes = index.device_bytes - b0
    print(f"{name}: table built in {build_s:.3f} s, {nsamp_bytes / 1e9:.3f} GB ({nsamp_bytes / max(n_text, 1):.3f} B per symbol), {len(ids)} sequences", flush=True)
    # whole text
    r = np.zeros(len(ids), dtype=TEXT_RANGE_DTYPE)
    r["seq_id"], r["len"] = ids, lens
    out = torch.empty(n_text + 64, dtype=torch.uint8, device=dev)

    def whole():
        cnt, _, st = index.extract(r, out=capi_view(out), want_stats=True)
        assert cnt == n_text
        return st
    st, runs = best(whole)
    same = bool(torch.equal(out[:n_text], text))
    print(f"{name}: whole text {n_text / 1e6:.1f} M symbols: kernel {st.kernel_ms:.2f} ms, {st.lf_steps / 1e6:.1f} M LF steps, {st.lf_steps / st.kernel_ms / 1e6:.3f} G steps/s, "
          f"{n_text / st.kernel_ms / 1e6:.3f} G symbols/s | identical {same} | runs {runs}", flush=True)
    # random windows
    g = torch.Generator(device=dev); g.manual_seed(5)
    nseq = len(ids)
    lens_t = torch.from_numpy(lens.astype(np.int64)).to(dev)
    ok = torch.nonzero(lens_t >= wl).flatten()
    s = ok[torch.randint(0, ok.numel(), (args.windows,), generator=g, device=dev)]
    p = (torch.rand(args.windows, generator=g, device=dev, dtype=torch.float64) * (lens_t[s] - wl + 1).double()).long()
    rt = torch.stack([s, p, torch.full_like(s, wl)], dim=1).contiguous()
    wout = torch.empty(args.windows * wl, dtype=torch.uint8, device=dev)

    def windows():
        cnt, _, st = index.extract(capi_view(rt), out=capi_view(wout), want_stats=True)
        assert cnt == args.windows * wl
        return st
    st, runs = best(windows)
    k = min(args.windows, 100_000)
    starts = seq_off[s[:k]] + p[:k]
    same = bool(torch.equal(wout[: k * wl].view(k, wl), text[starts[:, None] + torch.arange(wl, device=dev)[None, :]]))
    print(f"{name}: {args.windows} windows of {wl}: kernel {st.kernel_ms:.2f} ms, {st.lf_steps / 1e6:.1f} M LF steps ({st.lf_steps / (args.windows * wl):.3f} per symbol), "
          f"{st.lf_steps / st.kernel_ms / 1e6:.3f} G steps/s, {args.windows / st.kernel_ms / 1e3:.2f} M windows/s | first {k} identical {same} | runs {runs}", flush=True)
    del out, wout, rt
    index.accelerate_extract(False)
    # locate on the same index
    rows = np.random.default_rng(3).integers(0, index.n, size=args.locate_rows, dtype=np.uint64)
    lst = min((index.locate(rows, want_stats=True)[3] for _ in range(args.runs)), key=lambda s_: s_.kernel_ms)
    print(f"{name}: fmgpu_locate {args.locate_rows} rows: kernel {lst.kernel_ms:.2f} ms, {lst.lf_steps / args.locate_rows:.2f} steps per row, "
          f"{lst.lf_steps / lst.kernel_ms / 1e6:.3f} G steps/s", flush=True)


class capi_view:
    """a torch tensor as a device buffer (ptr + nbytes)"""

    def __init__(self, t):
        self.t, self.ptr, self.nbytes = t, t.data_ptr(), t.numel() * t.element_size()

    def cpu(self):
        return self.t.cpu()


# ---- genome stand-in
lengths = [max(1000, int(l * args.scale)) for l in bench.GRCH38_LENGTHS]
text, _ = datasets.genome_like_text(lengths, seed=42, device=dev)
seq_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])).to(dev)
t0 = time.time()
index = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
print(f"genome stand-in: {text.numel() / 1e6:.1f} Mbp, {len(lengths)} sequences, index built in {time.time() - t0:.1f} s, formats 0x{index.formats:x}", flush=True)
measure("genome, LF table", index, text, seq_off, args.window_len)
index.accelerate_lf(False)
measure("genome, fused blocks", index, text, seq_off, args.window_len)
del index, text
torch.cuda.empty_cache()

# ---- protein text
if args.protein_seqs:
    sigma, plen = 28, 500
    total = args.protein_seqs * plen
    g = torch.Generator(device=dev); g.manual_seed(42)
    text = torch.empty(total, dtype=torch.uint8, device=dev)
    for lo in range(0, total, 1 << 28):
        hi = min(total, lo + (1 << 28))
        text[lo:hi] = torch.randint(1, sigma, (hi - lo,), generator=g, device=dev, dtype=torch.uint8)
    seq_off = torch.arange(args.protein_seqs + 1, device=dev, dtype=torch.int64) * plen
    with fm.options(lf_table=0):
        t0 = time.time()
        index = fm.FMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), sigma, "WAVELET", 16)
    print(f"protein: {total / 1e6:.1f} M residues, {args.protein_seqs} sequences, index built in {time.time() - t0:.1f} s, formats 0x{index.formats:x}", flush=True)
    measure("protein, tree", index, text, seq_off, min(args.window_len, plen))
