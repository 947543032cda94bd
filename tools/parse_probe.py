"""dev probe: fmgpu_queries_parse against the copies around it, on a synthetic FASTQ of --nq x --length bases and the same reads as single-line FASTA (made on the
device from a seed).  One job on one card; the legs are alternated --rounds times, each figure the mean of --steps runs after --warmup, host clock around work that
ends in a synchronise:
  (a) fmgpu_queries_parse on device-resident text with device outputs: the whole call (it returns after completion), FASTQ and FASTA;
  (b) one hipMemcpyAsync of the same bytes from pinned host memory to the device;
  (c) a device-to-device copy of the same bytes: the streaming ceiling, for reference;
  (d) host parsers on one core, once: tools/parse_probe_host.cpp (the example's readFasta rule, compiled here with g++) and a numpy table lookup over the FASTA bytes.
The bar: (a) takes less time than (b) on the FASTQ, by more than the spread (max - min) of the rounds of either.  --only-parse runs leg (a) alone, --steps times, for
`rocprofv3 --kernel-trace --stats -- python tools/parse_probe.py --only-parse` (the sum of the call's kernels).  Writes profiles/parse_probe.log (or --log)."""
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

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--nq", type=int, default=10_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--only-parse", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "parse_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    if not args.only_parse:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if not torch.cuda.is_available():
    raise SystemExit("parse_probe needs a GPU: nothing is measured without one")
dev = torch.device("cuda", 0)
L = capi.lib()
props = torch.cuda.get_device_properties(0)
say(f"# python tools/parse_probe.py --nq {args.nq} --length {args.length} --rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}")
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; clock_rate {getattr(props, 'clock_rate', 0) / 1e3:.0f} MHz; "
    f"memory_clock_rate {getattr(props, 'memory_clock_rate', 0) / 1e3:.0f} MHz; {props.total_memory / 2**30:.0f} GiB")

# ---- the texts, made on the device: "@r%08d\n" seq "\n+\n" qual "\n" and ">r%08d\n" seq "\n"
nq, m = args.nq, args.length
gen = torch.Generator(device=dev).manual_seed(5)
ranks = torch.randint(1, 5, (nq, m), dtype=torch.uint8, device=dev, generator=gen)
letters = torch.tensor(list(b"$ACGT"), dtype=torch.uint8, device=dev)[ranks.long()]
ids = torch.arange(nq, device=dev) % 100_000_000
digits = torch.stack([(ids // 10 ** (7 - k)) % 10 + ord("0") for k in range(8)], dim=1).to(torch.uint8)


def column(byte):
    return torch.full((nq, 1), byte, dtype=torch.uint8, device=dev)


quality = torch.randint(33, 74, (nq, m), dtype=torch.uint8, device=dev, generator=gen)
fastq = torch.cat([column(ord("@")), column(ord("r")), digits, column(10), letters, column(10), column(ord("+")), column(10), quality, column(10)], dim=1).reshape(-1)
fasta = torch.cat([column(ord(">")), column(ord("r")), digits, column(10), letters, column(10)], dim=1).reshape(-1)
del letters, quality, digits, ids
want = ranks.reshape(-1)
torch.cuda.synchronize()
say(f"# {nq} reads x {m} bases: FASTQ {fastq.numel()} bytes, single-line FASTA {fasta.numel()} bytes")

table = fm.symbol_table.dna5()
qbuf, qoff = fm.DeviceBuffer(nq * m), fm.DeviceBuffer((nq + 1) * 8)


def parse(text, fmt):
    res = capi.ParseResult()
    capi.check(L.fmgpu_queries_parse(C.c_void_p(text.data_ptr()), text.numel(), fmt, 1, capi.ptr(table), capi.ptr(qbuf), nq * m, capi.ptr(qoff), nq, None, None, C.byref(res), None))
    return res


for text, fmt in ((fastq, fm.FASTQ), (fasta, fm.FASTA)):                 # the outputs are the generated ranks
    res = parse(text, fmt)
    host = qbuf.to_array(np.uint8, nq * m)
    assert (res.reads, res.symbols, res.consumed, res.foreign) == (nq, nq * m, text.numel(), 0), (res.reads, res.symbols, res.consumed, res.foreign)
    assert np.array_equal(host, want.cpu().numpy()), "parsed symbols differ from the generated reads"
    ends = qoff.to_array(np.uint64, nq + 1)
    assert np.array_equal(ends, np.arange(nq + 1, dtype=np.uint64) * np.uint64(m))
    del host, ends
say("# parsed FASTQ and FASTA equal the generated reads (symbols, offsets, counts)")


def timed(run):
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


if args.only_parse:
    say(f"parse FASTQ {timed(lambda: parse(fastq, fm.FASTQ)):.2f} ms, FASTA {timed(lambda: parse(fasta, fm.FASTA)):.2f} ms (under a profiler: not a figure)")
    raise SystemExit(0)

pinned = torch.empty(fastq.numel(), dtype=torch.uint8).pin_memory()
pinned.copy_(fastq)
landing = torch.empty_like(fastq)
legs = {
    "a  parse FASTQ (device text -> device qbuf/qoff)": lambda: parse(fastq, fm.FASTQ),
    "a' parse FASTA (device text -> device qbuf/qoff)": lambda: parse(fasta, fm.FASTA),
    "b  hipMemcpyAsync pinned host -> device, FASTQ bytes": lambda: landing.copy_(pinned, non_blocking=True),
    "b' hipMemcpyAsync pinned host -> device, FASTA bytes": lambda: landing[: fasta.numel()].copy_(pinned[: fasta.numel()], non_blocking=True),
    "c  device -> device copy, FASTQ bytes": lambda: landing.copy_(fastq),
}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for k, run in legs.items():
        times[k].append(timed(run))
    say(f"round {r}: " + "; ".join(f"{k.split()[0]} {times[k][-1]:.2f} ms" for k in legs))
for k, v in times.items():
    nbytes = fasta.numel() if "FASTA" in k else fastq.numel()
    say(f"({k}): mean {np.mean(v):8.2f} ms, min {min(v):8.2f}, max {max(v):8.2f}  = {nbytes / np.mean(v) / 1e6:7.1f} GB/s of text")

# ---- (d) one core of the host
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "parse_probe_host")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "parse_probe_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, str(nq), str(m)], check=True, capture_output=True, text=True).stdout.split()
say(f"(d  host, one core, the example's readFasta rule over {out[0]} FASTA bytes): {float(out[3]) * 1e3:8.1f} ms = {int(out[0]) / float(out[3]) / 1e9:.2f} GB/s ({out[1]} records, {out[2]} symbols)")
raw = fasta.cpu().numpy()
t0 = time.perf_counter()
looked = table[raw]
t1 = time.perf_counter()
say(f"(d' host, one core, numpy table lookup over {raw.size} FASTA bytes, no line structure): {(t1 - t0) * 1e3:8.1f} ms = {raw.size / (t1 - t0) / 1e9:.2f} GB/s")
del looked

a, b = times["a  parse FASTQ (device text -> device qbuf/qoff)"], times["b  hipMemcpyAsync pinned host -> device, FASTQ bytes"]
spread = max(max(a) - min(a), max(b) - min(b))
ok = np.mean(b) - np.mean(a) > spread
say(f"verdict: parse {np.mean(a):.2f} ms against upload {np.mean(b):.2f} ms of the same FASTQ bytes, spread of the rounds {spread:.2f} ms: "
    + ("the parse is faster than the copy that feeds it" if ok else "the parse does NOT clear the upload"))
