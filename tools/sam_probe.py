"""dev probe: fmgpu_positions_sam on --n synthetic records of 101 bp reads, resident on the device with their batch, read names (20 .. 40 bytes), qualities and 25
sequence names: of every 8 reads one is unmapped, one has two records, one has three (so --n records belong to 0.8 --n reads), strands at random, errors 0 .. 2.  One
job on one card; the legs are alternated --rounds times, each figure the mean of --steps runs after --warmup:
  (a) the baseline: one hipMemcpy of the records into pinned host memory, then a snprintf loop writing the same lines into a memory buffer from host copies of the
      batch and the tables, no file I/O — tools/sam_probe_host.cpp, built here with g++ -O2, ONE host thread; wall clock, once per round;
  (b) fmgpu_positions_sam device to device: the whole call between two events; (b0) its counting call alone (every pass but the write pass, and the read-back), so
      (b) - (b0) is the write pass with its launch and the read-back of the batch's size;
  (c) the same call with a pinned host `out`: wall clock (the staging buffer, the write pass and one device-to-host copy of the text);
  (d) one device-to-device copy of as many bytes as the text has;
  (f) fmgpu_positions_format on the same records (read_name, seq_id, pos, errors) device to device, and (f0) its counting call: (f) - (f0) is its write pass.
The texts of (a) and (b) are compared byte for byte first.  --only-sam runs leg (b) alone, --steps times, for
`rocprofv3 --kernel-trace --stats -- python tools/sam_probe.py --only-sam` (the passes kernel by kernel: this probe times whole calls only, and the record of such a run is kept by hand as profiles/sam_probe_kernels.log).  Writes
profiles/sam_probe.log (or --log)."""
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
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--only-sam", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "sam_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    if not args.only_sam:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if not torch.cuda.is_available():
    raise SystemExit("sam_probe needs a GPU: nothing is measured without one")
dev = torch.device("cuda", 0)
L = capi.lib()
props = torch.cuda.get_device_properties(0)
say(f"# python tools/sam_probe.py --n {args.n} --rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}")
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; clock_rate {getattr(props, 'clock_rate', 0) / 1e3:.0f} MHz; "
    f"memory_clock_rate {getattr(props, 'memory_clock_rate', 0) / 1e3:.0f} MHz; {props.total_memory / 2**30:.0f} GiB")

# ---- the batch, the tables and the records, made on the device
M = 101
n = args.n - args.n % 10
nq = n // 10 * 8
gen = torch.Generator(device=dev).manual_seed(13)
per_read = torch.tensor([1, 1, 2, 0, 1, 3, 1, 1], device=dev).repeat(nq // 8)
read_of = torch.repeat_interleave(torch.arange(nq, device=dev), per_read)
assert read_of.numel() == n
rec = torch.empty((n, 4), dtype=torch.int64, device=dev)                 # four 64-bit words each (the last one errors | hit << 32)
rec[:, 0] = 2 * read_of + torch.randint(0, 2, (n,), device=dev, generator=gen)
rec[:, 1] = torch.randint(0, 25, (n,), device=dev, generator=gen)
rec[:, 2] = torch.randint(0, 250_000_000, (n,), device=dev, generator=gen)
rec[:, 3] = torch.randint(0, 3, (n,), device=dev, generator=gen) | ((torch.arange(n, device=dev) & 0xffffffff) << 32)
qbuf = torch.randint(1, 5, (nq * M,), dtype=torch.uint8, device=dev, generator=gen)
qoff = torch.arange(nq + 1, device=dev) * M
qual_bytes = torch.randint(33, 127, (nq * M,), dtype=torch.uint8, device=dev, generator=gen)
qual_spans = torch.stack([qoff[:-1], torch.full((nq,), M, device=dev)], dim=1).contiguous()
name_len = 20 + (torch.arange(nq, device=dev) * 7) % 21
name_spans = torch.stack([torch.cumsum(name_len, 0) - name_len, name_len], dim=1).contiguous()
name_bytes = torch.randint(48, 123, (int(name_len.sum().item()),), dtype=torch.uint8, device=dev, generator=gen)
seq_data, seq_spans_np = fm.pack_names(["chr%d" % (s + 1) for s in range(25)])
seq_bytes, seq_spans = torch.from_numpy(seq_data.copy()).to(dev), torch.from_numpy(seq_spans_np.view(np.uint64).reshape(-1, 2).astype(np.int64)).to(dev)
torch.cuda.synchronize()
rec_bytes = rec.numel() * 8

char_of = fm.char_table("dna5")
comp = np.array(fm.DNA5_COMPLEMENT, dtype=np.uint8)
strands = capi.Strands(comp.ctypes.data_as(capi.u8p), 5, 0)
tables = [capi.NameTable(b.data_ptr(), b.numel(), s.data_ptr(), s.shape[0]) for b, s in ((name_bytes, name_spans), (qual_bytes, qual_spans), (seq_bytes, seq_spans))]
sam_spec = capi.SamSpec(qbuf.data_ptr(), qoff.data_ptr(), nq, char_of.ctypes.data, C.pointer(strands), C.pointer(tables[0]), C.pointer(tables[1]), C.pointer(tables[2]),
                        1, 1, 0, 60, 0, (C.c_uint8 * 3)(0, 0, 0))
cols = [capi.COLUMNS[c] for c in ("read_name", "seq_id", "pos", "errors")]
fmt_spec = capi.FormatSpec(4, (C.c_uint8 * 8)(*(cols + [0] * 4)), ord("\t"), 1, 1, 0, 1, C.pointer(tables[0]), None)


def sam(out, capacity):
    nbytes, nlines = C.c_uint64(), C.c_uint64()
    capi.check(L.fmgpu_positions_sam(C.c_void_p(rec.data_ptr()), n, C.byref(sam_spec), None if out is None else C.c_void_p(out.data_ptr()), capacity, C.byref(nbytes), None,
                                     C.byref(nlines), None))
    return int(nbytes.value), int(nlines.value)


def fmt(out, capacity):
    nbytes = C.c_uint64()
    capi.check(L.fmgpu_positions_format(C.c_void_p(rec.data_ptr()), n, C.byref(fmt_spec), None if out is None else C.c_void_p(out.data_ptr()), capacity, C.byref(nbytes), None, None))
    return int(nbytes.value)


(text_bytes, n_lines), fmt_bytes = sam(None, 0), fmt(None, 0)
text, fmt_text = torch.empty(text_bytes, dtype=torch.uint8, device=dev), torch.empty(fmt_bytes, dtype=torch.uint8, device=dev)
say(f"# {n} records of {nq} reads of {M} symbols = {rec_bytes} bytes of records; SAM: {n_lines} lines, {text_bytes} bytes ({text_bytes / n_lines:.2f} per line); "
    f"fmgpu_positions_format (read_name seq_id pos errors): {fmt_bytes} bytes ({fmt_bytes / n:.2f} per line)")


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


if args.only_sam:
    say(f"sam, device to device {timed(lambda: sam(text, text_bytes)):.2f} ms (under a profiler: not a figure)")
    raise SystemExit(0)

# ---- the baseline's helper, and the two texts against each other
tmp = tempfile.TemporaryDirectory()
so = os.path.join(tmp.name, "sam_probe_host.so")
subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "sam_probe_host.cpp"), "-o", so], check=True)
H = C.CDLL(so)
H.sam_loop.restype = C.c_uint64
H.sam_loop.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 8 + [C.c_uint, C.c_uint, C.c_void_p, C.c_uint64]
host = {k: v.cpu().numpy() for k, v in dict(qbuf=qbuf, qoff=qoff, name_bytes=name_bytes, name_spans=name_spans, qual_bytes=qual_bytes, qual_spans=qual_spans,
                                            seq_bytes=seq_bytes, seq_spans=seq_spans).items()}
char_of_comp = char_of[np.concatenate([comp, np.arange(5, 256, dtype=np.uint8)])]
pinned_rec = torch.empty((n, 4), dtype=torch.int64).pin_memory()
host_text = np.empty(text_bytes + 4096, dtype=np.uint8)               # (the loop wants room for a whole line in front of it)
pinned_out = torch.empty(text_bytes, dtype=torch.uint8).pin_memory()
parts = {"copy": [], "loop": []}


def baseline():
    t0 = time.perf_counter()
    pinned_rec.copy_(rec)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = H.sam_loop(pinned_rec.data_ptr(), n, host["qbuf"].ctypes.data, host["qoff"].ctypes.data, nq, char_of.ctypes.data, char_of_comp.ctypes.data,
                     host["name_bytes"].ctypes.data, host["name_spans"].ctypes.data, host["qual_bytes"].ctypes.data, host["qual_spans"].ctypes.data,
                     host["seq_bytes"].ctypes.data, host["seq_spans"].ctypes.data, 60, 0, host_text.ctypes.data, host_text.size)
    t2 = time.perf_counter()
    assert got == text_bytes, (got, text_bytes)
    parts["copy"].append((t1 - t0) * 1e3)
    parts["loop"].append((t2 - t1) * 1e3)


baseline()
sam(text, text_bytes)
assert np.array_equal(text.cpu().numpy(), host_text[:text_bytes]), "the device text differs from the snprintf loop's"
sam(pinned_out, text_bytes)
assert np.array_equal(pinned_out.numpy(), host_text[:text_bytes]), "the text in the pinned buffer differs from the snprintf loop's"
say("# the device text (device out and pinned host out) equals the snprintf loop's, byte for byte")
parts = {"copy": [], "loop": []}

src, landing = torch.empty(text_bytes, dtype=torch.uint8, device=dev), torch.empty(text_bytes, dtype=torch.uint8, device=dev)
legs = {
    "a  baseline: records to pinned host + snprintf loop, one host thread": (baseline, dict(events=False, steps=1, warmup=0)),
    "b  sam, device to device": (lambda: sam(text, text_bytes), {}),
    "b0 sam, the counting call alone (every pass but the write pass)": (lambda: sam(None, 0), {}),
    "c  sam into a pinned host out": (lambda: sam(pinned_out, text_bytes), dict(events=False)),
    "d  device -> device copy of the text's bytes": (lambda: landing.copy_(src), {}),
    "f  format (read_name seq_id pos errors), device to device": (lambda: fmt(fmt_text, fmt_bytes), {}),
    "f0 format, the counting call alone (measure + scan)": (lambda: fmt(None, 0), {}),
}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for k, (run, kw) in legs.items():
        times[k].append(timed(run, **kw))
    say(f"round {r}: " + "; ".join(f"{k.split()[0]} {times[k][-1]:.2f} ms" for k in legs))
mean = {k: float(np.mean(v)) for k, v in times.items()}
for k, v in times.items():
    nb = fmt_bytes if k.startswith("f") else text_bytes
    nl = n if k.startswith("f") else n_lines
    what = "copied" if k.startswith("d") else "of text"
    say(f"({k}): mean {mean[k]:9.2f} ms, min {min(v):9.2f}, max {max(v):9.2f}  = {nl / mean[k] / 1e3:9.1f} M lines/s, {nb / mean[k] / 1e6:8.2f} GB/s {what}")
say(f"(a  parts): hipMemcpy of {rec_bytes} bytes to pinned host mean {np.mean(parts['copy']):.2f} ms; the loop mean {np.mean(parts['loop']):.2f} ms = {n_lines / np.mean(parts['loop']) / 1e3:.1f} M lines/s")
ka, kb, kb0, kc, kd, kf, kf0 = (next(k for k in legs if k.split()[0] == tag) for tag in ("a", "b", "b0", "c", "d", "f", "f0"))
write, fwrite = mean[kb] - mean[kb0], mean[kf] - mean[kf0]
say(f"write passes: sam (b - b0) = {write:.2f} ms for {text_bytes} bytes = {text_bytes / write / 1e6:.1f} GB/s; format (f - f0) = {fwrite:.2f} ms for {fmt_bytes} bytes = "
    f"{fmt_bytes / fwrite / 1e6:.1f} GB/s; per output byte sam / format = {(text_bytes / write) / (fmt_bytes / fwrite):.2f}x; sam write pass / copy (d) = {write / mean[kd]:.2f}x")
say(f"ratios: baseline / device-to-device = {mean[ka] / mean[kb]:.1f}x; baseline / pinned host out = {mean[ka] / mean[kc]:.1f}x")
