"""dev probe: fmgpu_positions_format against the path a caller has today, on --n synthetic records shaped like a genome run (qidx < n ascending, seq_id < 25,
pos < 2.5e8, errors 0 .. 2), resident on the device.  One job on one card; the legs are alternated --rounds times, each figure the mean of --steps runs after --warmup:
  (a) the baseline: one hipMemcpy of the records into pinned host memory, then the example's loop (snprintf of four %zu) into a memory buffer, no file I/O —
      tools/format_probe_host.cpp, built here with g++ -O2, ONE host thread; wall clock, once per round;
  (b) fmgpu_positions_format device to device, four columns: the whole call between two events; (b0) its counting call alone (measure + scan + the read-back), so
      (b) - (b0) is the write pass with its launch; (b') the same with a read-name column (names of 20 .. 40 bytes in a device table);
  (c) the same call with a pinned host `out`: wall clock (the staging buffer, the write pass and one device-to-host copy of the text);
  (d) one device-to-device copy of (records read + text written) bytes: the yardstick for a streaming pass.
The texts of (a) and (b) are compared byte for byte first.  --only-format runs leg (b) alone, --steps times, for
`rocprofv3 --kernel-trace --stats -- python tools/format_probe.py --only-format` (the three passes kernel by kernel).  Writes profiles/format_probe.log (or --log)."""
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

import fmindex_collection_amd as fm  # noqa: F401
from fmindex_collection_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--only-format", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "format_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    if not args.only_format:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if not torch.cuda.is_available():
    raise SystemExit("format_probe needs a GPU: nothing is measured without one")
dev = torch.device("cuda", 0)
L = capi.lib()
props = torch.cuda.get_device_properties(0)
say(f"# python tools/format_probe.py --n {args.n} --rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}")
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; clock_rate {getattr(props, 'clock_rate', 0) / 1e3:.0f} MHz; "
    f"memory_clock_rate {getattr(props, 'memory_clock_rate', 0) / 1e3:.0f} MHz; {props.total_memory / 2**30:.0f} GiB")

# ---- the records, made on the device: four 64-bit words each (the last one errors | hit << 32)
n = args.n
gen = torch.Generator(device=dev).manual_seed(11)
rec = torch.empty((n, 4), dtype=torch.int64, device=dev)
rec[:, 0] = torch.sort(torch.randint(0, n, (n,), device=dev, generator=gen)).values
rec[:, 1] = torch.randint(0, 25, (n,), device=dev, generator=gen)
rec[:, 2] = torch.randint(0, 250_000_000, (n,), device=dev, generator=gen)
rec[:, 3] = torch.randint(0, 3, (n,), device=dev, generator=gen) | ((torch.arange(n, device=dev) & 0xffffffff) << 32)
# read names of 20 .. 40 bytes without a blank, back to back; one span (offset, len) per read
name_len = 20 + (torch.arange(n, device=dev) * 7) % 21
spans = torch.stack([torch.cumsum(name_len, 0) - name_len, name_len], dim=1).contiguous()
name_bytes = torch.randint(48, 123, (int(name_len.sum().item()),), dtype=torch.uint8, device=dev, generator=gen)
torch.cuda.synchronize()
rec_bytes = rec.numel() * 8


def spec_of(columns, names=None):
    cols = [capi.COLUMNS[c] for c in columns]
    return capi.FormatSpec(len(cols), (C.c_uint8 * 8)(*(cols + [0] * (8 - len(cols)))), ord(" "), 0, 0, 0, 0, None if names is None else C.pointer(names), None)


table = capi.NameTable(name_bytes.data_ptr(), name_bytes.numel(), spans.data_ptr(), n)
plain, named = spec_of(("qidx", "seq_id", "pos", "errors")), spec_of(("read_name", "seq_id", "pos", "errors"), table)


def fmt(spec, out, capacity):
    nbytes = C.c_uint64()
    capi.check(L.fmgpu_positions_format(C.c_void_p(rec.data_ptr()), n, C.byref(spec), None if out is None else C.c_void_p(out.data_ptr()), capacity, C.byref(nbytes), None, None))
    return int(nbytes.value)


text_bytes, named_bytes = fmt(plain, None, 0), fmt(named, None, 0)
text, named_text = torch.empty(text_bytes, dtype=torch.uint8, device=dev), torch.empty(named_bytes, dtype=torch.uint8, device=dev)
say(f"# {n} records = {rec_bytes} bytes; four columns: {text_bytes} bytes of text ({text_bytes / n:.2f} per line); with read names: {named_bytes} bytes ({named_bytes / n:.2f} per line)")


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


if args.only_format:
    say(f"format, four columns {timed(lambda: fmt(plain, text, text_bytes)):.2f} ms, with read names {timed(lambda: fmt(named, named_text, named_bytes)):.2f} ms (under a profiler: not a figure)")
    raise SystemExit(0)

# ---- the baseline's helper, and the two texts against each other
tmp = tempfile.TemporaryDirectory()
so = os.path.join(tmp.name, "format_probe_host.so")
subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "format_probe_host.cpp"), "-o", so], check=True)
H = C.CDLL(so)
H.format_loop.restype = C.c_uint64
H.format_loop.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
pinned_rec = torch.empty((n, 4), dtype=torch.int64).pin_memory()
host_text = np.empty(text_bytes + 64, dtype=np.uint8)
pinned_out = torch.empty(text_bytes, dtype=torch.uint8).pin_memory()
parts = {"copy": [], "loop": []}


def baseline():
    t0 = time.perf_counter()
    pinned_rec.copy_(rec)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = H.format_loop(pinned_rec.data_ptr(), n, host_text.ctypes.data, host_text.size)
    t2 = time.perf_counter()
    assert got == text_bytes, (got, text_bytes)
    parts["copy"].append((t1 - t0) * 1e3)
    parts["loop"].append((t2 - t1) * 1e3)


baseline()
fmt(plain, text, text_bytes)
assert np.array_equal(text.cpu().numpy(), host_text[:text_bytes]), "the device text differs from the snprintf loop's"
fmt(plain, pinned_out, text_bytes)
assert np.array_equal(pinned_out.numpy(), host_text[:text_bytes]), "the text in the pinned buffer differs from the snprintf loop's"
say("# the device text (device out and pinned host out) equals the snprintf loop's, byte for byte")
parts = {"copy": [], "loop": []}

copy_bytes = rec_bytes + text_bytes
src, landing = torch.empty(copy_bytes, dtype=torch.uint8, device=dev), torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
legs = {
    "a  baseline: records to pinned host + snprintf loop, one host thread": (baseline, dict(events=False, steps=1, warmup=0)),
    "b  format, device to device, four columns": (lambda: fmt(plain, text, text_bytes), {}),
    "b0 the counting call alone (measure + scan)": (lambda: fmt(plain, None, 0), {}),
    "b' format, device to device, read_name + three columns": (lambda: fmt(named, named_text, named_bytes), {}),
    "c  format into a pinned host out, four columns": (lambda: fmt(plain, pinned_out, text_bytes), dict(events=False)),
    "d  device -> device copy of records + text bytes": (lambda: landing.copy_(src), {}),
}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for k, (run, kw) in legs.items():
        times[k].append(timed(run, **kw))
    say(f"round {r}: " + "; ".join(f"{k.split()[0]} {times[k][-1]:.2f} ms" for k in legs))
mean = {k: float(np.mean(v)) for k, v in times.items()}
for k, v in times.items():
    nb = named_bytes if k.startswith("b'") else copy_bytes if k.startswith("d") else text_bytes
    what = "copied" if k.startswith("d") else "of text"
    say(f"({k}): mean {mean[k]:9.2f} ms, min {min(v):9.2f}, max {max(v):9.2f}  = {n / mean[k] / 1e3:9.1f} M lines/s, {nb / mean[k] / 1e6:8.2f} GB/s {what}")
say(f"(a  parts): hipMemcpy of {rec_bytes} bytes to pinned host mean {np.mean(parts['copy']):.2f} ms; the loop mean {np.mean(parts['loop']):.2f} ms = {n / np.mean(parts['loop']) / 1e3:.1f} M lines/s")
ka, kb, kb0, kc, kd = (next(k for k in legs if k.split()[0] == tag) for tag in ("a", "b", "b0", "c", "d"))
write = mean[kb] - mean[kb0]
say(f"ratios: baseline / device-to-device = {mean[ka] / mean[kb]:.1f}x; baseline / pinned host out = {mean[ka] / mean[kc]:.1f}x; "
    f"write pass (b - b0 = {write:.2f} ms, reads {rec_bytes + 8 * n} bytes of records and offsets, writes {text_bytes}) / copy (d) = {write / mean[kd]:.2f}x")
