"""dev probe: both strands of every read — fmgpu_map_strands and fmgpu_feed_map_text_strands (include/fmgpu.h) against the way a caller mapped both strands before them,
with the method of tools/map_probe.py.  The genome stand-in as a BiFMIndex<5, IB16> at sampling rate 16, --nq reads of --length symbols with
0 / 1 / 2 substitutions 1:1:1, every other read reverse-complemented before the run (so both strands occur), the Hamming ladder h2(k + 2, 0, k), k = 0, 1, 2, at most
--max-hits rows per read.  Every figure is the wall time of one call sequence, host clock, ending when its results have landed; legs alternated --rounds times,
--reps calls each.
    a   reverse complements made on the host (NumPy, fm.both_strands), then fmgpu_map on the doubled host batch
    b   fmgpu_map_strands, pair = 0, host pointers (forward strand only)
    c   fmgpu_map_strands, pair = 1
    ta  fmgpu_feed_map on the host-doubled batch (reads already parsed and doubled on the host: neither is in the time)
    tb  fmgpu_feed_map_text_strands on the FASTA bytes of the forward reads, pair = 0;   tc  the same, pair = 1
  and the strands kernel alone: fmgpu_queries_strands on device buffers against one device-to-device copy of the bytes it writes.
Writes profiles/strands_probe.log (or --log)."""
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
from fmindex_collection_amd.capi import HIT_DTYPE, POSITION_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--nq", type=int, default=1_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-hits", type=int, default=100)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "strands_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


def wall(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


dev = torch.device("cuda", 0)
c = types.SimpleNamespace(torch=torch, np=np, datasets=datasets, dev=dev, rank=0, args=types.SimpleNamespace(scale=args.scale))
L = capi.lib()
say("# python tools/strands_probe.py " + " ".join(a for a in sys.argv[1:] if not a.startswith("/")))
props = torch.cuda.get_device_properties(0)
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; {props.total_memory / 2**30:.0f} GiB")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
qbuf, qoff = bench.sample_reads(c, text, lengths, args.length, args.nq, 1000, "k2")
torch.cuda.synchronize()
t0 = time.time()
index = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
nq = args.nq
DNA = np.array([0, 4, 3, 2, 1], dtype=np.uint8)
hq, ho = qbuf.cpu().numpy().copy(), qoff.cpu().numpy().astype(np.uint64)
assert (np.diff(ho.astype(np.int64)) == args.length).all()
rows = hq.reshape(nq, args.length)
rows[1::2] = DNA[rows[1::2, ::-1]]                                    # every other read is handed over as its reverse complement
say(f"# genome stand-in, {int(text.numel())} symbols; BiFMIndex ({index.device_bytes / 1e9:.2f} GB) built in {time.time() - t0:.1f} s; {nq} reads x {args.length} symbols, "
    f"0 / 1 / 2 substitutions 1:1:1, every other one reverse-complemented; ladder h2(k + 2, 0, k), k = 0, 1, 2, Hamming; at most {args.max_hits} rows per read")

ladder = [fm.search_scheme.h2(k + 2, 0, k) for k in range(3)]
what, alive = fm._map_query(None, ladder, False, False, args.max_hits or fm.UINT64_MAX, True, 0)
strands = {p: capi.Strands(DNA.ctypes.data_as(capi.u8p), 5, p) for p in (0, 1)}
out = {}


def run(key, call, npos, nhits, nstr):
    """one call into fresh host arrays kept under `key` -> (rc, positions, hits)"""
    pos, hits, stratum = np.zeros(max(npos, 1), dtype=POSITION_DTYPE), np.zeros(max(nhits, 1), dtype=HIT_DTYPE), np.zeros(max(nstr, 1), dtype=np.uint8)
    cnt, hcnt = C.c_uint64(), C.c_uint64()
    sstats, lstats = (capi.Stats * 3)(), capi.Stats()
    rc = call(capi.ptr(pos), npos, C.byref(cnt), capi.ptr(hits), nhits, C.byref(hcnt), capi.ptr(stratum), sstats, C.byref(lstats))
    out[key] = (pos[: min(cnt.value, npos)], hits[: min(hcnt.value, nhits)], stratum[:nstr], [sstats[i] for i in range(3)])
    return rc, int(cnt.value), int(hcnt.value)


def leg_a(npos, nhits):
    dq, do = fm.both_strands((hq, ho), DNA)
    return run("a", lambda *a: L.fmgpu_map(index._h, capi.ptr(dq), capi.ptr(do), 2 * nq, C.byref(what), *a, None), npos, nhits, 2 * nq)


def leg_s(pair, npos, nhits):
    return run("bc"[pair], lambda *a: L.fmgpu_map_strands(index._h, capi.ptr(hq), capi.ptr(ho), nq, C.byref(what), C.byref(strands[pair]), *a, None), npos, nhits, 2 * nq)


# sizes from counting calls (the counts are exact on FMGPU_ERR_CAPACITY)
size = {}
for key, f in (("a", lambda n, h: leg_a(n, h)), ("b", lambda n, h: leg_s(0, n, h)), ("c", lambda n, h: leg_s(1, n, h))):
    rc, npos, nhits = f(0, 0)
    assert rc in (0, capi.FMGPU_ERR_CAPACITY), L.fmgpu_last_error()
    size[key] = (npos, nhits)
say(f"# records: a {size['a'][1]} hits / {size['a'][0]} positions, b {size['b'][1]} / {size['b'][0]}, c {size['c'][1]} / {size['c'][0]}")
assert size["a"] == size["b"]

# text legs: the forward reads as FASTA
letters = np.frombuffer(b"$ACGT", dtype=np.uint8)
rec = np.empty((nq, args.length + 4), dtype=np.uint8)
rec[:, 0], rec[:, 1], rec[:, 2], rec[:, -1] = ord(">"), ord("r"), ord("\n"), ord("\n")
rec[:, 3:-1] = letters[rows]
fasta = rec.reshape(-1)
table = fm.symbol_table("ACGT", 1, True, fm.FOREIGN)
feed = fm.Feed(index)
res = capi.ParseResult()


def leg_ta(npos, nhits):
    dq, do = out["doubled"]
    return run("ta", lambda *a: L.fmgpu_feed_map(feed._f, capi.ptr(dq), capi.ptr(do), 2 * nq, C.byref(what), *a), npos, nhits, 2 * nq)


def leg_t(pair, npos, nhits):
    return run("t" + "bc"[pair], lambda pos, cap, cnt, hits, hcap, hcnt, stratum, ss, ls: L.fmgpu_feed_map_text_strands(
        feed._f, capi.ptr(fasta), fasta.size, capi.TEXT_FASTA, 1, capi.ptr(table), 0, C.byref(what), C.byref(strands[pair]), pos, cap, cnt, hits, hcap, hcnt, stratum,
        None, None, None, nq, C.byref(res), ss, ls), npos, nhits, 2 * nq)


out["doubled"] = fm.both_strands((hq, ho), DNA)
LEGS = {
    "a": lambda: leg_a(*size["a"]), "b": lambda: leg_s(0, *size["b"]), "c": lambda: leg_s(1, *size["c"]),
    "ta": lambda: leg_ta(*size["a"]), "tb": lambda: leg_t(0, *size["b"]), "tc": lambda: leg_t(1, *size["c"]),
}
NAMES = {"a": "a  host revcomp + fmgpu_map", "b": "b  fmgpu_map_strands pair=0", "c": "c  fmgpu_map_strands pair=1",
         "ta": "ta fmgpu_feed_map, doubled batch", "tb": "tb feed_map_text_strands pair=0", "tc": "tc feed_map_text_strands pair=1"}
uploaded = {}
for k, f in LEGS.items():                                              # warm-up, the results, the bytes that travel
    rc = f()
    assert rc[0] == 0, (k, rc, L.fmgpu_last_error())
    if k.startswith("t"):
        uploaded[k] = feed.info()["uploaded_bytes"]
uploaded.update(a=2 * hq.size + 8 * (2 * nq + 1), b=hq.size + 8 * (nq + 1), c=hq.size + 8 * (nq + 1))
same = lambda x, y: all(out[x][i].tobytes() == out[y][i].tobytes() for i in range(3))
assert same("a", "b") and same("a", "ta") and same("a", "tb"), "pair = 0: results differ from fmgpu_map on the doubled batch"
assert same("c", "tc"), "pair = 1: the feed differs from the one-shot call"
ha, hc = out["a"][1], out["c"][1]
records = lambda h: set(np.ascontiguousarray(h).view(np.uint8).reshape(len(h), 40).view("V40").reshape(-1).tolist())
assert len(hc) <= len(ha) and records(hc) <= records(ha), "pair = 1: not a subset of the independent ladder's records"
say(f"# b, ta, tb return leg a's positions, hit records and strata byte for byte; tc returns c's; c's {len(hc)} records are among a's {len(ha)}")
say("# bytes uploaded: " + ", ".join(f"{k} {uploaded[k] / 1e6:.1f} MB" for k in LEGS))
for k in ("a", "c"):
    stratum, st = out[k][2], out[k][3]
    searched = [2 * nq] + [int((stratum >= i).sum()) for i in (1, 2)]      # a read still unfound (or found later) when stratum i starts
    say(f"# {NAMES[k]}: per stratum reads searched {searched}, kernel_ms " + " ".join(f"{s.kernel_ms:.2f}" for s in st) + ", lf_steps " + " ".join(str(s.lf_steps) for s in st)
        + f"; reads with stratum 0/1/2/none: {[int((stratum == v).sum()) for v in (0, 1, 2, 255)]}")

say(f"# legs, wall ms of one call sequence: round, leg, the {args.reps} calls, their median")
med = {k: [] for k in LEGS}
for r in range(args.rounds):
    for k, f in LEGS.items():
        t = [wall(f) for _ in range(args.reps)]
        med[k].append(float(np.median(t)))
        say(f"round {r + 1}  {NAMES[k]:<34s} " + " ".join(f"{x:9.2f}" for x in t) + f"   median {med[k][-1]:9.2f}")
for k in LEGS:
    say(f"# {NAMES[k]:<34s} median of the round medians {float(np.median(med[k])):9.2f} ms, spread (max - min) {max(med[k]) - min(med[k]):6.2f} ms")
t = [wall(lambda: fm.both_strands((hq, ho), DNA)) for _ in range(3)]
say(f"# inside leg a: fm.both_strands on the host alone {float(np.median(t)):.2f} ms")

# the strands kernel alone, against one device-to-device copy of the bytes it writes
dq, do = capi.DeviceBuffer.from_array(hq), capi.DeviceBuffer.from_array(ho)
oq, oo = capi.DeviceBuffer(2 * hq.size + 16), capi.DeviceBuffer((2 * nq + 1) * 8)
src = torch.empty(2 * hq.size, dtype=torch.uint8, device=dev)
dst = torch.empty_like(src)
call = lambda: L.fmgpu_queries_strands(capi.ptr(dq), capi.ptr(do), nq, capi.ptr(DNA), 5, capi.ptr(oq), capi.ptr(oo), None)
assert call() == 0
wq, wo = out["doubled"]
assert np.array_equal(oq.to_array(np.uint8, wq.size), wq) and np.array_equal(oo.to_array(np.uint64, wo.size), wo)
ts = sorted(wall(call) for _ in range(21))
tc = sorted(wall(lambda: dst.copy_(src)) for _ in range(21))
say(f"# fmgpu_queries_strands, device to device, {2 * hq.size / 1e6:.0f} MB written (the whole call: table upload, offsets pass, one read-back, symbol pass): "
    f"median {ts[10]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}); one device-to-device copy of as many bytes: median {tc[10]:.3f} ms (min {tc[0]:.3f}, max {tc[-1]:.3f})")
