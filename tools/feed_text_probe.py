"""dev probe: a read FILE in, located positions out — fmgpu_feed_map_text (include/fmgpu.h) against what a caller had before it.  The genome stand-in
(datasets.genome_like_text with bench.GRCH38_LENGTHS scaled by --scale) as a BiFMIndex<5, IB16> at sampling rate 16; a generated FASTQ of --nq reads of --length
symbols with 0 / 1 / 2 substitutions 1:1:1 (the reads of tools/map_probe.py), written to a temporary file; the Hamming ladder h2(k + 2, 0, k), k = 0, 1, 2, at most
--max-hits rows per read.  Two legs, alternated --rounds times, the file cut into --pieces windows:
    a   Feed.map_file: the file's bytes (np.memmap) through fmgpu_feed_map_text
    b   parse_stream with host output (fmgpu_queries_parse per chunk of the same size, the batch downloaded), then Feed.map per batch (uploaded again)
Per leg: wall time (host clock, results landed), device bytes the feed holds afterwards (fmgpu_feed_info; slots only ever grow, so this is their peak), the lowest free
device memory during the leg (hipMemGetInfo sampled every millisecond) against the idle level, bytes uploaded.  Both legs must give the same positions.
Writes profiles/feed_text_probe.log (or --log)."""
import argparse
import os
import sys
import tempfile
import threading
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import fmindex_collection_amd as fm
from fmindex_collection_amd import datasets

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--nq", type=int, default=1_000_000)
ap.add_argument("--length", type=int, default=101)
ap.add_argument("--pieces", type=int, default=16)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--max-hits", type=int, default=100)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "feed_text_probe.log"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


dev = torch.device("cuda", 0)
c = types.SimpleNamespace(torch=torch, np=np, datasets=datasets, dev=dev, rank=0, args=types.SimpleNamespace(scale=args.scale))
say("# python tools/feed_text_probe.py " + " ".join(a for a in sys.argv[1:] if not a.startswith("/")))
props = torch.cuda.get_device_properties(0)
say(f"# device 0: {torch.cuda.get_device_name(0)}; {props.multi_processor_count} CUs; clock_rate {getattr(props, 'clock_rate', 0) / 1e3:.0f} MHz; "
    f"memory_clock_rate {getattr(props, 'memory_clock_rate', 0) / 1e3:.0f} MHz; {props.total_memory / 2**30:.0f} GiB")
text, seq_off, lengths, tinfo = bench.make_text(c, "genome")
qbuf, qoff = bench.sample_reads(c, text, lengths, args.length, args.nq, 1000, "k2")
index = fm.BiFMIndex.from_sequences((bench._Dev(text), bench._Dev(seq_off)), 5, "IB16", 16)
nq, L = args.nq, args.length

# the FASTQ: "@r%08d\n", the read, "+\n", a quality line — fixed-width records, written once
reads = qbuf.cpu().numpy().reshape(nq, L)
rec = np.empty((nq, 11 + L + 1 + 2 + L + 1), dtype=np.uint8)
rec[:, 0], rec[:, 1], rec[:, 10] = ord("@"), ord("r"), ord("\n")
ids = np.arange(nq, dtype=np.int64)
for d in range(8):
    rec[:, 9 - d] = ord("0") + (ids // 10 ** d) % 10
rec[:, 11: 11 + L] = np.frombuffer(b"$ACGT", dtype=np.uint8)[reads]
rec[:, 11 + L], rec[:, 12 + L], rec[:, 13 + L] = ord("\n"), ord("+"), ord("\n")
rec[:, 14 + L: 14 + 2 * L] = 33 + (np.arange(L)[None, :] + ids[:, None]) % 41
rec[:, 14 + 2 * L] = ord("\n")
tmp = tempfile.NamedTemporaryFile(suffix=".fastq", delete=False)
tmp.write(rec.tobytes())
tmp.close()
nbytes = rec.size
del rec, reads
B = -(-nbytes // args.pieces)
say(f"# genome stand-in, {int(text.numel())} symbols; BiFMIndex {index.device_bytes / 1e9:.2f} GB; FASTQ of {nq} reads x {L} symbols, {nbytes} bytes, {args.pieces} windows of {B} bytes; "
    f"Hamming ladder k = 0, 1, 2, at most {args.max_hits} rows per read")

table = fm.symbol_table.dna5()
ladder = [fm.search_scheme.h2(k + 2, 0, k) for k in range(3)]
kw = dict(schemes=ladder, edit=False, n=args.max_hits)


class LowWater:
    """the lowest free device memory while the block runs, sampled every millisecond"""

    def __enter__(self):
        torch.cuda.synchronize()
        self.idle = self.low = torch.cuda.mem_get_info(0)[0]
        self.stop = False
        self.thread = threading.Thread(target=self.loop)
        self.thread.start()
        return self

    def loop(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info(0)[0])
            time.sleep(0.001)

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()


def leg_a():
    with fm.Feed(index) as feed, LowWater() as mem:
        t = time.perf_counter()
        m = feed.map_file(tmp.name, "fastq", table, chunk_bytes=B, **kw)
        ms = (time.perf_counter() - t) * 1e3
        info = feed.info()
    return ms, info["device_bytes"], mem.idle - mem.low, info["uploaded_bytes"], m.positions


def leg_b():
    with fm.Feed(index) as feed, LowWater() as mem, open(tmp.name, "rb") as f:
        t = time.perf_counter()
        parts, first, hits, uploaded = [], 0, 0, 0
        for batch in fm.parse_stream(f, "fastq", table, chunk_bytes=B):
            pos = feed.map(batch.batch, **kw)
            pos["qidx"] += first
            parts.append(pos)
            first += batch.reads
            uploaded += batch.consumed + feed.info()["uploaded_bytes"]         # the text the parse took to the device, then the batch the feed took there again
        ms = (time.perf_counter() - t) * 1e3
        info = feed.info()
    return ms, info["device_bytes"], mem.idle - mem.low, uploaded, np.concatenate(parts)


results = {"a": [], "b": []}
for r in range(args.rounds):
    for name, leg in (("a", leg_a), ("b", leg_b)):
        ms, held, peak, up, pos = leg()
        results[name].append(ms)
        say(f"round {r} leg {name}: {ms:9.1f} ms; feed holds {held / 1e6:8.1f} MB on the device; peak beside the index {peak / 1e6:8.1f} MB; uploaded {up / 1e6:8.1f} MB; {len(pos)} positions")
        if name == "a":
            want = pos[["qidx", "seq_id", "pos", "errors"]].copy()
        else:
            assert np.array_equal(want, pos[["qidx", "seq_id", "pos", "errors"]]), "the two legs differ"
for name in "ab":
    say(f"leg {name}: median {float(np.median(results[name])):.1f} ms, min {min(results[name]):.1f}, max {max(results[name]):.1f} over {args.rounds} rounds")
os.unlink(tmp.name)
