"""The example's --mates flag (fmindex-collection_amd/example/main.cpp): under --mode map both read files are mapped and their positions joined on the device
(fmgpu_positions_mates through fmc::joinMates); the --save_output file holds one line per pair, "fragment seqId posA strandA posB strandB tlen errors", and equals what
join_mates makes of the positions the plain runs on the two files report.  With --sam, --feed, --packed, --device-format, --queries or without --mode map it is refused."""
import subprocess

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd.capi import POSITION_DTYPE
from tests.test_example_cli import EXE, load_fasta
from tests.test_example_cli_parse import _build, _run

MAP = ["--mode", "map"]


def test_help_names_the_flag_and_the_combinations_that_are_refused(tmp_path):
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--mates" in r.stdout and "--min_tlen" in r.stdout and "--max_tlen" in r.stdout
    none = str(tmp_path / "none.fasta")
    for extra, word in (([], "--mates needs --mode map"), (["--mode", "besthits"], "--mates needs --mode map"), (MAP + ["--sam"], "--mates does not go with --sam or --feed"),
                        (MAP + ["--feed"], "--mates does not go with --sam or --feed"), (MAP + ["--packed"], "--mates needs byte reads"),
                        (MAP + ["--device-format"], "--mates needs byte reads"), (MAP + ["--queries", "10"], "--mates needs byte reads"),
                        (MAP + ["--min_tlen", "9", "--max_tlen", "8"], "--min_tlen lies above --max_tlen")):
        r = subprocess.run([EXE, "--index", none, "--query", none, "--mates", none] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)


def _pair_files(rng, tmp_path):
    """a reference of three sequences and 60 fragments of 90 .. 300 symbols cut from it: mate 1 = the first 36 symbols, mate 2 = the first 36 of the reverse complement,
    swapped for every third fragment, a substitution in every fourth read"""
    seqs = ["".join("ACGT"[i] for i in rng.integers(0, 4, size=n)) for n in (1800, 1200, 900)]
    ref = "".join(">chr%d\n%s\n" % (k, "\n".join(s[i: i + 60] for i in range(0, len(s), 60))) for k, s in enumerate(seqs))
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    files = ([], [])
    for f in range(60):
        s = seqs[f % 3]
        length = int(rng.integers(90, 301))
        at = int(rng.integers(0, len(s) - length + 1))
        frag = s[at: at + length]
        mates = [frag[:36], "".join(comp[c] for c in reversed(frag))[:36]]
        if f % 3 == 1:
            mates.reverse()
        for k in range(2):
            m = list(mates[k])
            if (f + k) % 4 == 0:
                j = int(rng.integers(0, 36))
                m[j] = comp[m[j]]
            files[k].append("".join(m))
    paths = [str(tmp_path / name) for name in ("ref.fasta", "mates1.fasta", "mates2.fasta")]
    texts = [ref] + ["".join(">frag%d/%d\n%s\n" % (i, k + 1, r) for i, r in enumerate(files[k])) for k in range(2)]
    for path, text in zip(paths, texts):
        with open(path, "w") as fh:
            fh.write(text)
    return paths, texts


def _positions(saved):
    return np.array([tuple(int(v) for v in ln.split()) + (0,) for ln in saved.decode().splitlines()], dtype=POSITION_DTYPE)


@pytest.mark.gpu
def test_pair_lines_equal_join_mates_of_the_plain_positions(tmp_path):
    _build()
    rng = np.random.default_rng(41)
    (rp, q1, q2), (_, t1, t2) = _pair_files(rng, tmp_path)
    ladder = MAP + ["--algo", "ng26", "--gen", "h2-k2", "--min_k", "2", "--max_k", "2"]
    out = str(tmp_path / "out.txt")
    seen = 0
    for extra, tlen in (([], []), (["--pair-strands"], ["--min_tlen", "120", "--max_tlen", "250"]), (["--no-reverse"], ["--max_tlen", "400"])):
        both = "--no-reverse" not in extra
        plain = []
        for q in (q1, q2):
            r, saved = _run(rp, q, out, ladder, extra)
            assert r.returncode == 0, (extra, r.stdout + r.stderr)
            plain.append(_positions(saved))
        qoff = [fm.flatten([np.array(x, dtype=np.uint8) for x in load_fasta(t, False)])[1] for t in (t1, t2)]
        lo, hi = (int(tlen[1]), int(tlen[3])) if len(tlen) == 4 else (0, int(tlen[1])) if tlen else (0, 1000)
        want = fm.join_mates(plain[0], qoff[0], plain[1], qoff[1], strands=both, orientation="fr" if both else "any", min_tlen=lo, max_tlen=hi)
        lines = []
        for p in want.pairs:
            a, b = plain[0][p["a"]], plain[1][p["b"]]
            sa, sb = ("-" if both and a["qidx"] & 1 else "+"), ("-" if both and b["qidx"] & 1 else "+")
            lines.append("%d %d %d %s %d %s %d %d" % (p["fragment"], a["seq_id"], a["pos"], sa, b["pos"], sb, p["tlen"], p["errors"]))
        r = subprocess.run([EXE, "--index", rp, "--query", q1, "--mates", q2, "--save_output", out] + ladder + extra + tlen, capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stdout + r.stderr)
        got = open(out).read().splitlines()
        assert got == lines, (extra, got[:3], lines[:3])
        assert "loaded 60 mates" in r.stdout or "loaded 120 mates" in r.stdout
        assert "pairs: %10d in" % len(lines) in r.stdout
        if both:
            assert len(lines) >= (25 if tlen else 50) and {ln.split()[3] for ln in lines} == {"+", "-"}      # nearly every fragment is found as a pair, mate 1 on either strand
        seen += len(lines)
    assert seen > 100
    # files of different read counts do not pair up
    short = str(tmp_path / "short.fasta")
    with open(short, "w") as fh:
        fh.write(t2[: t2.index(">frag50/")])
    r = subprocess.run([EXE, "--index", rp, "--query", q1, "--mates", short] + ladder, capture_output=True, text=True)
    assert r.returncode == 1 and "do not hold the same number of reads" in r.stderr
