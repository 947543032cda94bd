"""The example's --chain-seeds flag (fmindex-collection_amd/example/main.cpp): under --mode map the scheme search is replaced by fmgpu_search_smems ->
fmgpu_locate_hits -> fmgpu_seeds_chain; the --save_output file holds one line per chain, "qidx seq_id tbeg tend qbeg qend score n_anchors", and equals what
search_smems -> locate_hits -> chain_seeds give in Python on the same FASTA files.  Without --mode map, or with a flag whose path it replaces, it is refused."""
import subprocess

import numpy as np
import pytest

import fmindex_collection_amd as fm
from tests.test_example_cli import EXE, load_fasta
from tests.test_example_cli_parse import _build

MAP = ["--mode", "map"]


def test_help_names_the_flag_and_the_combinations_that_are_refused(tmp_path):
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--chain-seeds" in r.stdout and "--min_seed" in r.stdout and "--max_seed_rows" in r.stdout
    none = str(tmp_path / "none.fasta")
    for extra, word in (([], "--chain-seeds needs --mode map"), (["--mode", "besthits"], "--chain-seeds needs --mode map"), (MAP + ["--packed"], "--chain-seeds needs byte reads"),
                        (MAP + ["--feed"], "--chain-seeds needs byte reads"), (MAP + ["--pair-strands"], "--chain-seeds needs byte reads"),
                        (MAP + ["--device-format"], "--chain-seeds needs byte reads"), (MAP + ["--sam"], "--chain-seeds needs byte reads"),
                        (MAP + ["--mates", none], "--chain-seeds needs byte reads")):
        r = subprocess.run([EXE, "--index", none, "--query", none, "--chain-seeds"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([EXE, "--index", none, "--query", none, "--mode", "maps", "--chain-seeds"], capture_output=True, text=True)
    assert r.returncode == 1 and 'invalid mode "maps", must be any of "all", "besthits", "map"' in r.stderr          # the --mode parser is as it was


def _files(rng, tmp_path):
    """a reference of three sequences and 40 reads of 120 symbols cut from it, each with two substitutions and a deletion of three bases, every third one (13 of them)
    from the reverse strand: with both strands every read chains, with --no-reverse the other 27 do"""
    seqs = ["".join("ACGT"[i] for i in rng.integers(0, 4, size=n)) for n in (2400, 1500, 1100)]
    ref = "".join(">chr%d\n%s\n" % (k, "\n".join(s[i: i + 60] for i in range(0, len(s), 60))) for k, s in enumerate(seqs))
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    reads = []
    for r in range(40):
        s = seqs[r % 3]
        at = int(rng.integers(0, len(s) - 123))
        m = list(s[at: at + 70] + s[at + 73: at + 123])
        for j in (30, 95):
            m[j] = comp[m[j]]
        reads.append("".join(comp[c] for c in reversed(m)) if r % 3 == 2 else "".join(m))
    qry = "".join(">read%d\n%s\n" % (i, r) for i, r in enumerate(reads))
    paths = [str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fasta")]
    for path, text in zip(paths, (ref, qry)):
        with open(path, "w") as fh:
            fh.write(text)
    return paths, (ref, qry)


@pytest.mark.gpu
def test_chain_lines_equal_the_python_path(tmp_path):
    _build()
    (rp, qp), (ref, qry) = _files(np.random.default_rng(23), tmp_path)
    gx = fm.BiFMIndex.from_sequences([np.array(s, dtype=np.uint8) for s in load_fasta(ref, False)], 5, "IB16", 16)
    out = str(tmp_path / "out.txt")
    for extra, reverse, min_len, max_rows in (([], True, 19, 50), (["--min_seed", "12", "--max_seed_rows", "0"], True, 12, 0), (["--no-reverse", "--min_seed", "25"], False, 25, 50)):
        reads = [np.array(r, dtype=np.uint8) for r in load_fasta(qry, reverse)]
        hits, spans = fm.search_smems(gx, reads, min_len=min_len, max_rows=max_rows)
        pos = gx.locate_hits(hits)
        want = fm.chain_seeds(pos, spans, len(reads))
        lines = ["%d %d %d %d %d %d %d %d" % tuple(int(c[k]) for k in ("qidx", "seq_id", "tbeg", "tend", "qbeg", "qend", "score", "n_anchors")) for c in want.chains]
        r = subprocess.run([EXE, "--index", rp, "--query", qp, "--save_output", out, "--chain-seeds", "--algo", "ng26", "--min_k", "0", "--max_k", "0"] + MAP + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stdout + r.stderr)
        got = open(out).read().splitlines()
        assert got == lines, (extra, got[:3], lines[:3])
        assert "anchors: %10d chains: %10d in %10d of %10d queries" % (len(pos), len(lines), int((want.cls == 1).sum()), len(reads)) in r.stdout
        assert len(lines) >= (40 if reverse else 27) and int((want.chains["n_anchors"] >= 2).sum()) >= (20 if min_len < 25 else 1)
