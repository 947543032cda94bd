"""The example's --align-chains flag (fmindex-collection_amd/example/main.cpp): with --chain-seeds every chain is aligned between its ends (fmgpu_chains_align through
fmc::alignChains) and each line of the --save_output file gains "status n_match n_mismatch n_ins n_del cigar", equal to what align_chains gives in Python on the same
FASTA files.  Without the flag the file is what --chain-seeds alone writes; without --chain-seeds the flag is refused."""
import subprocess

import numpy as np
import pytest

import fmindex_collection_amd as fm
from tests.test_example_cli import EXE, load_fasta
from tests.test_example_cli_chain import MAP, _files
from tests.test_example_cli_parse import _build


def test_help_names_the_flag_and_it_needs_chain_seeds(tmp_path):
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--align-chains" in r.stdout and "status n_match n_mismatch n_ins n_del cigar" in r.stdout
    none = str(tmp_path / "none.fasta")
    r = subprocess.run([EXE, "--index", none, "--query", none, "--align-chains"] + MAP, capture_output=True, text=True)
    assert r.returncode == 1 and "--align-chains needs --chain-seeds" in r.stderr
    r = subprocess.run([EXE, "--index", none, "--query", none, "--align-chains", "--chain-seeds"], capture_output=True, text=True)
    assert r.returncode == 1 and "--chain-seeds needs --mode map" in r.stderr                                     # the checks of --chain-seeds are as they were


@pytest.mark.gpu
def test_alignment_columns_equal_the_python_path(tmp_path):
    _build()
    (rp, qp), (ref, qry) = _files(np.random.default_rng(23), tmp_path)
    gx = fm.BiFMIndex.from_sequences([np.array(s, dtype=np.uint8) for s in load_fasta(ref, False)], 5, "IB16", 16)
    out = str(tmp_path / "out.txt")
    for extra, reverse, min_len in (([], True, 19), (["--no-reverse", "--min_seed", "12"], False, 12)):
        reads = [np.array(r, dtype=np.uint8) for r in load_fasta(qry, reverse)]
        hits, spans = fm.search_smems(gx, reads, min_len=min_len, max_rows=50)
        pos = gx.locate_hits(hits)
        chained = fm.chain_seeds(pos, spans, len(reads))
        aligned = fm.align_chains(gx, chained, pos, spans, reads)
        plain = ["%d %d %d %d %d %d %d %d" % tuple(int(c[k]) for k in ("qidx", "seq_id", "tbeg", "tend", "qbeg", "qend", "score", "n_anchors")) for c in chained.chains]
        lines = [p + " %d %d %d %d %d " % tuple(int(r[k]) for k in ("status", "n_match", "n_mismatch", "n_ins", "n_del")) + aligned.cigar(i)
                 for i, (p, r) in enumerate(zip(plain, aligned.alignments))]
        base = [EXE, "--index", rp, "--query", qp, "--save_output", out, "--chain-seeds", "--algo", "ng26", "--min_k", "0", "--max_k", "0"] + MAP + extra
        r = subprocess.run(base + ["--align-chains"], capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stdout + r.stderr)
        got = open(out).read().splitlines()
        assert got == lines, (extra, got[:3], lines[:3])
        assert "align-chains" in r.stdout and "operations: %10d" % len(aligned.ops) in r.stdout
        assert len(lines) >= 27 and any("D" in ln.split()[-1] or "I" in ln.split()[-1] for ln in lines) and any("X" in ln.split()[-1] for ln in lines)
        # without the flag: the lines of --chain-seeds alone, and no word of the alignment on the terminal
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0 and open(out).read().splitlines() == plain and "align-chains" not in r.stdout
