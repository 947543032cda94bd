"""The example's --paired-sam flag (fmindex-collection_amd/example/main.cpp): with --mates the --save_output file is a paired-end SAM file, the header of --sam followed
by two records per fragment made on the device (fmgpu_positions_sam_mates through fmc::formatSamMates), and equals sam_header + format_sam_mates of the positions the
plain runs on the two files report and the pairs join_mates makes of them.  Without --mates it is refused; --mates --sam stays refused."""
import subprocess

import numpy as np
import pytest

import fmindex_collection_amd as fm
from tests.test_example_cli import EXE, load_fasta
from tests.test_example_cli_mates import MAP, _pair_files, _positions
from tests.test_example_cli_parse import _build, _run


def test_help_names_the_flag_and_it_needs_mates(tmp_path):
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--paired-sam" in r.stdout
    none = str(tmp_path / "none.fasta")
    for extra in ([], MAP, MAP + ["--sam"]):
        r = subprocess.run([EXE, "--index", none, "--query", none, "--paired-sam"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "--paired-sam needs --mates" in r.stderr, (extra, r.stderr)
    for extra, word in (([], "--mates needs --mode map"), (MAP + ["--sam"], "--mates does not go with --sam or --feed"), (MAP + ["--feed"], "--mates does not go with --sam or --feed"),
                        (MAP + ["--packed"], "--mates needs byte reads")):
        r = subprocess.run([EXE, "--index", none, "--query", none, "--mates", none, "--paired-sam"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)


@pytest.mark.gpu
def test_the_saved_file_equals_header_and_format_sam_mates_of_the_plain_positions(tmp_path):
    _build()
    rng = np.random.default_rng(41)
    (rp, q1, q2), (ref, t1, t2) = _pair_files(rng, tmp_path)
    ladder = MAP + ["--algo", "ng26", "--gen", "h2-k2", "--min_k", "2", "--max_k", "2"]
    out = str(tmp_path / "out.txt")
    names = [b"chr0", b"chr1", b"chr2"]
    head = fm.sam_header(names, [len(s) for s in load_fasta(ref, False)], "fmindex-collection-gpu-example")
    assert head.count(b"@SQ") == 3
    proper = 0
    for extra, tlen in (([], []), (["--pair-strands"], ["--min_tlen", "120", "--max_tlen", "250"]), (["--no-reverse"], ["--max_tlen", "400"])):
        both = "--no-reverse" not in extra
        plain = []
        for q in (q1, q2):
            r, saved = _run(rp, q, out, ladder, extra)
            assert r.returncode == 0, (extra, r.stdout + r.stderr)
            plain.append(_positions(saved))
        batches = [fm.flatten([np.array(x, dtype=np.uint8) for x in load_fasta(t, False)]) for t in (t1, t2)]
        lo, hi = (int(tlen[1]), int(tlen[3])) if len(tlen) == 4 else (0, int(tlen[1])) if tlen else (0, 1000)
        joined = fm.join_mates(plain[0], batches[0][1], plain[1], batches[1][1], strands=both, orientation="fr" if both else "any", min_tlen=lo, max_tlen=hi)
        want = head + fm.format_sam_mates(plain[0], batches[0], plain[1], batches[1], pairs=joined, strands="dna5" if both else None, seq_names=names, cigar=False)
        r = subprocess.run([EXE, "--index", rp, "--query", q1, "--mates", q2, "--paired-sam", "--save_output", out] + ladder + extra + tlen, capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stdout + r.stderr)
        got = open(out, "rb").read()
        assert got == want, (extra, got[len(head): len(head) + 200], want[len(head): len(head) + 200])
        records = [ln.split(b"\t") for ln in got[len(head):].splitlines()]
        assert len(records) == 120 and all(int(ln[1]) & 1 for ln in records) and [int(ln[0]) for ln in records] == [f // 2 for f in range(120)]
        assert sum(1 for ln in records if int(ln[1]) & 2) == 2 * int((joined.cls == 4).sum())
        proper += int((joined.cls == 4).sum())
        assert "pairs: %10d in" % len(joined.pairs) in r.stdout
    assert proper > 100
