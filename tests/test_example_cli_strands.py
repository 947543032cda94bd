"""The example's --pair-strands flag (fmindex-collection_amd/example/main.cpp): reverse complements made on the device and the best stratum per read.  The
--save_output file of a --pair-strands run holds the lines of the run on the host-doubled batch (the example's default: every read followed by its reverse complement,
the same numbering) with the pair rule applied to them: of a read's two strands only those found at the pair's lowest stratum keep their lines.  The ladder's stratum j
runs the scheme with exactly j errors, so a line's error count is its read's stratum."""
import subprocess

import numpy as np
import pytest

from tests.test_example_cli import EXE, _fasta
from tests.test_example_cli_parse import _build, _run


def pair_rule(saved):
    """the lines of the independent ladder on the doubled batch -> the lines the pair ladder leaves"""
    lines = [ln for ln in saved.decode().split("\n") if ln]
    best = {}
    for ln in lines:
        q, _, _, e = (int(x) for x in ln.split())
        best[q >> 1] = min(best.get(q >> 1, 255), e)
    return [ln for ln in lines if int(ln.split()[3]) == best[int(ln.split()[0]) >> 1]]


def test_help_names_the_flag_and_the_flag_needs_mode_map(tmp_path):
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--pair-strands" in r.stdout
    r = subprocess.run([EXE, "--index", str(tmp_path / "none.fasta"), "--query", str(tmp_path / "none.fasta"), "--pair-strands"], capture_output=True, text=True)
    assert r.returncode == 1 and "--pair-strands needs --mode map" in r.stderr


@pytest.mark.gpu
def test_pair_strands_writes_the_doubled_batch_run_under_the_pair_rule(tmp_path):
    _build()
    rng = np.random.default_rng(31)
    ref, qry, rp, qp = _fasta(rng, tmp_path)
    # one more read X' = 32 symbols of chrA with two substitutions, whose reverse complement is planted as a sequence of its own: found forward with 2 errors,
    # on strand 1 with none — the independent ladder reports both, the pair ladder strand 1 only
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    x = list(ref.split("\n")[1][10:42])
    for at in (7, 23):
        x[at] = comp[x[at]]
    x = "".join(x)
    rp, qp = str(tmp_path / "ref2.fasta"), str(tmp_path / "reads2.fasta")
    with open(rp, "w") as f:
        f.write(ref + ">chrD\n" + "".join(comp[ch] for ch in reversed(x)) + "\n")
    qry += ">readX\n" + x + "\n"
    with open(qp, "w") as f:
        f.write(qry)
    reads = [ln for ln in qry.split("\n") if ln and not ln.startswith(">")]
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join("@read%d\n%s\n+\n%s\n" % (i, r, "".join(chr(33 + (i + k) % 41) for k in range(len(r)))) for i, r in enumerate(reads)))
    ladder = ["--mode", "map", "--algo", "ng26", "--gen", "h2-k2", "--min_k", "2", "--max_k", "2"]
    out = str(tmp_path / "out.txt")
    doubled, saved = _run(rp, qp, out, ladder, [])                       # reverse complements made on the host, the independent ladder
    assert doubled.returncode == 0 and "incl reverse complements" in doubled.stdout, doubled.stdout + doubled.stderr
    want = pair_rule(saved)
    assert 0 < len(want) < len([ln for ln in saved.decode().split("\n") if ln])      # some strand was found again with more errors
    assert {int(ln.split()[0]) & 1 for ln in want} == {0, 1}                # both strands have hits
    for extra in ([], ["--feed"], ["--feed", "--device-parse"]):
        for path in (qp, str(fq)) if "--device-parse" in extra else (qp,):
            r, got = _run(rp, path, out, ladder, extra + ["--pair-strands"])
            assert r.returncode == 0, (extra, r.stdout + r.stderr)
            assert [ln for ln in got.decode().split("\n") if ln] == want, (extra, path)
            assert ("bytes of query text" in r.stdout) == ("--device-parse" in extra)      # the text path: no read was a vector on the host
    # exact search has no ladder: the pair run writes what the doubled batch writes
    exact = ["--mode", "map", "--algo", "noerror", "--min_k", "0", "--max_k", "0"]
    plain, saved = _run(rp, qp, out, exact, [])
    r, got = _run(rp, qp, out, exact, ["--feed", "--device-parse", "--pair-strands"])
    assert plain.returncode == 0 and r.returncode == 0 and got == saved and len(saved) > 0 and "bytes of query text" in r.stdout
    # without the flag the text path still needs --no-reverse
    r, got = _run(rp, qp, out, exact, ["--feed", "--device-parse"])
    assert r.returncode == 0 and "bytes of query text" not in r.stdout and got == saved
