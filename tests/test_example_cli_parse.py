"""The example's --device-parse flag (fmindex-collection_amd/example/main.cpp): the query file parsed by fmgpu_queries_parse — on a well-formed FASTA the run prints
and saves what the run without the flag does, a FASTQ of the same reads gives the same hits, and an unknown character fails without --convertUnknownChar."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_example_cli import EXE, PKG, _fasta


def _build():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(os.path.join(PKG, "example", "main.cpp")):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)


def _stable(stdout):
    """the lines of a run that do not hold times: what was loaded, and the result counts of every statistics line"""
    keep = []
    for ln in stdout.split("\n"):
        if ln.startswith(("loaded ", "using ", "start ")):
            keep.append(ln)
        elif " - results: " in ln and not ln.startswith("name"):
            keep.append(ln.split(":")[0] + ln[ln.index(" - results: "):])
    return keep


def test_help_names_the_flag():
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--device-parse" in r.stdout and "FASTQ" in r.stdout


def _run(rp, qp, out, flags, extra):
    r = subprocess.run([EXE, "--index", rp, "--query", qp, "--save_output", out] + flags + extra, capture_output=True, text=True)
    return r, (open(out, "rb").read() if r.returncode == 0 else b"")


@pytest.mark.gpu
def test_device_parse_writes_the_same_output(tmp_path):
    _build()
    rng = np.random.default_rng(17)
    ref, qry, rp, qp = _fasta(rng, tmp_path)
    reads = [ln for ln in qry.split("\n") if ln and not ln.startswith(">")]
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join("@read%d\n%s\n+\n%s\n" % (i, r, "".join(chr(33 + (i + k) % 41) for k in range(len(r)))) for i, r in enumerate(reads)))
    wrapped = tmp_path / "wrapped.fasta"                              # the same reads, each over several lines
    wrapped.write_text("".join(">read%d\n%s\n" % (i, "\n".join(r[k: k + 11] for k in range(0, len(r), 11))) for i, r in enumerate(reads)))
    cases = [
        ["--algo", "noerror", "--min_k", "0", "--max_k", "0"],
        ["--algo", "ng21", "--gen", "pigeon_opt", "--min_k", "0", "--max_k", "1", "--mode", "besthits", "--packed"],
    ]
    for flags in cases:
        out = str(tmp_path / "out.txt")
        plain, saved = _run(rp, qp, out, flags, [])
        assert plain.returncode == 0 and len(saved) > 0, (flags, plain.stdout + plain.stderr)
        for path in (qp, str(fq), str(wrapped)):
            r, got = _run(rp, path, out, flags, ["--device-parse"])
            assert r.returncode == 0, (flags, path, r.stdout + r.stderr)
            assert got == saved and _stable(r.stdout) == _stable(plain.stdout), (flags, path)
    r, _ = _run(rp, str(fq), str(tmp_path / "none.txt"), cases[0], [])          # FASTQ is read only with the flag
    assert r.returncode == 1 and "can't read fasta file" in r.stderr


@pytest.mark.gpu
def test_device_parse_unknown_characters_and_malformed_files(tmp_path):
    _build()
    rng = np.random.default_rng(18)
    ref, qry, rp, qp = _fasta(rng, tmp_path)
    flags = ["--algo", "noerror", "--min_k", "0", "--max_k", "0"]
    odd = tmp_path / "odd.fasta"
    odd.write_text(qry.replace("A", "N", 3))
    out = str(tmp_path / "out.txt")
    r, _ = _run(rp, str(odd), out, flags, ["--device-parse"])
    assert r.returncode == 1 and "unknown alphabet" in r.stderr
    r, got = _run(rp, str(odd), out, flags, ["--device-parse", "--convertUnknownChar"])
    r2, want = _run(rp, str(odd), out, flags, ["--convertUnknownChar"])
    assert r.returncode == 0 and r2.returncode == 0 and got == want and len(got) > 0
    bad = tmp_path / "bad.fastq"
    bad.write_text("@r0\nACGT\n+\nIII\n")
    r, _ = _run(rp, str(bad), out, flags, ["--device-parse"])
    assert r.returncode == 1 and "line 3" in r.stderr
