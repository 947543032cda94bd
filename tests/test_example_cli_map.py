"""The example's `--mode map` (fmindex-collection_amd/example/main.cpp): search, callback order and locate as one fmgpu_map call — the first three columns of its
`--save_output` file ("queryId seqId pos errors") are the file `--mode besthits` (for `noerror`: `all`) writes, and --feed (fmgpu_feed_map_v) writes the same file."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_example_cli import EXE, PKG, _fasta


def _build():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(os.path.join(PKG, "example", "main.cpp")):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)


def test_help_names_the_mode():
    _build()
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--mode [all, besthits, map]" in r.stdout
    r = subprocess.run([EXE, "--mode", "nope"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and '"map"' in r.stderr


@pytest.mark.gpu
def test_map_run_writes_the_besthits_rows_with_their_errors(tmp_path):
    _build()
    rng = np.random.default_rng(17)
    ref, qry, rp, qp = _fasta(rng, tmp_path)
    cases = [
        (["--algo", "noerror", "--min_k", "0", "--max_k", "0"], "all", (["--feed"],)),
        (["--algo", "ng26", "--gen", "h2-k2", "--min_k", "2", "--max_k", "2"], "besthits", (["--feed"], ["--packed"], ["--feed", "--packed"])),
        (["--algo", "ng26", "--gen", "h2-k2", "--min_k", "1", "--max_k", "1", "--maxhitperquery", "2", "--no-reverse"], "besthits", ()),
        (["--algo", "ng21", "--gen", "pigeon_opt", "--min_k", "1", "--max_k", "1"], "besthits", (["--feed"],)),
    ]
    for flags, mode, more in cases:
        outs = []
        for at, extra in enumerate([["--mode", mode], ["--mode", "map"]] + [["--mode", "map"] + m for m in more]):
            out = str(tmp_path / ("out%d.txt" % at))
            r = subprocess.run([EXE, "--index", rp, "--query", qp, "--save_output", out] + flags + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (flags, extra, r.stdout + r.stderr)
            outs.append(open(out).read().splitlines())
        assert len(outs[0]) > 0 and all(o == outs[1] for o in outs[2:]), flags
        assert [" ".join(line.split()[:3]) for line in outs[1]] == outs[0], flags
        assert all(len(line.split()) == 4 and int(line.split()[3]) <= int(flags[flags.index("--max_k") + 1]) for line in outs[1]), flags
