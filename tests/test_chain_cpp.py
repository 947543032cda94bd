"""tests/cpp/test_chain.cpp: fmc::ChainSpec, fmc::SeedChains and fmc::chainSeeds of include/fmc_gpu.hpp.  The host mirror and the argument checks of fmgpu_seeds_chain
are checked everywhere (the program exits 77 behind those checks where there is no device); on a GPU fmc::chainSeeds is held against cases the plain-Python model of
tests/chain_model.py wrote out."""
import os
import subprocess

import numpy as np
import pytest

from tests import chain_cases as cases
from tests import chain_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fmindex-collection_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_chain")


def _build():
    if not os.path.exists(os.path.join(PKG, "libfmgpu.so")):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_chain.cpp"), "-o", EXE,
                    "-L" + PKG, "-lfmgpu", "-Wl,-rpath," + PKG], check=True)


def write_cases(path):
    """inputs, parameters and the model's outputs as whitespace-separated numbers, in the order tests/cpp/test_chain.cpp reads them"""
    rng = np.random.default_rng(17)
    rows, q = [], 0
    for n in (1, 2, 31, 33, 64, 65, 300, 7):
        for seq in range(1 + n % 2):
            rows += cases.run_anchors(rng, n, q, seq, base=1000 if q % 3 else 1 << 33)
        q += 2 if n == 33 else 1
    nq = q + 1
    pos, spans = cases.pack(rows, rng)
    specs = [dict(), dict(max_lookback=3, gap_cost_q8=0), dict(max_lookback=256, min_anchors=2, max_chains=2), dict(max_anchors=64, min_score=40, max_skew=4, max_gap=200)]
    lines = [str(len(specs))]
    for kw in specs:
        full = dict(max_gap=5000, max_skew=500, gap_cost_q8=128, max_lookback=64, min_score=0, min_anchors=1, max_chains=0, max_anchors=0)
        full.update(kw)
        chains, off, cls, idx = model.chain(pos, spans, nq, **full)
        lines.append(" ".join(str(v) for v in [nq, len(pos), len(spans)] + list(full.values())))
        lines += ["%d %d %d %d" % (r["qidx"], r["seq_id"], r["pos"], r["hit"]) for r in pos]
        lines += ["%d %d" % (s["qbeg"], s["qlen"]) for s in spans]
        lines.append(str(len(chains)))
        lines += [" ".join(str(v) for v in c) for c in chains]
        lines += [" ".join(str(v) for v in off), " ".join(str(v) for v in cls), str(len(idx)), " ".join(str(v) for v in idx)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_chain_cpp_compiles_and_the_host_mirror_holds(tmp_path):
    _build()
    path = str(tmp_path / "chain_cases.txt")
    write_cases(path)                                                    # (read only where there is a device)
    r = subprocess.run([EXE, path], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 77), r.stdout + r.stderr
    assert "FAILED" not in r.stdout


@pytest.mark.gpu
def test_chain_cpp_on_gpu(tmp_path):
    _build()
    path = str(tmp_path / "chain_cases.txt")
    write_cases(path)
    r = subprocess.run([EXE, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
