"""tests/cpp/test_hamming_sm.cpp: fmc::search_hamming_sm (include/fmc_gpu.hpp): the masks of ScoringMatrix on the host; on a GPU the reference test's matrix and the
IUPAC helper against a brute-force scorer, and the identity matrix against search_ng26."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fmindex-collection_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_hamming_sm")


def _build():
    subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_hamming_sm.cpp"), "-o", EXE,
                    "-L" + PKG, "-lfmgpu", "-Wl,-rpath," + PKG], check=True)


def test_hamming_sm_cpp_compiles_and_masks():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 77), r.stdout + r.stderr            # (1: a mask check failed)


@pytest.mark.gpu
def test_hamming_sm_cpp_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
