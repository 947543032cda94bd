"""tests/cpp/test_sam_mates.cpp: fmc::SamMatesSpec, fmc::ArrayView and fmc::formatSamMates of include/fmc_gpu.hpp.  The host mirror and the argument checks of
fmgpu_positions_sam_mates are checked everywhere (the program exits 77 behind those checks where there is no device); on a GPU fmc::formatSamMates is held against
fixed lines."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fmindex-collection_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_sam_mates")


def _build():
    if not os.path.exists(os.path.join(PKG, "libfmgpu.so")):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_sam_mates.cpp"), "-o", EXE,
                    "-L" + PKG, "-lfmgpu", "-Wl,-rpath," + PKG], check=True)


def test_sam_mates_cpp_compiles_and_the_host_mirror_holds():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 77), r.stdout + r.stderr
    assert "FAILED" not in r.stdout


@pytest.mark.gpu
def test_sam_mates_cpp_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
