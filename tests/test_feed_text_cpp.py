"""tests/cpp/test_feed_text.cpp: fmc::Feed::mapText of include/fmc_gpu.hpp (fmgpu_feed_map_text) against fmc::map(parseQueries(...)) on one FASTA and one FASTQ text;
compiled everywhere, run on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fmindex-collection_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_feed_text")


def _build():
    if not os.path.exists(os.path.join(PKG, "libfmgpu.so")):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_feed_text.cpp"), "-o", EXE,
                    "-L" + PKG, "-lfmgpu", "-Wl,-rpath," + PKG], check=True)


def test_feed_text_cpp_compiles():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 77), r.stdout + r.stderr


@pytest.mark.gpu
def test_feed_text_cpp_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
