"""tests/cpp/test_parse.cpp: fmc::parseQueries, fmc::SymbolTable and fmc::ParsedQueries (include/fmc_gpu.hpp) — the ready-made tables on the host; on a GPU FASTA
and FASTQ parsed on the device, the parsed batch through the searches, the packer, fmc::map and a feed, and the thrown text error."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fmindex-collection_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_parse")


def _build():
    if not os.path.exists(os.path.join(PKG, "libfmgpu.so")):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_parse.cpp"), "-o", EXE,
                    "-L" + PKG, "-lfmgpu", "-Wl,-rpath," + PKG], check=True)


def test_parse_cpp_compiles_and_has_its_tables():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 77), r.stdout + r.stderr


@pytest.mark.gpu
def test_parse_cpp_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    assert "text error in line 7" in r.stdout
