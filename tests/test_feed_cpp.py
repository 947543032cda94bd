"""tests/cpp/test_feed_host.cpp: the host-only half of a feed (fmgpu_feed_host.h: planner, stagers, nibble packer, scatter, workers) against naive loops, as a
stand-alone program built with the address and undefined-behaviour sanitizers.  Nothing is loaded into python and nothing is preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_feed_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_feed_host")


def test_feed_host_code_under_the_sanitizers():
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-pthread", SRC, "-o", EXE], check=True)      # (the runtimes linked in: the program needs nothing from its environment)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
