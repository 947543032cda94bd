"""tests/cpp/align_checks.cpp: the paths of fmgpu_chains_align that return before the first device call, as a stand-alone program with its own main, built with the host
side of fmindex-collection_amd/csrc/fmgpu_align.hip under AddressSanitizer and UndefinedBehaviorSanitizer (the way the head of tests/cpp/chain_checks.cpp states).  It
runs on the CPU and needs no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fmindex-collection_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_pre_device_paths_under_a_host_sanitizer(tmp_path):
    if not os.path.exists(os.path.join(PKG, "libfmgpu.so")):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4", "-s"], check=True)
    exe = str(tmp_path / "align_checks")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(PKG, "csrc", "fmgpu_align.hip"), os.path.join(ROOT, "tests", "cpp", "align_checks.cpp"), "-o", exe, "-fsanitize=address,undefined",
                    "-L" + PKG, "-lfmgpu", "-Wl,-rpath," + PKG], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAILED" not in r.stdout and "runtime error" not in r.stderr
