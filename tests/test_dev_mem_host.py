"""granne_amd/csrc/dev_mem.h on the CPU: the two owners of HIP memory that the host layer is written with include
nothing from HIP, so tests/cpp/test_dev_mem.cpp puts counting fakes in place of hipMalloc / hipFree / hipHostMalloc /
hipHostFree and checks that every allocation is freed exactly once -- across scope exit, moves, reset, alloc onto a
non-empty owner, release, a failed allocation, reserve, and a growing vector of structs that hold owners. Once plain, once
as a stand-alone program under AddressSanitizer and UBSan where the machine has their runtimes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_dev_mem.cpp")


def _compile(out, extra):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + extra + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe, env=None):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout, out.stderr)
    return out


def test_dev_mem_owners(tmp_path):
    exe = str(tmp_path / "test_dev_mem")
    c = _compile(exe, [])
    assert c.returncode == 0, c.stderr
    out = _run(exe)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")


def test_dev_mem_owners_under_address_sanitizer(tmp_path):
    exe = str(tmp_path / "test_dev_mem_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtimes linked statically where they exist as archives: the program then starts whatever else the
    # environment loads first
    c = _compile(exe, san + ["-static-libasan", "-static-libubsan"])
    if c.returncode != 0:
        c = _compile(exe, san)
    if c.returncode != 0:
        pytest.skip("g++ cannot link -fsanitize=address,undefined here (no libasan / libubsan): the owners ran in a plain "
                    "build only (test_dev_mem_owners)")
    out = _run(exe)
    if out.returncode != 0 and "ASan runtime does not come first" in out.stderr:
        # the shared runtime refuses to start behind another preloaded library: nothing was checked
        pytest.skip("AddressSanitizer's shared runtime does not start in this environment: " + out.stderr.strip().splitlines()[0])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")


def test_dev_mem_header_includes_nothing_from_hip():
    text = open(os.path.join(ROOT, "granne_amd", "csrc", "dev_mem.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
    assert len(text.splitlines()) < 100
