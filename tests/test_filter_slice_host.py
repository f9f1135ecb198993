"""The bitmap slice's word rule on the host (tests/cpp/filter_slice_host.cpp): a stand-alone program that includes
granne_amd/csrc/filter_slice.h -- the text the slice kernel compiles -- and slices exact-size heap bitmaps. It checks the
values bit by bit, once in a plain build and once under AddressSanitizer and UBSan, which is what shows that no word past
the bitmap's last is ever read. No GPU, no library: the program is run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "filter_slice_host.cpp")


def _compile(out, extra):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "granne_amd", "csrc")] + extra + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    return out


def test_slice_word_rule(tmp_path):
    exe = str(tmp_path / "filter_slice_host")
    c = _compile(exe, [])
    assert c.returncode == 0, c.stderr
    out = _run(exe)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")


def test_slice_word_rule_under_address_sanitizer(tmp_path):
    exe = str(tmp_path / "filter_slice_host_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtimes linked statically where they exist as archives: the program then starts whatever else the
    # environment loads first (as tests/test_dev_mem_host.py)
    c = _compile(exe, san + ["-static-libasan", "-static-libubsan"])
    if c.returncode != 0:
        c = _compile(exe, san)
    if c.returncode != 0:
        pytest.skip("g++ cannot link -fsanitize=address,undefined here (no libasan / libubsan): the rule ran in a plain build "
                    "only (test_slice_word_rule)")
    out = _run(exe)
    if out.returncode != 0 and "ASan runtime does not come first" in out.stderr:
        pytest.skip("AddressSanitizer's shared runtime does not start in this environment: " + out.stderr.strip().splitlines()[0])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")


def test_slice_header_includes_nothing_from_hip():
    text = open(os.path.join(ROOT, "granne_amd", "csrc", "filter_slice.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
