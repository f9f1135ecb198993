"""granne_amd/csrc/combiner.h on the CPU: the layer that lets concurrent host calls share a search launch is plain
C++17 (mutex, condition variable, a launch step passed in), so its protocol is checked here without a GPU --
tests/cpp/test_combiner.cpp drives it with a launch step that echoes every request's tag into its outputs:
exactly-once delivery (32 threads x 2,000 requests of mixed keys and nq), a failed launch returning every member through
the direct path, leadership passing on with requests still queued, the cap, no waiting when idle, and a wall-clock guard
of the program's own. Under ThreadSanitizer where the machine has it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_combiner.cpp")


def _compile(out, extra):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + extra + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe, env=None):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout, out.stderr)
    return out


def test_combiner_protocol(tmp_path):
    exe = str(tmp_path / "test_combiner")
    c = _compile(exe, [])
    assert c.returncode == 0, c.stderr
    out = _run(exe)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")


def test_combiner_protocol_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "test_combiner_tsan")
    c = _compile(exe, ["-fsanitize=thread"])
    if c.returncode != 0:
        pytest.skip("g++ cannot link -fsanitize=thread here (no libtsan): the protocol ran in a plain build only "
                    "(test_combiner_protocol)")
    env = dict(os.environ)
    env["TSAN_OPTIONS"] = "halt_on_error=1 exitcode=66 " + env.get("TSAN_OPTIONS", "")
    out = _run(exe, env)
    if out.returncode != 0 and "ThreadSanitizer" in out.stderr and "WARNING: ThreadSanitizer" not in out.stderr:
        # the runtime itself could not start (an address-space layout it does not know): nothing was checked
        pytest.skip("ThreadSanitizer's runtime does not start on this kernel: " + out.stderr.strip().splitlines()[0])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")


NEW_OPTIONS = {"COALESCE": 13, "COALESCE_MAX": 14, "COALESCE_WAIT_US": 15, "COALESCED_LAUNCHES": 16, "COALESCED_QUERIES": 17}


def test_coalesce_option_ids_agree_in_every_binding():
    """include/granne_hip.h, granne_amd/_lib.py and rust/granne-hip/src/gpu.rs name the five options with the same ids,
    continuing the enum at 13; the two limits agree with combiner.h; the C++ and Rust wrappers reach the option."""
    from granne_amd import _lib
    header = open(os.path.join(ROOT, "include", "granne_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "granne-hip", "src", "gpu.rs")).read()
    for name, want in NEW_OPTIONS.items():
        h = re.search(r"\bGRANNE_HIP_OPT_%s\s*=\s*(\d+)" % name, header)
        r = re.search(r"pub const GRANNE_HIP_OPT_%s: c_int = (\d+);" % name, rust)
        assert h and int(h.group(1)) == want, name
        assert r and int(r.group(1)) == want, name
        assert getattr(_lib, "OPT_" + name) == want, name
    combiner = open(os.path.join(ROOT, "granne_amd", "csrc", "combiner.h")).read()
    for macro, const, py in (("GRANNE_HIP_COALESCE_CALL_MAX", "CALL_MAX", _lib.COALESCE_CALL_MAX),
                             ("GRANNE_HIP_COALESCE_MAX", "CAP_MAX", _lib.COALESCE_MAX)):
        h = int(re.search(r"#define %s (\d+)" % macro, header).group(1))
        c = int(re.search(r"constexpr uint32_t %s = (\d+);" % const, combiner).group(1))
        assert h == c == py, macro
    depth = int(re.search(r"constexpr uint32_t DEPTH = (\d+);", combiner).group(1))
    assert 2 <= depth <= int(re.search(r"#define GRANNE_HIP_SEARCH_DEPTH (\d+)", header).group(1))
    assert "#include <hip" not in combiner and "hipStream" not in combiner  # no HIP in the combiner
    assert "pub fn set_coalesce(" in rust
    assert "void set_coalesce(" in open(os.path.join(ROOT, "include", "granne.hpp")).read()
    assert int(re.search(r"#define GRANNE_HIP_ABI_VERSION (\d+)", header).group(1)) == 3  # options are additive
