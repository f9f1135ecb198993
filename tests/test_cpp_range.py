"""include/granne.hpp: Granne::exact_range and Granne::search_range (tests/cpp/test_range_api.cpp). Compiles everywhere (g++, host
only); the program runs on the GPU."""
import os
import subprocess

import pytest

from granne_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_range_api.cpp")


def compile_program(out):
    build.build_library()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-L", build.LIB_DIR,
           "-lgranne_hip", "-Wl,-rpath," + build.LIB_DIR, "-Wl,--allow-shlib-undefined", "-o", out]
    subprocess.check_call(cmd)


def test_cpp_range_mirror_compiles(tmp_path):
    compile_program(str(tmp_path / "test_range_api"))


@pytest.mark.gpu
def test_range_search_through_the_cpp_mirror(tmp_path):
    exe = str(tmp_path / "test_range_api")
    compile_program(exe)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")
