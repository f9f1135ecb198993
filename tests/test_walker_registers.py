"""The sketched compacted f32 walkers (walk_fast.h, fast_kernel's CR) are built for as many waves per
SIMD as each list length fits WITHOUT scratch (cr_waves): a wave's allocation is 512 / waves registers rounded down
to the allocation unit of 8, and a walker that needs more spills to the private segment -- on the hot path of every
expansion. Compiles the three instantiations and the tail kernel alone for gfx950 (no GPU needed) and reads the kernels'
metadata: no private segment, VGPRs within the allocation, and the tail blocks a kernel symbol of their own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

TU = """
#include "search_kernel.h"
#include "walk_fast.h"
namespace granne_hip {
template __global__ void fast_kernel<DT_F32, 100, 1, false, 5, false, GRANNE_HIP_CR_G>(const SlowParams);
template __global__ void fast_kernel<DT_F32, 100, 2, false, 5, false, GRANNE_HIP_CR_G>(const SlowParams);
template __global__ void fast_kernel<DT_F32, 100, 4, false, 5, false, GRANNE_HIP_CR_G>(const SlowParams);
template __global__ void tail_kernel<DT_F32>(const SlowParams);
}
using namespace granne_hip;
extern "C" __device__ __attribute__((used)) const int granne_split_waves[3] = {
    fast_waves_per_simd(DT_F32, 100, 1, false, true, GRANNE_HIP_CR_G),
    fast_waves_per_simd(DT_F32, 100, 2, false, true, GRANNE_HIP_CR_G),
    fast_waves_per_simd(DT_F32, 100, 4, false, true, GRANNE_HIP_CR_G)};
"""


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("walker_registers")
    src, out = d / "split_walkers.hip", d / "split_walkers.s"
    src.write_text(TU)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-DGRANNE_HIP_USE_DPP=1",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "granne_amd", "csrc"),
                           "--cuda-device-only", "-S", "-Wno-unused-command-line-argument", str(src), "-o", str(out)])
    return out.read_text()


def _kernels(txt):
    """mangled name -> the fields of its entry in the code object's kernel metadata"""
    found = {}
    for entry in re.split(r"\n  - \.agpr_count:", txt.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0])[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\S+)", entry))
        found[f["name"]] = f
    return found


def test_split_walkers_fit_their_waves_without_scratch(asm):
    m = re.search(r"^granne_split_waves:\n((?:\s+\.long\s+\d+.*\n){3})", asm, re.M)
    assert m, "the waves-per-SIMD table of the translation unit"
    waves = [int(v) for v in re.findall(r"\.long\s+(\d+)", m.group(1))]
    kernels = _kernels(asm)
    for S, w in zip((1, 2, 4), waves):
        assert 4 <= w <= 6, (S, w)
        name = "_ZN10granne_hip11fast_kernelILi0ELi100ELi%dELb0ELi5ELb0ELi8EEEvNS_10SlowParamsE" % S
        assert name in kernels, (S, sorted(kernels))
        k = kernels[name]
        print("list slots %d: %d waves per SIMD, %s VGPRs, private segment %s" % (S, w, k["vgpr_count"], k["private_segment_fixed_size"]))
        assert int(k["private_segment_fixed_size"]) == 0, (S, k)
        assert int(k["vgpr_count"]) <= (512 // w) // 8 * 8, (S, w, k)


def test_tail_blocks_are_a_kernel_of_their_own(asm):
    kernels = _kernels(asm)
    tails = [n for n in kernels if "tail_kernel" in n]
    assert len(tails) == 1, sorted(kernels)
    assert re.search(r"^\s+\.amdhsa_kernel\s+" + re.escape(tails[0]) + r"\s*$", asm, re.M)
