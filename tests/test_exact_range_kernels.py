"""The range scan's kernels (granne_amd/csrc/exact_range.h) compiled alone for gfx950 (no GPU needed), and their metadata
read, by the method of tests/test_exact_topk_kernels.py: the register-resident forms of er_scan_kernel -- a group's row of
up to eight 128-byte blocks held in registers across the query loop, for each of the three sources, f32 and int8 -- use no
private segment, spill no register and stay within 128 VGPRs; the memory forms, the rank kernel and the scatter kernel
are kernels of the code object too; the header adds no second kernel whose name contains et_rank_kernel."""
import os
import shutil
import subprocess

import pytest

from tests.test_exact_topk_kernels import HIPCC, ROOT, _kernels

BLOCKS = (1, 2, 4, 8)
SOURCES = ("ET_ALL", "ET_LIST", "ET_BITS")
TU = '#include "exact_range.h"\nnamespace granne_hip {\n' + "".join(
    "template __global__ void er_scan_kernel<%s, %d, %s>(const ErParams);\n" % (i8, nblk, src)
    for src in SOURCES for i8 in ("false", "true") for nblk in BLOCKS + (0,)) + "}\n"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("exact_range_kernels")
    src, out = d / "exact_range.hip", d / "exact_range.s"
    src.write_text(TU)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-DGRANNE_HIP_USE_DPP=1",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "granne_amd", "csrc"),
                           "--cuda-device-only", "-S", "-Wno-unused-command-line-argument", str(src), "-o", str(out)])
    return _kernels(out.read_text())


def _scan_name(i8, nblk, src):
    return "_ZN10granne_hip14er_scan_kernelILb%dELi%dELNS_5EtSrcE%dEEEvNS_8ErParamsE" % (i8, nblk, src)


@pytest.mark.parametrize("src", [0, 1, 2], ids=["all", "list", "bits"])
def test_resident_scan_forms_keep_their_row_in_registers(kernels, src):
    for i8 in (0, 1):
        for nblk in BLOCKS:
            name = _scan_name(i8, nblk, src)
            assert name in kernels, (name, sorted(kernels))
            k = kernels[name]
            print("%s, int8 %d, %d blocks: %s VGPRs, private segment %s, spills %s" %
                  (SOURCES[src], i8, nblk, k["vgpr_count"], k["private_segment_fixed_size"], k["vgpr_spill_count"]))
            assert int(k["private_segment_fixed_size"]) == 0, k
            assert int(k["vgpr_spill_count"]) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, k
            assert int(k["vgpr_count"]) <= 128, k


def test_every_kernel_of_the_range_scan_is_in_the_code_object(kernels):
    for src in (0, 1, 2):
        for i8 in (0, 1):
            assert _scan_name(i8, 0, src) in kernels  # the memory forms
    assert len([n for n in kernels if "er_scan_kernel" in n]) == 3 * 2 * 5
    rank = [n for n in kernels if "er_rank_kernel" in n]
    assert len(rank) == 1, sorted(kernels)
    assert int(kernels[rank[0]]["group_segment_fixed_size"]) == 4096 * 8  # the ranked keys: 32 KB of LDS
    assert int(kernels[rank[0]]["private_segment_fixed_size"]) == 0
    assert len([n for n in kernels if "er_scatter_kernel" in n]) == 1
    assert len([n for n in kernels if "et_rank_kernel" in n]) == 1  # exact_topk.h's own, emitted by every unit that includes it
