"""The kernels of the exact scan under an id bitmap (granne_amd/csrc/exact_topk_filtered.h) compiled alone for gfx950 (no
GPU needed), and their metadata read: the register-resident forms of both scans -- the list form and the bit-tested form,
1, 2, 4 and 8 blocks of 128 bytes, f32 and int8, each of the three passes -- use no private segment, spill no register and
stay within 128 VGPRs, like exact_topk's own (tests/test_exact_topk_kernels.py); the memory forms, the four selection
kernels and the three compaction kernels (the scatter for u32 and u64 ids) are kernels of the code object too."""
import os
import shutil
import subprocess

import pytest

from tests.test_exact_topk_kernels import HIPCC, ROOT, _kernels

BLOCKS = (1, 2, 4, 8)
TU = '#include "exact_topk_filtered.h"\nnamespace granne_hip {\n' + "".join(
    "template __global__ void etf_scan_kernel<%s, %d, %d, %s>(const EtfParams);\n" % (i8, nblk, p, lst)
    for lst in ("true", "false") for i8 in ("false", "true") for nblk in BLOCKS + (0,) for p in (1, 2, 3)) + "".join(
    "template __global__ void etf_select_kernel<%d, %s>(const uint32_t*, uint32_t, uint64_t, uint64_t, const uint64_t*, uint32_t*, EtSel*, "
    "uint32_t, uint32_t*);\n" % (level, lst) for level in (1, 2) for lst in ("true", "false")) + """
template __global__ void fl_scatter_kernel<uint32_t>(const uint32_t*, uint64_t, const uint32_t*, uint32_t*);
template __global__ void fl_scatter_kernel<uint64_t>(const uint32_t*, uint64_t, const uint32_t*, uint64_t*);
}
"""


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("exact_topk_filtered_kernels")
    src, out = d / "exact_topk_filtered.hip", d / "exact_topk_filtered.s"
    src.write_text(TU)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-DGRANNE_HIP_USE_DPP=1",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "granne_amd", "csrc"),
                           "--cuda-device-only", "-S", "-Wno-unused-command-line-argument", str(src), "-o", str(out)])
    return _kernels(out.read_text())


def _scan_name(i8, nblk, p, lst):
    return "_ZN10granne_hip15etf_scan_kernelILb%dELi%dELi%dELb%dEEEvNS_9EtfParamsE" % (i8, nblk, p, lst)


@pytest.mark.parametrize("lst", [1, 0], ids=["list", "bits"])
def test_resident_scan_forms_keep_their_row_in_registers(kernels, lst):
    for i8 in (0, 1):
        for nblk in BLOCKS:
            for p in (1, 2, 3):
                name = _scan_name(i8, nblk, p, lst)
                assert name in kernels, (name, sorted(kernels))
                k = kernels[name]
                print("list %d, int8 %d, %d blocks, pass %d: %s VGPRs, private segment %s, spills %s" %
                      (lst, i8, nblk, p, k["vgpr_count"], k["private_segment_fixed_size"], k["vgpr_spill_count"]))
                assert int(k["private_segment_fixed_size"]) == 0, k
                assert int(k["vgpr_spill_count"]) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, k
                assert int(k["vgpr_count"]) <= 128, k


def test_every_kernel_is_in_the_code_object(kernels):
    for lst in (0, 1):
        for i8 in (0, 1):
            for p in (1, 2, 3):
                assert _scan_name(i8, 0, p, lst) in kernels
    assert len([n for n in kernels if "etf_scan_kernel" in n]) == 2 * 2 * 5 * 3
    select = [n for n in kernels if "etf_select_kernel" in n]
    assert len(select) == 4, sorted(kernels)
    for n in select:
        assert int(kernels[n]["private_segment_fixed_size"]) == 0
    assert len([n for n in kernels if "fl_count_kernel" in n]) == 1
    assert len([n for n in kernels if "fl_scan_kernel" in n]) == 1
    scatter = [n for n in kernels if "fl_scatter_kernel" in n]
    assert len(scatter) == 2, sorted(kernels)  # u32 ids for the scan, u64 for granne_hip_filter_to_ids_device
    for n in scatter:
        assert int(kernels[n]["private_segment_fixed_size"]) == 0, kernels[n]
    assert [n for n in kernels if "et_rank_kernel" in n]  # exact_topk's own, unchanged, ranks the candidates
