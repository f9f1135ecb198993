"""The exact selection's kernels (granne_amd/csrc/exact_topk.h, with the bitmap compaction of filter.h) compiled alone for
gfx950 (no GPU needed), and their metadata read: the register-resident forms of the scan -- a group's row of up to eight
128-byte blocks held in registers across the query loop, for each of the three sources (all rows, the compacted list, the
per-query bits), f32 and int8, in each of the three passes -- use no private segment, spill no register (a row that went
to scratch would be read back per query, the traffic the form exists to avoid) and stay within 128 VGPRs; the memory
forms, the four selection kernels (two levels; all rows are served by the list rule), the three compaction kernels (the
scatter for u32 and u64 ids) and the ranking kernel are kernels of the code object too."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

BLOCKS = (1, 2, 4, 8)  # register blocks of the resident forms (et_scan_fn)
SOURCES = ("ET_ALL", "ET_LIST", "ET_BITS")  # EtSrc, in the enum's order
TU = '#include "exact_topk.h"\nnamespace granne_hip {\n' + "".join(
    "template __global__ void et_scan_kernel<%s, %d, %d, %s>(const EtParams);\n" % (i8, nblk, p, src)
    for src in SOURCES for i8 in ("false", "true") for nblk in BLOCKS + (0,) for p in (1, 2, 3)) + "".join(
    "template __global__ void et_select_kernel<%d, %s>(const uint32_t*, uint32_t, uint64_t, uint64_t, const uint64_t*, uint64_t, uint32_t*, "
    "EtSel*, uint32_t, uint32_t*);\n" % (level, src) for level in (1, 2) for src in ("ET_LIST", "ET_BITS")) + """
template __global__ void fl_scatter_kernel<uint32_t>(const uint32_t*, uint64_t, const uint32_t*, uint32_t*);
template __global__ void fl_scatter_kernel<uint64_t>(const uint32_t*, uint64_t, const uint32_t*, uint64_t*);
}
"""


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("exact_topk_kernels")
    src, out = d / "exact_topk.hip", d / "exact_topk.s"
    src.write_text(TU)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-DGRANNE_HIP_USE_DPP=1",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "granne_amd", "csrc"),
                           "--cuda-device-only", "-S", "-Wno-unused-command-line-argument", str(src), "-o", str(out)])
    return _kernels(out.read_text())


def _kernels(txt):
    """mangled name -> the fields of its entry in the code object's kernel metadata"""
    found = {}
    for entry in re.split(r"\n  - \.agpr_count:", txt.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0])[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\S+)", entry))
        found[f["name"]] = f
    return found


def _scan_name(i8, nblk, p, src):
    return "_ZN10granne_hip14et_scan_kernelILb%dELi%dELi%dELNS_5EtSrcE%dEEEvNS_8EtParamsE" % (i8, nblk, p, src)


@pytest.mark.parametrize("src", [0, 1, 2], ids=["all", "list", "bits"])
def test_resident_scan_forms_keep_their_row_in_registers(kernels, src):
    for i8 in (0, 1):
        for nblk in BLOCKS:
            for p in (1, 2, 3):
                name = _scan_name(i8, nblk, p, src)
                assert name in kernels, (name, sorted(kernels))
                k = kernels[name]
                print("%s, int8 %d, %d blocks, pass %d: %s VGPRs, private segment %s, spills %s" %
                      (SOURCES[src], i8, nblk, p, k["vgpr_count"], k["private_segment_fixed_size"], k["vgpr_spill_count"]))
                assert int(k["private_segment_fixed_size"]) == 0, k
                assert int(k["vgpr_spill_count"]) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, k
                assert int(k["vgpr_count"]) <= 128, k  # four waves per SIMD at the least


def test_every_kernel_of_the_selection_is_in_the_code_object(kernels):
    for i8 in (0, 1):
        for p in (1, 2, 3):
            assert _scan_name(i8, 0, p, 0) in kernels
    # all rows are served by the list rule's two selects (et_select_fn)
    assert len([n for n in kernels if "et_select_kernel" in n and "EtSrcE1E" in n]) == 2, sorted(kernels)
    rank = [n for n in kernels if "et_rank_kernel" in n]
    assert len(rank) == 1, sorted(kernels)
    assert int(kernels[rank[0]]["group_segment_fixed_size"]) == 4096 * 8  # the ranked keys: 32 KB of LDS
    assert int(kernels[rank[0]]["private_segment_fixed_size"]) == 0


def test_every_kernel_is_in_the_code_object(kernels):
    """the list and bits sources' kernels, the selects and the compaction (with the all-rows forms: 90 scans in all)"""
    for src in (1, 2):
        for i8 in (0, 1):
            for p in (1, 2, 3):
                assert _scan_name(i8, 0, p, src) in kernels
    assert len([n for n in kernels if "et_scan_kernel" in n and "EtSrcE0E" not in n]) == 2 * 2 * 5 * 3
    assert len([n for n in kernels if "et_scan_kernel" in n]) == 3 * 2 * 5 * 3
    select = [n for n in kernels if "et_select_kernel" in n]
    assert len(select) == 4, sorted(kernels)  # two levels x (the list rule, the bits rule)
    for n in select:
        assert int(kernels[n]["private_segment_fixed_size"]) == 0
    assert len([n for n in kernels if "fl_count_kernel" in n]) == 1
    assert len([n for n in kernels if "fl_scan_kernel" in n]) == 1
    scatter = [n for n in kernels if "fl_scatter_kernel" in n]
    assert len(scatter) == 2, sorted(kernels)  # u32 ids for the scan, u64 for granne_hip_filter_to_ids_device
    for n in scatter:
        assert int(kernels[n]["private_segment_fixed_size"]) == 0, kernels[n]
    assert len([n for n in kernels if "et_rank_kernel" in n]) == 1  # one rank kernel ranks every source's candidates
