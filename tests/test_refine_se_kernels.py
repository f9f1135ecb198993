"""The container re-rank kernel (granne_amd/csrc/refine_se_kernel.h) compiled alone for gfx950 (no GPU needed), and its
metadata read: every instantiation -- the four resident forms, which keep a candidate's whole term sum in registers, and
the two-pass form for longer rows -- uses no private segment and spills no register (a sum that went to scratch would be
written and read back per term, the traffic the register layout exists to avoid), within 128 VGPRs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FORMS = (0, 1, 3, 4, 8)  # refine_se_kernel<NBF>: full blocks held in registers; 0 = two passes (refine_se_resident_blocks)
TU = '#include "refine_se_kernel.h"\nnamespace granne_hip {\n' + "".join(
    "template __global__ void refine_se_kernel<%d>(const RefineSeParams);\n" % nbf for nbf in FORMS) + "}\n"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("refine_se_kernels")
    src, out = d / "refine_se.hip", d / "refine_se.s"
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
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", entry))
        found[f["name"]] = f
    return found


def test_every_form_keeps_its_sum_in_registers(asm):
    kernels = _kernels(asm)
    for nbf in FORMS:
        name = "_ZN10granne_hip16refine_se_kernelILi%dEEEvNS_14RefineSeParamsE" % nbf
        assert name in kernels, (name, sorted(kernels))
        k = kernels[name]
        print("%d resident blocks: %s VGPRs, %s SGPRs, private segment %s, spills %s / %s" %
              (nbf, k["vgpr_count"], k["sgpr_count"], k["private_segment_fixed_size"], k["vgpr_spill_count"],
               k.get("sgpr_spill_count", 0)))
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_spill_count"]) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, k
        assert int(k["vgpr_count"]) <= 128, k  # four waves per SIMD at the least


def test_the_dispatch_names_only_compiled_forms():
    """refine_se_resident_blocks (the header's rule) and the launch switch (refine_se_host.h) know the same forms."""
    header = open(os.path.join(ROOT, "granne_amd", "csrc", "refine_se_kernel.h")).read()
    host = open(os.path.join(ROOT, "granne_amd", "csrc", "refine_se_host.h")).read()
    rule = header[header.index("inline int refine_se_resident_blocks"):]
    rule = rule[:rule.index("}")]
    named = sorted(set(int(v) for v in re.findall(r"\? (\d+)", rule)) | {int(re.search(r": (\d+);", rule).group(1))})
    assert named == sorted(FORMS)
    launched = sorted(int(v) for v in re.findall(r"refine_se_kernel<(\d+)>", host))
    assert launched == sorted(FORMS)
