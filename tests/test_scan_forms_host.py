"""The literals that the exact-scan tests assert against GRANNE_HIP_OPT_LAST_SCAN (tests/test_gpu_bruteforce.py,
tests/value_edges.py SCAN_RAN, tests/test_gpu_scan_forms.py), held on the CPU to the host restatement of
granne_hip_brute_force_device's launch rule (tests/scan_forms.py scan_rule) -- and that restatement to the rule's source."""
import os
import re

import pytest

from tests import scan_forms as sf
from tests import value_edges as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_restated_rule_reads_like_the_source():
    """plan_scan's rows and the priming condition, as text: a change of either shows up here before any GPU run."""
    hip = open(os.path.join(ROOT, "granne_amd", "csrc", "granne_hip.hip")).read()
    plan = hip[hip.index("static ScanPlan plan_scan("):hip.index("// the scan's scratch:")]
    assert len(re.findall(r"GRANNE_HIP_SCAN_[A-Z0-9_]+, bf_", plan)) == len(sf.FORMS) == 10
    for form in sf.FORMS:
        assert "GRANNE_HIP_SCAN_%s," % form in plan, form
    assert "* 64u < 256u) P.max_ranges = 128;" in plan and "uint64_t max_ranges = 64;" in hip
    scan = hip[hip.index('extern "C" int granne_hip_brute_force_device('):hip.index("// host convenience over the scan")]
    assert "const bool primed = G >= 32 && Gs >= kk;" in scan and "if (primed) {" in scan
    assert "k + BF_EXTRA < BF_KMAX ? k + BF_EXTRA : BF_KMAX" in scan
    bf = open(os.path.join(ROOT, "granne_amd", "csrc", "brute_force.h")).read()
    assert "BF_EXTRA = 6;" in bf and "BF_KMAX = 16;" in bf and "BF_RING_ROWS = 128;" in bf and "BF_RING_QT = 512," in bf


@pytest.mark.parametrize("tile,ranges,at_kk16", [(32, 64, 30_721), (64, 64, 61_441), (128, 64, 122_881), (128, 128, 245_761)])
def test_fewest_rows_that_prime(tile, ranges, at_kk16):
    form = {32: "B16_16_1", 64: "B16_13_2", 128: "RING"}[tile]
    nq = 64 if ranges == 128 or form != "RING" else 1537
    sizes = sf.boundary_sizes(tile, ranges)
    assert sizes[-1] == at_kk16
    for i, n in enumerate(sizes):
        for k in range(1, 17):
            r = sf.scan_rule(form, n, nq, k)
            assert r["ranges"] == ranges and r["prime_ranges"] == sf.BOUNDARY_GS[i]
            assert r["primed"] == (sf.BOUNDARY_GS[i] >= min(k + 6, 16))
    assert not sf.scan_rule(form, at_kk16 - 1, nq, 16)["primed"]


def test_value_edge_inputs_run_what_their_table_says():
    assert sorted(ve.SCAN_RAN) == sorted(ve.SCAN_INPUTS)
    for name, (_kind, _dim, n, nq, _seed) in ve.SCAN_INPUTS.items():
        form, ranges, primed_ks = ve.SCAN_RAN[name]
        for k in ve.SCAN_KS:
            r = sf.scan_rule(form, n, nq, k)
            assert (r["ranges"], r["primed"]) == (ranges, k in primed_ks), (name, k, r)
        if name.endswith("primed"):
            assert primed_ks == ve.SCAN_KS


def test_brute_force_cases_run_what_their_tables_say():
    from tests import test_gpu_bruteforce as tb
    for (int8, dim, n), (form, ranges) in tb.UNPRIMED_RAN.items():
        for k in (1, 10, 16):
            r = sf.scan_rule(form, n, 70, k)
            assert (r["ranges"], r["primed"]) == (ranges, False), (dim, n, k, r)
    marks = [m for m in tb.test_primed_scan_with_the_shared_threshold_matches_the_scalar_scan.pytestmark if m.name == "parametrize"]
    cases = marks[0].args[1]
    assert sorted((c[0], c[1], c[2]) for c in cases) == sorted(tb.PRIMED_RAN)
    for int8, dim, n, nq in cases:
        form, ranges = tb.PRIMED_RAN[int8, dim, n]
        for k in (1, 10, 16):
            r = sf.scan_rule(form, n, nq, k)
            assert (r["ranges"], r["primed"]) == (ranges, True), (dim, n, k, r)
