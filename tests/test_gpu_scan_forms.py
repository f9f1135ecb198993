"""Every kernel form of the exact scan (granne_amd/csrc/brute_force.h, plan_scan in granne_hip.hip), unprimed and with the
priming pass and the threshold its ranges share, held to the contract of brute_force.h's header (tests/scan_forms.py
states it and holds the checks): no cap on near-tied ranks is needed, so the rows may be clustered or tied exactly.

Every scan asserts what GRANNE_HIP_OPT_LAST_SCAN reports -- form, ranges, priming sub-ranges, primed -- against a
literal, runs twice, and prints the largest |d - true d| and the share of ids that are the oracle's. The sizes are the
smallest that reach a path: ranges * tile * (kk - 1) + 1 rows are the fewest whose first range holds kk = min(k + 6, 16)
tiles, which is when the priming pass runs."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

from tests import scan_forms as sf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _default_forms():
    if os.environ.get("GRANNE_HIP_BF_B16") is not None or os.environ.get("GRANNE_HIP_BF_RING") is not None:
        pytest.skip("an experiment knob selects other scan kernels than the ones this test names")


# case -> (form, int8, dim, nq, ranges, the six sizes: one tile below and at the thresholds of kk = 7, 15, 16)
T32 = (12_257, 12_289, 28_641, 28_673, 30_689, 30_721)
T64 = (24_513, 24_577, 57_281, 57_345, 61_377, 61_441)
T128 = (49_025, 49_153, 114_561, 114_689, 122_753, 122_881)
T128_WIDE = (98_177, 98_305, 229_249, 229_377, 245_633, 245_761)
BOUNDARY = {
    "b16_7_4_100": ("B16_7_4", False, 100, 64, 64, T128),
    "b16_13_2_200": ("B16_13_2", False, 200, 64, 64, T64),
    "b16_16_1_209": ("B16_16_1", False, 209, 64, 64, T32),
    "b16_16_1_256": ("B16_16_1", False, 256, 64, 64, T32),
    "b16_chunked_300": ("B16_CHUNKED", False, 300, 64, 64, T64),
    "b16_chunked_384": ("B16_CHUNKED", False, 384, 64, 64, T64),
    "b16_chunked_768": ("B16_CHUNKED", False, 768, 64, 64, T64),
    "i8_64": ("I8", True, 64, 64, 64, T128),
    "i8_chunked_256": ("I8_CHUNKED", True, 256, 64, 64, T128),
    "i8_chunked_512": ("I8_CHUNKED", True, 512, 64, 64, T128),
    "ring_four_query_tiles": ("RING", True, 128, 1537, 64, T128),
    "ring_128_ranges": ("RING", True, 100, 64, 128, T128_WIDE),
}


@pytest.mark.parametrize("size", range(6))
@pytest.mark.parametrize("case", sorted(BOUNDARY))
def test_forms_at_the_priming_boundary(ga, oracle, case, size):
    """k = 1, 9, 10, 13, 16 at each size: sizes 0 / 2 / 4 hold kk - 1 = 6 / 14 / 15 sub-ranges (unprimed at the k whose
    kk that is), sizes 1 / 3 / 5 hold 7 / 15 / 16 (primed at it)."""
    _default_forms()
    form, int8, dim, nq, ranges, sizes = BOUNDARY[case]
    sf.run_boundary(ga, oracle, form, int8, dim, nq, ranges, sizes, 100 + sorted(BOUNDARY).index(case), which=(size,))


# one unprimed case per form: (form, int8, dim)
UNPRIMED = {"b16_7_4": ("B16_7_4", False, 100), "b16_13_2": ("B16_13_2", False, 200), "b16_16_1": ("B16_16_1", False, 256),
            "b16_chunked": ("B16_CHUNKED", False, 300), "i8": ("I8", True, 64), "i8_chunked": ("I8_CHUNKED", True, 256),
            "ring": ("RING", True, 128)}


@pytest.mark.parametrize("part", ["tiles", "every_k", "nq"])
@pytest.mark.parametrize("case", sorted(UNPRIMED))
def test_forms_below_the_thresholds(ga, oracle, case, part):
    """31 / 32 / 64 / 65 tiles (fewer than 32 ranges, 32, the cap, past it: the ring's two-step merge of 65 lists); every k
    from 1 to 16; 1 .. 257 queries (the ring: .. 513 and 1,537) at 3,001 rows."""
    _default_forms()
    form, int8, dim = UNPRIMED[case]
    sf.run_unprimed(ga, oracle, form, int8, dim, 300 + 10 * sorted(UNPRIMED).index(case), part)


@pytest.mark.parametrize("primed", [False, True])
@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("kind", ["latent", "mixture", "duplicates", "grid"])
def test_structured_rows(ga, oracle, kind, int8, primed):
    """The rows the walker modules draw from, 100-d, as f32 (bf_b16_kernel<7, 4>) and quantised (the ring, 128 ranges):
    6,000 rows and the smallest size that primes at every k. 64 queries from the generator and 16 member rows, whose nearest
    must be themselves (or a copy). duplicates and grid hold exact score ties, which a range keeps or drops with the moment
    the shared threshold reaches it: both runs are held to the contract, the ids need not repeat."""
    _default_forms()
    n = 6000 if not primed else 245_761 if int8 else 122_881
    form = "RING" if int8 else "B16_7_4"
    expect = (form, 47, False, 1) if not primed else (form, 128 if int8 else 64, True, 16)
    seed = 500 + 4 * ["latent", "mixture", "duplicates", "grid"].index(kind) + 2 * int8 + primed
    w = sf.structured_world(oracle, kind, int8, n, seed)
    ix = ga.Granne("angular_int" if int8 else "angular", w.el, [])
    for k in (1, 10, 16):
        w.scan(ix, k, expect, "%s_%s" % (kind, "i8" if int8 else "f32"), ids_repeat=kind in ("latent", "mixture"))
    ix.close()


@pytest.mark.parametrize("knob", ["GRANNE_HIP_BF_B16", "GRANNE_HIP_BF_RING"])
def test_forms_behind_a_knob(oracle, knob):
    """GRANNE_HIP_BF_B16=0 (bf_f32_kernel<52, 4>, <100, 2>, <128, 1>; 300 dims stay chunked) and GRANNE_HIP_BF_RING=0
    (bf_i8_kernel on 128-byte rows), each in one fresh process: scan_forms.knob_main holds them to the same contract and
    the same reported form."""
    if os.environ.get("GRANNE_HIP_BF_B16") is not None or os.environ.get("GRANNE_HIP_BF_RING") is not None:
        pytest.skip("the knob is set in the environment already")
    env = dict(os.environ, **{knob: "0"})
    r = subprocess.run([sys.executable, "-c", "from tests import scan_forms; scan_forms.knob_main(%r)" % knob], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "scan knob ok" in r.stdout
