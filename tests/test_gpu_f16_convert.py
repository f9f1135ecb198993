"""The conversions of "angular_f16" elements on the GPU (granne_hip_f32_to_f16*, granne_hip_f16_to_f32*): f32 -> halves
has the bytes of numpy's astype(float16) (round to nearest, ties to even); halves -> f32 is exact and, normalised, has the
bytes of oracle.normalize_f32 over the widened rows -- the rows an F16 index stands for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import random_floats  # noqa: E402

DIMS = [1, 3, 31, 32, 33, 64, 100, 257]


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def test_f32_to_f16_has_numpys_bytes_on_random_rows(ga):
    rng = np.random.default_rng(7)
    for n, dim in ((513, 100), (64, 257), (1000, 3)):
        rows = random_floats(rng, n, dim) * np.float32(4.0)
        assert ga.to_f16(rows).tobytes() == rows.astype(np.float16).tobytes()


def test_f32_to_f16_edge_values(ga):
    sub_max = np.float32(2.0 ** -14 - 2.0 ** -24)  # the largest f16 subnormal
    sub_min = np.float32(2.0 ** -24)               # the smallest
    row = np.array([0.0, -0.0, 3e-6, -3e-6, sub_max, -sub_max, sub_min, 65504.0, -65504.0,
                    2.0 ** -25, 2.0 ** -25 * 0.99, -(2.0 ** -26), 1e-9,      # at and below half the smallest subnormal: 0
                    2.0 ** -25 * 1.01,                                       # just above it: the smallest subnormal
                    1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11),  # exact ties: to even
                    1.0 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -14, 2.0 ** -14 + 2.0 ** -25,  # (the last: a tie at the f16 normal boundary)
                    65519.0, 0.1, -1.0 / 3.0, 1.0], np.float32)[None]
    want = row.astype(np.float16)
    got = ga.to_f16(row)
    assert got.tobytes() == want.tobytes(), (got.view(np.uint16), want.view(np.uint16))
    assert got[0, 0].tobytes() == b"\x00\x00" and got[0, 1].tobytes() == b"\x00\x80"  # +0, -0
    assert got[0, 9] == 0 and got[0, 10] == 0 and got[0, 11] == 0 and got[0, 12] == 0
    assert got[0, 14] == np.float16(1.0) and got[0, 15].view(np.uint16) == 0x3C02


@pytest.mark.parametrize("dim", DIMS)
def test_f16_to_f32_normalised_has_the_oracles_bytes(ga, oracle, dim):
    rng = np.random.default_rng(100 + dim)
    rows16 = random_floats(rng, 300, dim).astype(np.float16)
    rows16[5] = 0  # an all-zero row stays zero
    rows16[6] = (rng.integers(1, 1024, dim).astype(np.uint16)).view(np.float16)  # a row of f16 subnormals
    rows16[7] = np.float16(65504.0)
    wide = rows16.astype(np.float32)
    assert ga.from_f16(rows16, normalized=False).tobytes() == wide.tobytes()
    want = oracle.normalize_f32(wide)
    got = ga.from_f16(rows16)
    assert got.tobytes() == want.tobytes()
    assert not got[5].any()
    assert abs(float(np.dot(got[6].astype(np.float64), got[6].astype(np.float64))) - 1.0) < 1e-5


def test_unprepared_rows_are_normalised_in_f32_then_rounded(ga, oracle):
    rng = np.random.default_rng(3)
    raw = random_floats(rng, 200, 100) * np.float32(7.0)
    assert ga.to_f16(raw, prepared=False).tobytes() == oracle.normalize_f32(raw).astype(np.float16).tobytes()


def test_the_largest_dim_the_conversion_stages(ga, oracle):
    """A row is staged whole in LDS: 15,359 components is the largest (include/granne_hip.h); beyond is refused, not wrong."""
    rng = np.random.default_rng(9)
    rows16 = random_floats(rng, 2, 15359).astype(np.float16)
    assert ga.from_f16(rows16).tobytes() == oracle.normalize_f32(rows16.astype(np.float32)).tobytes()
    with pytest.raises(ga.GranneHipError) as e:
        ga.from_f16(np.zeros((2, 15360), np.float16))
    assert "dim too large" in str(e.value)
