"""Row sketches (GRANNE_HIP_OPT_SKETCH, walk_fast.h FastWalker::sketch_rejects): the device table is the host model's
bytes (tests/test_sketch_bound.py) after create, after a load from files and after reorder; searches with the sketch on
and off return the same ids, distance bits, counts and counters (a rejected neighbor is one the filter would have
dropped), and the oracle's; an index made without a sketch searches as before."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import random_floats  # noqa: E402
from tests.scan_forms import structured_rows as _data  # noqa: E402
from tests.test_sketch_bound import row_sketch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


def _index(ga, oracle, kind, seed, n=6000):
    rng = np.random.default_rng(seed)
    el = oracle.normalize_f32(_data(kind, rng, n))
    q = oracle.normalize_f32(_data(kind, rng, 300))
    oix = oracle.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
    return el, q, oix, ga.Granne("angular", el, oix.layers)


def test_table_is_the_host_model(ga, oracle, tmp_path):
    from granne_amd import _lib
    el, q, oix, gix = _index(ga, oracle, "uniform", 1, n=3000)
    assert gix.get_option(_lib.OPT_SKETCH) == 1
    tab = gix.get_sketch()
    assert tab is not None and tab.tobytes() == row_sketch(el).tobytes()
    # loaded from files: made again, the same bytes
    gix.save_index(str(tmp_path / "i.granne"))
    gix.save_elements(str(tmp_path / "e.bin"))
    g2 = ga.Granne.from_files(str(tmp_path / "i.granne"), "angular", str(tmp_path / "e.bin"))
    assert g2.get_sketch().tobytes() == tab.tobytes()
    g2.close()
    # after reorder the rows moved: so did their lines
    order = gix.reorder().astype(np.int64)
    assert gix.get_sketch().tobytes() == row_sketch(el[order]).tobytes()
    # rows with a component that is not finite, zero rows, subnormal rows: the device makes the model's bytes too
    odd = el[:64].copy()
    odd[0, 3] = np.inf
    odd[1, 5] = np.nan
    odd[2] = 0.0
    odd[3] = np.float32(1e-41)
    odd[4, :] = -0.0
    g3 = ga.Granne("angular", odd, [np.full((64, 30), 0xFFFFFFFF, np.uint32)])
    assert g3.get_sketch().tobytes() == row_sketch(odd).tobytes()
    g3.close()
    gix.close()


@pytest.mark.parametrize("kind", ["uniform", "latent", "mixture", "duplicates", "grid"])
def test_on_off_identical(ga, oracle, kind):
    """Every launch skips revisits here (SEEN_MIN 0), the walks the sketch serves: on and off give the same bits."""
    if os.environ.get("GRANNE_HIP_SEEN_MIN") is not None or os.environ.get("GRANNE_HIP_SKETCH") is not None:
        pytest.skip("an experiment knob overrides the options this test switches")
    from granne_amd import _lib
    el, q, oix, gix = _index(ga, oracle, kind, {"uniform": 11, "latent": 12, "mixture": 13, "duplicates": 14, "grid": 15}[kind])
    gix.set_option(_lib.OPT_SEEN_MIN, 0)
    for ef in (1, 10, 50, 200, 1024):
        gix.set_option(_lib.OPT_SKETCH, 0)
        assert gix.get_option(_lib.OPT_SKETCH) == 0
        r0 = gix.search_batch(q, ef, 10, stats=True)
        gix.set_option(_lib.OPT_SKETCH, 1)
        assert gix.get_option(_lib.OPT_SKETCH) == 1
        r1 = gix.search_batch(q, ef, 10, stats=True)
        for a, b in zip(r0, r1):
            assert a.tobytes() == b.tobytes(), (kind, ef)
        oi, od, oc, octr = oix.search_batch(q, ef, 10)
        ids, ds, cnt, st = r1
        assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes(), (kind, ef)
        assert (st[:, 1:] == octr[:, 1:]).all()
    gix.close()


def test_default_launch_matches_oracle(ga, oracle):
    """The default options, a launch of many walks (the bench's shape: revisits skipped, sketch on)."""
    el, q, oix, gix = _index(ga, oracle, "uniform", 21)
    rng = np.random.default_rng(22)
    q = oracle.normalize_f32(random_floats(rng, 2304, 100))
    ids, ds, cnt, st = gix.search_batch(q, 50, 10, stats=True)
    oi, od, oc, octr = oix.search_batch(q, 50, 10)
    assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes()
    assert (st[:, 1:] == octr[:, 1:]).all()
    gix.close()


_NO_SKETCH = r"""
import numpy as np, granne_amd
from granne_amd import _lib
from oracle import oracle as orc
orc.build()
rng = np.random.default_rng(31)
el = orc.normalize_f32(rng.random((4000, 100), dtype=np.float32) - 0.5)
q = orc.normalize_f32(rng.random((2304, 100), dtype=np.float32) - 0.5)
oix = orc.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
gix = granne_amd.Granne("angular", el, oix.layers)
assert gix.get_sketch() is None and gix.get_option(_lib.OPT_SKETCH) == 0
ids, ds, cnt, st = gix.search_batch(q, 50, 10, stats=True)
oi, od, oc, octr = oix.search_batch(q, 50, 10)
assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes()
print("no-sketch ok")
"""


def test_index_without_sketch(oracle):
    """GRANNE_HIP_SKETCH=0 (the path of an index that had no room for its sketch): no table, the same results."""
    env = dict(os.environ, GRANNE_HIP_SKETCH="0")
    r = subprocess.run([sys.executable, "-c", _NO_SKETCH], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "no-sketch ok" in r.stdout
