"""GranneBuilder over "angular_f16" rows on the GPU: the build is the f32 build over R = normalize_f32(widen(rows16)),
so its layers equal oracle.build_index(R, ...) row for row; the index it hands out holds the halves, searches like the
oracle, and goes through the Vectors file format with 2-byte scalars."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import random_floats  # noqa: E402

CASES = [
    # n, dim, num_neighbors, max_search, reinsert, batch_max
    (1500, 28, 20, 20, False, 64),
    (2000, 100, 30, 40, True, 256),
]


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


@pytest.mark.parametrize("n,dim,nn,ms,reinsert,bmax", CASES)
def test_f16_build_equals_the_oracles_build_over_the_widened_rows(ga, oracle, tmp_path, n, dim, nn, ms, reinsert, bmax):
    from granne_amd import _lib
    rng = np.random.default_rng(n * 7 + dim)
    rows16 = oracle.normalize_f32(random_floats(rng, n, dim)).astype(np.float16)
    rows16[n // 2] = 0  # a zero element: the reference's builder leaves it out of the graph (src/index/mod.rs:813)
    R = oracle.normalize_f32(rows16.astype(np.float32))
    b = ga.GranneBuilder("angular_f16", rows16, num_neighbors=nn, max_search=ms, reinsert_elements=reinsert,
                         batch_max=bmax, batch_div=8)
    b.build()
    assert len(b) == n and b.num_elements() == n
    oix = oracle.build_index(R, num_neighbors=nn, max_search=ms, reinsert_elements=reinsert, batch_max=bmax, batch_div=8,
                             n_threads=0)
    assert b.num_layers() == len(oix.layers)
    for l, want in enumerate(oix.layers):
        got = b.get_layer(l)
        assert got.shape == want.shape
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (l, bad[:5], got[bad[:1]], want[bad[:1]])
    # normalised on read, every non-zero element is a unit vector to the builder and gets neighbors: widened only, a
    # quarter of them would be more than 100 epsilon off the sphere and be treated as zero vectors
    bottom = b.get_layer(b.num_layers() - 1)
    nonzero = np.nonzero(rows16.astype(np.float32).any(axis=1))[0]
    assert (bottom[nonzero, 0] != 0xFFFFFFFF).all()
    # the index it hands out holds the halves and searches like the oracle
    gix = b.get_index()
    assert gix.dtype_code == _lib.F16 and lib_dtype(gix) == _lib.F16
    assert gix.get_element(7).tobytes() == rows16[7].tobytes()
    q = oracle.normalize_f32(random_floats(rng, 16, dim))
    want = oix.search_batch(q, 30, 10)
    ids, ds, cnt = gix.search_batch(q, 30, 10)
    assert (ids == want[0]).all() and ds.tobytes() == want[1].tobytes() and (cnt == want[2]).all()
    # save_elements -> from_files: the Vectors layout [u64 dim][2-byte scalars]
    ip, ep = str(tmp_path / "index.granne"), str(tmp_path / "elements.f16")
    b.save_index(ip)
    b.save_elements(ep)
    blob = open(ep, "rb").read()
    assert len(blob) == 8 + n * dim * 2
    assert int(np.frombuffer(blob[:8], "<u8")[0]) == dim
    assert blob[8:] == rows16.tobytes()
    loaded = ga.Granne.from_files(ip, "angular_f16", ep)
    assert loaded.dim == dim and len(loaded) == n and lib_dtype(loaded) == _lib.F16
    ids2, ds2, cnt2 = loaded.search_batch(q, 30, 10)
    assert (ids2 == want[0]).all() and ds2.tobytes() == want[1].tobytes() and (cnt2 == want[2]).all()
    # the index's own save gives the same bytes; a truncated file is an error
    ep2 = str(tmp_path / "elements2.f16")
    loaded.save_elements(ep2)
    assert open(ep2, "rb").read() == blob
    with open(ep2, "wb") as f:
        f.write(blob[:-1])
    with pytest.raises(ga.GranneHipError):
        ga.Granne.from_files(ip, "angular_f16", ep2)
    with open(ep2, "wb") as f:
        f.write(blob[:-dim * 2])  # one row short of the index's elements
    with pytest.raises(ga.GranneHipError):
        ga.Granne.from_files(ip, "angular_f16", ep2)
    assert os.path.getsize(ep) == len(blob)


def lib_dtype(ix):
    from granne_amd import _lib
    return int(_lib.lib().granne_hip_index_dtype(ix._h))


def test_unprepared_rows_and_the_device_entry(ga, oracle):
    """prepared=False: normalised in f32, then rounded; from_device: halves already in HBM."""
    import torch
    rng = np.random.default_rng(31)
    raw = random_floats(rng, 600, 32) * np.float32(5.0)
    rows16 = oracle.normalize_f32(raw).astype(np.float16)
    R = oracle.normalize_f32(rows16.astype(np.float32))
    oix = oracle.build_index(R, num_neighbors=12, max_search=20, batch_max=64, batch_div=8, n_threads=0)
    b1 = ga.GranneBuilder("angular_f16", raw, num_neighbors=12, max_search=20, batch_max=64, batch_div=8, prepared=False)
    b1.build()
    t = torch.from_numpy(rows16.view(np.int16)).cuda()
    b2 = ga.GranneBuilder.from_device("angular_f16", t.data_ptr(), 600, 32, num_neighbors=12, max_search=20, batch_max=64,
                                      batch_div=8)
    b2.build()
    for b in (b1, b2):
        for l, want in enumerate(oix.layers):
            assert (b.get_layer(l) == want).all()
    assert b1.get_index().get_element(5).tobytes() == rows16[5].tobytes()
