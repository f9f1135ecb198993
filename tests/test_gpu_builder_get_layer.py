"""GranneBuilder.get_layer past its packing chunk: granne_hip_builder_get_layer packs 2^20 lists at a time on the device
before they come down. A bottom layer of 2^20 + 777 lists spans two chunks; its rows on both sides of the boundary and at
both ends must be the lists the index made from the same builder returns, one by one (granne_hip_index_get_neighbors)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_layer_of_more_than_one_chunk():
    from granne_amd.builder import GranneBuilder
    chunk, n = 1 << 20, (1 << 20) + 777
    rng = np.random.default_rng(31)
    el = (rng.random((n, 4), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    b = GranneBuilder("angular", el, prepared=False, num_neighbors=6, max_search=8, reinsert_elements=False)
    b.build()
    layer = b.get_layer(b.num_layers() - 1)
    assert layer.shape == (n, 6)
    ix = b.get_index()
    for i in [0, 1, chunk - 2, chunk - 1, chunk, chunk + 1, chunk + 500, n - 2, n - 1]:
        row = [int(x) for x in layer[i] if x != 0xFFFFFFFF]
        assert row == ix.get_neighbors(i), i
        assert row and all(0 <= x < n and x != i for x in row), i
    ix.close()
