"""The device codec of granne's index files (granne_amd/csrc/codec_kernels.h, codec_host.h): the `*_on_device` entry
points against the host codec (granne_amd/csrc/fileformat_host.h) and against oracle/fileformat.py.

The indexes are made from hand-written adjacency over tiny elements (dim 4): graph shape is under test, not search
quality. The host entries are the yardstick: bytes written on the device equal theirs, an index loaded on the device
equals theirs (layers, neighbors, hbm_bytes, search results, and the bytes it encodes back).

The raw form at count >= 4 is not reachable at a testable size: it needs stream-vbyte to be no shorter than 4 * count
bytes, i.e. nearly every delta of four or more ascending ids at 2^24 or more, so ids near 2^32 (the reference limits an
index to fewer than 2^32 - 1 elements, and such a layer alone would be 512 GiB of rows). The cases here reach the raw form
at counts 0, 1, 2 (the smallest: lengths summing to 5) and 3 (4 + 3 + 3)."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fileformat as off  # noqa: E402
from oracle import oracle as orc  # noqa: E402

UNUSED = 0xFFFFFFFF
MIN = 64 << 10  # GRANNE_HIP_CODEC_STAGING_MIN
DEFAULT = 64 << 20  # GRANNE_HIP_CODEC_STAGING_DEFAULT
STAGINGS = [None, MIN]
COUNTS = [0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64]
BOTTOMS = [0, 1, 59, 60, 61, 119, 120, 121]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def elements_of(n, kind):
    """n rows of dim 4, as stored: int8, normalised f32, or halves."""
    rng = np.random.default_rng(n + 7)
    raw = (rng.random((n, 4), dtype=np.float32) - np.float32(0.5)).astype(np.float32) + np.float32(0.01)
    if kind == "angular_int":
        return orc.quantize(raw)
    nrm = orc.normalize_f32(raw)
    return nrm.astype(np.float16) if kind == "angular_f16" else nrm


def hand_layer(n, width, seed, shift=0):
    """[n][width] rows: node i has COUNTS[(i + shift) % 11] ids (as many as n and width allow), distinct, in unsorted
    insertion order; every third row holds its ids around an UNUSED slot, every fifth names one id twice."""
    rng = np.random.default_rng(seed)
    rows = np.full((n, width), UNUSED, np.uint32)
    for i in range(n):
        c = min(COUNTS[(i + shift) % len(COUNTS)], n, width)
        ids = rng.permutation(n)[:c].astype(np.uint32)  # insertion order, not sorted
        if i % 5 == 4 and c >= 2:
            ids[-1] = ids[0]  # a duplicate id: delta 0
        if i % 3 == 2 and 0 < c < width:
            at = c // 2  # the ids around a hole
            rows[i, :at] = ids[:at]
            rows[i, at + 1:c + 1] = ids[at:]
        else:
            rows[i, :c] = ids
    return rows


def pyramid(n):
    """Prefix-nested layers down to a bottom of n nodes: 32- and 64-wide layers in one index."""
    lens = sorted({max(1, n // 20), max(1, n // 3), n}) if n else []
    return [hand_layer(m, 64 if (len(lens) - 1 - k) % 2 == 0 else 32, 100 * n + k, shift=k) for k, m in enumerate(lens)]


def n_chunks(layers):
    return [1 + l.shape[0] // 60 for l in layers]


def check_encode_info(info, layers, staging, fallback=0):
    """out_info of an encoding call against the bounds of include/granne_hip.h, which follow from the parameter alone:
    device scratch <= 2 * staging + 16 bytes per chunk of 60 nodes (and per layer's closing entry) + the scan's temporary
    storage (allowed 1 MiB here: hipcub's is a few bytes per tile of thousands of items); host staging <= the ring + a
    page, unless a layer fell back."""
    staging = staging or DEFAULT
    print("info", info, "staging", staging)
    assert info[0] == len(layers) - fallback and info[1] == fallback
    assert info[2] <= 2 * staging + sum(16 * (c + 1) for c in n_chunks(layers)) + (1 << 20)
    if not fallback:
        assert info[3] <= staging + 4096


class World:
    """An index, the file bytes the host codec and the oracle give for it, and its elements file."""

    def __init__(self, ga, layers, kind="angular_int", n_elements=None):
        self.layers, self.kind = layers, kind
        n = n_elements if n_elements is not None else (layers[-1].shape[0] if layers else 4)
        self.el = elements_of(n, kind)
        self.gix = ga.Granne(kind, self.el, layers)
        self.host_bytes = self.gix.index_bytes()
        self.el_bytes = off.write_elements(self.el)


@pytest.fixture(scope="module")
def small(ga):
    return {n: World(ga, pyramid(n)) for n in BOTTOMS}


@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
@pytest.mark.parametrize("n", BOTTOMS)
def test_bytes_equal_the_host_encoders_and_the_oracles(small, n, staging):
    w = small[n]
    got = w.gix.index_bytes(on_device=True, staging_bytes=staging)
    assert got == w.host_bytes
    assert got == off.write_index(w.layers)
    check_encode_info(w.gix.last_codec_info, w.layers, staging)


def layer_70k():
    """70,000 nodes, up to 30 ids: first values of 1, 2 and 3 bytes, deltas of 1 and 2 (and, across the layer, 3) bytes.
    Node 7 holds the two ids whose lengths sum to 5 (300: 2 bytes, + 65,700: 3 bytes): vbyte would take 1 + 5 + 2 padding
    bytes = 8 = 4 * 2, the smallest case where count 2 goes raw; node 8's sum to 4 and stay vbyte."""
    n = 70000
    rng = np.random.default_rng(70)
    rows = np.full((n, 30), UNUSED, np.uint32)
    cnt = rng.integers(0, 31, n)
    near = (np.arange(n)[:, None] + rng.integers(-120, 120, (n, 30))) % n  # small deltas
    far = rng.integers(0, n, (n, 30))                                       # two-byte deltas, a few of three
    ids = np.where(rng.random((n, 30)) < 0.5, near, far).astype(np.uint32)
    rows[np.arange(30)[None, :] < cnt[:, None]] = ids[np.arange(30)[None, :] < cnt[:, None]]
    rows[7] = UNUSED
    rows[7, :2] = [66000, 300]
    rows[8] = UNUSED
    rows[8, :2] = [65000, 300]
    rows[9] = UNUSED
    rows[9, :3] = [69999, 3, 2]  # 1 + 1 + 3 bytes
    return rows


@pytest.fixture(scope="module")
def w70k(ga):
    return World(ga, [hand_layer(50, 32, 5), layer_70k()])


@pytest.fixture(scope="module")
def oracle_70k(w70k):
    return off.write_index(w70k.layers)


@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
def test_delta_widths_and_the_raw_decision_70k(w70k, oracle_70k, staging):
    w = w70k
    # the records the case is about, by the oracle's encoder: raw at count 2 (9 bytes), vbyte at count 2, 3-byte delta
    assert len(orc.set_encode(np.array([300, 66000], np.uint32))) == 9
    assert len(orc.set_encode(np.array([300, 65000], np.uint32))) == 8
    assert len(orc.set_encode(np.array([2, 3, 69999], np.uint32))) == 1 + 1 + 1 + 1 + 3 + 1
    got = w.gix.index_bytes(on_device=True, staging_bytes=staging)
    assert got == w.host_bytes
    assert got == oracle_70k
    check_encode_info(w.gix.last_codec_info, w.layers, staging)


# The 4 + 3 + 3 record needs a first id of at least 2^24 and two deltas of at least 2^16, so ids up to 2^24 + 2^17: the layer
# has 2^24 + 2^17 + 64 nodes (2^24 + 64 would hold no such record).
BIG = (1 << 24) + (1 << 17) + 64
RAW3 = [(1 << 24) + (1 << 17), 1 << 24, (1 << 24) + (1 << 16)]  # insertion order; sorted: 2^24, + 2^16, + 2^16


def big_rows():
    """node -> ids of the few hundred nodes of the large layer that have any: first values of four bytes (ids from 2^24
    on), and the count-3 raw case: 4 + 3 + 3 bytes, + 1 padding byte + 1 control byte = 12 = 4 * 3."""
    rng = np.random.default_rng(24)
    rows = {}
    for node in rng.integers(0, BIG, 300):
        c = int(rng.integers(1, 31))
        rows[int(node)] = [int(x) for x in rng.integers(0, BIG, c)]
    for node in (59, 60, 61, BIG - 60, BIG - 59, (1 << 24) - 1, 1 << 24):
        rows[node] = [int(x) for x in rng.integers(1 << 24, BIG, 4)]  # four-byte first values around chunk edges
    rows.update({0: [BIG - 1, 5], 1: list(RAW3), BIG - 1: [1 << 24], BIG - 61: [7, 7]})
    return rows


def sparse_index_bytes(n, rows):
    """oracle/fileformat.py's write_index for one layer of n nodes whose rows are empty except `rows`: the same layout
    (offsets.rs chunks, the oracle's set_encode for every record that has ids), made with numpy instead of a Python loop
    over 2^24 rows."""
    lens = np.ones(n, np.int64)  # an empty list is the single byte 0
    recs = {i: orc.set_encode(np.sort(np.asarray(ids, np.uint32))) for i, ids in rows.items()}
    for i, r in recs.items():
        lens[i] = len(r)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    data = np.zeros(int(offsets[-1]), np.uint8)
    for i, r in recs.items():
        data[offsets[i]:offsets[i] + len(r)] = np.frombuffer(r, np.uint8)
    nc = 1 + n // 60
    idx = np.arange(nc * 60, dtype=np.int64).reshape(nc, 60)
    valid = idx <= n
    o = offsets[np.minimum(idx, n)]
    deltas = np.diff(o, axis=1, prepend=o[:, :1])
    assert deltas.max() < 0xFFFF
    table = np.empty((nc, 64), np.uint16)
    table[:, :4] = o[:, 0].astype("<u8").view(np.uint16).reshape(nc, 4)
    table[:, 4:] = np.where(valid, deltas, 0xFFFF)
    blob = struct.pack("<Q", nc * 128) + table.tobytes() + data.tobytes()
    meta = {"granne_version": "0.5.2", "version": 2, "num_elements": n, "num_layers": 1, "num_neighbors": len(rows.get(0, [])),
            "layer_counts": [n], "layer_sizes": [len(blob)], "compressed": True}
    head = ("granne" + json.dumps(meta, sort_keys=True, separators=(",", ":"))).encode()
    return head.ljust(1024, b" ") + blob


@pytest.fixture(scope="module")
def big(ga):
    """One layer of 2^24 + 2^17 + 64 nodes, made on the device (the rows alone are 2 GiB)."""
    import torch
    rows = big_rows()
    adj = torch.full((BIG, 32), -1, dtype=torch.int32, device="cuda")
    keys = sorted(rows)
    host = np.full((len(keys), 32), UNUSED, np.uint32)
    for k, node in enumerate(keys):
        host[k, :len(rows[node])] = rows[node]
    adj[torch.tensor(keys, device="cuda")] = torch.from_numpy(host.view(np.int32)).cuda()
    el = torch.zeros((BIG, 4), dtype=torch.int8, device="cuda")
    el[:, 0] = 1
    gix = ga.Granne.from_device("angular_int", el.data_ptr(), BIG, 4, [BIG], [adj.data_ptr()], [32])
    torch.cuda.synchronize()
    del adj, el
    return dict(gix=gix, rows=rows, host_bytes=gix.index_bytes())


@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
def test_four_byte_values_and_raw_at_count_3_in_a_layer_past_2_24(big, staging):
    assert len(orc.set_encode(np.sort(np.array(RAW3, np.uint32)))) == 1 + 12  # raw: vbyte would be 1 + 10 + 1 bytes too
    assert len(orc.set_encode(np.array([1 << 24], np.uint32))) == 1 + 4
    got = big["gix"].index_bytes(on_device=True, staging_bytes=staging)
    assert got == big["host_bytes"]
    assert got == sparse_index_bytes(BIG, big["rows"])
    check_encode_info(big["gix"].last_codec_info, [np.broadcast_to(np.uint8(0), (BIG, 32))], staging)


# ---- load equals load ---------------------------------------------------------------------------------------------
def same_index(a, b, sample=None):
    assert a.num_layers() == b.num_layers()
    assert a.hbm_bytes() == b.hbm_bytes()
    for l in range(a.num_layers()):
        assert a.layer_len(l) == b.layer_len(l)
        nodes = range(a.layer_len(l)) if sample is None or a.layer_len(l) <= 200 else sample
        for i in nodes:
            if i >= a.layer_len(l):
                continue
            assert a.get_neighbors(i, l) == b.get_neighbors(i, l), (l, i)


@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
@pytest.mark.parametrize("kind", ["angular_int", "angular", "angular_f16"])
@pytest.mark.parametrize("n", BOTTOMS)
def test_load_equals_load(ga, small, n, kind, staging):
    w = small[n]
    el = off.write_elements(elements_of(n if n else 4, kind))
    files = [w.host_bytes]
    ob = off.write_index(w.layers)
    if ob != w.host_bytes:  # (they are equal -- asserted above -- so one load covers both writers)
        files.append(ob)
    for fb in files:
        host = ga.Granne.from_bytes(fb, kind, el)
        dev = ga.Granne.from_bytes(fb, kind, el, on_device=True, staging_bytes=staging)
        info = dev.last_codec_info
        print("info", info)
        assert info[0] == len(w.layers) and info[1] == 0
        assert info[2] <= 2 * (staging or DEFAULT) and info[3] <= (staging or DEFAULT) + 4096
        same_index(dev, host)
        for i in range(len(dev)):
            assert dev.get_element(i).tobytes() == host.get_element(i).tobytes()
        assert dev.index_bytes() == fb  # round trip
        assert dev.index_bytes(on_device=True, staging_bytes=staging) == fb


@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
def test_load_equals_load_70k(ga, w70k, staging):
    w = w70k
    host = ga.Granne.from_bytes(w.host_bytes, w.kind, w.el_bytes)
    dev = ga.Granne.from_bytes(w.host_bytes, w.kind, w.el_bytes, on_device=True, staging_bytes=staging)
    assert dev.last_codec_info[:2] == (2, 0)
    same_index(dev, host, sample=list(range(0, 70000, 997)) + [7, 8, 9, 59, 60, 61, 69999])
    assert dev.get_neighbors(7) == [300, 66000] and dev.get_neighbors(9) == [2, 3, 69999]
    assert dev.index_bytes() == w.host_bytes


@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
def test_load_equals_load_past_2_24(ga, big, staging):
    el = np.zeros((BIG, 4), np.int8)
    el[:, 0] = 1
    eb = off.write_elements(el)
    host = ga.Granne.from_bytes(big["host_bytes"], "angular_int", eb)
    dev = ga.Granne.from_bytes(big["host_bytes"], "angular_int", eb, on_device=True, staging_bytes=staging)
    assert dev.last_codec_info[:2] == (1, 0)
    sample = sorted(big["rows"]) + [2, 3, BIG - 2]
    same_index(dev, host, sample=sample)
    for node, ids in big["rows"].items():
        assert dev.get_neighbors(node) == sorted(ids), node
    assert dev.index_bytes(on_device=True, staging_bytes=staging) == big["host_bytes"]


@pytest.fixture(scope="module")
def golden(ga):
    """The golden f32_d28 index (2,000 x 28-d, built by the oracle) and its files by the host codec."""
    z = np.load(os.path.join(HERE, "golden", "f32_d28.npz"))
    layers = [z["layer%d" % l] for l in range(int(z["n_layers"]))]
    gix = ga.Granne("angular", z["elements"], layers)
    return dict(gix=gix, q=z["queries"], layers=layers, el=z["elements"], index=gix.index_bytes(), elements=off.write_elements(z["elements"]))


@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
def test_search_results_of_a_loaded_index_are_the_host_loaders(ga, golden, staging):
    assert golden["index"] == off.write_index(golden["layers"])
    host = ga.Granne.from_bytes(golden["index"], "angular", golden["elements"])
    dev = ga.Granne.from_bytes(golden["index"], "angular", golden["elements"], on_device=True, staging_bytes=staging)
    same_index(dev, host, sample=range(0, 2000, 37))
    for ms, k in ((50, 10), (200, 25)):
        a, b, d = host.search_batch(golden["q"], ms, k), dev.search_batch(golden["q"], ms, k), golden["gix"].search_batch(golden["q"], ms, k)
        for x, y, v in zip(a, b, d):
            assert x.tobytes() == y.tobytes() == v.tobytes()


# ---- files ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
def test_files_written_on_the_device_load_on_the_host_and_back(ga, golden, w70k, tmp_path, staging):
    for name, w_gix, kind, index, elements in (("golden", golden["gix"], "angular", golden["index"], golden["elements"]),
                                               ("70k", w70k.gix, w70k.kind, w70k.host_bytes, w70k.el_bytes)):
        di, de, hi, he = (str(tmp_path / (name + s)) for s in (".dev.index", ".dev.elements", ".host.index", ".host.elements"))
        w_gix.save(di, de, on_device=True, staging_bytes=staging)
        info = w_gix.last_codec_info
        assert info[1] == 0 and info[3] <= (staging or DEFAULT) + 4096
        w_gix.save(hi, he)
        # 2,000 rows of 112 bytes and 70,000 rows of 4: neither count is a multiple of the rows a slot holds (292; 8,192)
        assert open(de, "rb").read() == open(he, "rb").read() == elements
        assert open(di, "rb").read() == open(hi, "rb").read() == index
        a = ga.Granne.from_files(di, kind, de)  # written on the device, read on the host
        b = ga.Granne.from_files(hi, kind, he, on_device=True, staging_bytes=staging)  # and the other way round
        assert b.last_codec_info[1] == 0
        same_index(a, b, sample=range(0, len(a), 211))
        assert a.index_bytes() == b.index_bytes() == index
        for i in (0, 1, len(a) // 2, len(a) - 1):
            assert a.get_element(i).tobytes() == b.get_element(i).tobytes() == w_gix.get_element(i).tobytes()
        # save_index / save_elements alone
        w_gix.save_index(di + "2", on_device=True, staging_bytes=staging)
        w_gix.save_elements(de + "2", on_device=True, staging_bytes=staging)
        assert open(di + "2", "rb").read() == index and open(de + "2", "rb").read() == elements


def test_builder_saves_through_the_device_codec(ga, golden, tmp_path):
    b = ga.GranneBuilder("angular", golden["el"], num_neighbors=20, max_search=20, batch_max=64)
    b.build()
    b.save_index(str(tmp_path / "host"))
    b.save_index(str(tmp_path / "dev"), on_device=True)
    assert (tmp_path / "dev").read_bytes() == (tmp_path / "host").read_bytes()
    assert b.last_codec_info[0] == b.num_layers() and b.last_codec_info[1] == 0


# ---- fallback ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staging", STAGINGS, ids=["default", "min"])
def test_a_layer_wider_than_64_ids_goes_through_the_host_codec(ga, staging):
    rng = np.random.default_rng(96)
    wide = np.full((200, 96), UNUSED, np.uint32)
    for i in range(200):
        c = int(rng.integers(0, 71)) if i else 70
        wide[i, :c] = rng.permutation(200)[:c]
    layers = [hand_layer(9, 32, 1), wide]
    w = World(ga, layers)
    got = w.gix.index_bytes(on_device=True, staging_bytes=staging)
    assert got == w.host_bytes == off.write_index(layers)
    check_encode_info(w.gix.last_codec_info, layers, staging, fallback=1)
    host = ga.Granne.from_bytes(got, w.kind, w.el_bytes)
    dev = ga.Granne.from_bytes(got, w.kind, w.el_bytes, on_device=True, staging_bytes=staging)
    assert dev.last_codec_info[:2] == (1, 1)
    same_index(dev, host)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_compact_sum_embeddings_handle_refuses_elements_path(ga, tmp_path):
    rng = np.random.default_rng(3)
    tab = (rng.random((50, 8), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    lists = [[int(x) for x in rng.integers(0, 50, 3)] for _ in range(61)]
    se = ga.SumEmbeddings(tab, lists)
    layers = [hand_layer(3, 32, 2), hand_layer(61, 32, 3)]
    cix = ga.Granne("embeddings", se, layers, compact=True)
    with pytest.raises(ga.GranneHipError) as h:
        cix.save(str(tmp_path / "h.index"), str(tmp_path / "h.elements"))
    with pytest.raises(ga.GranneHipError) as d:
        cix.save(str(tmp_path / "d.index"), str(tmp_path / "d.elements"), on_device=True)
    assert h.value.code == d.value.code == -1
    # the index file is written before the refusal, by both
    assert (tmp_path / "d.index").read_bytes() == (tmp_path / "h.index").read_bytes() == off.write_index(layers)
    assert not (tmp_path / "d.elements").exists()
    assert cix.index_bytes(on_device=True) == cix.index_bytes()


def test_bad_files(ga, tmp_path):
    """The malformed files of tests/test_gpu_files.py::test_bad_files."""
    (tmp_path / "x").write_bytes(b"not an index" + b" " * 1100)
    (tmp_path / "e").write_bytes(off.write_elements(np.zeros((4, 8), np.float32)))
    with pytest.raises(ga.GranneHipError) as e:
        ga.Granne.from_files(str(tmp_path / "x"), "angular", str(tmp_path / "e"), on_device=True)
    assert e.value.code == -5
    with pytest.raises(ga.GranneHipError) as e:
        ga.Granne.from_files(str(tmp_path / "missing"), "angular", str(tmp_path / "e"), on_device=True)
    assert e.value.code == -5
    with pytest.raises(ga.GranneHipError) as e:
        ga.Granne.from_bytes((tmp_path / "x").read_bytes(), "angular", (tmp_path / "e").read_bytes(), on_device=True)
    assert e.value.code == -5


def corruptible():
    """A one-layer file of 121 nodes whose records are known byte for byte: node 0 is [120] (raw: 1, then 120 as four
    bytes), every other node holds eight consecutive ids (count, two control bytes of zeros, eight one-byte values: 11
    bytes). Data offset of node j >= 1: 5 + 11 (j - 1)."""
    rows = np.full((121, 32), UNUSED, np.uint32)
    rows[0, 0] = 120
    for j in range(1, 121):
        rows[j, :8] = (j % 100) + np.arange(8)
    buf = bytearray(off.write_index([rows]))
    table = 1024 + 8
    data = table + 3 * 128
    assert buf[data:data + 5] == bytes([1, 120, 0, 0, 0]) and buf[data + 5] == 8 and len(buf) == data + 5 + 11 * 120
    return rows, buf, table, data


def corruptions():
    rows, good, table, data = corruptible()
    out = {}
    b = bytearray(good)
    b[data + 5 + 11 * 4] = 9  # node 5 says nine ids: three control bytes + nine values do not fit its ten payload bytes
    out["a count byte raised"] = b
    b = bytearray(good)
    d7 = table + 8 + 2 * 7
    assert struct.unpack_from("<H", b, d7)[0] == 11
    struct.pack_into("<H", b, d7, 10)  # offset 7 one byte early: node 6 is one byte short of its eight values
    out["a record shortened by one byte through its offset delta"] = b
    b = bytearray(good)
    assert struct.unpack_from("<Q", b, table + 128)[0] == 5 + 11 * 59
    struct.pack_into("<Q", b, table + 128, 0)  # chunk 1 starts before chunk 0 ends
    out["a non-monotone initial"] = b
    b = bytearray(good)
    struct.pack_into("<H", b, table + 8 + 2 * 30, 0xFFFE)  # offsets 30 .. 59 lie far behind the data
    out["an offset beyond the data"] = b
    b = bytearray(good)
    b[data + 1] = 121  # node 0's only id
    out["an id equal to the layer length"] = b
    b = bytearray(good[:-1])  # the last record loses its last byte, and layer_sizes says so
    size = len(good) - 1024
    head = bytes(b[:1024]).replace(b'"layer_sizes":[%d]' % size, b'"layer_sizes":[%d]' % (size - 1))
    assert head != bytes(b[:1024]) and len(head) == 1024
    b[:1024] = head
    out["a truncated last record"] = b
    return rows, bytes(good), out


ROWS_121, GOOD_121, CORRUPT = corruptions()


@pytest.mark.parametrize("what", sorted(CORRUPT))
def test_record_level_corruptions_are_io_errors(ga, golden, what):
    """Each input is rejected by a bounds check -- on the host for what the host can see in the offset entries it reads,
    in the kernels for the rest -- and the device answers an ordinary search right after."""
    el = off.write_elements(elements_of(121, "angular_int"))
    bad = bytes(CORRUPT[what])
    assert ga.Granne.from_bytes(GOOD_121, "angular_int", el, on_device=True, staging_bytes=MIN).get_neighbors(0) == [120]
    with pytest.raises(ga.GranneHipError) as h:  # the host loader rejects it: the test cannot pass by both accepting
        ga.Granne.from_bytes(bad, "angular_int", el)
    assert h.value.code == -5
    for staging in STAGINGS:
        with pytest.raises(ga.GranneHipError) as d:
            ga.Granne.from_bytes(bad, "angular_int", el, on_device=True, staging_bytes=staging)
        assert d.value.code == -5, (what, staging, str(d.value))
        print(what, "->", d.value)
    ids, ds, cnt = golden["gix"].search_batch(golden["q"][:8], 50, 10)
    assert (cnt == 10).all() and np.isfinite(ds).all()
