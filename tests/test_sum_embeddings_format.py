"""The SumEmbeddings container's files (no GPU): the elements file is the reference's
VariableWidthSliceVector<ThreeByteInt, FiveByteInt> (src/slice_vector/mod.rs:623-634, 660-676, odd_byte_int.rs:3-36) --
u64 LE n, n + 1 offsets of 5 bytes LE counted in ids (the first 0), the ids at 3 bytes LE each -- and the table an
ordinary f32 Vectors file. The packer below is written from that layout; the library must agree with it byte for byte."""
import ctypes as C
import struct

import numpy as np
import pytest

from granne_amd import _lib, build


@pytest.fixture(scope="module")
def ga():
    build.build_library()
    import granne_amd
    return granne_amd


def pack_elements(term_lists):
    out = [struct.pack("<Q", len(term_lists))]
    at = 0
    out.append(at.to_bytes(5, "little"))
    for t in term_lists:
        at += len(t)
        out.append(at.to_bytes(5, "little"))
    for t in term_lists:
        for x in t:
            out.append(int(x).to_bytes(3, "little"))
    return b"".join(out)


def table(v, dim, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.random((v, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


CASES = {
    "none": [],
    "one": [[3, 1, 2]],
    "one_empty": [[]],
    "empty_last": [[0, 5], [7], []],
    "mixed": [[], [9, 9], [0], list(range(40)), [], [16777215 % 50], [1, 2, 3, 4, 5, 6]],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_elements_file_is_the_reference_layout_and_reads_back(ga, tmp_path, name):
    lists = CASES[name]
    tab = table(50, 7)
    se = ga.SumEmbeddings(tab, lists)
    assert len(se) == len(lists) and se.num_embeddings() == 50 and se.dim == 7
    pe, pt = str(tmp_path / "elements.bin"), str(tmp_path / "table.bin")
    se.save_elements(pe)
    se.save_embeddings(pt)
    want = pack_elements(lists)
    assert open(pe, "rb").read() == want
    assert open(pt, "rb").read() == struct.pack("<Q", 7) + tab.tobytes()
    back = ga.SumEmbeddings.from_files(pt, pe)
    assert len(back) == len(lists) and back.num_embeddings() == 50 and back.dim == 7
    assert [back.get_terms(i) for i in range(len(lists))] == [list(map(int, t)) for t in lists]
    again = ga.SumEmbeddings.from_bytes(tab, want)
    assert [again.get_terms(i) for i in range(len(lists))] == [list(map(int, t)) for t in lists]


def test_three_byte_ids_up_to_the_last_one(ga, tmp_path):
    """The largest term id the format holds (2^24 - 1) survives; the table only has to be that tall for the check."""
    v = 1 << 24
    tab = np.zeros((v, 1), np.float32)
    lists = [[v - 1, 0, 65536, 255, 256]]
    se = ga.SumEmbeddings(tab, lists)
    p = str(tmp_path / "e.bin")
    se.save_elements(p)
    assert open(p, "rb").read() == pack_elements(lists)
    assert ga.SumEmbeddings.from_bytes(tab, pack_elements(lists)).get_terms(0) == lists[0]


def test_push_appends_elements(ga, tmp_path):
    tab = table(20, 4)
    se = ga.SumEmbeddings(tab, [[1, 2]])
    se.push([3])
    se.push([])
    se.extend([[4, 4, 4], [19]])
    lists = [[1, 2], [3], [], [4, 4, 4], [19]]
    assert len(se) == 5 and [se.get_terms(i) for i in range(5)] == lists
    p = str(tmp_path / "e.bin")
    se.save_elements(p)
    assert open(p, "rb").read() == pack_elements(lists)
    with pytest.raises(ga.GranneHipError) as e:
        se.push([20])
    assert e.value.code == _lib.ERR_INVALID and len(se) == 5


def _create(lib, tab, off, ids):
    h = C.c_void_p()
    off = np.asarray(off, np.uint64)
    ids = np.asarray(ids, np.uint32)
    rc = lib.granne_hip_sum_embeddings_create(C.byref(h), tab.ctypes.data_as(C.c_void_p), tab.shape[0], tab.shape[1],
                                              off.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), off.size - 1, 0)
    if h.value:
        lib.granne_hip_sum_embeddings_destroy(h)
    return rc, lib.granne_hip_last_error()


def _load(lib, tab, data):
    h = C.c_void_p()
    buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
    rc = lib.granne_hip_sum_embeddings_load(C.byref(h), tab.ctypes.data_as(C.c_void_p), tab.shape[0], tab.shape[1],
                                            buf.ctypes.data_as(C.c_void_p), len(data), 0)
    if h.value:
        lib.granne_hip_sum_embeddings_destroy(h)
    return rc, lib.granne_hip_last_error()


def test_malformed_input_is_invalid_with_a_message(ga, tmp_path):
    lib = _lib.lib()
    tab = table(10, 3)
    # a term id that is not below the number of embeddings
    rc, msg = _create(lib, tab, [0, 2], [1, 10])
    assert rc == _lib.ERR_INVALID and msg
    rc, msg = _load(lib, tab, pack_elements([[1, 10]]))
    assert rc == _lib.ERR_INVALID and msg
    # offsets that decrease, or do not start at 0
    rc, msg = _create(lib, tab, [0, 2, 1], [1, 2])
    assert rc == _lib.ERR_INVALID and b"decrease" in msg
    rc, msg = _create(lib, tab, [1, 2], [1, 2])
    assert rc == _lib.ERR_INVALID and msg
    good = pack_elements([[1, 2], [3]])
    bad = bytearray(good)
    bad[8 + 5:8 + 10] = (3).to_bytes(5, "little")  # offsets 0, 3, 3 -> fine; then make the last one smaller
    bad[8 + 10:8 + 15] = (2).to_bytes(5, "little")
    rc, msg = _load(lib, tab, bytes(bad))
    assert rc == _lib.ERR_INVALID and msg
    # truncated files: inside the header, inside the offsets, inside the ids, and nothing at all
    for cut in (0, 4, 8, 8 + 7, len(good) - 1, len(good) - 3):
        rc, msg = _load(lib, tab, good[:cut])
        assert rc == _lib.ERR_INVALID and msg, cut
    assert _load(lib, tab, good)[0] == 0
    # a count that promises more offsets than any file holds
    rc, msg = _load(lib, tab, struct.pack("<Q", 1 << 62) + b"\0" * 64)
    assert rc == _lib.ERR_INVALID and msg
    # on write: more embeddings than 3-byte ids address
    big = ga.SumEmbeddings(np.zeros(((1 << 24) + 1, 1), np.float32), [[1 << 24]])
    with pytest.raises(ga.GranneHipError) as e:
        big.save_elements(str(tmp_path / "big.bin"))
    assert e.value.code == _lib.ERR_INVALID
    # null handles and buffers never crash
    assert lib.granne_hip_sum_embeddings_create(None, None, 0, 3, None, None, 0, 0) == _lib.ERR_INVALID
    assert lib.granne_hip_sum_embeddings_save_elements(None, b"x") == _lib.ERR_INVALID
    assert lib.granne_hip_sum_embeddings_get_terms(None, 0, None, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_sum_embeddings_len(None) == 0 and lib.granne_hip_sum_embeddings_dim(None) == 0
    assert lib.granne_hip_index_create_sum_embeddings(None, None, 0, None, None, None, 0) == _lib.ERR_INVALID
    assert lib.granne_hip_builder_get_index_compact(None, None) == _lib.ERR_INVALID
    assert lib.granne_hip_sum_embeddings_materialize_device(None, 0, 0, 0, None, 0, None) == _lib.ERR_INVALID
    lib.granne_hip_sum_embeddings_destroy(None)


def test_the_largest_five_byte_offset_is_read_whole(ga, tmp_path):
    """A container of 2^40 ids cannot be held in a test, so the writer's bound (offsets[-1] < 2^40) is not reached here.
    What is checked: the reader takes the largest offset a 5-byte field holds whole (no wrap-around) and then reports
    the ids it promises as missing."""
    tab = table(4, 2)
    data = struct.pack("<Q", 1) + (0).to_bytes(5, "little") + ((1 << 40) - 1).to_bytes(5, "little")
    rc, msg = _load(_lib.lib(), tab, data)  # the offsets are read whole (no wrap-around), the ids are then missing
    assert rc == _lib.ERR_INVALID and b"truncated ids" in msg
