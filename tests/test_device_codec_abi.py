"""The device codec's entry points without a GPU: exported, declared alike in the three bindings, arguments and file
headers refused before any device work -- and the codec kernels compiled alone for gfx950: no scratch memory."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = ["granne_hip_index_encode_on_device", "granne_hip_index_save_on_device", "granne_hip_index_load_on_device",
           "granne_hip_index_load_files_on_device"]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


def test_the_four_entries_are_exported_and_declared_in_every_binding(lib):
    raw = C.CDLL(build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "granne_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "granne-hip", "src", "gpu.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "granne.hpp")).read()
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.search(r"\bfn %s\(" % name, rust), name
    # uint64_t staging_bytes and uint64_t* out_info close every prototype, in the header and in ctypes
    for name in ENTRIES[1:]:
        assert _lib.SIGNATURES[name][1][-2:] == [C.c_uint64, C.c_void_p], name
        assert re.search(r"%s\([^;]*uint64_t staging_bytes, uint64_t\* out_info\);" % name, header), name
    assert _lib.SIGNATURES[ENTRIES[0]][1][1] is C.c_uint64
    # the safe wrappers
    assert "granne_hip_index_save_on_device(self.handle" in rust and "pub fn save_on_device(" in rust
    assert "granne_hip_index_load_files_on_device(&mut h" in rust and "pub fn from_files_on_device(" in rust
    assert "void save_on_device(" in hpp and "static Granne load_files_on_device(" in hpp
    # the documented staging sizes agree
    assert int(re.search(r"#define GRANNE_HIP_CODEC_STAGING_DEFAULT \((\d+)ull << 20\)", header).group(1)) << 20 == _lib.CODEC_STAGING_DEFAULT
    assert int(re.search(r"#define GRANNE_HIP_CODEC_STAGING_MIN \((\d+)ull << 10\)", header).group(1)) << 10 == _lib.CODEC_STAGING_MIN
    assert lib.granne_hip_abi_version() == 3


def test_argument_validation_needs_no_device(lib, tmp_path):
    h, out, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    info = (C.c_uint64 * 4)()
    buf = np.zeros(2048, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    INV = _lib.ERR_INVALID
    assert lib.granne_hip_index_encode_on_device(None, 0, C.byref(out), C.byref(n), info) == INV
    assert lib.granne_hip_index_save_on_device(None, b"x", b"y", 0, info) == INV
    assert lib.granne_hip_index_load_on_device(None, p, 2048, p, 2048, _lib.I8, 0, 0, info) == INV
    assert lib.granne_hip_index_load_on_device(C.byref(h), None, 2048, p, 2048, _lib.I8, 0, 0, info) == INV
    assert lib.granne_hip_index_load_on_device(C.byref(h), p, 2048, None, 2048, _lib.I8, 0, 0, info) == INV
    assert lib.granne_hip_index_load_on_device(C.byref(h), p, 2048, p, 2048, 7, 0, 0, info) == INV  # dtype
    assert b"dtype" in lib.granne_hip_last_error()
    assert lib.granne_hip_index_load_files_on_device(None, b"x", b"y", _lib.I8, 0, 0, info) == INV
    assert lib.granne_hip_index_load_files_on_device(C.byref(h), None, b"y", _lib.I8, 0, 0, info) == INV
    assert lib.granne_hip_index_load_files_on_device(C.byref(h), b"x", None, _lib.I8, 0, 0, info) == INV
    assert lib.granne_hip_index_load_files_on_device(C.byref(h), b"x", b"y", 7, 0, 0, None) == INV
    assert not h.value


def test_what_is_wrong_with_a_file_is_an_io_error_before_any_device_work(lib, tmp_path):
    """Everything the host reads in the headers -- the files themselves, the library string, the JSON, layer_sizes against
    the file, a blob's offset-table size, its node count -- is refused as by the host loader, GPU or not."""
    from oracle import fileformat as off
    h = C.c_void_p()
    IO = _lib.ERR_IO
    el = np.frombuffer(off.write_elements(np.zeros((61, 4), np.int8)), np.uint8)
    rows = np.full((61, 32), 0xFFFFFFFF, np.uint32)
    rows[:, 0] = np.arange(61)[::-1]
    good = off.write_index([rows])

    def load(index, elements=el):
        a, b = np.frombuffer(bytes(index), np.uint8), np.ascontiguousarray(elements)
        rc = lib.granne_hip_index_load_on_device(C.byref(h), a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size,
                                                 _lib.I8, 0, 0, None)
        host = lib.granne_hip_index_load(C.byref(h), a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, _lib.I8, 0)
        assert host == IO  # the yardstick refuses it too
        return rc

    assert load(b"not an index" + b" " * 1100) == IO
    assert load(good[:900]) == IO
    assert load(good, el[:5]) == IO and load(good, el[:-1]) == IO  # no width; the width does not divide the data
    assert load(good[:-1]) == IO  # layer_sizes runs past the file
    assert load(good.replace(b'"num_layers":1', b'"num_layers":2')) == IO
    bad = bytearray(good)
    bad[1024:1032] = (3 * 128).to_bytes(8, "little")  # an offset table larger than the blob says a different node count
    assert load(bad) == IO
    bad = bytearray(good)
    bad[1024:1032] = (100).to_bytes(8, "little")  # not whole entries
    assert load(bad) == IO
    assert load(good.replace(b'"layer_counts":[61]', b'"layer_counts":[60]')) == IO
    (tmp_path / "e").write_bytes(el.tobytes())
    assert lib.granne_hip_index_load_files_on_device(C.byref(h), os.fsencode(tmp_path / "missing"), os.fsencode(tmp_path / "e"), _lib.I8, 0, 0,
                                                     None) == IO
    (tmp_path / "i").write_bytes(good)
    assert lib.granne_hip_index_load_files_on_device(C.byref(h), os.fsencode(tmp_path / "i"), os.fsencode(tmp_path / "missing"), _lib.I8, 0, 0,
                                                     None) == IO
    assert not h.value


TU = """
#include "codec_kernels.h"
namespace granne_hip {
#define ENC(W, MODE) template __global__ void codec_encode_kernel<W, MODE>(const uint32_t*, uint64_t, uint64_t, uint64_t, uint64_t*, const uint64_t*, uint8_t*);
ENC(32, ENC_SUMS) ENC(32, ENC_TABLE) ENC(32, ENC_DATA) ENC(64, ENC_SUMS) ENC(64, ENC_TABLE) ENC(64, ENC_DATA)
template __global__ void dec_rows_kernel<32>(const uint8_t*, uint32_t, const uint32_t*, uint64_t, uint64_t, uint64_t, uint32_t*, uint32_t*, uint32_t*);
template __global__ void dec_rows_kernel<64>(const uint8_t*, uint32_t, const uint32_t*, uint64_t, uint64_t, uint64_t, uint32_t*, uint32_t*, uint32_t*);
}
"""


def test_codec_kernels_use_no_scratch(tmp_path):
    """In the style of tests/test_walker_registers.py: the kernels' entries in the code object's metadata. Ten kernels --
    the encoder's three modes at both row widths, the cut, the two decoder kernels at both widths -- none with a private
    segment or a spilled register, and the encoder's LDS is what one chunk of 64-id records needs."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    src, out = tmp_path / "codec.hip", tmp_path / "codec.s"
    src.write_text(TU)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "granne_amd", "csrc"),
                           "--cuda-device-only", "-S", "-Wno-unused-command-line-argument", str(src), "-o", str(out)])
    txt = out.read_text()
    kernels = {}
    for entry in re.split(r"\n  - \.agpr_count:", txt.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0])[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\S+)", entry))
        kernels[f["name"]] = f
    assert len(kernels) == 10, sorted(kernels)
    for name, k in sorted(kernels.items()):
        print(name, k)
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
        assert int(k["vgpr_count"]) <= 64, k  # eight waves per SIMD
        assert int(k["group_segment_fixed_size"]) <= 60 * (1 + 16 + 256) + 8 + 512 + 16, k
