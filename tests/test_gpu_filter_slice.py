"""granne_hip_filter_slice_device against tests/sharded_filter_model.slice_words: one filter and strided filters, the
output stride equal to the word count and larger, garbage past n_bits in the source, and one case of a million bits
(many blocks). tests/README_sharded_filtered.md says what each test pins."""
import ctypes as C

import numpy as np
import pytest

from tests import sharded_filter_model as sm

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xDEADBEEF)


def _slice(words, n_bits, stride, n_filters, first, n_out, out_stride):
    """the entry on device copies of `words` ([n_filters][stride or word count] u32); returns [n_filters][out_stride]"""
    from granne_amd import _lib
    from granne_amd.filters import _DeviceBlock
    lib = _lib.lib()
    src, out_host = _DeviceBlock(words.nbytes, 0), np.full((n_filters, out_stride), SENTINEL, np.uint32)
    out = _DeviceBlock(out_host.nbytes, 0)
    if words.size:
        src.upload(words)
    if out_host.size:
        out.upload(out_host)
    _lib.check(lib.granne_hip_filter_slice_device(C.c_void_p(src.ptr), n_bits, stride, n_filters, first, n_out, C.c_void_p(out.ptr),
                                                  out_stride, 0, None))
    _lib.check(lib.granne_hip_stream_synchronize(None, 0))
    return out.download(np.uint32, n_filters * out_stride).reshape(n_filters, out_stride) if out_host.size else out_host


def _source(rng, n_bits, n_filters, pad):
    """n_filters random bitmaps over n_bits ids, `pad` words of garbage after each, garbage past n_bits in the last word"""
    w = (n_bits + 31) // 32
    words = rng.integers(0, 1 << 32, (n_filters, w + pad), dtype=np.uint64).astype(np.uint32)
    return words, w + pad


@pytest.mark.parametrize("first_mod", [0, 1, 9, 31])
def test_slices_equal_the_model(first_mod):
    rng = np.random.default_rng(first_mod)
    for n_out in (0, 1, 31, 32, 33, 937):
        for first in (first_mod, 64 + first_mod):
            for n_bits in (first + n_out, first + n_out + 77):  # the slice ends exactly at n_bits, or before it
                for n_filters, pad, out_pad in ((1, 0, 0), (1, 0, 3), (3, 0, 0), (3, 2, 5)):
                    words, stride = _source(rng, n_bits, n_filters, pad)
                    ow = (n_out + 31) // 32
                    got = _slice(words, n_bits, 0 if n_filters == 1 and pad == 0 else stride, n_filters, first, n_out, ow + out_pad)
                    for f in range(n_filters):
                        assert (got[f, :ow] == sm.slice_words(words[f], n_bits, first, n_out)).all(), (n_out, first, n_bits, n_filters, f)
                    assert (got[:, ow:] == SENTINEL).all()  # nothing is written past a filter's words


def test_slice_past_the_bitmaps_end_reads_zeros():
    rng = np.random.default_rng(3)
    words, _ = _source(rng, 70, 1, 0)
    got = _slice(words, 70, 0, 1, 60, 40, 2)  # 10 real bits, then 30 past the bitmap
    assert (got[0] == sm.slice_words(words[0], 70, 60, 40)).all()


def test_the_fixtures_shards():
    rng = np.random.default_rng(4)
    words, stride = _source(rng, sm.N, 2, 1)
    for off, n in zip(sm.offsets(), sm.LENGTHS):
        got = _slice(words, sm.N, stride, 2, off, n, (n + 31) // 32)
        for f in range(2):
            assert (got[f] == sm.slice_words(words[f], sm.N, off, n)).all(), off


@pytest.mark.parametrize("first", [0, 777])
def test_a_million_bits(first):
    n_bits = 1_000_003
    rng = np.random.default_rng(first)
    words, _ = _source(rng, n_bits, 1, 0)
    n_out = n_bits - first
    got = _slice(words, n_bits, 0, 1, first, n_out, (n_out + 31) // 32)
    assert (got[0] == sm.slice_words(words[0], n_bits, first, n_out)).all()
