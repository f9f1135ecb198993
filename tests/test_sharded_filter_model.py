"""tests/sharded_filter_model.py on the CPU: the slice in numpy against pack_bits of the mask's slice, and the claim the
partitioned exact selection rests on -- the merge of per-shard exact answers IS the exact answer over the whole set."""
import numpy as np
import pytest

from tests import exact_topk_filtered_model as etm
from tests import filter_model as fm
from tests import sharded_filter_model as sm


@pytest.mark.parametrize("first_mod", [0, 1, 9, 31])
@pytest.mark.parametrize("n_out", [0, 1, 31, 32, 33, 937])
def test_slice_words_is_pack_bits_of_the_masks_slice(first_mod, n_out):
    rng = np.random.default_rng(first_mod * 1000 + n_out)
    for first in (first_mod, 64 + first_mod, 1000 - (1000 % 32) + first_mod):
        for n_bits in (first + n_out, first + n_out + 5, first + n_out + 77):  # the slice ends exactly at n_bits, or before
            mask = rng.random(n_bits) < 0.5
            words = etm.words(mask, garbage_past_n=True)
            got = sm.slice_words(words, n_bits, first, n_out)
            assert got.dtype == np.uint32 and len(got) == (n_out + 31) // 32
            assert (got == fm.pack_bits(mask[first:first + n_out])).all()


def test_slice_words_reads_zeros_past_n_bits():
    mask = np.ones(70, bool)
    got = sm.slice_words(etm.words(mask, garbage_past_n=True), 70, 60, 40)  # 10 real bits, 30 past the bitmap
    assert (got == fm.pack_bits(np.r_[np.ones(10, bool), np.zeros(30, bool)])).all()


@pytest.mark.parametrize("int8", [False, True])
def test_merged_per_shard_exact_answers_are_the_exact_answer(oracle, int8):
    el, q = sm.fixture_rows(oracle, int8)
    offs = sm.offsets()
    rng = np.random.default_rng(5)
    for k in (1, 17, 100):
        for name, mask in etm.shared_filters(rng, sm.N, k).items():
            parts = [etm.oracle_subset(oracle, el[o:o + n], mask[o:o + n], q, k) for o, n in zip(offs, sm.LENGTHS)]
            got = sm.merge(parts, offs, k)
            want = sm.expected_exact(oracle, el, mask, q, k)
            assert (got[2] == want[2]).all(), name
            assert (got[0] == want[0]).all(), name
            assert got[1].tobytes() == want[1].tobytes(), name
    # distance 0 is covered: queries 0 and 1 are rows of the set
    d0 =sm.expected_exact(oracle, el, np.ones(sm.N, bool), q[:2], 1)
    assert (d0[0][:, 0] == [17, offs[-1] + 5]).all() and (np.abs(d0[1][:, 0]) < 1e-6).all()
