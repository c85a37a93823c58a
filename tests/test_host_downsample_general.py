"""The general branch of ``F.spdownsample`` (stride neither 1 nor the kernel size: k = 3, s = 2), without a GPU: known answers
of the numpy restatement the GPU test compares the device path with (tests/downsample_general_ref.py), the per-row candidate
bound the device buffer is sized by, and the host-side argument checks of the new C-ABI entry."""
import itertools

import numpy as np
import pytest

from downsample_general_ref import kept_candidates, max_candidates_per_row, ref_spdownsample_general


def _c(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def _cube(values, b):
    return [(x, y, z, b) for x, y, z in itertools.product(values, repeat=3)]


def test_lone_odd_voxel_keeps_only_the_candidate_above_the_minimum():
    # candidates per axis 0, 1, 2; multiples of 2: 0 and 2; 0 is below cmin = 1
    assert (ref_spdownsample_general(_c([(1, 1, 1, 0)]), 2, 3, 1) == _c([(2, 2, 2, 0)])).all()


def test_two_voxels_give_eight_outputs():
    got = ref_spdownsample_general(_c([(0, 0, 0, 0), (1, 1, 1, 0)]), 2, 3, 1)
    assert got.dtype == np.int32 and (got == _c(_cube((0, 2), 0))).all()      # n_out = 8 > n_in = 2, sorted by (b, x, y, z)


def test_minimum_is_shared_across_batches():
    two = [(0, 0, 0, 0), (1, 1, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]
    assert (ref_spdownsample_general(_c(two), 2, 3, 1) == _c(_cube((0, 2), 0) + _cube((0, 2), 1))).all()
    # batch 1 holds the odd voxel alone: on its own it would keep (2,2,2) only; the minimum 0 comes from batch 0
    got = ref_spdownsample_general(_c([(1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 0)]), 2, 3, 1)
    assert (got == _c(_cube((0, 2), 0) + _cube((0, 2), 1))).all()


def test_negative_odd_coordinate():
    # x candidates -4, -3, -2: both even ones are multiples (Python remainder), -4 is below the minimum -3
    assert (ref_spdownsample_general(_c([(-3, 1, 1, 0)]), 2, 3, 1) == _c([(-2, 2, 2, 0)])).all()
    got = ref_spdownsample_general(_c([(-3, 1, 1, 0), (-5, 1, 1, 0)]), 2, 3, 1)
    assert (got == _c([(-4, 2, 2, 0), (-2, 2, 2, 0)])).all()


def test_axis_with_stride_one_is_dilated():
    assert (ref_spdownsample_general(_c([(0, 0, 5, 0)]), (2, 2, 1), 3, 1) == _c([(0, 0, 5, 0), (0, 0, 6, 0)])).all()
    got = ref_spdownsample_general(_c([(0, 0, 5, 0), (0, 0, 9, 0)]), (2, 2, 1), (3, 3, 3), 1)
    assert (got == _c([(0, 0, z, 0) for z in (5, 6, 8, 9, 10)])).all()


def test_tensor_stride_two():
    got = ref_spdownsample_general(_c([(0, 0, 0, 0), (2, 2, 2, 0)]), 2, 3, 2)
    assert (got == _c(_cube((0, 4), 0))).all()
    # a coordinate that is no multiple of the tensor stride has no candidate on the stride-4 lattice
    assert ref_spdownsample_general(_c([(1, 1, 1, 0)]), 2, 3, 2).shape == (0, 4)


def test_empty_input():
    got = ref_spdownsample_general(np.zeros((0, 4), dtype=np.int32), 2, 3, 1)
    assert got.shape == (0, 4) and got.dtype == np.int32


@pytest.mark.parametrize('ts,ks,st', [(1, 3, 2), (2, 3, 2), (1, (3, 3, 3), (2, 2, 1)), (1, (3, 3, 1), (2, 2, 1)), (1, 2, 3), (3, 3, 2),
                                      (1, (3, 2, 1), (2, 3, 4))])
def test_no_row_has_more_than_m_kept_candidates(ts, ks, st):
    rng = np.random.default_rng(17)
    c = rng.integers(-20, 40, (500, 4)).astype(np.int32)
    c[:, :3] *= ts
    c[:, 3] = rng.integers(0, 3, 500)
    cand, kept = kept_candidates(c, st, ks, ts)
    m = max_candidates_per_row(st, ks)
    per_row = kept.sum(0)
    assert per_row.max() <= m and per_row.sum() > 0
    if (ts, ks, st) == (1, 3, 2):
        assert m == 8 and cand.shape[0] == 27 and per_row.max() == 8


def test_c_abi_entry_checks_its_arguments_on_the_host():
    """u2mkd_downsample_keys_general sizes a row's slots by m = prod ceil(kernel / stride): a caller whose buffer was sized by
    another m is refused before any launch (n = 0: nothing is launched, so this runs without a GPU)."""
    from u2mkd_amd import _lib as L
    args = lambda ks, st, m: (None, 0, 1, 1, 1) + ks + st + (None, m, None, None, None)
    L.call('u2mkd_downsample_keys_general', *args((3, 3, 3), (2, 2, 2), 8))
    L.call('u2mkd_downsample_keys_general', *args((3, 3, 3), (2, 2, 1), 12))
    with pytest.raises(RuntimeError, match='prod ceil'):
        L.call('u2mkd_downsample_keys_general', *args((3, 3, 3), (2, 2, 2), 27))
    with pytest.raises(RuntimeError, match='positive'):
        L.call('u2mkd_downsample_keys_general', *args((3, 3, 3), (2, 0, 2), 8))
