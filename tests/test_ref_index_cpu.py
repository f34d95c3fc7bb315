"""The reference batch as unique convolution operands (csrc/ref_index.h through dne_debug_ref_index, no GPU) against numpy:

  * U1 and U2 equal the np.unique counts of the conv1 patches / the conv2 windows;
  * the patch table indexed by idx1 reproduces the im2col of the zero-padded frames byte for byte;
  * the windows indexed by idx2 reproduce each position's sixteen conv1 ids, -1 exactly on the SAME padding;
  * an all-zero batch has one patch (a padding zero equals a pixel zero), a random batch has none in common;
  * the route: the oracle's frames take the dedup route, random bytes the dense one."""
import time

import numpy as np
import pytest

import ref_dedup_support as S


@pytest.fixture(scope="module")
def hip(oracle):
    from dne_hip import _lib
    return _lib


def _check(hip, ref):
    idx1, patches, idx2, windows, dedup = hip.debug_ref_index(ref)
    F = ref.shape[0]
    cols = S.im2col1(ref)
    U1 = np.unique(cols.reshape(-1, 256), axis=0).shape[0]
    assert patches.shape == (U1, 256)
    assert idx1.min() >= 0 and idx1.max() == U1 - 1
    assert np.array_equal(patches[idx1], cols)
    want = S.windows2(idx1)
    U2 = np.unique(want.reshape(-1, 16), axis=0).shape[0]
    assert windows.shape == (U2, 16)
    assert idx2.min() >= 0 and idx2.max() == U2 - 1
    assert np.array_equal(windows[idx2], want)
    assert np.array_equal(windows[idx2] < 0, np.broadcast_to(S.padding_mask2(), (F, S.N2, 16)))
    assert len(np.unique(idx1)) == U1 and len(np.unique(idx2)) == U2      # every table row is used
    return U1, U2, dedup


@pytest.mark.parametrize("seed", [0, 1])
def test_fixture_frames(hip, seed):
    U1, U2, dedup = _check(hip, S.fixture_frames(16, seed))
    print("F=16 seed %d: U1/N1 = %d/%d, U2/N2 = %d/%d" % (seed, U1, 16 * S.N1, U2, 16 * S.N2))
    assert dedup


def test_full_batch_counts_and_cost(hip):
    ref = S.fixture_frames(128, 0)
    U1, U2, dedup = _check(hip, ref)
    print("F=128 seed 0: U1/N1 = %d/%d, U2/N2 = %d/%d" % (U1, 128 * S.N1, U2, 128 * S.N2))
    assert dedup
    t0 = time.perf_counter()
    hip.debug_ref_index(ref)
    print("dne_debug_ref_index at F=128: %.1f ms" % (1e3 * (time.perf_counter() - t0)))


def test_all_zero_batch_is_one_patch(hip):
    U1, U2, dedup = _check(hip, np.zeros((16, 84, 84, 4), np.uint8))
    assert U1 == 1 and dedup
    assert U2 == 9                                   # the windows differ only by where their padding lies: 3 x 3 kinds


def test_flat_batch_is_a_handful(hip):
    U1, U2, dedup = _check(hip, S.flat_frames(16))
    assert U1 == 9 and dedup


def test_random_batch_has_nothing_to_share(hip):
    U1, U2, dedup = _check(hip, S.random_frames(16))
    assert U1 == 16 * S.N1 and U2 == 16 * S.N2 and not dedup


def test_odd_table_sizes(hip):
    U1, U2, dedup = _check(hip, S.odd_frames(16))
    assert U1 % 16 and U2 % 16 and dedup
