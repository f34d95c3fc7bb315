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


@pytest.mark.parametrize("F", [16, 32])
def test_route_sweep_from_the_fixture_to_random_bytes(hip, F):
    """the fixture's frames with k = 0 .. F of them replaced by random bytes: the verdict of dne_debug_ref_index equals the restatement of
    ref_dedup_pays / ref_dedup_fits (ref_dedup_support.pays) on the U1 / U2 it returns, is True at k = 0 and False at k = F.  At F = 16
    the k = 3 batch is the longest that takes the dedup route (tests/test_gpu_ref_dedup.py runs it): its slack in the dense route's y1 is
    below one step of k_conv2_ref_uniq, both its tables end in a segment shorter than steps_per_wg, and one more frame neither pays nor
    fits.  At F = 32 the verdict flips between k = 14 and k = 16 with room still positive at 14: there the cost decides, not the room."""
    rows = {}
    for k in range(F + 1):
        _, patches, _, windows, dedup = hip.debug_ref_index(S.mixed_frames(F, k))
        U1, U2 = patches.shape[0], windows.shape[0]
        rows[k] = (U1, U2, dedup)
        print("F=%d k=%2d: U1 = %5d, U2 = %4d, cost %.2f (dense %.2f), room %6d floats per member: %s"
              % (F, k, U1, U2, S.cost(F, U1, U2), S.MS_CONV1_DENSE + S.MS_CONV2_DENSE, S.room(F, U1, U2), "dedup" if dedup else "dense"))
        assert dedup == S.pays(F, U1, U2), (F, k, U1, U2)
    assert rows[0][2] and not rows[F][2]
    assert rows[F][:2] == (F * S.N1, F * S.N2)
    if F == 16:
        U1, U2, dedup = rows[3]
        assert (U1, U2) == (4060, 1416) and dedup
        assert abs(float(S.cost(F, U1, U2)) - 29.36) < 0.005
        assert (S.pad(U1, S.U1_PAD), S.pad(U2, S.U2_PAD)) == (4064, 1472)
        assert 0 <= S.room(F, U1, U2) == 768 < S.C2U_ROWS * 32                      # the slack is below one U2 step
        assert (4064 // S.C1U_ROWS, 1472 // S.C2U_ROWS) == (127, 23)                # 127 steps over segments of 32, 23 over segments of 16
        assert 127 % S.SPW1 and 23 % S.SPW2
        assert rows[4] == (4428, 1498, False)
        assert S.room(F, 4428, 1498) < 0 and not S.cost(F, 4428, 1498) < S.MS_CONV1_DENSE + S.MS_CONV2_DENSE   # neither fits nor pays
        assert not any(rows[k][2] for k in range(4, F + 1))
    else:
        assert rows[14][2] and S.room(F, *rows[14][:2]) > 0 and not rows[16][2]
        assert not any(rows[k][2] for k in range(16, F + 1))
