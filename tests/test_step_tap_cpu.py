"""CPU: the step-by-step oracle loop behind the GPU lock-step taps (tests/step_tap_support.py) IS oracle.rollout -- same actions, return,
sign-return, length and RAM rows -- for every small engine kind, so that a wrong helper cannot make tests/test_gpu_step_taps.py vacuous.
Also: the tap populations do what the GPU tests assert of them (every episode alive at the last tapped step)."""
import numpy as np
import pytest

import step_tap_support as S
from step_tap_support import NACT, KIND_ES, KIND_ES_VBN


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def _check_against_rollout(O, L, th, ref, seed, T, es):
    y, logits, actions, (ret, sign, length) = S.oracle_last_step(L, th, ref, seed, T)
    tap = S.oracle_taps(L, th, ref, seed, (T,))[T]
    r, s, l, bc, acts = O.rollout(L, th, ref, seed, T, want_bc=True, want_actions=True)
    assert (ret, sign, length) == (r, s, l)
    assert np.array_equal(actions, acts) and len(acts) == l
    if es:
        assert np.array_equal(tap["ram"], bc)                  # one RAM row per step
    else:
        assert np.array_equal(tap["ram"][-1], bc)              # GA: the final RAM
    # the tapped values are the forward pass of the observation the last action was chosen from
    assert int(np.argmax(logits)) == acts[-1] == S.argmax_first(logits)
    assert [a.shape for a in y] == [(7056,), (3872,), (256,)] and logits.shape == (NACT,)
    return l


@pytest.mark.parametrize("T", [1, 2, 12])
def test_helper_is_rollout_es(O, small_noise, T):
    assert np.array_equal(small_noise, S.small_noise())
    L = O.layout(O.KIND_ES, NACT)
    idx = S.edge_indices(S.P_ES)
    seeds = S.tap_seeds(22)
    for m in (0, 1, 15, 21):                                    # index 0 (+/-), the repeated slice, the last legal slice
        sc = np.float32(0.02) if m % 2 == 0 else -np.float32(0.02)
        th = S.es_member_theta(KIND_ES, int(idx[m // 2]), float(sc))
        assert np.array_equal(th, O.perturb(S.base_theta(KIND_ES), small_noise, idx[m // 2], 0.02, 1 if m % 2 == 0 else -1))
        assert _check_against_rollout(O, L, th, S.ref_batch(), seeds[m], T, True) == T


@pytest.mark.parametrize("T", [1, 2, 12])
def test_helper_is_rollout_vbn(O, T):
    from vbn_support import expand
    L = O.layout(O.KIND_ES, NACT)
    idx = S.edge_indices(S.P_VBN)
    seeds = S.tap_seeds(22)
    for m in (2, 21):
        sc = np.float32(0.02) if m % 2 == 0 else -np.float32(0.02)
        th = S.es_member_theta(KIND_ES_VBN, int(idx[m // 2]), float(sc))
        assert np.array_equal(th, expand(O.perturb(S.base_theta(KIND_ES_VBN), S.small_noise(), idx[m // 2], 0.02, 1 if m % 2 == 0 else -1), NACT))
        assert _check_against_rollout(O, L, th, S.ref_batch(), seeds[m], T, True) == T


@pytest.mark.parametrize("T", [1, 2, 12])
def test_helper_is_rollout_ga(O, T):
    L = O.layout(O.KIND_GA, NACT)
    for chain, seed in zip(S.GA_GEN0[:2] + S.ga_gen1()[:2], S.GA_SEEDS[0][:2].tolist() + S.GA_SEEDS[1][:2].tolist()):
        th = O.ga_rebuild(L, S.small_noise(), list(chain), S.GA_SIGMA)
        assert _check_against_rollout(O, L, th, None, seed, T, False) == T


def test_helper_on_an_episode_that_ends_before_T(O, small_noise):
    """idx 42, the -sigma member, seed 9 * 2654435761 mod 2^32 (the last member of test_every_step_kernel_variant_is_bit_exact): game over at
    step 110; the tap then holds the values of step 110, as the engine's rows do (finished members are skipped)"""
    L = O.layout(O.KIND_ES, NACT)
    th = S.es_member_theta(KIND_ES, 42, float(-np.float32(0.02)))
    seed = S.tap_seeds(10)[9]
    assert _check_against_rollout(O, L, th, S.ref_batch(), seed, 120, True) == 110
    taps = S.oracle_taps(L, th, S.ref_batch(), seed, (110, 120))
    assert taps[110]["length"] == taps[120]["length"] == 110
    assert all(np.array_equal(a, b) for a, b in zip(taps[110]["y"], taps[120]["y"]))


def test_tap_populations_reach_the_last_tapped_step(O):
    """what the GPU tests assert as lengths == T: every compared episode of every population is alive at step max(TAP_STEPS)"""
    T = max(S.TAP_STEPS)
    for kind, P in ((KIND_ES, S.P_ES), (KIND_ES_VBN, S.P_VBN)):
        idx = S.edge_indices(P)
        for sigma, seeds in ((0.02, S.tap_seeds(22)), (0.05, S.tap_seeds(22)), (0.0, np.repeat(S.tap_seeds(11), 2))):
            for m in range(22):
                sc = np.float32(sigma) if m % 2 == 0 else -np.float32(sigma)
                assert S.es_member_taps(kind, int(idx[m // 2]), float(sc), int(seeds[m]))[T]["length"] == T, (kind, sigma, m)
    for w in S.WIDTHS:
        idx = S.width_indices(w, S.P_ES)
        seeds = S.tap_seeds(2 * w)
        for m in S.sampled_members(idx):
            sc = np.float32(0.02) if m % 2 == 0 else -np.float32(0.02)
            assert S.es_member_taps(KIND_ES, int(idx[m // 2]), float(sc), int(seeds[m]))[T]["length"] == T, (w, m)
    for gen, seeds in zip((S.GA_GEN0, S.ga_gen1()), S.GA_SEEDS):
        for chain, seed in zip(gen, seeds):
            assert S.ga_member_taps(tuple(chain), S.GA_SIGMA, int(seed), S.GA_TAP_STEPS)[max(S.GA_TAP_STEPS)]["length"] == max(S.GA_TAP_STEPS)


def test_constants_are_the_layouts(O, small_noise):
    """N - P is the last legal slice only while these are the layouts' sizes"""
    from dne_hip import _lib, policies
    assert S.NOISE_LEN == small_noise.size
    assert S.P_ES == O.layout(O.KIND_ES, NACT).P == policies.flat_layout(_lib.KIND_ES, NACT)[1]
    assert S.P_GA == O.layout(O.KIND_GA, NACT).P == policies.flat_layout(_lib.KIND_GA, NACT)[1]
    assert S.P_VBN == policies.flat_layout(_lib.KIND_ES_VBN, NACT)[1] == S.base_theta(KIND_ES_VBN).size
    assert (S.KIND_ES, S.KIND_GA, S.KIND_ES_VBN) == (_lib.KIND_ES, _lib.KIND_GA, _lib.KIND_ES_VBN)
    assert S.edge_indices(S.P_ES).max() + S.P_ES == S.NOISE_LEN and max(c[0] for c in S.GA_GEN0) + S.P_GA == S.NOISE_LEN


def test_sampling_rule():
    for w in S.WIDTHS:
        idx = S.width_indices(w, S.P_ES)
        mem = S.sampled_members(idx)
        if w <= 11:
            assert mem == list(range(2 * w))
        else:
            assert len(mem) >= S.MIN_SAMPLED and len(set(mem)) == len(mem)
            for p in (0, w - 1, int(np.argmin(idx)), int(np.argmax(idx))):
                assert 2 * p in mem and 2 * p + 1 in mem


def test_activated_y2_is_two_roundings():
    rs = np.random.RandomState(0)
    y2 = rs.randn(3872).astype(np.float32)
    bn = rs.randn(608).astype(np.float32)
    a = S.activated_y2(y2, bn)
    c = np.arange(3872) % 32
    # an independent form: the exact float64 product rounded to float32, then the float64 sum of two float32 rounded to float32
    prod = (y2.astype(np.float64) * bn[32 + c].astype(np.float64)).astype(np.float32)
    want = np.maximum((prod.astype(np.float64) + bn[64 + c].astype(np.float64)).astype(np.float32), np.float32(0))
    assert a.dtype == np.float32 and np.array_equal(a, want)
    fused = np.maximum((y2.astype(np.float64) * bn[32 + c] + bn[64 + c]).astype(np.float32), 0)   # one rounding: what it must NOT be
    assert not np.array_equal(a, fused)
