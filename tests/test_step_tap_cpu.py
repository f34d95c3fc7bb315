"""CPU: the step-by-step oracle loop behind the GPU lock-step taps (tests/step_tap_support.py) IS oracle.rollout -- same actions, return,
sign-return, length and RAM rows -- for every small engine kind, so that a wrong helper cannot make tests/test_gpu_step_taps.py vacuous.
Also: the tap populations do what the GPU tests assert of them (every episode alive at the last tapped step), at 18 actions and at the
widths of tests/test_gpu_action_widths.py, where the oracle's episodes also take every action of the short sets at least once."""
import numpy as np
import pytest

import step_tap_support as S
from step_tap_support import NACT, KIND_ES, KIND_ES_VBN


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def _check_against_rollout(O, L, th, ref, seed, T, es, nact=NACT):
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
    assert [a.shape for a in y] == [(7056,), (3872,), (256,)] and logits.shape == (nact,)
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


# ---- the widths of tests/test_gpu_action_widths.py ---------------------------------------------------------------------------------------
TAP_WIDTHS = (3, 4, 9, 17)          # its lock-step section: ES at all four, ModelVirtualBN / GA / LargeModel at 3 and 9
SHORT_WIDTHS = (3, 9)
ALL_WIDTHS = tuple(range(2, 19))    # its forward / flat-vector section


def _es_width_members(kind, nact):
    """(idx, scale, seed) of every member the GPU file compares at this kind and width: the 11 edge-index pairs, and (ES) 2 and 5 pairs"""
    P = S.num_params(kind, nact)
    pops = [(S.edge_indices(P), S.tap_seeds(22))]
    if kind == KIND_ES:
        pops += [(S.width_indices(w, P), S.tap_seeds(2 * w)) for w in (2, 5)]
    return [(int(idx[m // 2]), float(np.float32(0.02) if m % 2 == 0 else -np.float32(0.02)), int(seeds[m]))
            for idx, seeds in pops for m in range(2 * len(idx))]


@pytest.mark.parametrize("nact", ALL_WIDTHS)
def test_constants_are_the_layouts_at_every_width(O, nact):
    """P = 1004432 + 257 A (ES), 1003824 + 257 A (GA, ModelVirtualBN), 4043424 + 513 A (LargeModel): step_tap_support.num_params against the
    oracle's layout and the package's; the last legal slice of every population is N - P of ITS width"""
    from dne_hip import _lib, policies
    assert S.num_params(KIND_ES, nact) == 1004432 + 257 * nact == O.layout(O.KIND_ES, nact).P == policies.flat_layout(_lib.KIND_ES, nact)[1]
    assert S.num_params(S.KIND_GA, nact) == 1003824 + 257 * nact == O.layout(O.KIND_GA, nact).P == policies.flat_layout(_lib.KIND_GA, nact)[1]
    assert S.num_params(KIND_ES_VBN, nact) == 1003824 + 257 * nact == policies.flat_layout(_lib.KIND_ES_VBN, nact)[1]
    assert S.num_params(S.KIND_GA_LARGE, nact) == O.layout(O.KIND_GA_LARGE, nact).P == policies.flat_layout(_lib.KIND_GA_LARGE, nact)[1]
    assert S.KIND_GA_LARGE == _lib.KIND_GA_LARGE
    for kind in (KIND_ES, S.KIND_GA, KIND_ES_VBN):
        assert S.num_params(kind, nact) % 4 == nact % 4                 # the residues the widths are chosen for
    assert S.edge_indices(S.num_params(KIND_ES, nact)).max() + S.num_params(KIND_ES, nact) == S.NOISE_LEN
    assert max(c[0] for c in S.ga_gen0(nact)) + S.num_params(S.KIND_GA, nact) == S.NOISE_LEN
    assert max(g[0] for g in S.large_genomes(6, nact)) + S.num_params(S.KIND_GA_LARGE, nact) == S.LARGE_NOISE_LEN
    if nact in SHORT_WIDTHS:
        assert S.base_theta(KIND_ES_VBN, nact).size == S.num_params(KIND_ES_VBN, nact)
    if nact == NACT:
        assert S.ga_gen0(nact) == S.GA_GEN0 and S.ga_mutations(nact) == S.GA_MUTATIONS and S.ga_gen1(nact) == S.ga_gen1()


@pytest.mark.parametrize("nact", TAP_WIDTHS)
def test_helper_is_rollout_at_other_widths(O, small_noise, nact):
    """the pin of test_helper_is_rollout_es / _vbn / _ga / (LargeModel) at the widths of the GPU file: index 0 (+/-), the repeated slice and the
    last legal slice of that width"""
    from vbn_support import expand
    L = O.layout(O.KIND_ES, nact)
    T = max(S.TAP_STEPS)
    for kind in (KIND_ES, KIND_ES_VBN) if nact in SHORT_WIDTHS else (KIND_ES,):
        idx = S.edge_indices(S.num_params(kind, nact))
        seeds = S.tap_seeds(22)
        for m in (0, 1, 15, 21):
            sg = 1 if m % 2 == 0 else -1
            th = S.es_member_theta(kind, int(idx[m // 2]), float(sg * np.float32(0.02)), nact)
            want = O.perturb(S.base_theta(kind, nact), small_noise, idx[m // 2], 0.02, sg)
            assert np.array_equal(th, want if kind == KIND_ES else expand(want, nact))
            assert _check_against_rollout(O, L, th, S.ref_batch(nact), seeds[m], T, True, nact) == T
            tap = S.es_member_taps(kind, int(idx[m // 2]), float(sg * np.float32(0.02)), int(seeds[m]), nact)[T]
            r = O.rollout(L, th, S.ref_batch(nact), seeds[m], T, want_bc=True, want_actions=True)
            assert (tap["ret"], tap["sign"], tap["length"]) == r[:3] and np.array_equal(tap["ram"], r[3]) and np.array_equal(tap["actions"], r[4])
    if nact not in SHORT_WIDTHS:
        return
    Lg = O.layout(O.KIND_GA, nact)
    for chain, seed in zip(S.ga_gen0(nact)[:2] + S.ga_gen1(nact)[:2], S.GA_SEEDS[0][:2].tolist() + S.GA_SEEDS[1][:2].tolist()):
        th = O.ga_rebuild(Lg, S.small_noise(), list(chain), S.GA_SIGMA)
        assert _check_against_rollout(O, Lg, th, None, seed, max(S.GA_TAP_STEPS), False, nact) == max(S.GA_TAP_STEPS)
    from dne_hip import ga_gpu
    Ll = O.layout(O.KIND_GA_LARGE, nact)
    Tl = max(S.LARGE_TAP_STEPS)
    for m in (1, 5):                                            # the root on the last legal slice and a child
        th = O.ga_gpu_rebuild(S.big_noise(), S.large_genomes(6, nact)[m], ga_gpu.model_scale_by(nact, S.KIND_GA_LARGE))
        tap = S.large_member_taps(6, m, nact)[Tl]
        r = O.rollout(Ll, th, None, S.tap_seeds(6)[m], Tl, want_bc=True, want_actions=True)
        assert (tap["ret"], tap["sign"], tap["length"]) == r[:3] and np.array_equal(tap["ram"][-1], r[3]) and np.array_equal(tap["actions"], r[4])
        assert [a.shape for a in tap["y"]] == [(14112,), (7744,), (7744,), (512,)] and tap["logits"].shape == (nact,)


@pytest.mark.parametrize("nact", TAP_WIDTHS)
def test_tap_populations_reach_the_last_tapped_step_at_other_widths(O, nact):
    """lengths == T of the GPU file, for every member it compares: the ES populations at 3, 4, 9 and 17 actions; ModelVirtualBN, GA and
    LargeModel at 3 and 9"""
    T = max(S.TAP_STEPS)
    for kind in (KIND_ES, KIND_ES_VBN) if nact in SHORT_WIDTHS else (KIND_ES,):
        for idx, sc, seed in _es_width_members(kind, nact):
            assert S.es_member_taps(kind, idx, sc, seed, nact)[T]["length"] == T, (kind, nact, idx, sc)
    if nact not in SHORT_WIDTHS:
        return
    Tg = max(S.GA_TAP_STEPS)
    for gen, seeds in zip((S.ga_gen0(nact), S.ga_gen1(nact)), S.GA_SEEDS):
        for chain, seed in zip(gen, seeds):
            assert S.ga_member_taps(chain, S.GA_SIGMA, int(seed), S.GA_TAP_STEPS, nact)[Tg]["length"] == Tg, (nact, chain)
    for m in range(6):
        assert S.large_member_taps(6, m, nact)[max(S.LARGE_TAP_STEPS)]["length"] == max(S.LARGE_TAP_STEPS), (nact, m)


@pytest.mark.parametrize("kind,nact", [(KIND_ES, 3), (KIND_ES, 4), (KIND_ES, 9), (KIND_ES_VBN, 3), (KIND_ES_VBN, 9)])
def test_tapped_episodes_take_every_action_of_a_short_set(O, kind, nact):
    """over the 22 tapped episodes of a width the oracle's policy picks every action 0..A-1 at least once: every candidate lane of the
    speculative tail and of k_tail_step's fifth wave is adopted (and its outcome compared through the RAM trajectory) at least once; an
    argmax that could never reach some action fails there.  (The GA and LargeModel populations at 9 actions take 6 of the 9 in their 84 and
    18 decisions; at 3 actions all three.)"""
    T = max(S.TAP_STEPS)
    idx = S.edge_indices(S.num_params(kind, nact))
    seeds = S.tap_seeds(22)
    taken = set()
    for m in range(22):
        sc = np.float32(0.02) if m % 2 == 0 else -np.float32(0.02)
        tap = S.es_member_taps(kind, int(idx[m // 2]), float(sc), int(seeds[m]), nact)[T]
        assert tap["actions"].shape == (T,) and tap["ram"].shape == (T, 128)
        assert np.array_equal(tap["ram"][:, 38], tap["actions"])    # RAM byte 38: the action of the step's frames -- what the GPU file compares
        taken |= set(tap["actions"].tolist())
    assert taken == set(range(nact)), (kind, nact, sorted(taken))
    if nact == 3:
        ga = {a for gen, sd in zip((S.ga_gen0(3), S.ga_gen1(3)), S.GA_SEEDS) for c, s in zip(gen, sd)
              for a in S.ga_member_taps(c, S.GA_SIGMA, int(s), S.GA_TAP_STEPS, 3)[max(S.GA_TAP_STEPS)]["actions"].tolist()}
        large = {a for m in range(6) for a in S.large_member_taps(6, m, 3)[max(S.LARGE_TAP_STEPS)]["actions"].tolist()}
        assert ga == large == {0, 1, 2}, (ga, large)
