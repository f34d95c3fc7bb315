"""CPU: the premise of the streaming fc's dead rows (tests/test_gpu_dead_rows.py checks the kernels).  k_fc_sub and
k_fc_duo do not fetch a weight row whose activation relu(bn2(y2)) is +0 in BOTH members of an antithetic pair.  That pays only while a
good share of the 3872 rows is dead in both: on the Xavier start point with sigma = 0.02 the oracle gives 27 .. 31 % (each member alone:
49 %).  If this ever fails, the optimisation has nothing to skip on this workload."""
import numpy as np

import oracle as O
import step_tap_support as S

STEPS, SIGMA = 20, 0.02


def _activations(L, theta, ref, seed):
    """relu(bn2(y2)) of the member's first STEPS decisions on its own episode"""
    bn = O.es_ref_pass(L, theta, ref)
    env = O.WrappedEnv()
    ob = env.reset(seed)
    out = []
    for _ in range(STEPS):
        _, y2, _, logits = O.forward_debug(L, theta, bn, ob)
        out.append(S.activated_y2(y2, bn))
        ob, _, done = env.step(S.argmax_first(logits))
        assert not done
    return np.stack(out)


def test_three_in_ten_rows_are_dead_in_both_members_of_a_pair():
    L = O.layout(O.KIND_ES, S.NACT)
    th, noise, ref = S.base_theta(S.KIND_ES), S.small_noise(), S.ref_batch()
    seeds = S.tap_seeds(4)
    for p, idx in enumerate((11, 1_234_567)):
        plus = _activations(L, O.perturb(th, noise, idx, SIGMA, 1), ref, int(seeds[2 * p]))
        minus = _activations(L, O.perturb(th, noise, idx, SIGMA, -1), ref, int(seeds[2 * p + 1]))
        both = ((plus == 0) & (minus == 0)).mean(axis=1)   # per lock-step
        print("pair %d: rows dead in member + %.3f, in member - %.3f, in both min %.3f mean %.3f max %.3f"
              % (p, (plus == 0).mean(), (minus == 0).mean(), both.min(), both.mean(), both.max()))
        assert both.min() >= 0.20, (p, both.tolist())
