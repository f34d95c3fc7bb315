"""TEST-ONLY: the CPU oracle stepped one policy decision at a time, for the lock-step taps of tests/test_gpu_step_taps.py.

Inside an evaluation every policy head of the engine stores the member's fc output y3 (bias added, before batch norm / relu) and every
convolution path its y2; finished members are skipped afterwards, so after an evaluation each member's row holds the values of ITS last
lock-step.  oracle_last_step() gives the same values from the oracle: reference pass, reset, then T times forward_debug -> first-maximum
argmax -> env.step -- the loop of orc_rollout (oracle/dne_oracle.c) written out, which tests/test_step_tap_cpu.py pins to oracle.rollout.

Also here: the populations of the tap tests (module constants: the oracle side is worked out once per session and shared by every
regime) and the per-member parameter vectors of each engine kind."""
import functools

import numpy as np

import oracle as O

NACT, NREF = 18, 16
TAP_STEPS = (1, 3, 9)              # first lock-step of a burst, inside a burst, and (DNE_BURST=4) behind two compactions
NOISE_LEN = 4_000_000              # conftest.small_noise
KIND_ES, KIND_GA, KIND_GA_LARGE, KIND_ES_VBN = 0, 1, 2, 3
P_ES, P_GA, P_VBN = 1009058, 1008450, 1008450
LARGE_NOISE_LEN = 9_000_000        # big_noise of tests/test_gpu_large.py and tests/test_gpu_step_taps.py


def num_params(kind, nact=NACT):
    """P of a kind at an action-set width: the output layer is [256][nact] weights + nact biases (LargeModel: [512][nact] + nact), so P moves
    by 257 (513) per action; the rest of the flat vector does not depend on the width.  tests/test_step_tap_cpu.py holds these against
    oracle.layout and policies.flat_layout at every width the tests use."""
    if kind == KIND_GA_LARGE:
        return 4043424 + 513 * nact
    return (1004432 if kind == KIND_ES else 1003824) + 257 * nact


assert (num_params(KIND_ES), num_params(KIND_GA), num_params(KIND_ES_VBN)) == (P_ES, P_GA, P_VBN)


def tap_seeds(n):
    return ((np.arange(n, dtype=np.uint64) * 2654435761) % (1 << 32)).astype(np.uint32)


def edge_indices(P, N=NOISE_LEN):
    """11 pairs: every residue mod 4, 16-byte and 256-byte aligned starts, the first and the last legal slice, the same slice twice (equal
    keys in k_unit_order, rows shared inside a ring workgroup), slices one float apart, two slices that abut"""
    return np.array([0, 4, 64, 127, 1, 2, 3, 1_000_000, 1_000_000, 1_000_000 + P, N - P], np.int64)


def width_indices(n_pairs, P, N=NOISE_LEN):
    """random slices of the table, seeded by the width"""
    return np.random.RandomState(n_pairs).randint(0, N - P + 1, n_pairs).astype(np.int64)


WIDTHS = (2, 5, 9, 33, 65)         # pairs: one full ring workgroup (8 units); a partial last one + an odd count; 9; 66 and 130 members
MIN_SAMPLED = 16                   # members compared at 33 / 65 pairs, at least


def sampled_members(idx):
    """members to compare: all of them up to 11 pairs; above, both members of the first and the last pair and of the pairs with the lowest and
    the highest index (first and last unit of the table order), and a seeded sample of the rest -- MIN_SAMPLED members at least"""
    n = len(idx)
    if n <= 11:
        return list(range(2 * n))
    pairs = {0, n - 1, int(np.argmin(idx)), int(np.argmax(idx))}
    rest = [p for p in np.random.RandomState(n).permutation(n).tolist() if p not in pairs]
    pairs |= set(rest[:MIN_SAMPLED // 2 + 2 - len(pairs)])
    members = sorted(2 * p + s for p in pairs for s in (0, 1))
    assert len(members) >= MIN_SAMPLED
    return members


def argmax_first(x):
    """tf.argmax: index of the first maximum (argmax_first of dne_oracle.c)"""
    best = 0
    for i in range(1, len(x)):
        if x[i] > x[best]:
            best = i
    return best


def oracle_taps(L, theta_i, ref, env_seed, taps, large=False):
    """The oracle's episode of one member, stepped in Python up to max(taps) decisions.  ref: the reference batch (ES kinds: virtual batch norm
    from the reference pass of THIS member's vector) or None (GA kinds).  Returns {T: tap} for every T in taps, tap = dict(y=(y1, y2, y3[, y4])
    of the episode's LAST decision at or before step T, logits, bn (the reference pass's 608 floats or None), actions, ret, sign, length, ram=[length, 128]) -- for an episode that ends
    before T the values of its final step, as the engine's rows keep them."""
    theta_i = np.ascontiguousarray(theta_i, np.float32)
    bn = O.es_ref_pass(L, theta_i, ref) if ref is not None else None
    env = O.WrappedEnv()
    ob = env.reset(env_seed)
    out, acts, rams = {}, [], []
    ret, sign = np.float32(0.0), np.float32(0.0)
    last, done = None, False
    for t in range(1, max(taps) + 1):
        if not done:
            fw = O.forward_large_debug(L, theta_i, ob) if large else O.forward_debug(L, theta_i, bn, ob)
            a = argmax_first(fw[-1])
            ob, rew, done = env.step(a)
            acts.append(a); rams.append(env.ram())
            ret = np.float32(ret + np.float32(rew))                                  # es.py:425 rews.sum(), float32 like orc_rollout
            sign = np.float32(sign + np.float32((rew > 0) - (rew < 0)))
            last = fw
        if t in taps:
            out[t] = dict(y=last[:-1], logits=last[-1], bn=bn, actions=np.array(acts, np.int32), ret=float(ret), sign=float(sign),
                          length=len(acts), ram=np.array(rams, np.uint8).reshape(-1, O.RAM))
    return out


def oracle_last_step(L, theta_i, ref, env_seed, T, large=False):
    """(y1, y2, y3[, y4]), logits, actions, (return, sign-return, length) of the member's last decision within T steps"""
    tap = oracle_taps(L, theta_i, ref, env_seed, (T,), large)[T]
    return tap["y"], tap["logits"], tap["actions"], (tap["ret"], tap["sign"], tap["length"])


def activated_y2(y2, bn):
    """what the ring regime leaves in the y2 row: relu(bn2(y2)) as k_conv12 (act2) / k_y2_activate compute it -- multiply, then add, then the
    oracle's select t > 0 ? t : 0, two float32 roundings (bn: the member's 608 floats, scale2 at 32, shift2 at 64; channel = i % 32).
    The select sends NaN and -0 to +0 as bn_relu of oracle/dne_oracle.c does; np.maximum, which stood here before, hands NaN on.  On every
    t that is not a NaN the two are equal under np.array_equal, which is how the tests of finite values compare, so nothing they assert has
    moved (tests/test_value_edges_cpu.py holds this function to the oracle's bn_relu on NaN, +-inf, +-0, a subnormal and a NaN scale)."""
    y2 = np.asarray(y2, np.float32)
    c = np.arange(y2.size) & 31
    with np.errstate(invalid="ignore", over="ignore"):
        t = (y2 * bn[32 + c]).astype(np.float32)
        t = (t + bn[64 + c]).astype(np.float32)
        return np.where(t > 0, t, np.float32(0.0)).astype(np.float32)


# ---- base vectors and member vectors per engine kind ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_noise():
    """conftest.small_noise, for the cached oracle side below (the fixture's array is compared against it by the tests that use both)"""
    return np.random.RandomState(123).randn(NOISE_LEN).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ref_batch(nact):
    return O.get_ref_batch(seed=0, batch_size=NREF, nact=nact)


def ref_batch(nact=NACT):
    """the reference batch of a width: its frames come from random play over that width's actions (es.py:105-113)"""
    return _ref_batch(int(nact))


@functools.lru_cache(maxsize=None)
def _base_theta(kind, nact):
    if kind == KIND_ES:
        return O.es_init_theta(O.layout(O.KIND_ES, nact), 0)
    assert kind == KIND_ES_VBN
    from dne_hip import policies
    P = num_params(KIND_ES_VBN, nact)
    rs = np.random.RandomState(11)                      # a ModelVirtualBN start point moved off it so that every BatchNorm/b is nonzero
    return small_noise()[777:777 + P] * policies.vbn_scale_by(nact) + (0.01 * rs.randn(P)).astype(np.float32)


def base_theta(kind, nact=NACT):
    """the vector an engine of that kind and width gets with set_theta (native layout)"""
    return _base_theta(int(kind), int(nact))


def es_member_theta(kind, idx, scale, nact=NACT, noise=None):
    """member = base + fl(scale * noise[idx : idx + P]) in the kind's own layout, then (ModelVirtualBN) expanded onto the ES layout the oracle runs
    (noise: another table than small_noise())"""
    th = base_theta(kind, nact)
    v = (np.float32(scale) * (small_noise() if noise is None else noise)[idx:idx + th.size]).astype(np.float32)
    m = (th + v).astype(np.float32)
    if kind == KIND_ES_VBN:
        from vbn_support import expand
        m = expand(m, nact)
    return m


@functools.lru_cache(maxsize=None)
def _es_member_taps(kind, idx, scale, seed, nact):
    L = O.layout(O.KIND_ES, nact)
    return oracle_taps(L, es_member_theta(kind, idx, scale, nact), ref_batch(nact), seed, TAP_STEPS)


def es_member_taps(kind, idx, scale, seed, nact=NACT):
    """{T: tap} for T in TAP_STEPS of one ES / ES_VBN member, cached per width: the regimes share their populations"""
    return _es_member_taps(int(kind), int(idx), float(scale), int(seed), int(nact))


@functools.lru_cache(maxsize=None)
def _ga_member_taps(chain, sigma, seed, taps, nact):
    L = O.layout(O.KIND_GA, nact)
    return oracle_taps(L, O.ga_rebuild(L, small_noise(), list(chain), sigma), None, seed, taps)


def ga_member_taps(chain, sigma, seed, taps, nact=NACT):
    return _ga_member_taps(tuple(chain), float(sigma), int(seed), tuple(taps), int(nact))


# ---- GA (GAAtariPolicy): 7 fresh genomes, then 7 children of two of them; roots and mutation seeds from the edge set ------------------------
GA_SIGMA = 0.005
GA_TAP_STEPS = (1, 6)
def ga_gen0(nact=NACT):
    hi = NOISE_LEN - num_params(KIND_GA, nact)          # the last legal slice
    return [(0,), (hi,), (4,), (1_000_001,), (64,), (127,), (1_000_000,)]


def ga_mutations(nact=NACT):
    """first / last slice, a multiple of 4, odd, one seed for both parents, a slice that abuts another"""
    P = num_params(KIND_GA, nact)
    return (0, NOISE_LEN - P, 4, 1_000_001, 1_000_001, 3, 1_000_000 + P)


GA_GEN0 = ga_gen0()
GA_MUTATIONS = ga_mutations()
GA_SEEDS = (tap_seeds(14)[:7], tap_seeds(14)[7:])


def ga_gen1(nact=NACT):
    gen0, mut = ga_gen0(nact), ga_mutations(nact)
    parents = (gen0[1], gen0[3])
    return [parents[i % 2] + (mut[i],) for i in range(7)]


# ---- LargeModel: the genomes of test_large_model_taps ------------------------------------------------------------------------------------
LARGE_TAP_STEPS = (1, 3)


@functools.lru_cache(maxsize=None)
def big_noise():
    """first 9M entries of the reference noise stream (a LargeModel slice is 4.05M floats)"""
    return np.random.RandomState(123).randn(LARGE_NOISE_LEN).astype(np.float32)


def large_genomes(n, nact=NACT, noise_len=LARGE_NOISE_LEN):
    """n members: four roots (slice 0, the last legal slice, an odd and a 16-byte aligned start) unmutated, the rest their children with one
    mutation each (seeded indices, powers 0.002 / 0.004)"""
    hi = noise_len - num_params(KIND_GA_LARGE, nact)
    roots = [(0,), (hi,), (1_234_567,), (2_000_000,)]
    rs = np.random.RandomState(n)
    return roots + [roots[i % 4] + ((int(rs.randint(0, hi + 1)), 0.002 if i % 2 else 0.004),) for i in range(n - 4)]


@functools.lru_cache(maxsize=None)
def large_member_taps(n, m, nact=NACT):
    """{T: tap} for T in LARGE_TAP_STEPS of member m of large_genomes(n, nact) on episode tap_seeds(n)[m]"""
    from dne_hip import ga_gpu
    L = O.layout(O.KIND_GA_LARGE, nact)
    th = O.ga_gpu_rebuild(big_noise(), large_genomes(n, nact)[m], ga_gpu.model_scale_by(nact, KIND_GA_LARGE))
    return oracle_taps(L, th, None, int(tap_seeds(n)[m]), LARGE_TAP_STEPS, large=True)
