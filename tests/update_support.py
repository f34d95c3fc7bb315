"""TEST-ONLY support for the update path (csrc/reduce.h: k_centered_ranks, k_pair_weights, k_weighted_sum, k_adam / k_sgd, k_materialize,
k_ga_select): the reference's own lines restated in numpy, and the inputs both tests/test_update_cpu.py and tests/test_gpu_update.py run.

The restatements are written from es_distributed/es.py:70-85 (ranks), :281-298 (return processing, weighted sum, l2), :413-419 (theta +- v),
optimizers.py:10-50 (SGD, Adam, the ratio) and ga.py:145 (truncation selection) -- not from the kernels and not from the C oracle, which
test_update_cpu.py holds to them before the kernels are.  Every array operation is float32; every scalar is formed in Python doubles as the
reference writes it and cast ONCE (numpy >= 2 would otherwise promote the array to float64).

The order of returns is numpy's: every NaN sorts after +inf, NaNs among themselves by index, equal values by flat index."""
import math

import numpy as np

from maze_support import fmaf32, same_nan   # noqa: F401 (same_nan: re-exported for the two test files)

f32 = np.float32
DENORMAL = 1e-42            # a float32 denormal (the smallest normal is 1.18e-38)
T_LAST = 2 ** 31 - 2        # the largest step count dne_optimizer_set_state takes: the next step makes it 2^31 - 1
_CHUNK = 1 << 14


def same_bits(a, b):
    """equal shapes and equal float32 bits, the sign of a zero and the payload of a NaN included"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


# ---- es.py:70-85 -------------------------------------------------------------------------------------------------------------------------
def rank_ints(x):
    """es.py:76-77  ranks[x.argsort()] = arange(len(x)), with the sort that keeps equal values in index order"""
    x = np.asarray(x, np.float32).reshape(-1)
    ranks = np.empty(x.size, dtype=int)
    ranks[x.argsort(kind="stable")] = np.arange(x.size)
    return ranks


def ranks_np(x):
    """es.py:82-84  y = ranks.astype(float32); y /= (x.size - 1); y -= .5"""
    x = np.asarray(x, np.float32)
    y = rank_ints(x).reshape(x.shape).astype(np.float32)
    y = y / f32(x.size - 1)
    y = y - f32(0.5)
    assert y.dtype == np.float32
    return y


def is_rank_permutation(y):
    """round((y + 0.5) * (n - 1)) is a permutation of 0..n-1 (computed in float64 from the float32 ranks)"""
    y = np.asarray(y, np.float32).reshape(-1).astype(np.float64)
    n = y.size
    if np.any(np.isnan(y)):
        return False
    r = np.rint((y + 0.5) * (n - 1)).astype(np.int64)
    return bool(np.array_equal(np.sort(r), np.arange(n)))


# ---- es.py:281-298 -----------------------------------------------------------------------------------------------------------------------
def proc_np(returns_n2, signreturns_n2, mode):
    if mode == "centered_rank":
        return ranks_np(np.asarray(returns_n2, np.float32))
    if mode == "sign":
        return np.asarray(signreturns_n2, np.float32)
    if mode == "centered_sign_rank":
        return ranks_np(np.asarray(signreturns_n2, np.float32))
    raise NotImplementedError(mode)


def pair_weights_np(proc_n2):
    """es.py:292  proc_returns_n2[:, 0] - proc_returns_n2[:, 1]"""
    w = proc_n2[:, 0] - proc_n2[:, 1]
    assert w.dtype == np.float32
    return w


def weighted_chain_np(noise, idx, w, P):
    """per parameter the i-ordered chain acc = fmaf32(w[i], noise[idx[i] + p], acc) from +0, all p at once"""
    acc = np.zeros(P, np.float32)
    idx, w = np.asarray(idx, np.int64), np.asarray(w, np.float32)
    for p0 in range(0, P, _CHUNK):              # parameters are independent: a block of them at a time stays in the cache
        p1 = min(P, p0 + _CHUNK)
        a = acc[p0:p1]
        for i, wi in zip(idx, w):
            a = fmaf32(np.full(p1 - p0, wi, np.float32), noise[i + p0:i + p1], a)
        acc[p0:p1] = a
    return acc


def weighted_sum_np(noise, idx, w, P, denom, chain=None):
    """es.py:291-296: the chain, then ONE float32 division by float32(denom).  chain: weighted_chain_np of the same inputs, if at hand"""
    acc = weighted_chain_np(noise, idx, w, P) if chain is None else chain
    g = acc / f32(denom)
    assert g.dtype == np.float32
    return g


def weighted_terms_f64(noise, idx, w, P):
    """the same terms accumulated in float64: (sum_i w_i * noise_i, sum_i |w_i * noise_i|) per parameter"""
    s, mag = np.zeros(P), np.zeros(P)
    for i, wi in zip(np.asarray(idx, np.int64), np.asarray(w, np.float32)):
        t = float(wi) * noise[i:i + P].astype(np.float64)
        s += t
        mag += np.abs(t)
    return s, mag


def within_f64_bound(g, terms, n, denom):
    """|g - g64| <= (n + 2) * 2^-24 * sum_i |w_i * noise_i| / denom per parameter: n roundings of the chain (each at most 2^-24 of a partial
    sum, itself at most the sum of magnitudes, to first order), one of the division, one of float32(denom)"""
    s, mag = terms
    return bool(np.all(np.abs(np.asarray(g, np.float32).astype(np.float64) - s / float(denom)) <= (n + 2) * 2.0 ** -24 * mag / float(denom)))


# ---- optimizers.py:10-50 -----------------------------------------------------------------------------------------------------------------
def _ratio(step, theta_old):
    """optimizers.py:14  norm(step) / norm(theta), both sums of squares in float64"""
    ss = np.sum(np.square(step.astype(np.float64)))
    tt = np.sum(np.square(theta_old.astype(np.float64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sqrt(ss) / np.sqrt(tt))


def adam_np(theta, m, v, g, t, l2coeff, stepsize, beta1=0.9, beta2=0.999, epsilon=1e-08):
    """one Adam update with self.t == t (already incremented, optimizers.py:11) -> theta, m, v, ratio"""
    theta, m, v, g = (np.asarray(a, np.float32) for a in (theta, m, v, g))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        globalg = -g + f32(l2coeff) * theta                                                   # es.py:298
        a = stepsize * math.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)                           # optimizers.py:46, Python doubles
        m = f32(beta1) * m + f32(1 - beta1) * globalg                                         # :47
        v = f32(beta2) * v + f32(1 - beta2) * (globalg * globalg)                             # :48
        step = f32(-a) * m / (np.sqrt(v) + f32(epsilon))                                      # :49
        new = theta + step                                                                    # :15
    assert new.dtype == m.dtype == v.dtype == step.dtype == np.float32
    return new, m, v, _ratio(step, theta)


def sgd_np(theta, v, g, l2coeff, stepsize, momentum=0.9):
    theta, v, g = (np.asarray(a, np.float32) for a in (theta, v, g))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        globalg = -g + f32(l2coeff) * theta
        v = f32(momentum) * v + f32(1. - momentum) * globalg                                  # optimizers.py:30
        step = f32(-stepsize) * v                                                             # :31
        new = theta + step
    assert new.dtype == v.dtype == step.dtype == np.float32
    return new, v, _ratio(step, theta)


def ratio_close(got, want, P):
    """the kernel adds the P squares block by block, numpy pairwise: two orders of a double sum of P non-negative terms differ by at most
    P * 2^-52 relative.  inf equals inf (theta = 0, a step that is not) and NaN equals NaN (0 / 0)"""
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= P * 2.0 ** -52 * abs(want)


# ---- es.py:413-419, ga.py:145 ------------------------------------------------------------------------------------------------------------
def materialize_np(theta, noise, idx, sigma):
    """v = noise_stdev * noise.get(idx, P); rows 2i / 2i+1 = theta + v / theta - v"""
    theta = np.asarray(theta, np.float32)
    out = np.empty((len(idx), 2, theta.size), np.float32)
    for i, off in enumerate(np.asarray(idx, np.int64)):
        v = f32(sigma) * noise[off:off + theta.size]
        out[i, 0] = theta + v
        out[i, 1] = theta - v
    return out


def select_np(r, t):
    """the first t of the order (descending return, NaN greatest as numpy's partition has it, then arrival index).  A stable ascending sort
    of the REVERSED array puts equal values in descending original index; read backwards that is descending value, ascending index."""
    r = np.asarray(r, np.float32).reshape(-1)
    asc = (r.size - 1) - np.argsort(r[::-1], kind="stable")
    return asc[::-1][:t].astype(np.int32)


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------
RANK_NS = (2, 3, 255, 256, 257, 511, 512, 513, 1000, 4099)      # one value either side of one, two workgroups of 256; many blocks
SELECT_MS = (1, 2, 255, 256, 257, 513, 1000)
WS_NS_SMALL = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 250, 1001)   # every remainder of the 8-way unroll, and long chains
WS_NS_ES = (1, 7, 8, 9, 97)
MODES = ("centered_rank", "sign", "centered_sign_rank")
ADAM_SETS = (dict(stepsize=0.01, beta1=0.9, beta2=0.999, epsilon=1e-8, l2=0.005, zero_first=False),
             dict(stepsize=0.001, beta1=0.5, beta2=0.9, epsilon=1e-3, l2=0.0, zero_first=False),
             dict(stepsize=0.01, beta1=0.9, beta2=0.999, epsilon=0.0, l2=0.0, zero_first=True))    # first step 0 / (0 + 0)
SGD_MOMENTA = (0.0, 0.9, 0.99)
RESTORE_TS = (0, 1, 999, 100_000, T_LAST)
_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 3.4e38, -3.4e38, 1.0, -1.0, 1.1754944e-38], np.float32)


def _nan_sets(base):
    """base with NaNs planted: one, at index 0, at index n-1, at 255 / 256 (the last lane of a workgroup and the first of the next),
    every second value, all"""
    n = base.size
    out = []

    def put(name, where):
        x = base.copy()
        x[where] = np.nan
        out.append((name, x))
    put("nan_one", [n // 2])
    put("nan_first", [0])
    put("nan_last", [n - 1])
    if n > 256:
        put("nan_255_256", [255, 256])
        put("nan_256", [256])
    put("nan_every_second", np.arange(0, n, 2))
    put("nan_every_second_odd", np.arange(1, n, 2))
    put("nan_all", np.arange(n))
    return out


def rank_inputs(n):
    """[(name, float32[n])]; the names of the sets that hold a NaN start with 'nan'"""
    rs = np.random.RandomState(7000 + n)
    distinct = (rs.permutation(4 * n)[:n].astype(np.float32) - f32(2 * n)) * f32(0.25)        # exact in float32, no two equal
    ties = (10 * rs.poisson(20, n)).astype(np.float32)
    mix = _SPECIALS[rs.randint(0, _SPECIALS.size, n)]
    mix[:min(n, _SPECIALS.size)] = _SPECIALS[:min(n, _SPECIALS.size)]
    base = ties.copy()                                                                        # the NaN sets: ties, and infinities to sort NaN against
    base[rs.randint(0, n, max(1, n // 16))] = np.inf
    base[rs.randint(0, n, max(1, n // 16))] = -np.inf
    out = [("distinct", distinct), ("ties", ties), ("equal", np.full(n, 7.0, np.float32)),
           ("ascending", np.arange(n, dtype=np.float32)), ("descending", np.arange(n, 0, -1).astype(np.float32)), ("mix", mix)]
    return out + _nan_sets(base)


def select_inputs(m):
    rs = np.random.RandomState(8000 + m)
    ties = (10 * rs.poisson(2, m)).astype(np.float32)                                         # a handful of values: ties at and above every cut
    mix = _SPECIALS[rs.randint(0, 4, m)]                                                      # +-0 and +-inf only
    base = ties.copy()
    base[rs.randint(0, m, max(1, m // 16))] = np.inf
    base[rs.randint(0, m, max(1, m // 16))] = -np.inf
    return [("ties", ties), ("inf_zero", mix), ("equal", np.zeros(m, np.float32))] + _nan_sets(base)


def select_ts(m):
    return sorted({1, m} | ({m // 2} if m // 2 >= 1 else set()))


def _rank_weights(rs, n):
    """the centred-rank differences of a real return set of n pairs (never zero: no two ranks are equal)"""
    returns = (10 * rs.poisson(20, (n, 2))).astype(np.float32)
    return pair_weights_np(ranks_np(returns))


def ws_cases(n, P, noise_size, huge=True, spread=True):
    """[(name, idx int64[n], w float32[n])].  spread: random slices, with 0 and the last legal one.  struct: 0, the last, one repeated, slices one
    float apart, abutting slices; weights 0.0, -0.0 and a denormal in front of rank differences (in front: a zero weight at the end would
    hide a dropped tail).  huge: struct with 1e30 in the middle and -1e30 last.  (huge / spread False: without that set, where a chain over a
    million parameters would make the numpy side slow.)"""
    rs = np.random.RandomState(9000 + 13 * n + P % 1000)
    hi = noise_size - P
    assert 7 + 2 * P <= noise_size and hi - P >= 0
    rand = rs.randint(0, hi + 1, n).astype(np.int64)
    rand[0] = 0
    if n > 1:
        rand[-1] = hi
    w = _rank_weights(rs, n)
    pattern = [hi, 0, 5, 5, 6, 7, 7 + P, hi - P, 5]
    struct = np.concatenate([pattern, rs.randint(0, hi + 1, max(0, n - len(pattern)))])[:n].astype(np.int64)
    ws = w.copy()
    for k, val in enumerate((0.0, -0.0, DENORMAL)):
        if k < n - 1:
            ws[k] = val
    out = ([("spread", rand, w)] if spread else []) + [("struct", struct, ws)]
    if huge:
        wh = ws.copy()
        wh[n // 2] = 1e30
        wh[n - 1] = -1e30 if n > 1 else 1e30
        out.append(("huge", struct, wh))
    return out


def ws_denoms(n):
    return (1.0, float(2 * n), 3.0)


def update_case(P, noise_size, seed, n=257):
    """n = 257 pairs: 514 values, three workgroups of ranks, a ragged chain.  Sign-returns from {-3..3}: centered_sign_rank is almost all ties"""
    rs = np.random.RandomState(6000 + seed)
    idx = rs.randint(0, noise_size - P + 1, n).astype(np.int64)
    idx[0], idx[-1] = noise_size - P, 0
    returns = (10 * rs.poisson(20, (n, 2))).astype(np.float32)
    signs = rs.randint(-3, 4, (n, 2)).astype(np.float32)
    return idx, returns, signs


def horizon_case(P, noise_size, steps, seed, n=17):
    """fixed slices and fresh weights for every step: the rank differences of a fresh return set"""
    rs = np.random.RandomState(5000 + seed)
    idx = rs.randint(0, noise_size - P + 1, n).astype(np.int64)
    return idx, [_rank_weights(rs, n) for _ in range(steps)]


def start_theta(P, seed=0):
    return (np.random.RandomState(4000 + seed).randn(P) * 0.1).astype(np.float32)
