"""CPU: the numpy restatements of the update path (tests/update_support.py) against the C oracle bit for bit, against the goldens made by
the real es.py / optimizers.py, and against float64 -- so that tests/test_gpu_update.py can hold the kernels of csrc/reduce.h to them.
The inputs are update_support's case lists, the ones the GPU file runs."""
import numpy as np
import pytest

import update_support as U
from maze_support import maze_noise

SMALL = {"cartpole": 386, "maze": 498, "pendulum": 4481}


@pytest.fixture(scope="module")
def table():
    t = maze_noise()
    t.setflags(write=False)
    return t


def es_P(oracle, nact):
    return oracle.num_params(oracle.KIND_ES, nact)


# ---- ranks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", U.RANK_NS)
def test_ranks_equal_the_oracle_on_finite_input(oracle, n):
    for name, x in U.rank_inputs(n):
        if not name.startswith("nan"):
            want = U.ranks_np(x)
            assert U.is_rank_permutation(want), name
            assert U.same_bits(oracle.centered_ranks(x), want), name


@pytest.mark.parametrize("n", U.RANK_NS)
def test_ranks_equal_the_oracle_with_nan_returns(oracle, n):
    """the oracle's order is numpy's: NaN after +inf, NaNs by index"""
    for name, x in U.rank_inputs(n):
        if name.startswith("nan"):
            got = oracle.centered_ranks(x)
            assert U.is_rank_permutation(got), name
            assert U.same_bits(got, U.ranks_np(x)), name


@pytest.mark.parametrize("n", U.RANK_NS)
def test_ranks_np_is_the_reference_line_on_nan_input(n):
    """es.py:77 literally, and its property: every rank given once"""
    cases = [c for c in U.rank_inputs(n) if c[0].startswith("nan")]
    assert len(cases) >= 6
    for name, x in cases:
        assert np.isnan(x).any()
        ranks = np.empty(len(x), dtype=int)
        ranks[x.argsort(kind="stable")] = np.arange(len(x))
        assert np.array_equal(U.rank_ints(x), ranks), name
        assert np.array_equal(np.sort(ranks), np.arange(n)), name
        nan = np.isnan(x)
        assert np.array_equal(ranks[nan], n - nan.sum() + np.arange(nan.sum())), name          # the NaNs take the top ranks, in index order
        assert U.is_rank_permutation(U.ranks_np(x)), name


def test_the_issue_s_example():
    x = np.array([3, np.nan, 1, np.inf, np.nan, -np.inf, 1], np.float32)
    assert U.rank_ints(x).tolist() == [3, 5, 1, 4, 6, 0, 2]
    assert U.select_np(x, 3).tolist() == [1, 4, 3]
    assert U.select_np(x, 7).tolist() == [1, 4, 3, 0, 2, 6, 5]


def test_ranks_against_the_goldens(golden):
    x = golden["ranks_distinct_in"]
    assert U.same_bits(U.ranks_np(x), golden["ranks_distinct_out"])
    # tied returns, as tests/test_oracle_golden.py treats them: the reference's tie order is implementation-defined
    x = golden["ranks_tied_in"].reshape(-1)
    ref = golden["ranks_tied_out"].reshape(-1)
    y = U.ranks_np(x)
    assert np.array_equal(np.sort(y), np.sort(ref))
    for v in np.unique(x):
        m = x == v
        assert np.array_equal(np.sort(y[m]), np.sort(ref[m]))
        assert np.all(np.diff(y[m]) > 0)


# ---- weighted sum --------------------------------------------------------------------------------------------------------------------------
def check_weighted_sum(oracle, noise, P, n, small):
    for name, idx, w in U.ws_cases(n, P, noise.size, huge=small, spread=small):
        chain = U.weighted_chain_np(noise, idx, w, P)
        terms = U.weighted_terms_f64(noise, idx, w, P)
        for denom in U.ws_denoms(n):
            g = U.weighted_sum_np(noise, idx, w, P, denom, chain=chain)
            assert U.same_bits(g, oracle.weighted_sum(noise, idx, w, P, denom)), (name, denom)
            assert U.within_f64_bound(g, terms, n, denom), (name, denom)


@pytest.mark.parametrize("n", U.WS_NS_SMALL)
@pytest.mark.parametrize("kind", sorted(SMALL))
def test_weighted_sum_small(oracle, table, kind, n):
    check_weighted_sum(oracle, table, SMALL[kind], n, True)


@pytest.mark.parametrize("n", U.WS_NS_ES)
@pytest.mark.parametrize("nact", (18, 3))
def test_weighted_sum_es(oracle, small_noise, nact, n):
    check_weighted_sum(oracle, small_noise, es_P(oracle, nact), n, n <= 9)


def test_weighted_sum_cases_hold_what_they_name(table):
    P, hi = 498, table.size - 498
    for n in U.WS_NS_SMALL:
        cases = {name: (idx, w) for name, idx, w in U.ws_cases(n, P, table.size)}
        idx, w = cases["spread"]
        assert idx[0] == 0 and (n == 1 or idx[-1] == hi) and idx.max() <= hi and not np.any(w == 0)
        idx, w = cases["struct"]
        assert idx[0] == hi and w[-1] != 0
        if n >= 9:
            assert idx[2] == idx[3] and idx[4] == idx[3] + 1 and idx[6] == idx[5] + P and idx[7] + P == hi
            assert w[0] == 0 and not np.signbit(w[0]) and w[1] == 0 and np.signbit(w[1]) and 0 < w[2] < 1.1754944e-38
        idx, w = cases["huge"]
        assert np.abs(w).max() == np.float32(1e30) and abs(w[-1]) == np.float32(1e30)


# ---- optimizers ----------------------------------------------------------------------------------------------------------------------------
HORIZONS = (("maze", 40), ("pendulum", 12))


@pytest.mark.parametrize("k", range(len(U.ADAM_SETS)))
@pytest.mark.parametrize("kind,steps", HORIZONS)
def test_adam_over_a_horizon(oracle, table, kind, steps, k):
    P, hp = SMALL[kind], U.ADAM_SETS[k]
    idx, ws = U.horizon_case(P, table.size, steps, k)
    th0 = U.start_theta(P)
    th, m, v = th0.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32)
    opt = oracle.Adam(th0, hp["stepsize"], hp["beta1"], hp["beta2"], hp["epsilon"])
    for t, w in enumerate(ws, 1):
        if hp["zero_first"] and t == 1:
            w = np.zeros_like(w)
        g = U.weighted_sum_np(table, idx, w, P, 2 * len(idx))
        th, m, v, ratio = U.adam_np(th, m, v, g, t, hp["l2"], hp["stepsize"], hp["beta1"], hp["beta2"], hp["epsilon"])
        oratio, oth = opt.update(g, hp["l2"])
        assert U.same_nan(oth, th) and U.same_nan(opt.m, m) and U.same_nan(opt.v, v), t
        assert U.ratio_close(oratio, ratio, P), t
        if hp["zero_first"] and t == 1:
            assert np.all(np.isnan(th)) and np.isnan(ratio)          # 0 / (0 + 0) everywhere; the run goes on from the start vector
            th = th0.copy()
            opt.theta = th0.copy()
        else:
            assert U.same_bits(oth, th) and not np.any(np.isnan(th))
    assert not U.same_bits(th, th0)


@pytest.mark.parametrize("momentum", U.SGD_MOMENTA)
@pytest.mark.parametrize("kind,steps", HORIZONS)
def test_sgd_over_a_horizon(oracle, table, kind, steps, momentum):
    P = SMALL[kind]
    idx, ws = U.horizon_case(P, table.size, steps, 10)
    th0 = U.start_theta(P)
    th, v = th0.copy(), np.zeros(P, np.float32)
    opt = oracle.SGD(th0, 0.01, momentum)
    for t, w in enumerate(ws, 1):
        g = U.weighted_sum_np(table, idx, w, P, 2 * len(idx))
        th, v, ratio = U.sgd_np(th, v, g, 0.005, 0.01, momentum)
        oratio, oth = opt.update(g, 0.005)
        assert U.same_bits(oth, th) and U.same_bits(opt.v, v), t
        assert U.ratio_close(oratio, ratio, P), t
    assert not U.same_bits(th, th0)


@pytest.mark.parametrize("t", U.RESTORE_TS)
def test_adam_at_a_restored_step_count(oracle, table, t):
    """the bias correction a(t + 1) far from the start: float32(-a) is -stepsize itself from t = 100 000 on"""
    P = SMALL["maze"]
    idx, ws = U.horizon_case(P, table.size, 2, 20)
    rs = np.random.RandomState(t % 1000)
    th0, m0, v0 = U.start_theta(P), (rs.randn(P) * 1e-3).astype(np.float32), (rs.rand(P) * 1e-6).astype(np.float32)
    g = U.weighted_sum_np(table, idx, ws[0], P, 2 * len(idx))
    th, m, v, ratio = U.adam_np(th0, m0, v0, g, t + 1, 0.005, 0.01)
    opt = oracle.Adam(th0, 0.01)
    opt.m, opt.v, opt.t = m0.copy(), v0.copy(), t
    oratio, oth = opt.update(g, 0.005)
    assert opt.t == t + 1 and U.same_bits(oth, th) and U.same_bits(opt.m, m) and U.same_bits(opt.v, v)
    assert U.ratio_close(oratio, ratio, P)
    a = 0.01 * np.sqrt(1 - 0.999 ** (t + 1)) / (1 - 0.9 ** (t + 1))
    assert (np.float32(-a) == np.float32(-0.01)) == (t >= 100_000)


def test_ratio_of_a_zero_vector(oracle, table):
    """theta = 0: a step that is not zero gives inf, a zero step 0 / 0 -- numpy's division, and the oracle's"""
    P = SMALL["cartpole"]
    idx, ws = U.horizon_case(P, table.size, 1, 30)
    z = np.zeros(P, np.float32)
    g = U.weighted_sum_np(table, idx, ws[0], P, 2 * len(idx))
    for gg, want in ((g, np.inf), (z, np.nan)):
        th, v, ratio = U.sgd_np(z, z, gg, 0.005, 0.01, 0.9)
        assert U.ratio_close(ratio, want, P)
        oratio, oth = oracle.SGD(z, 0.01, 0.9).update(gg, 0.005)
        assert U.ratio_close(oratio, want, P) and U.same_bits(oth, th)
        th, m, v, ratio = U.adam_np(z, z, z, gg, 1, 0.005, 0.01)
        oratio, oth = oracle.Adam(z, 0.01).update(gg, 0.005)
        assert U.ratio_close(ratio, want, P) and U.ratio_close(oratio, want, P) and U.same_bits(oth, th)


def test_optimizers_against_the_goldens(golden):
    """within the bounds tests/test_oracle_golden.py holds the oracle to (the golden run computed Adam's step in float64)"""
    theta0, gs = golden["opt_theta0"], golden["opt_gs"]
    P = theta0.size
    for name in ("adam", "sgd"):
        th, m, v = theta0.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32)
        for t, g in enumerate(gs):
            if name == "adam":
                th, m, v, ratio = U.adam_np(th, m, v, g, t + 1, 0.005, 0.01)
            else:
                th, v, ratio = U.sgd_np(th, v, g, 0.005, 0.01, 0.9)
            ref = golden["opt_%s_thetas" % name][t]
            assert np.abs(th - ref).max() <= 1.5e-7 * max(1.0, np.abs(ref).max()) * 4
            assert abs(ratio - golden["opt_%s_ratios" % name][t]) <= 1e-5 * golden["opt_%s_ratios" % name][t]


# ---- whole updates -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("kind", ("cartpole", "maze"))
def test_whole_update(oracle, table, kind, mode):
    """es.py:281-298 from the restatements alone against the same lines from the oracle's pieces"""
    P = SMALL[kind]
    idx, returns, signs = U.update_case(P, table.size, U.MODES.index(mode))
    proc = U.proc_np(returns, signs, mode)
    src = {"centered_rank": returns, "sign": None, "centered_sign_rank": signs}[mode]
    oproc = signs if src is None else oracle.centered_ranks(src.reshape(-1)).reshape(-1, 2)
    assert U.same_bits(proc, oproc)
    if mode == "centered_sign_rank":
        assert np.unique(signs).size == 7                                           # 514 values, seven distinct: almost all ties
    w = U.pair_weights_np(proc)
    assert U.same_bits(w, oproc[:, 0] - oproc[:, 1])
    g = U.weighted_sum_np(table, idx, w, P, returns.size)
    assert U.same_bits(g, oracle.weighted_sum(table, idx, w, P, float(returns.size)))
    if mode == "centered_rank":
        assert U.same_bits(g, oracle.es_gradient(table, idx, returns, P))
    th0 = U.start_theta(P)
    z = np.zeros(P, np.float32)
    th, m, v, ratio = U.adam_np(th0, z, z, g, 1, 0.005, 0.01)
    oratio, oth = oracle.Adam(th0, 0.01).update(g, 0.005)
    assert U.same_bits(th, oth) and U.ratio_close(oratio, ratio, P)
    th, v, ratio = U.sgd_np(th0, z, g, 0.005, 0.01, 0.9)
    oratio, oth = oracle.SGD(th0, 0.01, 0.9).update(g, 0.005)
    assert U.same_bits(th, oth) and U.ratio_close(oratio, ratio, P)


# ---- materialize, selection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(SMALL))
def test_materialize(oracle, table, kind):
    P = SMALL[kind]
    th = U.start_theta(P)
    th[::7] = -0.0
    for n in (1, 2, 65):
        idx = np.random.RandomState(n).randint(0, table.size - P + 1, n).astype(np.int64)
        idx[0], idx[-1] = 0, table.size - P
        for sigma in (0.02, -0.02, 0.0):
            out = U.materialize_np(th, table, idx, sigma)
            for i in range(n):
                assert U.same_bits(out[i, 0], oracle.perturb(th, table, idx[i], sigma, 1)), (n, sigma, i)
                assert U.same_bits(out[i, 1], oracle.perturb(th, table, idx[i], sigma, -1)), (n, sigma, i)


def check_select(oracle, m, want_nan):
    seen = 0
    for name, r in U.select_inputs(m):
        if name.startswith("nan") != want_nan:
            continue
        seen += 1
        for t in U.select_ts(m):
            want = U.select_np(r, t)
            assert len(set(want.tolist())) == t, (name, t)
            assert np.array_equal(oracle.ga_select(r, t), want), (name, t)
            # ga.py:145 as written returns the same returns (which of two equal candidates it takes is left open)
            ref = np.argpartition(r, (-t, -1))[-1:-t - 1:-1]
            assert U.same_nan(np.sort(r[ref] + np.float32(0)), np.sort(r[want] + np.float32(0))), (name, t)   # (+ 0: a zero's sign is not ordered)
            assert U.same_nan(r[ref[:1]] + np.float32(0), r[want[:1]] + np.float32(0)), (name, t)                   # ga.py:149: the first is the maximum
    assert seen >= 3


@pytest.mark.parametrize("m", U.SELECT_MS)
def test_select_equals_the_oracle_on_finite_input(oracle, m):
    check_select(oracle, m, False)


@pytest.mark.parametrize("m", U.SELECT_MS)
def test_select_equals_the_oracle_with_nan_returns(oracle, m):
    check_select(oracle, m, True)
