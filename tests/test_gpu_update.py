"""GPU: the update path of every engine kind (csrc/reduce.h: k_centered_ranks, k_pair_weights, k_weighted_sum, k_adam / k_sgd,
k_materialize, k_ga_select) against the reference's lines restated in numpy (tests/update_support.py; tests/test_update_cpu.py holds
those to the oracle, the goldens and float64 first).  Every comparison is bit for bit unless it says otherwise.  Shapes: either side of
one and two workgroups of 256, every remainder of the weighted sum's 8-way unroll, parameter counts with a ragged last block (386, 498,
4481, 1 009 058 and the odd count of 3 actions), three return-processing modes, both optimizers over a horizon and at restored step
counts up to the last one an int32 holds, and returns with NaN among them (numpy's order: NaN after +inf, NaNs by index)."""
import numpy as np
import pytest

import update_support as U
from maze_support import maze_noise

pytestmark = pytest.mark.gpu
SMALL = {"cartpole": 386, "maze": 498, "pendulum": 4481}
HORIZONS = (("maze", 40), ("pendulum", 12))


@pytest.fixture(scope="module")
def table():
    t = maze_noise()
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def engines(table, small_noise):
    """engine by name, each made once at its first use; all closed with the module"""
    from dne_hip import _lib
    made = {}

    def get(name):
        if name not in made:
            if name == "cartpole":
                e = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=4)
            elif name == "maze":
                e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=4)
            elif name == "pendulum":
                e = _lib.Engine(_lib.KIND_PENDULUM, 1, max_members=4, hidden=64, ac_mode="continuous", nonlin="tanh")
            else:
                e = _lib.Engine(_lib.KIND_ES, int(name[2:]), max_members=8, ref_count=16)
            e.noise_upload(small_noise if name.startswith("es") else table)
            e.set_theta(U.start_theta(e.P))
            assert e.P == SMALL.get(name, e.P)
            made[name] = e
        return made[name]
    get.made = made
    yield get
    for e in made.values():
        e.close()


# ---- ranks ---------------------------------------------------------------------------------------------------------------------------------
def check_ranks(e, n, want_nan):
    seen = 0
    for name, x in U.rank_inputs(n):
        if name.startswith("nan") != want_nan:
            continue
        seen += 1
        got = e.centered_ranks(x)
        assert U.is_rank_permutation(got), name
        assert U.same_bits(got, U.ranks_np(x)), name
    assert seen >= 6


@pytest.mark.parametrize("n", U.RANK_NS)
def test_ranks_finite(engines, n):
    check_ranks(engines("cartpole"), n, False)


@pytest.mark.parametrize("n", U.RANK_NS)
def test_ranks_with_nan_returns(engines, n):
    check_ranks(engines("cartpole"), n, True)


# ---- weighted sum --------------------------------------------------------------------------------------------------------------------------
def check_weighted_sum(e, noise, n, small):
    P = e.P
    for name, idx, w in U.ws_cases(n, P, noise.size, huge=small, spread=small):
        chain = U.weighted_chain_np(noise, idx, w, P)
        terms = U.weighted_terms_f64(noise, idx, w, P)
        for denom in U.ws_denoms(n):
            g = e.weighted_sum(idx, w, denom)
            assert U.same_bits(g, U.weighted_sum_np(noise, idx, w, P, denom, chain=chain)), (name, denom)
            assert U.within_f64_bound(g, terms, n, denom), (name, denom)


@pytest.mark.parametrize("n", U.WS_NS_SMALL)
@pytest.mark.parametrize("kind", sorted(SMALL))
def test_weighted_sum_small(engines, table, kind, n):
    check_weighted_sum(engines(kind), table, n, True)


@pytest.mark.parametrize("n", U.WS_NS_ES)
@pytest.mark.parametrize("nact", (18, 3))
def test_weighted_sum_es(engines, small_noise, nact, n):
    e = engines("es%d" % nact)
    assert e.P == {18: 1009058, 3: 1005203}[nact]
    check_weighted_sum(e, small_noise, n, n <= 9)


# ---- whole updates -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ("adam", "sgd"))
@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("kind", ("cartpole", "maze"))
def test_whole_update(engines, table, kind, mode, opt):
    """257 pairs through dne_es_update, and the same through dne_records_set + dne_es_update_gathered"""
    from dne_hip import _lib
    e = engines(kind)
    P = e.P
    idx, returns, signs = U.update_case(P, table.size, U.MODES.index(mode))
    g = U.weighted_sum_np(table, idx, U.pair_weights_np(U.proc_np(returns, signs, mode)), P, returns.size)
    th0, z = U.start_theta(P), np.zeros(P, np.float32)
    if opt == "adam":
        th, m, v, ratio = U.adam_np(th0, z, z, g, 1, 0.005, 0.01)
    else:
        th, v, ratio = U.sgd_np(th0, z, g, 0.005, 0.01, 0.9)
        m = z
    rec = np.zeros(len(idx), _lib.RECORD)
    rec["noise_idx"], rec["ret"], rec["aux"] = idx, returns, signs
    for route in ("direct", "gathered"):
        e.set_theta(th0); e.optimizer_reset()
        if route == "direct":
            got = e.es_update(idx, returns, signs, mode, opt, 0.005, 0.01)
        else:
            e.records_set(rec)
            got = e.es_update_gathered(mode, opt, 0.005, 0.01)
        gm, gv, gt = e.optimizer_get_state()
        assert U.same_bits(e.get_theta(), th) and U.same_bits(gm, m) and U.same_bits(gv, v) and gt == 1, route
        assert U.ratio_close(got, ratio, P), (route, got, ratio)
    assert not U.same_bits(th, th0)


# ---- optimizers over a horizon ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(U.ADAM_SETS)))
@pytest.mark.parametrize("kind,steps", HORIZONS)
def test_adam_over_a_horizon(engines, table, kind, steps, k):
    e, hp = engines(kind), U.ADAM_SETS[k]
    P = e.P
    idx, ws = U.horizon_case(P, table.size, steps, k)
    th0 = U.start_theta(P)
    th, m, v = th0.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32)
    e.set_theta(th0); e.optimizer_reset()
    for t, w in enumerate(ws, 1):
        if hp["zero_first"] and t == 1:
            w = np.zeros_like(w)
        th, m, v, ratio = U.adam_np(th, m, v, U.weighted_sum_np(table, idx, w, P, 2 * len(idx)), t, hp["l2"], hp["stepsize"], hp["beta1"],
                                    hp["beta2"], hp["epsilon"])
        assert e.weighted_sum(idx, w, 2 * len(idx), copy_out=False) is None           # g stays on the device
        got = e.optimizer_step("adam", hp["l2"], hp["stepsize"], hp["beta1"], hp["beta2"], hp["epsilon"])
        gm, gv, gt = e.optimizer_get_state()
        if hp["zero_first"] and t == 1:
            assert np.all(np.isnan(th)) and np.isnan(ratio)                           # 0 / (0 + 0) on both sides
            assert U.same_nan(e.get_theta(), th) and U.same_nan(gm, m) and U.same_nan(gv, v) and gt == t
            th = th0.copy()                                                           # the run goes on from the start vector
            e.set_theta(th0)
        else:
            assert U.same_bits(e.get_theta(), th) and U.same_bits(gm, m) and U.same_bits(gv, v) and gt == t, t
        assert U.ratio_close(got, ratio, P), (t, got, ratio)
    assert not np.any(np.isnan(th)) and not U.same_bits(th, th0)


@pytest.mark.parametrize("momentum", U.SGD_MOMENTA)
@pytest.mark.parametrize("kind,steps", HORIZONS)
def test_sgd_over_a_horizon(engines, table, kind, steps, momentum):
    e = engines(kind)
    P = e.P
    idx, ws = U.horizon_case(P, table.size, steps, 10)
    th0 = U.start_theta(P)
    th, v = th0.copy(), np.zeros(P, np.float32)
    e.set_theta(th0); e.optimizer_reset()
    for t, w in enumerate(ws, 1):
        th, v, ratio = U.sgd_np(th, v, U.weighted_sum_np(table, idx, w, P, 2 * len(idx)), 0.005, 0.01, momentum)
        e.weighted_sum(idx, w, 2 * len(idx), copy_out=False)
        got = e.optimizer_step("sgd", 0.005, 0.01, momentum)
        gm, gv, gt = e.optimizer_get_state()
        assert U.same_bits(e.get_theta(), th) and U.same_bits(gv, v) and not gm.any() and gt == t, t
        assert U.ratio_close(got, ratio, P), (t, got, ratio)
    assert not U.same_bits(th, th0)


@pytest.mark.parametrize("t", U.RESTORE_TS)
@pytest.mark.parametrize("kind", ("maze", "pendulum"))
def test_adam_at_a_restored_step_count(engines, table, kind, t):
    """dne_optimizer_set_state(m, v, t), one step, against adam_np at t + 1: the bias correction far from the start"""
    e = engines(kind)
    P = e.P
    idx, ws = U.horizon_case(P, table.size, 2, 20)
    rs = np.random.RandomState(t % 1000)
    th0, m0, v0 = U.start_theta(P), (rs.randn(P) * 1e-3).astype(np.float32), (rs.rand(P) * 1e-6).astype(np.float32)
    th, m, v, ratio = U.adam_np(th0, m0, v0, U.weighted_sum_np(table, idx, ws[0], P, 2 * len(idx)), t + 1, 0.005, 0.01)
    e.set_theta(th0)
    e.optimizer_set_state(m0, v0, t)
    gm, gv, gt = e.optimizer_get_state()
    assert U.same_bits(gm, m0) and U.same_bits(gv, v0) and gt == t
    e.weighted_sum(idx, ws[0], 2 * len(idx), copy_out=False)
    got = e.optimizer_step("adam", 0.005, 0.01)
    gm, gv, gt = e.optimizer_get_state()
    assert U.same_bits(e.get_theta(), th) and U.same_bits(gm, m) and U.same_bits(gv, v) and gt == t + 1
    assert U.ratio_close(got, ratio, P), (got, ratio)


def test_set_state_refuses_the_last_int32(engines):
    """t = 2^31 - 1 would overflow at the next step's t += 1: refused by name, and the state stays what it was"""
    from dne_hip import _lib
    e = engines("maze")
    P = e.P
    m0, v0 = np.full(P, 0.25, np.float32), np.full(P, 0.5, np.float32)
    e.optimizer_set_state(m0, v0, 7)
    with pytest.raises(_lib.DneError, match="dne_optimizer_set_state"):
        e.optimizer_set_state(np.zeros(P, np.float32), np.zeros(P, np.float32), 2 ** 31 - 1)
    with pytest.raises(_lib.DneError):
        e.optimizer_set_state(m0, v0, -1)
    gm, gv, gt = e.optimizer_get_state()
    assert U.same_bits(gm, m0) and U.same_bits(gv, v0) and gt == 7
    e.optimizer_set_state(m0, v0, U.T_LAST)
    assert e.optimizer_get_state()[2] == 2 ** 31 - 2


@pytest.mark.parametrize("kind", sorted(SMALL))
def test_ratio_of_a_zero_vector(engines, table, kind):
    """theta = 0: a step that is not zero gives inf, a zero step 0 / 0 -- as numpy's division does"""
    e = engines(kind)
    P = e.P
    idx, ws = U.horizon_case(P, table.size, 1, 30)
    z = np.zeros(P, np.float32)
    for w, want in ((ws[0], np.inf), (np.zeros_like(ws[0]), np.nan)):
        g = U.weighted_sum_np(table, idx, w, P, 2 * len(idx))
        for opt in ("sgd", "adam"):
            if opt == "sgd":
                th, v, ratio = U.sgd_np(z, z, g, 0.005, 0.01, 0.9)
            else:
                th, m, v, ratio = U.adam_np(z, z, z, g, 1, 0.005, 0.01)
            assert U.ratio_close(ratio, want, P)
            e.set_theta(z); e.optimizer_reset()
            e.weighted_sum(idx, w, 2 * len(idx), copy_out=False)
            got = e.optimizer_step(opt, 0.005, 0.01)
            assert U.ratio_close(got, want, P), (opt, got, want)
            assert U.same_bits(e.get_theta(), th), opt


# ---- materialize, selection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(SMALL))
def test_materialize(engines, table, kind):
    e = engines(kind)
    P = e.P
    th = U.start_theta(P)
    th[::7] = -0.0
    e.set_theta(th)
    for n in (1, 2, 65):
        idx = np.random.RandomState(n).randint(0, table.size - P + 1, n).astype(np.int64)
        idx[0], idx[-1] = 0, table.size - P                     # the first and the last legal slice
        for sigma in (0.02, -0.02, 0.0):
            out = e.materialize(idx, sigma)
            want = U.materialize_np(th, table, idx, sigma)
            assert out.shape == (n, 2, P) and U.same_bits(out, want), (n, sigma)
            if sigma == 0.0:
                assert np.signbit(want[:, :, ::7]).any()        # -0.0 is among the bits compared


def check_select(e, m, want_nan):
    seen = 0
    for name, r in U.select_inputs(m):
        if name.startswith("nan") != want_nan:
            continue
        seen += 1
        for t in U.select_ts(m):
            got = e.ga_select(r, t)
            assert len(set(got.tolist())) == t, (name, t)
            assert np.array_equal(got, U.select_np(r, t)), (name, t)
    assert seen >= 3


@pytest.mark.parametrize("m", U.SELECT_MS)
def test_select_finite(engines, m):
    check_select(engines("maze"), m, False)


@pytest.mark.parametrize("m", U.SELECT_MS)
def test_select_with_nan_returns(engines, m):
    check_select(engines("maze"), m, True)


def test_redzones_are_intact(engines):
    """last in the file: no kernel above wrote outside its buffers"""
    for name in ("cartpole", "maze", "pendulum", "es18", "es3"):
        assert engines(name).check_redzones() == 0, name
