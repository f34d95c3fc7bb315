"""GPU: k_mjmaze_rollout<H, TANH> (csrc/mjmaze.h: whole hard-maze episodes of MujocoPolicy in one launch, one workgroup of H threads per member,
l0/w in LDS, the member's l1/w column in registers, the walls dealt over each wave's lanes) on a DNE_KIND_MJMAZE engine against
dne_mjmaze_rollout_host -- the same header compiled for the CPU -- BIT FOR BIT: returns, sign-returns, lengths, final (x, y), observation
statistics as doubles and counts, the per-step trace.  All six instantiations under the continuous action and 2 and 8 uniform bins a dimension;
1, 3 and 5 members, one unperturbed, some with action noise (one reading the table's last 800 values), some flagged, one with a NaN theta
beside healthy ones; timestep limits 400, 7 and 1; the one-wall, the 64-wall and the edge mazes at H = 64.  Then the engine level (pairs
through dne_es_eval, device-resident novelty at archive sizes 0, 1, 10 and 65, the kind's refusals) and nses / nsr / es run_master +
run_worker on this engine against the same drivers on the host-function engine."""
import functools

import numpy as np
import pytest

import mjmaze_support as S
from maze_support import same_nan

pytestmark = pytest.mark.gpu
SHAPES = tuple((H, nl, mode, O) for H in S.HS for nl in S.NONLINS for mode, O in S.MODES)
AC_STD = 0.05
RUNS = ((5, 400), (3, 7), (1, 1))          # (members, timestep limit)


@functools.lru_cache(maxsize=None)
def noise():
    return S.maze_noise()


@functools.lru_cache(maxsize=None)
def bases(H, O):
    """base slots: 0 = a random theta, 1 = NaN everywhere"""
    th = S.random_theta(H, O, 7 + H + O)
    return [th, np.full_like(th, np.nan)]


@functools.lru_cache(maxsize=None)
def members(P):
    """(slot, offset, scale, ac_off, flag) of the 5 members: 0 unperturbed and flagged; 1 the NaN theta, with action noise, flagged; 2 and 3 an
    antithetic pair with action noise, 3 reading the table's last 800 values and flagged; 4 at scale 1 over the last legal slice of the table"""
    rs = np.random.RandomState(5)
    off = rs.randint(0, noise().size - P + 1, size=5).astype(np.int64)
    off[3] = off[2]
    off[4] = noise().size - P
    scale = np.array([0.0, 0.0, 0.02, -0.02, 1.0], np.float32)
    slot = np.array([0, 1, 0, 0, 0], np.int32)
    ac_off = np.array([-1, 77, 1234, noise().size - S.AC_NOISE, -1], np.int64)
    flag = np.array([1, 1, 0, 1, 0], np.uint8)
    return slot, off, scale, ac_off, flag


@functools.lru_cache(maxsize=None)
def host(sh, maze_name, n, tslimit):
    """the CPU side of the comparison, once per shape, maze, member count and limit"""
    from dne_hip import _lib
    H, nl, mode, O = sh
    P = _lib.mjmaze_num_params(H, O)
    slot, off, scale, ac_off, flag = members(P)
    th = np.stack([S.perturbed(bases(H, O)[slot[i]], noise(), int(off[i]), scale[i]) for i in range(n)])
    header, lines = S.mazes()[maze_name]
    return _lib.mjmaze_rollout_host(th, header, lines, H, S.MEAN, S.STD, n_out=O, ac_mode=mode, nonlin=nl, tslimit=tslimit, ac_noise_std=AC_STD,
                                    table=noise(), ac_off=ac_off[:n], stat_flag=flag[:n], want_trace=True)


_engines = []


@functools.lru_cache(maxsize=None)
def engine(sh):
    """one engine per shape, made at its first use and closed with the module"""
    from dne_hip import _lib
    H, nl, mode, O = sh
    e = _lib.Engine(_lib.KIND_MJMAZE, O, max_members=16, hidden=H, ac_mode=mode, nonlin=nl)
    assert e.P == _lib.mjmaze_num_params(H, O) == S.offsets(H, O)[6]
    e.noise_upload(noise())
    for s, th in enumerate(bases(H, O)):
        e.set_theta(th, slot=s)
    e.mjmaze_set_ob_stat(S.MEAN, S.STD)
    _engines.append(e)
    return e


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    while _engines:
        _engines.pop().close()
    engine.cache_clear()


def device(e, sh, maze_name, n, tslimit):
    slot, off, scale, ac_off, flag = members(e.P)
    e.maze_set_walls(*S.mazes()[maze_name])
    e.set_members(slot[:n], off[:n], scale[:n])
    e.mjmaze_set_rollout_options(n, AC_STD, ac_off[:n], flag[:n])
    ret, sg, ln = e.eval_members(n, tslimit, np.zeros(n, np.uint32))
    s, q, c = e.mjmaze_ob_stats(n)
    return dict(returns=ret, signreturns=sg, lengths=ln, xy=e.maze_final_state(n), ob_sum=s, ob_sumsq=q, ob_count=c)


def assert_same(got, want, what):
    for k in ("returns", "signreturns", "xy", "ob_sum", "ob_sumsq"):
        assert same_nan(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("lengths", "ob_count"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def test_member_set_is_what_the_docstring_says():
    """held on the host function alone: the navigator moves, members differ, the NaN theta ends at NaN with the return -500, statistics only
    where flagged"""
    sh = (64, "tanh", "continuous", 2)
    r = host(sh, "fixture", 5, 400)
    assert (r["lengths"] == 400).all() and len(np.unique(r["returns"][[0, 2, 3, 4]])) == 4
    assert np.isnan(r["xy"][1]).all() and r["returns"][1] == -500.0 and not np.isnan(r["xy"][[0, 2, 3, 4]]).any()
    assert np.array_equal(r["ob_count"], 400 * members(5058)[4].astype(np.int32)) and not r["ob_sum"][[2, 4]].any()
    assert not np.array_equal(r["trace"][2, :, 11:13], r["trace"][2, :, 13:15])          # the noise moves the action


@pytest.mark.parametrize("sh", SHAPES, ids=lambda s: "%d-%s-%s-%d" % s)
def test_kernel_equals_host_bit_for_bit(sh):
    e = engine(sh)
    for n, tslimit in RUNS:
        assert_same(device(e, sh, "fixture", n, tslimit), host(sh, "fixture", n, tslimit), (sh, n, tslimit))
    assert e.check_redzones() == 0


@pytest.mark.parametrize("maze_name", ["one_wall", "full"] + ["edge_" + n for n in S.EDGE_MAZES])
def test_other_mazes_at_h64(maze_name):
    sh = (64, "tanh", "continuous", 2)
    assert_same(device(engine(sh), sh, maze_name, 5, 400), host(sh, maze_name, 5, 400), maze_name)


@pytest.mark.parametrize("H", S.HS)
def test_debug_trace_equals_the_twins(H):
    sh = (H, "tanh", "uniform", 16)
    e = engine(sh)
    slot, off, scale, ac_off, flag = members(e.P)
    e.maze_set_walls(*S.mazes()["fixture"])
    e.set_members(slot, off, scale)
    from dne_hip import _lib
    th = S.perturbed(bases(H, 16)[0], noise(), int(off[2]), scale[2])
    header, lines = S.mazes()["fixture"]
    want = _lib.mjmaze_rollout_host(th[None], header, lines, H, S.MEAN, S.STD, n_out=16, ac_mode="uniform", nonlin="tanh", want_trace=True)["trace"][0]
    got = e.mjmaze_debug_trace(2)
    assert got.shape == (400, S.TRACE_W) and same_nan(got, want)
    assert same_nan(e.mjmaze_debug_trace(2, tslimit=7), want[:7])


# ---- the engine level --------------------------------------------------------------------------------------------------------------------------------
def test_es_eval_and_device_resident_novelty():
    from dne_hip import _lib
    sh = (64, "tanh", "continuous", 2)
    e = engine(sh)
    header, lines = S.mazes()["fixture"]
    e.maze_set_walls(header, lines)
    idx = np.array([10, 5000, 77777, noise().size - e.P], np.int64)
    ret, sg, ln = e.es_eval(idx, 0.02, 400, np.zeros(8, np.uint32))
    th = np.stack([S.perturbed(bases(64, 2)[0], noise(), int(i), s) for i in idx for s in (0.02, -0.02)])
    want = _lib.mjmaze_rollout_host(th, header, lines, 64, S.MEAN, S.STD)
    xy = e.maze_final_state(8)
    assert same_nan(ret.reshape(-1), want["returns"]) and same_nan(sg.reshape(-1), want["signreturns"]) and same_nan(xy, want["xy"])
    assert (ln == 400).all() and not e.mjmaze_ob_stats(8)[2].any()
    e.maze_archive_clear()
    with pytest.raises(_lib.DneError, match="the archive is empty"):
        e.maze_novelty(10)
    pts = (np.random.RandomState(3).uniform(0, 200, (65, 2))).astype(np.float32)
    have = 0
    for size in (1, 10, 65):
        e.maze_archive_append(pts[have:size])
        have = size
        assert e.maze_archive_size() == size and np.array_equal(e.maze_archive(), pts[:size])
        got = e.maze_novelty(10, n=8)
        assert np.array_equal(S.bits(got), S.bits(_lib.maze_novelty_host(xy, pts[:size], 10))), size
    assert e.maze_novelty_last_ms() >= 0
    e.maze_archive_clear()


def test_refusals():
    from dne_hip import _lib
    sh = (64, "tanh", "continuous", 2)
    e = engine(sh)
    for mode, O in (("continuous", 4), ("uniform", 2), ("uniform", 18), ("uniform", 5)):
        with pytest.raises(_lib.DneError, match="DNE_KIND_MJMAZE"):
            _lib.Engine(_lib.KIND_MJMAZE, O, max_members=4, hidden=64, ac_mode=mode, nonlin="tanh")
    with pytest.raises(_lib.DneError, match="hidden width 96"):
        _lib.Engine(_lib.KIND_MJMAZE, 2, max_members=4, hidden=96)
    for kw in (dict(record_bc=True, bc_max_steps=4), dict(bc_final_only=True)):
        with pytest.raises(_lib.DneError, match="record_bc / bc_final_only are not available on a DNE_KIND_MJMAZE"):
            _lib.Engine(_lib.KIND_MJMAZE, 2, max_members=4, hidden=64, **kw)
    fresh = _lib.Engine(_lib.KIND_MJMAZE, 2, max_members=4, hidden=64)
    try:
        fresh.noise_upload(noise())
        fresh.set_members(np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros(2, np.float32))
        with pytest.raises(_lib.DneError, match="no maze loaded"):
            fresh.eval_members(2, 400, np.zeros(2, np.uint32))
        fresh.maze_set_walls(*S.mazes()["fixture"])
        with pytest.raises(_lib.DneError, match="dne_mjmaze_set_ob_stat"):
            fresh.eval_members(2, 400, np.zeros(2, np.uint32))
        with pytest.raises(_lib.DneError, match="past the noise table"):
            fresh.mjmaze_set_rollout_options(2, 0.01, np.array([0, noise().size - S.AC_NOISE + 1], np.int64), None)
        fresh.mjmaze_set_rollout_options(2, 0.01, np.array([0, noise().size - S.AC_NOISE], np.int64), None)      # at the table's end: accepted
        fresh.mjmaze_set_ob_stat(S.MEAN, S.STD)
        fresh.noise_upload(noise()[:5000])                                                                      # ... and checked again at the launch
        with pytest.raises(_lib.DneError, match="past the noise table"):
            fresh.eval_members(2, 400, np.zeros(2, np.uint32))
    finally:
        fresh.close()
    with pytest.raises(_lib.DneError, match="bc must be NULL"):
        e.eval_members(1, 400, np.zeros(1, np.uint32), want_bc=True)
    for call, word in ((lambda: e.env_reset(np.zeros(1, np.uint32)), "dne_env_reset is not available on a DNE_KIND_MJMAZE"),
                       (lambda: e.act(1), "DNE_KIND_MJMAZE"),
                       (lambda: e.ga_eval([[1]], 0.02, 10, np.zeros(1, np.uint32)), "DNE_KIND_MJMAZE"),
                       (lambda: e.maze_debug_trace(0), r"needs a DNE_KIND_MAZE engine \(this one: kind 7\)"),
                       (lambda: e.maze_ga_parents(), r"needs a DNE_KIND_MAZE engine \(this one: kind 7\)"),
                       (lambda: e.maze_novelty_pool(3, xy=np.zeros((4, 2), np.float32)), r"dne_maze_novelty_pool needs a DNE_KIND_MAZE engine"),
                       (lambda: e.maze_archive_append_members([0]), r"needs a DNE_KIND_MAZE engine"),
                       (lambda: e.cartpole_final_state(1), r"needs a DNE_KIND_CARTPOLE engine \(this one: kind 7\)"),
                       (lambda: e.pendulum_set_ob_stat(np.zeros(3), np.ones(3)), r"needs a DNE_KIND_PENDULUM engine \(this one: kind 7\)"),
                       (lambda: e.pendulum_final_state(1), r"needs a DNE_KIND_PENDULUM engine \(this one: kind 7\)"),
                       (lambda: e.stepenv_reset(np.arange(1)), r"this one: kind 7")):
        with pytest.raises(_lib.DneError, match=word):
            call()


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------------
def _hip_pair():
    from dne_hip import _lib
    pair = [_lib.Engine(_lib.KIND_MJMAZE, 2, max_members=16, hidden=64, ac_mode="continuous", nonlin="tanh") for _ in range(2)]
    _engines.extend(pair)
    return pair


@pytest.mark.parametrize("algo", ["ns", "nsr"])
def test_nses_drivers_equal_the_host_twins(oracle, tmp_path, algo):
    from dne_hip import es
    noise_table = es.SharedNoiseTable(count=400_000)
    exp = S.humanoid_nses_exp(algo_type=algo)
    runs = []
    for k, (me, we) in enumerate((_hip_pair(), (S.MjMazeHostEngine(), S.MjMazeHostEngine()))):
        seen = S.spy_novelty(we)
        log = tmp_path / str(k)
        log.mkdir()
        runs.append(S.run_nses(exp, me, we, noise_table, log))
        S.check_nses_run(runs[-1], exp, noise_table, seen)
    got, want = runs
    assert got["parents"] == want["parents"] and np.array_equal(S.bits(got["archive"]), S.bits(want["archive"]))
    for p in range(5):
        assert np.array_equal(S.bits(got["theta_dict"][p]), S.bits(want["theta_dict"][p])), p
        for a, b in zip(got["optimizer_dict"][p][:2], want["optimizer_dict"][p][:2]):
            assert np.array_equal(S.bits(a), S.bits(b)), p
        assert got["optimizer_dict"][p][2] == want["optimizer_dict"][p][2]
        sg, sw = got["obstat_dict"][p], want["obstat_dict"][p]
        assert sg.count == sw.count and np.array_equal(S.bits(sg.sum), S.bits(sw.sum)) and np.array_equal(S.bits(sg.sumsq), S.bits(sw.sumsq))
    for (tg, rg), (tw, rw) in zip(got["pushed"], want["pushed"]):
        assert tg == tw and np.array_equal(rg.noise_inds_n, rw.noise_inds_n) and rg.ob_count == rw.ob_count
        for f in ("returns_n2", "signreturns_n2", "lengths_n2", "ob_sum", "ob_sumsq"):
            assert np.array_equal(getattr(rg, f), getattr(rw, f)), f


def test_es_driver_equals_the_host_twins(oracle, tmp_path):
    import es_driver_support as D
    from dne_hip import es
    noise_table = es.SharedNoiseTable(count=400_000)
    exp = S.humanoid_exp(pop=8, eval_prob=1.0)
    runs, states = [], []
    for k, (me, we) in enumerate((_hip_pair(), (S.MjMazeHostEngine(), S.MjMazeHostEngine()))):
        log = tmp_path / str(k)
        log.mkdir()
        runs.append(D.run_driver(es, exp, me, we, noise_table, log, 2, worker_seed=1234))
        states.append(me.optimizer_get_state())
    D.assert_same_run(runs[1], runs[0], "es on DNE_KIND_MJMAZE")
    for (_, rg), (_, rw) in zip(runs[0].pushed, runs[1].pushed):
        D._same_array(rg.ob_sum, rw.ob_sum, "ob_sum")
        D._same_array(rg.ob_sumsq, rw.ob_sumsq, "ob_sumsq")
    assert np.array_equal(S.bits(states[0][0]), S.bits(states[1][0])) and np.array_equal(S.bits(states[0][1]), S.bits(states[1][1]))
    assert states[0][2] == states[1][2] == 2
    assert np.array_equal(runs[0].policy.ob_mean, runs[1].policy.ob_mean) and np.array_equal(runs[0].policy.ob_std, runs[1].policy.ob_std)
