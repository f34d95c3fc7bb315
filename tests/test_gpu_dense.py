"""The dense kind on the device (DNE_KIND_DENSE, k_dense_run of csrc/dense.h, dne_stepenv_act / dne_stepenv_run) against
its CPU twins, bit for bit: the forward pass, one act -> step round at a time, k rounds per launch, whole episodes through dne_eval_members and
dne_es_eval (on (16, 16) relu with the maze's and the cart-pole's own kernels as a second witness), two generations of ES and the es_gpu.py
driver with exp['model'] = 'LinearClassifier', and every refusal on a live handle.  One handle per (environment, shape), made at first use."""
import numpy as np
import pytest

import dense_support as D
import maze_support as MS
import stepenv_support as SS

pytestmark = pytest.mark.gpu
M = 16
IDS = [D.case_id(c) for c in D.CASES]
ORDERS = {1: ([2], [5]), 2: ([3, 0], [1, 1]), 5: ([4, 0, 2, 1, 3], [3, 0, 6, 0, 2]), 7: ([6, 5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5, 6])}   # n -> (environments, members)


@pytest.fixture(scope="module")
def engines():
    """handles by (case, which): `which` 0 is the one under test, 1 a second one that goes act + step where the first goes run"""
    made = {}

    def get(case, which=0):
        if (case, which) not in made:
            made[case, which] = D.device_engine(case, M)
        return made[case, which]
    get.made = made
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(autouse=True)
def redzones(engines):
    yield
    for key, e in engines.made.items():
        assert e.check_redzones() == 0, key


def off_the_reset(engs, env, n=7, steps=3):
    """the first n environments of every engine given, reset and moved three scripted steps"""
    seeds = SS.mixed_seeds(n)
    acts = SS.scripted_actions(env, n, steps)
    for e in engs:
        e.stepenv_reset(n=n, seeds=seeds)
        for t in range(steps):
            e.stepenv_step(acts[t])


# ---- 1. the forward pass ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_forward_equals_twin(engines, case):
    from dne_hip import _lib
    env, hidden, nl = case
    e = engines(case)
    th = D.load_members(e, case, extra=D.knife_thetas(env, hidden) if env == "cartpole" else None)
    off_the_reset([e], env)
    before = SS.snapshot(e, 7)

    def twin(members, idx):
        return _lib.dense_forward_host(th[members], before[3][idx], SS.kind_id(env), hidden, nl, D.N_OUT[env])[1:]

    for n, (idx, members) in ORDERS.items():
        out, act = e.stepenv_act(np.array(idx, np.int32), np.array(members, np.int32))
        want_out, want_act = twin(members, idx)
        assert D.same(out, want_out) and D.same(act, want_act), (n, out, want_out)
    out, act = e.stepenv_act(n=7)                                        # members = NULL: member i behind environment i
    want_out, want_act = twin(list(range(7)), list(range(7)))
    assert D.same(out, want_out) and D.same(act, want_act)
    assert len({o.tobytes() for o in out}) == 7                          # seven members, seven answers
    if env == "cartpole":                                                # the argmax's edge: equal logits -> 0; one ulp either way -> 1 / 0
        out, act = e.stepenv_act(np.array([0, 1, 2], np.int32), np.array([7, 8, 9], np.int32))
        want_out, want_act = twin([7, 8, 9], [0, 1, 2])
        assert D.same(out, want_out) and D.same(act, want_act) and act.tolist() == [0, 1, 0]
        assert out[0, 0] == out[0, 1] == 0 and out[1, 1] == np.nextafter(out[1, 0], np.float32(2)) and out[2, 0] == np.nextafter(out[2, 1], np.float32(2))
    assert SS.same_snapshot(SS.snapshot(e, 7), before)                   # the forward pass moves nothing


# ---- 2. one round at a time -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_run_one_round_at_a_time(engines, case):
    """stepenv_run(1) on one handle, stepenv_act + stepenv_step on a second, the twin's run(1): reward, done, steps taken after every step;
    observation, state and steps for the first 40 steps and at the end"""
    env, hidden, nl = case
    e, e2, h = engines(case), engines(case, 1), D.host_engine(case, M)
    n = 5
    idx, members = np.array(ORDERS[5][0], np.int32), np.array(ORDERS[5][1], np.int32)
    th = D.load_members(e, case); D.load_members(e2, case); D.load_members(h, case)
    seeds = D.spread_seeds(case, th[members]) if env == "cartpole" else SS.mixed_seeds(n)
    for x in (e, e2, h):
        x.stepenv_reset(idx, seeds)
    t, done, total = 0, np.zeros(n, bool), np.zeros(n)
    while not done.all():
        was_done = done
        rew, took, done = e.stepenv_run(1, idx, members)
        out, act = e2.stepenv_act(idx, members)
        rew2, done2 = e2.stepenv_step(act, idx)
        hrew, htook, hdone = h.stepenv_run(1, idx, members)
        assert D.same(rew, rew2) and D.same(rew, hrew) and np.array_equal(done, done2) and np.array_equal(done, hdone), (t, rew, rew2, hrew)
        assert np.array_equal(took, htook) and np.array_equal(took, (~was_done).astype(np.int32))
        total += rew
        t += 1
        if t <= 40 or done.all():
            s = SS.snapshot(e, n)
            assert SS.same_snapshot(tuple(a[:n] for a in s), SS.snapshot(e2, n)) and SS.same_snapshot(tuple(a[:n] for a in s), SS.snapshot(h, n)), t
    steps = e.stepenv_state(idx)[1]
    print(D.case_id(case), "steps", steps.tolist(), "totals", total.tolist())
    assert t <= SS.OWN_LIMIT[env] and (env == "cartpole" or t == SS.OWN_LIMIT[env])
    if env == "cartpole":
        assert len(set(steps.tolist())) >= 3                             # ended at different steps, frozen while the others went on
    before = SS.snapshot(e, n)
    rew, took, done = e.stepenv_run(3, idx, members)                     # everyone is done: nothing moves
    assert D.same(rew, np.zeros(n, np.float32)) and not took.any() and done.all() and SS.same_snapshot(SS.snapshot(e, n), before)


# ---- 3. k rounds a launch ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_run_in_pieces(engines, case):
    """7, then 1, then the rest against one run to the end: the same state; each piece's totals (one float64 sum, cast once per call) against the
    twin split the same way, the whole run's against the whole-episode twin"""
    from dne_hip import _lib
    env, hidden, nl = case
    e, e2, h = engines(case), engines(case, 1), D.host_engine(case, M)
    n = 5
    idx, members = np.array(ORDERS[5][0], np.int32), np.array(ORDERS[5][1], np.int32)
    th = D.load_members(e, case); D.load_members(e2, case); D.load_members(h, case)
    seeds = SS.mixed_seeds(n)
    for x in (e, e2, h):
        x.stepenv_reset(idx, seeds)
    for k in (7, 1, 100000):
        got, want = e.stepenv_run(k, idx, members), h.stepenv_run(k, idx, members)
        assert D.same(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (k, got, want)
        assert e.stepenv_last_ms() > 0
    whole = e2.stepenv_run(100000, idx, members)
    assert whole[2].all() and SS.same_snapshot(SS.snapshot(e, n), SS.snapshot(e2, n)) and SS.same_snapshot(SS.snapshot(e, n), SS.snapshot(h, n))
    r = _lib.dense_rollout_host(th[members], SS.kind_id(env), hidden, nl, D.N_OUT[env], seeds=seeds, **h.envs._maze())
    assert D.same(whole[0], r["returns"]) and D.same(whole[1], r["lengths"]) and D.same(e2.stepenv_state(idx)[0], r["state"])


# ---- 4. whole episodes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_whole_episodes(engines, case):
    from dne_hip import _lib
    env, hidden, nl = case
    e = engines(case)
    th = D.load_members(e, case)
    off_the_reset([e], env)
    before = SS.snapshot(e, 7)
    seeds = SS.mixed_seeds(7)
    maze = dict(zip(("header", "lines"), MS.fixture_maze())) if env == "maze" else {}
    witness = None
    if hidden == (16, 16) and env != "pendulum":                        # the kernel of the baked shape on the same theta, table, members and seeds
        witness = SS.device_engine(env, M)
        witness.noise_upload(D.noise())
        bases = D.base_thetas(env, hidden)
        witness.set_theta(bases[0], 0); witness.set_theta(bases[1], 1)
    try:
        for tslimit in (1, 7, SS.OWN_LIMIT[env]):
            D.load_members(e, case)
            ret, sg, ln = e.eval_members(7, tslimit, seeds)
            want = _lib.dense_rollout_host(th, SS.kind_id(env), hidden, nl, D.N_OUT[env], seeds=seeds, tslimit=tslimit, **maze)
            assert D.same(ret, want["returns"]) and D.same(sg, want["signreturns"]) and D.same(ln, want["lengths"]), (tslimit, ret, want["returns"])
            assert D.same(e.dense_final_state(7), want["state"])
            if witness is not None:
                witness.set_members(*D.member_table(env, hidden))
                wret, wsg, wln = witness.eval_members(7, tslimit, seeds)
                assert D.same(ret, wret) and D.same(sg, wsg) and D.same(ln, wln)
                if env == "maze":
                    assert D.same(e.dense_final_state(7)[:, :2].astype(np.float32), witness.maze_final_state(7))
                else:
                    assert D.same(e.dense_final_state(7), witness.cartpole_final_state(7))
            # five antithetic pairs over base slot 0
            idx = np.array([100, 31, 7777, 0, D.noise().size - e.P], np.int64)
            pair_seeds = SS.mixed_seeds(10)
            ret, sg, ln = e.es_eval(idx, D.SIGMA, tslimit, pair_seeds)
            pth = np.stack([(th[4] + np.float32(s) * D.noise()[i:i + e.P]).astype(np.float32) for i in idx for s in (D.SIGMA, -D.SIGMA)])   # (member 4 is base slot 0 at scale 0)
            want = _lib.dense_rollout_host(pth, SS.kind_id(env), hidden, nl, D.N_OUT[env], seeds=pair_seeds, tslimit=tslimit, **maze)
            assert D.same(ret.reshape(-1), want["returns"]) and D.same(sg.reshape(-1), want["signreturns"]) and D.same(ln.reshape(-1), want["lengths"])
            assert D.same(e.dense_final_state(10), want["state"])
            if witness is not None:
                wret, wsg, wln = witness.es_eval(idx, D.SIGMA, tslimit, pair_seeds)
                assert D.same(ret, wret) and D.same(sg, wsg) and D.same(ln, wln)
        assert SS.same_snapshot(SS.snapshot(e, 7), before)               # an evaluation leaves the step-at-a-time batch as it was
    finally:
        if witness is not None:
            assert witness.check_redzones() == 0
            witness.close()


# ---- 5. ES ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ("maze", "cartpole"))
def test_two_generations_of_es(engines, env):
    from dne_hip import policies
    case = (env, (), "relu")
    e = engines(case)
    want = D.plain_loop(env, 2)
    tab, P = D.noise(), e.P
    rs = np.random.RandomState(4)
    e.set_theta(tab[rs.randint(0, tab.size - P + 1):][:P] * policies.dense_scale_by(SS.kind_id(env), (), 2))
    e.optimizer_reset()
    rs.randint(0, 2 ** 32, size=2, dtype=np.uint64)
    for it in range(2):
        idx = np.array([rs.randint(0, tab.size - P + 1) for _ in range(5)], np.int64)
        seeds = rs.randint(0, 2 ** 32, size=10, dtype=np.uint64).astype(np.uint32)
        rets, sgn, lens = e.es_eval(idx, 0.02, SS.OWN_LIMIT[env], seeds)
        assert D.same(rets, want[it][3]) and np.array_equal(lens, want[it][4])
        e.es_update(idx, rets, sgn, "centered_rank", "adam", 0.005, 0.01)
        rs.randint(0, 2 ** 32, size=2, dtype=np.uint64)
        m, v, t = e.optimizer_get_state()
        assert D.same(e.get_theta(), want[it][0]) and D.same(m, want[it][1]) and D.same(v, want[it][2]) and t == it + 1
    assert not D.same(want[1][0], want[0][0])


@pytest.mark.parametrize("env", ("maze", "cartpole"))
def test_driver_on_the_live_handle_equals_the_host_engine(engines, env, tmp_path):
    from dne_hip import es_gpu
    case = (env, (), "relu")
    states = []
    for name, eng in (("device", engines(case)), ("host", D.host_engine(case, M))):
        states.append(es_gpu.main(str(tmp_path / name), engine=eng, noise=D.shared_noise(), seed=4, max_iters=2, **D.exp(SS.GAMES[env])))
    dev, host = states
    assert dev.model == host.model == "LinearClassifier" and dev.it == host.it == 2 and dev.timesteps_so_far == host.timesteps_so_far
    assert D.same(dev.theta, host.theta) and D.same(dev.optimizer[0], host.optimizer[0]) and D.same(dev.optimizer[1], host.optimizer[1])
    rows = D.log_rows(tmp_path / "device")
    assert len(rows) == 2 and D.same_rows(rows, D.log_rows(tmp_path / "host")), rows
    assert D.same(dev.theta, D.plain_loop(env, 2)[1][0])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("maze", (5, 33), "relu"), ("cartpole", (), "relu"), ("pendulum", (64,), "tanh")], ids=lambda c: D.case_id(c))
def test_refusals_leave_batch_and_members_alone(engines, case):
    from dne_hip import _lib
    env, hidden, nl = case
    e = engines(case)
    D.load_members(e, case)
    n = 4
    e.stepenv_reset(n=n, seeds=SS.mixed_seeds(n))
    e.stepenv_run(2, n=n)
    before, members = SS.snapshot(e, n), e.debug_members()

    def refused(pattern, fn):
        with pytest.raises(_lib.DneError, match=pattern):
            fn()
        assert SS.same_snapshot(SS.snapshot(e, n), before), pattern
        assert all(np.array_equal(a, b) for a, b in zip(e.debug_members(), members)), pattern

    one = np.array([0], np.int32)
    refused(D.REFUSED["max_steps"], lambda: e.stepenv_run(0, n=n))
    refused(D.REFUSED["max_steps"], lambda: e.stepenv_run(-5, n=n))
    refused(D.REFUSED["member"], lambda: e.stepenv_run(1, n=2, members=[0, 7]))
    refused(D.REFUSED["member"], lambda: e.stepenv_act(n=2, members=[-1, 0]))
    refused(D.REFUSED["member"], lambda: e.stepenv_act(np.array([3], np.int32), members=[100]))
    refused(SS.REFUSED["never"], lambda: e.stepenv_run(1, np.array([0, M - 2], np.int32), members=[0, 1]))   # (no test of this file resets past environment 6)
    refused(SS.REFUSED["never"], lambda: e.stepenv_act(np.array([M - 1], np.int32), members=[0]))
    refused(SS.REFUSED["twice"], lambda: e.stepenv_run(1, np.array([1, 1], np.int32), members=[0, 1]))
    refused(SS.REFUSED["range"], lambda: e.stepenv_act(np.array([M], np.int32), members=[0]))
    refused(SS.REFUSED["n"], lambda: e.stepenv_run(1, np.zeros(0, np.int32)))
    # the evaluation's own refusals
    refused("bc must be NULL", lambda: e.eval_members(2, 5, SS.mixed_seeds(2), want_bc=True))
    refused("timestep limit must be positive", lambda: e.eval_members(2, 0, SS.mixed_seeds(2)))
    # the calls of the other kinds refuse this one in their own words
    refused(r"dne_maze_final_state needs a DNE_KIND_MAZE engine \(this one: kind 8\)", lambda: e.maze_final_state(1))
    refused(r"dne_cartpole_final_state needs a DNE_KIND_CARTPOLE engine \(this one: kind 8\)", lambda: e.cartpole_final_state(1))
    refused(r"dne_pendulum_final_state needs a DNE_KIND_PENDULUM engine \(this one: kind 8\)", lambda: e.pendulum_final_state(1))
    refused(r"dne_maze_debug_trace needs a DNE_KIND_MAZE engine \(this one: kind 8\)", lambda: e.maze_debug_trace(0))
    refused(r"dne_maze_ga_parents needs a DNE_KIND_MAZE engine \(this one: kind 8\)", lambda: e.maze_ga_parents())
    refused(r"dne_maze_archive_clear needs a DNE_KIND_MAZE engine \(this one: kind 8\)", lambda: e.maze_archive_clear())
    refused(r"dne_act is not available on a DNE_KIND_DENSE engine \(kind 8\)", lambda: e.act(1))
    refused(r"dne_env_reset is not available on a DNE_KIND_DENSE engine", lambda: e.env_reset(np.zeros(1, np.uint32)))
    if env != "maze":
        refused(r"dne_maze_set_walls needs a DNE_KIND_MAZE engine \(this one: kind 8\)", lambda: e.maze_set_walls(*MS.fixture_maze()))
    assert e.lib.dne_dense_env_kind(e.h) == SS.kind_id(env) == e.env_kind
    assert _lib.num_params(_lib.KIND_DENSE, D.N_OUT[env]) == -1 and e.P == D.num_params(env, hidden)


def test_fresh_handles_and_other_kinds_refuse_by_name(engines):
    from dne_hip import _lib
    fresh = _lib.Engine(_lib.KIND_DENSE, 2, max_members=4, env=_lib.KIND_MAZE, hidden=(3,), nonlin="relu")
    try:
        with pytest.raises(_lib.DneError, match=SS.REFUSED["walls"]):
            fresh.stepenv_reset(n=1)
        fresh.noise_upload(D.noise())
        fresh.set_members(np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float32))
        with pytest.raises(_lib.DneError, match="no maze loaded"):
            fresh.eval_members(1, 5, np.zeros(1, np.uint32))
        with pytest.raises(_lib.DneError, match=SS.REFUSED["walls"]):
            fresh.stepenv_act(n=1)
        fresh.maze_set_walls(*MS.fixture_maze())
        with pytest.raises(_lib.DneError, match=SS.REFUSED["never"]):
            fresh.stepenv_run(1, n=1)
        fresh.stepenv_reset(n=2)
        assert fresh.stepenv_run(1, n=2, members=[0, 0])[1].tolist() == [1, 1]
        assert fresh.check_redzones() == 0
    finally:
        fresh.close()
    fresh = _lib.Engine(_lib.KIND_DENSE, 2, max_members=4, env=_lib.KIND_CARTPOLE, hidden=(), nonlin="relu")
    try:
        fresh.noise_upload(D.noise())
        fresh.stepenv_reset(n=2, seeds=[1, 2])
        with pytest.raises(_lib.DneError, match=D.REFUSED["members"]):
            fresh.stepenv_act(n=2)
        with pytest.raises(_lib.DneError, match=D.REFUSED["members"]):
            fresh.stepenv_run(1, n=2)
        fresh.set_members(np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float32))
        with pytest.raises(_lib.DneError, match="env_seed is NULL"):
            fresh._ck(fresh.lib.dne_eval_members(fresh.h, 1, 5, None, None, None, None, None))
    finally:
        fresh.close()
    for kind in SS.KINDS:                                                # the environments' own kinds have no policy behind them
        other = SS.device_engine(kind, 4)
        try:
            other.stepenv_reset(n=2, seeds=[1, 2])
            before = SS.snapshot(other, 2)
            with pytest.raises(_lib.DneError, match=r"dne_stepenv_act needs a DNE_KIND_DENSE engine \(this one: kind %d\)" % SS.kind_id(kind)):
                other.stepenv_act(n=2)
            with pytest.raises(_lib.DneError, match=r"dne_stepenv_run needs a DNE_KIND_DENSE engine \(this one: kind %d\)" % SS.kind_id(kind)):
                other.stepenv_run(1, n=2)
            with pytest.raises(_lib.DneError, match=r"dne_dense_final_state needs a DNE_KIND_DENSE engine"):
                other.dense_final_state(1)
            assert SS.same_snapshot(SS.snapshot(other, 2), before) and other.env_kind == other.kind == other.lib.dne_dense_env_kind(other.h)
        finally:
            other.close()
    # dne_create refuses a shape that is not built, by name
    K = _lib.KIND_MAZE
    for match, kw in ((r"environment 7 is refused", dict(n_actions=2, env=7, hidden=())),
                      (r"environment 0 is refused", dict(n_actions=2, env=0, hidden=())),
                      (r"4 hidden layers are refused", dict(n_actions=2, env=K, hidden=(4, 4, 4, 4))),
                      (r"width 65 of hidden layer 1 is refused", dict(n_actions=2, env=K, hidden=(3, 65))),
                      (r"width 0 of hidden layer 0 is refused", dict(n_actions=2, env=K, hidden=(0,))),
                      (r"n_actions 3 is refused", dict(n_actions=3, env=K, hidden=())),
                      (r"n_actions 2 is refused", dict(n_actions=2, env=_lib.KIND_PENDULUM, hidden=(4,))),
                      (r"n_actions 1 is refused", dict(n_actions=1, env=_lib.KIND_CARTPOLE, hidden=(4,))),
                      (r"nonlinearity 2 is refused", dict(n_actions=2, env=K, hidden=(4,), nonlin=2)),
                      (r"record_bc / bc_final_only are not available on a DNE_KIND_DENSE engine", dict(n_actions=2, env=K, hidden=(), record_bc=True, bc_max_steps=4)),
                      (r"record_bc / bc_final_only are not available on a DNE_KIND_DENSE engine", dict(n_actions=2, env=K, hidden=(), bc_final_only=True))):
        with pytest.raises(_lib.DneError, match=match):
            _lib.Engine(_lib.KIND_DENSE, max_members=4, **kw)
    cfg = _lib.Config(device_id=0, policy_kind=_lib.KIND_DENSE, n_actions=2, max_members=4)
    cfg.reserved[0], cfg.reserved[1], cfg.reserved[3], cfg.reserved[5] = K, 1, 4, 9      # one hidden layer, and a width behind it
    h = _lib.C.c_void_p()
    assert _lib.load().dne_create(_lib.C.byref(cfg), _lib.C.byref(h)) != 0
    assert "1 hidden layers, and a width of 9 behind them (entry 2)" in _lib.load().dne_last_error(None).decode()


def test_envs_run_on_the_device(engines):
    """envs.make(game, batch, hidden=...) opens an engine of this kind; envs.run keeps the episodes on the device and equals envs.rollout under
    the twin's forward pass"""
    from dne_hip import _lib, envs
    n = 7
    for game, env, hidden, nl in (("gym.CartPole-v1", "cartpole", (), "relu"), ("maze", "maze", (5, 33), "relu"), ("Pendulum-v0", "pendulum", (64,), "tanh")):
        case = (env, hidden, nl)
        e = envs.make(game, n, hidden=hidden, nonlin=nl, **({"maze_file": MS.MAZE_FILE} if env == "maze" else {}))
        try:
            assert e.engine.kind == _lib.KIND_DENSE and e.engine.env_kind == SS.kind_id(env) and e.engine.hidden == hidden
            e.engine.noise_upload(D.noise())
            th = D.load_members(e.engine, case)
            seeds = SS.mixed_seeds(n)
            ret, ln = envs.run(e, seeds=seeds)
            final = e.state()[0]
            want = envs.rollout(e, lambda obs: _lib.dense_forward_host(th[:n], obs, SS.kind_id(env), hidden, nl, D.N_OUT[env])[2], seeds=seeds)
            assert D.same(ret, want[0]) and D.same(ln, want[1]) and D.same(final, e.state()[0])
            members = [3, 0, 6, 0, 2, 5, 1]                              # permuted, one member behind two environments; in launches of 3 rounds
            ret7, ln7 = envs.run(e, members=members, seeds=seeds, max_frames=7, max_steps=3)
            r = _lib.dense_rollout_host(th[members], SS.kind_id(env), hidden, nl, D.N_OUT[env], seeds=seeds, tslimit=7,
                                        **(dict(zip(("header", "lines"), MS.fixture_maze())) if env == "maze" else {}))
            assert D.same(ln7, r["lengths"]) and D.same(e.state()[0], r["state"]) and (env == "pendulum" or D.same(ret7, r["returns"]))
            assert e.engine.check_redzones() == 0
        finally:
            e.close()
