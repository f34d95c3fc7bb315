"""GPU: the step-at-a-time environments (csrc/step_env.h: k_stepenv_reset_* / k_stepenv_step_* / k_stepenv_gather behind dne_stepenv_*) on live
handles of the three kinds, BIT FOR BIT against the same header compiled for the CPU (stepenv_support.StepEnvHostEngine) under the same
actions -- reward, done, observation, state and steps after each of the first 40 steps and after the last, at batch sizes that cross a row and
a workgroup edge (maze 1, 3, 4, 5: 16 lanes per environment, four per wave, a partial last wave; cart-pole and pendulum 1, 63, 64, 65) --
and against the whole-episode kernels: envs.rollout on the device under the host forward twin equals dne_eval_members in returns, lengths and
final states.  Subsets, permuted lists, frozen done environments, set_state and the refusals run as on the CPU; evaluations and the batch
leave each other alone."""
import numpy as np
import pytest

import maze_support as MS
import pendulum_support as PS
import stepenv_support as S

pytestmark = pytest.mark.gpu
M = 66
SIZES = {"maze": (1, 3, 4, 5), "cartpole": (1, 63, 64, 65), "pendulum": (1, 63, 64, 65)}
SIGMA = {"maze": 1.0, "cartpole": 1.0, "pendulum": 0.02}          # members of the kinds' own GPU tests


@pytest.fixture(scope="module")
def engines():
    """one handle per kind for the module, made at first use"""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = S.device_engine(kind, M)
        return made[kind]
    yield get
    for e in made.values():
        assert e.check_redzones() == 0
        e.close()


def both_snapshots_equal(e, h, n):
    return S.same_snapshot(S.snapshot(e, n), S.snapshot(h, n))


# ---- 1. device against twin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [(k, n) for k in S.KINDS for n in SIZES[k]] + [("cartpole", 5), ("pendulum", 5)])
def test_device_equals_twin_step_by_step(engines, kind, n):
    e, h = engines(kind), S.host_engine(kind, n)
    seeds = S.mixed_seeds(n)
    acts = S.scripted_actions(kind, n)
    e.stepenv_reset(n=n, seeds=seeds)
    h.stepenv_reset(n=n, seeds=seeds)
    assert both_snapshots_equal(e, h, n)
    total_e, total_h, t, done = np.zeros(n), np.zeros(n), 0, np.zeros(n, bool)
    while not done.all():
        rew, done = e.stepenv_step(acts[t])
        hrew, hdone = h.stepenv_step(acts[t])
        assert S.same(rew, hrew) and np.array_equal(done, hdone), (kind, n, t)
        total_e += rew
        total_h += hrew
        t += 1
        if t <= 40 or done.all():
            assert both_snapshots_equal(e, h, n), (kind, n, t)
    assert t <= S.OWN_LIMIT[kind] and (kind == "cartpole" or t == S.OWN_LIMIT[kind])
    assert S.same(total_e, total_h)                                              # the full-episode totals
    steps = e.stepenv_state(n=n)[1]
    print(kind, n, "steps", steps[:8].tolist(), "totals", total_e[:5].tolist())
    if kind == "cartpole" and n >= 5:
        assert len(set(steps.tolist())) >= 3                                     # the members ended at different steps, frozen while the others went on
    before = S.snapshot(e, n)
    for k in range(3):                                                           # everyone is done: three more steps change nothing
        rew, done = e.stepenv_step(acts[k])
        assert S.same(rew, np.zeros(n, np.float32)) and done.all() and S.same_snapshot(S.snapshot(e, n), before)
    assert e.check_redzones() == 0


# ---- 2. against the whole-episode kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hidden,nonlin", (("maze", 0, ""), ("cartpole", 0, ""), ("pendulum", 64, "tanh"), ("pendulum", 256, "relu")))
def test_rollout_on_the_device_equals_eval_members(kind, hidden, nonlin):
    from dne_hip import envs
    n = 10
    e = S.device_engine(kind, n, hidden=hidden, nonlin=nonlin)
    try:
        noise = MS.maze_noise()
        base = S.closed_loop_thetas(kind, hidden or 64)[0]
        e.noise_upload(noise)
        e.set_theta(base)
        if kind == "pendulum":
            e.pendulum_set_ob_stat(S.PD_MEAN, S.PD_STD)
        offs = np.array([100, 7777, 31, 50_000, noise.size - base.size], np.int64)
        sigma = SIGMA[kind]
        # the members' thetas through the existing calls: theta 0 as it is, base + fl(sigma * eps) materialised on the device
        thetas = np.concatenate([np.tile(e.get_theta(0), (5, 1)), e.materialize(offs, sigma)[:, 0, :]])
        assert S.same(thetas[0], base) and S.same(thetas[5:], np.stack([PS.perturbed(base, noise, int(o), sigma) for o in offs]))
        seeds = S.mixed_seeds(n)
        e.set_members(np.zeros(n, np.int32), np.concatenate([np.zeros(5, np.int64), offs]), np.array([0.0] * 5 + [sigma] * 5, np.float32))
        ret, _, ln = e.eval_members(n, 5000, seeds)
        final = {"maze": e.maze_final_state, "cartpole": e.cartpole_final_state, "pendulum": e.pendulum_final_state}[kind](n)
        env = envs.make(S.GAMES[kind], n, engine=e)
        got_ret, got_ln = envs.rollout(env, S.policy(kind, thetas, hidden, nonlin), seeds=seeds)
        print(kind, hidden, nonlin, "lengths", ln.tolist(), "returns", ret.tolist())
        assert S.same(got_ret, ret) and np.array_equal(got_ln, ln) and S.same(S.final_of(kind, env), final)
        if kind == "cartpole":
            assert len(set(ln.tolist())) >= 3
        # the evaluation's results are still there after 500 step calls
        assert S.same({"maze": e.maze_final_state, "cartpole": e.cartpole_final_state, "pendulum": e.pendulum_final_state}[kind](n), final)
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("kind", S.KINDS)
def test_make_opens_an_engine_of_its_own(kind):
    """envs.make without an engine: a handle of the game's kind (the maze with the fixture's walls), a controller no kernel contains, the
    CPU twin under the same controller"""
    from dne_hip import envs
    act = {"maze": lambda obs: np.stack([obs[:, 3] - obs[:, 1], 0.5 * obs[:, 3]], axis=1).astype(np.float32),
           "cartpole": lambda obs: (obs[:, 2] + 0.5 * obs[:, 3] > 0).astype(np.int32),
           "pendulum": lambda obs: (-2.0 * obs[:, 1] - 0.5 * obs[:, 2]).astype(np.float32)}[kind]
    seeds = S.mixed_seeds(3)
    env = envs.make(S.GAMES[kind], 3)
    try:
        assert env.engine.kind == S.kind_id(kind) and env.engine.max_members == 3
        ret, ln = envs.rollout(env, act, seeds=seeds)
        twin = envs.make(S.GAMES[kind], 3, engine=S.host_engine(kind, 3))
        hret, hln = envs.rollout(twin, act, seeds=seeds)
        print(kind, "lengths", ln.tolist(), "returns", ret.tolist())
        assert S.same(ret, hret) and np.array_equal(ln, hln) and all(S.same(a, b) for a, b in zip(env.state(), twin.state()))
        assert S.same(env.final_state(), twin.final_state()) and env.engine.check_redzones() == 0
    finally:
        env.close()
    assert env.engine is None


# ---- 3. subsets, done, set_state, limits: the CPU file's checks on the device ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_subsets_and_the_order_of_the_list(engines, kind):
    S.check_subsets(engines(kind), kind)


@pytest.mark.parametrize("kind", S.KINDS)
def test_done_environments_keep_every_bit(engines, kind):
    S.check_done_freezes(engines(kind), kind)


@pytest.mark.parametrize("kind", S.KINDS)
def test_set_state(engines, kind):
    S.check_set_state(engines(kind), kind)


def test_set_state_equals_twin_on_states_no_reset_gives(engines):
    """the observation set_state recomputes and the steps that follow, on both sides: the maze at headings across the wrap and against a wall,
    on a permuted list"""
    e, h = engines("maze"), S.host_engine("maze", 8)
    hdr, _ = MS.fixture_maze()
    rs = np.random.RandomState(3)
    st = np.zeros((5, 7))
    st[:, 0], st[:, 1] = float(hdr[2]) + rs.uniform(-6, 6, 5), float(hdr[3]) + rs.uniform(-6, 6, 5)
    st[:, 2], st[:, 3], st[:, 4] = (0.0, 359.5, 180.25, 90.0, 271.0), rs.uniform(-3, 3, 5), rs.uniform(-3, 3, 5)
    st[:, 6] = (0, 1, 7, 0, 399)
    idx = np.array([6, 1, 4, 0, 3], np.int32)
    for x in (e, h):
        x.stepenv_set_state(st, steps=[0, 10, 398, 399, 5], indices=idx, max_steps=0)
    assert S.same(e.stepenv_observation(idx), h.stepenv_observation(idx)) and all(S.same(a, b) for a, b in zip(e.stepenv_state(idx), h.stepenv_state(idx)))
    acts = S.scripted_actions("maze", 5, 4)
    for t in range(4):
        (rew, done), (hrew, hdone) = e.stepenv_step(acts[t], idx), h.stepenv_step(acts[t], idx)
        assert S.same(rew, hrew) and np.array_equal(done, hdone)
        assert S.same(e.stepenv_observation(idx), h.stepenv_observation(idx)) and all(S.same(a, b) for a, b in zip(e.stepenv_state(idx), h.stepenv_state(idx)))
    assert done.tolist() == [False, False, True, True, False] and hrew[2] == 0 and hrew[3] == 0


def test_maze_limits(engines):
    S.check_maze_limits(engines("maze"))


# ---- 4. evaluations and the batch leave each other alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_evaluations_and_environments_are_independent(kind):
    n = 6
    e = S.device_engine(kind, 8)
    try:
        noise = MS.maze_noise()
        base = S.closed_loop_thetas(kind)[0]
        e.noise_upload(noise)
        e.set_theta(base)
        if kind == "pendulum":
            e.pendulum_set_ob_stat(S.PD_MEAN, S.PD_STD)
        final = {"maze": e.maze_final_state, "cartpole": e.cartpole_final_state, "pendulum": e.pendulum_final_state}[kind]
        members = (np.zeros(n, np.int32), np.arange(n, dtype=np.int64) * 1000, np.array([0.0, 0.02, -0.02, 1.0, -1.0, 0.0], np.float32))
        seeds, acts = S.mixed_seeds(n), S.scripted_actions(kind, n, 3)
        e.set_members(*members)
        first = e.eval_members(n, 5000, seeds) + (final(n),)                     # before the batch exists
        e.stepenv_reset(n=n, seeds=seeds[::-1].copy())
        e.stepenv_step(acts[0])
        snap = S.snapshot(e, n)
        e.set_members(*members)
        res = e.eval_members(n, 5000, seeds) + (final(n),)
        assert S.same_snapshot(S.snapshot(e, n), snap)                           # an evaluation between two steps changes no environment
        assert all(S.same(a, b) for a, b in zip(res, first))
        rew, done = e.stepenv_step(acts[1])
        e.set_members(*members)
        e.stepenv_step(acts[2])                                                  # a step between set_members and eval_members ...
        res2 = e.eval_members(n, 5000, seeds) + (final(n),)
        assert all(S.same(a, b) for a, b in zip(res2, first))                    # ... changes no result of the evaluation
        h = S.host_engine(kind, n)
        h.stepenv_reset(n=n, seeds=seeds[::-1].copy())
        for t in range(3):
            h.stepenv_step(acts[t])
        assert S.same_snapshot(S.snapshot(e, n), S.snapshot(h, n))               # and the environments went on as if nothing had run between
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_refusals_on_a_live_handle(kind):
    from dne_hip import _lib

    def fresh():
        return S.device_engine(kind, 8) if kind != "maze" else _lib.Engine(_lib.KIND_MAZE, 2, max_members=8)   # (the maze: no walls yet)
    e = S.device_engine(kind, 8)
    try:
        S.check_refusals(e, kind, fresh)
        # dne_env_* keep refusing the kind, in their old words
        name = {"maze": "DNE_KIND_MAZE", "cartpole": "DNE_KIND_CARTPOLE", "pendulum": "DNE_KIND_PENDULUM"}[kind]
        with pytest.raises(_lib.DneError, match="dne_env_reset is not available on a %s engine" % name):
            e.env_reset(np.zeros(2, np.uint32))
        with pytest.raises(_lib.DneError, match="dne_env_step is not available on a %s engine" % name):
            e.env_step(np.zeros(2, np.int32))
        assert e.check_redzones() == 0
    finally:
        e.close()


def test_every_call_is_refused_on_an_atari_handle():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_ES, 18, max_members=8, ref_count=16)
    try:
        calls = (lambda: e.stepenv_reset(n=2, seeds=np.zeros(2, np.uint32)), lambda: e.stepenv_step(np.zeros(2, np.float32)),
                 lambda: e.stepenv_step(np.zeros(2, np.int32)), lambda: e.stepenv_observation(n=2), lambda: e.stepenv_state(n=2),
                 lambda: e.stepenv_set_state(np.zeros((2, 1)), indices=np.arange(2, dtype=np.int32)))
        for call in calls:
            with pytest.raises(_lib.DneError, match=S.REFUSED["kind"] + r" \(this one: kind 0\)"):
                call()
        assert e.stepenv_last_ms() == -1.0
    finally:
        e.close()
