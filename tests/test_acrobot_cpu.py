"""CPU: gym.Acrobot-v1 outside the kernels -- csrc/acrobot.h compiled for the host behind dne_stepenv_*_host, dne_acrobot_actions_host and
dne_dense_*_host on environment id 9 (DNE_ENV_ACROBOT).  The twins against the contract in plain Python, bit for bit (reset, every action,
500-step open-loop sequences, hand-placed states on the terminal threshold, at +-pi, at the velocity clamps, NaN); the contract's distance to a
libm restatement in gym's spelling, and the issue's three anchors; early termination and full runs of the named members; the dense shapes and
the three-way argmax; the four drivers on AcrobotHostEngine; what stays refused; and the headers under AddressSanitizer + UBSan in a
stand-alone program.  DESIGN.md section 19."""
import math
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import acrobot_support as A
import dense_support as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def open_loop():
    """name -> (actions, init, the twin's rows [500][5], the contract's rows)"""
    from dne_hip import _lib
    return {name: (a, init, _lib.acrobot_actions_host(a[None], init[None])[0], A.actions_py(a, init)) for name, a, init in A.open_loop_cases()}


@pytest.fixture(scope="module")
def random_set():
    """the 200 random LinearClassifier members: their whole-episode twin results and their lock-step traces"""
    th, seeds = A.random_members()
    return th, seeds, A.rollout(th, (), "relu", seeds), A.traces(th, (), "relu", seeds)


# ---- 1. the contract against the twin ----------------------------------------------------------------------------------------------------------
def test_ids_and_dims():
    from dne_hip import _lib
    text = open(os.path.join(ROOT, "include", "dne_hip.h")).read()
    assert "#define DNE_ENV_ACROBOT 9" in text and _lib.ENV_ACROBOT == 9 and _lib.ACROBOT_STEPS == 500
    assert _lib.STEPENV_KINDS == (4, 5, 6) and _lib.STEP_ENVS == (4, 5, 6, 9)
    assert _lib.stepenv_dims(_lib.ENV_ACROBOT) == (6, 1, 4, True)
    assert _lib.dense_bc_dim(_lib.ENV_ACROBOT) == 4
    assert hasattr(_lib.load(), "dne_acrobot_actions_host")


def test_reset_is_the_cartpole_stream_over_twice_the_width():
    from dne_hip import _lib
    assert tuple(A.reset_py(0)) == A.SEED0_STATE
    seeds = np.array([0, 1, 2 ** 32 - 1], np.uint32)
    state, steps, limit, done, obs = _lib.stepenv_reset_host(A.ENV, 3, seeds)
    for i, seed in enumerate(seeds.tolist()):
        want = np.array(A.reset_py(seed))
        assert A.same(state[i], want) and np.all(want >= -0.1) and np.all(want < 0.1)
        assert A.same(obs[i], A.obs_py(want))
    assert tuple(state[0].tolist()) == A.SEED0_STATE
    assert steps.tolist() == [0, 0, 0] and limit.tolist() == [500, 500, 500] and done.tolist() == [0, 0, 0]
    for max_steps, want in ((7, 7), (500, 500), (5000, 500), (0, 500), (-3, 500)):   # a larger cutoff leaves 500 in force
        assert _lib.stepenv_reset_host(A.ENV, 1, [5], max_steps)[2][0] == want


def test_every_action_from_every_reset_and_the_reward():
    from dne_hip import _lib
    seeds = np.array([0, 1, 2 ** 32 - 1], np.uint32)
    for a in range(3):
        batch = _lib.stepenv_reset_host(A.ENV, 3, seeds)
        rew = _lib.stepenv_step_host(A.ENV, np.full(3, a, np.int32), *batch)
        for i, seed in enumerate(seeds.tolist()):
            want, over = A.step_py(A.reset_py(seed), a)
            assert A.same(batch[0][i], np.array(want)) and A.same(batch[4][i], A.obs_py(want)) and not over
        assert rew.tolist() == [-1.0] * 3 and batch[1].tolist() == [1] * 3 and batch[3].tolist() == [0] * 3


def test_open_loop_sequences_bit_for_bit(open_loop):
    """500 steps under all-0, all-2, alternating and random actions: the stand-alone stepper, the contract, and the step twin one action at a time"""
    from dne_hip import _lib
    for name, (acts, init, rows, want) in open_loop.items():
        assert rows.shape == (500, 5) and A.same(rows, want), name
    acts, init, rows, _ = open_loop["random"]
    batch = _lib.stepenv_reset_host(A.ENV, 1, [0])
    assert A.same(batch[0][0], init)
    for t in range(500):
        rew = _lib.stepenv_step_host(A.ENV, acts[t:t + 1], *batch)
        if batch[3][0]:
            break
        assert A.same(batch[0][0], rows[t, :4]) and rew[0] == -1.0 and batch[1][0] == t + 1
    over = np.flatnonzero(rows[:, 4])
    assert batch[1][0] == (over[0] + 1 if over.size else 500) and A.same(batch[0][0], rows[batch[1][0] - 1, :4])
    # the random sequence drives the system hard: the velocities leave the reset's range by two orders of magnitude
    assert np.abs(rows[:, 2]).max() > 3.0 and np.abs(rows[:, 3]).max() > 8.0


def _step_twin(state, a, steps=0, max_steps=0):
    """one step of one hand-placed state on the twin -> (state', reward, done, obs')"""
    from dne_hip import _lib
    batch = list(_lib.stepenv_reset_host(A.ENV, 1, [0], max_steps))
    batch[0][0] = state
    batch[1][0] = steps
    batch[4][:] = _lib.stepenv_observe_host(A.ENV, batch[0])
    rew = _lib.stepenv_step_host(A.ENV, np.array([a], np.int32), *batch)
    return batch[0][0], float(rew[0]), bool(batch[3][0]), batch[4][0]


def test_the_terminal_threshold_is_strict():
    """states whose step lands ON -cos(th1) - cos(th1 + th2) == 1.0, one ulp below and one ulp above: only the last is terminal, at reward 0"""
    found = A.threshold_states()
    assert set(found) == {"equal", "below", "above"}
    for name, state in found.items():
        want, over = A.step_py(state, 1)
        got, rew, done, obs = _step_twin(state, 1)
        v = A.terminal_value(want)
        assert A.same(got, np.array(want)) and A.same(obs, A.obs_py(want))
        assert v == {"equal": 1.0, "below": np.nextafter(1.0, 0.0), "above": np.nextafter(1.0, 2.0)}[name]
        assert done == over == (name == "above") and rew == (0.0 if done else -1.0), name
    # the last step of the limit is done without being terminal: reward -1
    got, rew, done, _ = _step_twin(found["below"], 1, steps=6, max_steps=7)
    assert done and rew == -1.0


def test_hand_placed_states_pi_clamps_and_nan():
    from dne_hip import _lib
    hit1 = hit2 = inside1 = inside2 = 0
    for state in A.edge_states():
        finite = all(math.isfinite(v) for v in state)
        for a in range(3):
            want, over = A.step_py(state, a)
            got, rew, done, obs = _step_twin(state, a)
            assert A.same_nan(got, np.array(want)) and A.same_nan(obs, A.obs_py(want)) and done == over, (state, a)
            if finite:
                assert A.same(got, np.array(want)) and -A.PI <= got[0] <= A.PI and -A.PI <= got[1] <= A.PI
                assert abs(got[2]) <= A.MAX_VEL_1 and abs(got[3]) <= A.MAX_VEL_2
                hit1 += abs(got[2]) == A.MAX_VEL_1; hit2 += abs(got[3]) == A.MAX_VEL_2
                inside1 += abs(state[2]) == np.nextafter(A.MAX_VEL_1, 0.0); inside2 += abs(state[3]) == np.nextafter(A.MAX_VEL_2, 0.0)
            else:                                                         # a NaN state is never done, and what the policy sees is NaN
                assert not done and rew == -1.0 and np.isnan(got).all() and np.isnan(obs).all()
    assert hit1 and hit2 and inside1 and inside2                          # both clamps were reached, and states one ulp inside each were stepped
    # the floor form sends pi to -pi (gym keeps pi): ours, and the same angle
    assert A.norm_angle(A.PI) == -A.PI and _lib.pendulum_math_host("norm", [A.PI, -A.PI])[0] == -A.PI
    ob = _lib.stepenv_observe_host(A.ENV, np.array([[A.PI, -A.PI, 1.0, -2.0], [float("nan"), 0.0, 0.0, 0.0]]))
    assert A.same(ob[0], A.obs_py((A.PI, -A.PI, 1.0, -2.0))) and ob[0, 0] == -1.0 and ob[0, 2] == -1.0 and np.isnan(ob[1, :2]).all() and ob[1, 2] == 1.0


# ---- 2. the distance to libm in gym's spelling -----------------------------------------------------------------------------------------------------
def test_distance_to_libm_and_the_anchors(open_loop):
    """every state the open-loop sequences visit, stepped once by the contract and by the libm restatement: the largest difference of a state
    value (an angle at pi and one at -pi being the same angle) within four times the measured one; the same terminal flag; the issue's anchors"""
    worst, flips = 0.0, 0
    for name, (acts, init, rows, _) in open_loop.items():
        states = [init] + [r[:4] for r in rows[:-1]]
        for s, a in zip(states, acts):
            c, over_c = A.step_py(s, int(a))
            l, over_l = A.step_libm(s, int(a))
            worst = max(worst, A.state_gap(c, l))
            flips += over_c != over_l
    print("largest |contract - libm| after one step:", repr(worst), "(measured: %r)" % A.MEASURED_LIBM)
    assert A.TOL_LIBM == 4 * A.MEASURED_LIBM and worst <= A.TOL_LIBM and flips == 0
    s = [0.0, 0.0, 0.0, 0.0]
    for a, anchor in zip(A.ANCHOR_ACTIONS, A.ANCHORS):
        s, _ = A.step_py(s, a)
        assert A.state_gap(s, anchor) <= A.TOL_LIBM, (a, s, anchor)


# ---- 3. early termination and the full run, on the twin alone ----------------------------------------------------------------------------------------
def test_the_solving_member_ends_early_and_the_zero_member_never():
    seeds = np.arange(20, dtype=np.uint32)
    r = A.rollout(np.stack([A.solver_theta()] * 20), (), "relu", seeds)
    assert np.all(r["lengths"] < 500) and np.all(r["lengths"] > 1)
    assert A.same(r["returns"], (-(r["lengths"] - 1)).astype(np.float32)) and A.same(r["signreturns"], r["returns"])
    for i in range(20):                                                    # the final state is terminal, and it is the first such state
        assert A.terminal_value(r["state"][i]) > 1.0
    z = A.rollout(np.stack([A.zero_theta()] * 20), (), "relu", seeds)
    assert z["lengths"].tolist() == [500] * 20 and z["returns"].tolist() == [-500.0] * 20
    zero_actions = A.actions_py(np.zeros(500, np.int32), A.reset_py(3))    # action 0 always: the open-loop stepper gives the same end
    assert A.same(z["state"][3], zero_actions[-1, :4]) and not zero_actions[:, 4].any()
    # a cutoff is honoured, and a larger one leaves 500 in force
    for limit, want in ((1, 1), (7, 7), (499, 499), (5000, 500)):
        assert A.rollout(A.zero_theta()[None], (), "relu", [0], limit)["lengths"][0] == want


def test_two_hundred_random_members(random_set):
    th, seeds, whole, tr = random_set
    assert A.same(tr["lengths"], whole["lengths"]) and A.same(tr["returns"], whole["returns"]) and A.same(tr["states"][-1], whole["state"])
    ln, states = whole["lengths"], tr["states"]
    early = ln < 500
    assert early.any() and (~early).any()
    assert A.same(whole["returns"], (-(ln - early)).astype(np.float32))
    assert (np.abs(states[:, :, 2]) == A.MAX_VEL_1).any() or (np.abs(states[:, :, 3]) == A.MAX_VEL_2).any()   # a clamp is hit (each one: the hand-placed states)
    assert np.abs(states[:, :, 2]).max() <= A.MAX_VEL_1 and np.abs(states[:, :, 3]).max() <= A.MAX_VEL_2
    assert (np.abs(np.diff(states[:, :, :2], axis=0)) > A.PI).any()        # an angle wraps: a jump of more than pi between two steps
    assert np.abs(states[:, :, :2]).max() <= A.PI


# ---- 4. dense shapes ------------------------------------------------------------------------------------------------------------------------------------
def test_shapes_and_their_refusals():
    from dne_hip import _lib, policies
    # (5, 33): 6 * 5 + 5 + 5 * 33 + 33 + 33 * 3 + 3 = 335
    for hidden, P in (((), 21), ((16, 16), 435), ((5, 33), 335), ((64, 64, 64), 8963)):
        assert _lib.dense_num_params(A.ENV, hidden, 3) == P == A.num_params(hidden)
        assert policies.dense_scale_by(A.ENV, hidden, 3).shape == (P,)
    for hidden, n_out in (((), 2), ((), 1), ((), 4), ((65,), 3), ((16, 65), 3), ((1, 2, 3, 4), 3), ((0,), 3)):
        assert _lib.dense_num_params(A.ENV, hidden, n_out) == -1, (hidden, n_out)
    th, obs = np.zeros(21, np.float32), np.zeros((1, 6), np.float32)
    for match, args in ((r"has 3 outputs on environment 9 .* n_actions 2 is refused", (A.ENV, (), "relu", 2)),
                        (r"hidden widths 1\.\.64; width 65 of hidden layer 1 is refused", (A.ENV, (3, 65), "relu", 3)),
                        (r"0\.\.3 hidden layers; 4 hidden layers are refused", (A.ENV, (1, 2, 3, 4), "relu", 3))):
        with pytest.raises(_lib.DneError, match=match):
            _lib.dense_forward_host(th, obs, *args)
        with pytest.raises(_lib.DneError, match=match):
            _lib.dense_rollout_host(th, *args, seeds=[1])
    with pytest.raises(_lib.DneError, match="seeds is NULL"):
        _lib.dense_rollout_host(th[None], A.ENV, (), "relu", 3)
    sb = policies.dense_scale_by(A.ENV, (16, 16), 3)                       # SimpleClassifier: the out layer at std 0.1
    f = np.float32
    want = np.concatenate([np.full(96, f(1.0 / np.sqrt(6))), np.zeros(16), np.full(256, f(1.0 / 4)), np.zeros(16), np.full(48, f(0.1 / 4)), np.zeros(3)]).astype(f)
    assert A.same(sb, want)


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "x".join(str(w) for w in s[0]) or "linear")
def test_forward_matches_the_fmaf_chains(shape):
    from dne_hip import _lib
    hidden, nl = shape
    P = A.num_params(hidden)
    rs = np.random.RandomState(5)
    tab = D.noise()
    th = np.stack([tab[k * 997:k * 997 + P] * np.float32(s) for k, s in enumerate((0.3, 1.0, 3.0, -1.0))])
    obs = rs.uniform(-2, 2, (4, 6)).astype(np.float32)
    layers, out, act = _lib.dense_forward_host(th, obs, A.ENV, hidden, nl, 3)
    want_layers, want_out = A.forward_np(hidden, nl, th, obs)
    assert A.same(layers, want_layers) and A.same(out, want_out) and out.shape == (4, 3)
    assert act.dtype == np.int32 and act.tolist() == [A.pick_action(o) for o in want_out]


def test_the_three_way_argmax_on_ties_and_nan():
    """all weights 0: the outputs are the last biases.  Exact ties of two and of three logits give the first maximum; a NaN never wins"""
    from dne_hip import _lib
    one, up, nan = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)), np.float32("nan")
    cases = (((one, one, one), 0), ((up, up, one), 0), ((one, up, up), 1), ((up, one, up), 0), ((one, one, up), 2), ((one, up, one), 1),
             ((np.float32(-0.0), np.float32(0.0), np.float32(0.0)), 0), ((nan, nan, nan), 0), ((nan, one, up), 0), ((one, nan, up), 2),
             ((one, up, nan), 1), ((one, nan, nan), 0), ((nan, -one, nan), 0), ((np.float32("-inf"), np.float32("-inf"), np.float32("-inf")), 0),
             ((np.float32("-inf"), one, np.float32("inf")), 2))
    for hidden, nl in A.SHAPES:
        th = np.zeros((len(cases), A.num_params(hidden)), np.float32)
        for i, (b, _) in enumerate(cases):
            th[i, -3:] = b
        _, out, act = _lib.dense_forward_host(th, np.ones((len(cases), 6), np.float32), A.ENV, hidden, nl, 3)
        assert A.same_nan(out, (np.float32(0.0) + np.array([c[0] for c in cases], np.float32)).astype(np.float32))   # (+0.0 + b: a bias of -0.0 leaves +0.0)
        assert act.tolist() == [c[1] for c in cases] == [A.pick_action(c[0]) for c in cases]


# ---- 5. envs.py -----------------------------------------------------------------------------------------------------------------------------------------
def test_envs_make_rollout_and_run():
    from dne_hip import _lib, envs
    eng = A.host_engine((), "relu", 8)
    env = envs.make(A.GAME, 5, engine=eng, seed=11)
    assert type(env) is envs.HipAcrobotEnv and env.observation_space == (6,) and env.action_space == 3 and env.discrete_action is True
    assert env.env_default_timestep_cutoff == 500 and env.batch_size == 5
    th = np.stack([A.solver_theta(), A.zero_theta(), A.solver_theta(), A.random_members(2)[0][1], A.zero_theta()])
    seeds = np.array([3, 4, 5, 6, 7], np.uint32)
    want = A.rollout(th, (), "relu", seeds)
    policy = lambda obs: _lib.dense_forward_host(th, obs, A.ENV, (), "relu", 3)[2]
    ret, ln = envs.rollout(env, policy, seeds=seeds)
    assert A.same(ret, want["returns"]) and A.same(ln, want["lengths"]) and A.same(env.state()[0], want["state"])
    for k, t in enumerate(th):
        eng.set_theta(t, k)
    eng.set_members(np.arange(5, dtype=np.int32), np.zeros(5, np.int64), np.zeros(5, np.float32))
    ret, ln = envs.run(env, seeds=seeds)
    assert A.same(ret, want["returns"]) and A.same(ln, want["lengths"])
    ret, ln = envs.run(env, seeds=seeds, max_steps=37)                    # in rounds of 37: integer rewards, the split is exact
    assert A.same(ret, want["returns"]) and A.same(ln, want["lengths"])
    with pytest.raises(ValueError, match="gym.Acrobot-v1.*kind 8"):
        envs.make(A.GAME, 4, engine=D.host_engine(("cartpole", (), "relu"), 8))
    for name in ("gym.Acrobot-v0", "gym.MountainCar-v0", "gym.CartPole-v0"):
        with pytest.raises(NotImplementedError, match=name):
            envs.make(name, 4)


# ---- 6. the drivers on AcrobotHostEngine -----------------------------------------------------------------------------------------------------------------
def _finite_rows(log_dir, want):
    rows = D.log_rows(log_dir)
    assert len(rows) == want
    for row in rows:
        for key, val in row.items():
            if val not in ("None", "True", "False"):
                assert math.isfinite(float(val)), (key, val)
    return rows


def _other_game_engine():
    import dense_gans_support as GN
    return GN.host_engine(("cartpole", (), "relu"), 16)


@pytest.mark.parametrize("model", ("LinearClassifier", "SimpleClassifier"))
def test_es_driver(model, tmp_path):
    from dne_hip import acrobot_run, es_gpu
    hidden = acrobot_run.MODEL_HIDDEN[model]

    def run(log_dir, iters, eng=None, **over):
        eng = eng or A.host_engine(hidden, "relu", 16)
        return es_gpu.main(str(log_dir), engine=eng, noise=D.shared_noise(), seed=4, max_iters=iters, **A.es_exp(**dict({"model": model}, **over))), eng

    st2, e2 = run(tmp_path / "two", 2)
    rows = _finite_rows(tmp_path / "two", 2)
    assert st2.game == A.GAME and st2.model == model and st2.it == 2 and st2.num_params == e2.P == A.num_params(hidden) and st2.tslimit == 60
    assert all(-60.0 <= float(r["PopulationEpRewMean"]) <= 0.0 for r in rows) and rows[0]["PopulationEpCount"] == "16"
    assert st2.timesteps_so_far == st2.num_frames <= 2 * 16 * 60
    snap = pickle.load(open(tmp_path / "two" / "snapshot.pkl", "rb"))
    assert snap.game == A.GAME and snap.model == model and snap.flat_layout == "native" and snap.num_params == e2.P
    run(tmp_path / "one", 1)
    st1b, _ = run(tmp_path / "one", 1)                                    # resumes: one more iteration
    assert st1b.it == 2 and A.same(st1b.theta, st2.theta) and A.same(st1b.optimizer[0], st2.optimizer[0])
    with pytest.raises(ValueError, match=r"holds game 'gym.Acrobot-v1'; this run is game 'gym.CartPole-v1'"):
        es_gpu.main(str(tmp_path / "two"), engine=_other_game_engine(), noise=D.shared_noise(), seed=4, max_iters=1, **D.exp("gym.CartPole-v1"))
    # 'env_default' means 500, and a larger cutoff leaves 500 in force
    st, e = run(tmp_path / "default", 0, episode_cutoff_mode="env_default")
    assert st.tslimit is None and es_gpu._env_limit(e) == 500 and acrobot_run.step_limit(None) == 500 and acrobot_run.step_limit(5000) == 500
    # the name, the engine and the game have to agree
    with pytest.raises(ValueError, match="gym.Acrobot-v1.*kind 8 on environment kind 5"):
        run(tmp_path / "x", 1, eng=_other_game_engine())
    with pytest.raises(ValueError, match=r"game 'maze' asked for.*runs 'gym.Acrobot-v1'"):
        run(tmp_path / "x", 1, game="maze")
    with pytest.raises(ValueError, match="model 'ModelVirtualBN' asked for"):
        run(tmp_path / "x", 1, model="ModelVirtualBN")
    wide = A.host_engine((5, 33), "tanh", 16)                              # a caller's engine of any shape
    stw = es_gpu.main(str(tmp_path / "wide"), engine=wide, noise=D.shared_noise(), seed=4, max_iters=1, **A.es_exp(None))
    assert stw.model == "Dense(5, 33; tanh)" and stw.num_params == 335 and stw.game == A.GAME


@pytest.mark.parametrize("threshold", (4, 0))
def test_ga_driver(threshold, oracle, tmp_path):
    from dne_hip import ga_gpu

    def run(log_dir, iters, eng=None, **over):
        eng = eng or A.host_engine((16, 16), "relu", 16)
        return ga_gpu.dense_main(str(log_dir), engine=eng, noise=D.shared_noise(), seed=4, max_iters=iters,
                                 **A.ga_exp("SimpleClassifier", selection_threshold=threshold, **over)), eng

    (test2, val2, st2), e2 = run(tmp_path / "two", 2)
    _finite_rows(tmp_path / "two", 2)
    assert st2.game == A.GAME and st2.model == "SimpleClassifier" and st2.algo == "ga" and st2.it == 2 and st2.num_params == e2.P == 435
    assert math.isfinite(test2) and -500.0 <= test2 <= 0.0
    builds = [c for c in e2.calls if c[0] == "dense_ga_build"]
    assert (len(builds) == 0) == (threshold == 0)                          # selection_threshold 0 remains random search: roots every generation, no bank
    snap = pickle.load(open(tmp_path / "two" / "snapshot.pkl", "rb"))
    assert snap.game == A.GAME and snap.model == "SimpleClassifier"
    run(tmp_path / "one", 1)
    (test1b, _, st1b), _ = run(tmp_path / "one", 1)
    assert st1b.it == 2 and test1b == test2 and [o.seeds for o in st1b.population] == [o.seeds for o in st2.population]
    with pytest.raises(ValueError, match=r"holds game 'gym.Acrobot-v1' under model 'SimpleClassifier'; this run is game 'gym.CartPole-v1' under model 'LinearClassifier'"):
        ga_gpu.dense_main(str(tmp_path / "two"), engine=_other_game_engine(), noise=D.shared_noise(), seed=4, max_iters=1,
                          **A.ga_exp("LinearClassifier", game="gym.CartPole-v1"))
    # main routes the game to dense_main
    (_, _, stm), _ = (ga_gpu.main(str(tmp_path / "main"), engine=A.host_engine((), "relu", 16), noise=D.shared_noise(), seed=4, max_iters=1,
                                  **A.ga_exp("LinearClassifier", selection_threshold=threshold)), None)
    assert stm.game == A.GAME and stm.model == "LinearClassifier" and stm.num_params == 21


def test_ga_ns_driver(oracle, tmp_path):
    from dne_hip import ga_gpu
    ns = {"k": 3, "archive_prob": 0.3}

    def run(log_dir, iters, eng=None, **over):
        eng = eng or A.host_engine((), "relu", 16)
        return ga_gpu.dense_ns_main(str(log_dir), engine=eng, noise=D.shared_noise(), seed=4, max_iters=iters,
                                    **A.ga_exp("LinearClassifier", novelty_search=ns, **over)), eng

    (_, _, st2), e2 = run(tmp_path / "two", 2)
    rows = _finite_rows(tmp_path / "two", 2)
    assert st2.game == A.GAME and st2.model == "LinearClassifier" and st2.algo == "ga_ns" and st2.it == 2 and st2.num_params == 21
    assert st2.archive.shape[1] == 4 and int(rows[-1]["ArchiveSize"]) == len(st2.archive) > 0
    assert [c for c in e2.calls if c[0] == "dense_novelty_pool"] == [("dense_novelty_pool", 3)] * 2
    snap = pickle.load(open(tmp_path / "two" / "snapshot.pkl", "rb"))
    assert snap.game == A.GAME and snap.model == "LinearClassifier" and snap.k == 3
    run(tmp_path / "one", 1)
    (_, _, st1b), _ = run(tmp_path / "one", 1)
    assert st1b.it == 2 and A.same(st1b.archive, st2.archive) and [o.seeds for o in st1b.population] == [o.seeds for o in st2.population]
    with pytest.raises(ValueError, match=r"holds game 'gym.Acrobot-v1' under model 'LinearClassifier'; this run is game 'gym.CartPole-v1'"):
        ga_gpu.dense_ns_main(str(tmp_path / "two"), engine=_other_game_engine(), noise=D.shared_noise(), seed=4, max_iters=1,
                             **A.ga_exp("LinearClassifier", game="gym.CartPole-v1", novelty_search=ns))


@pytest.mark.parametrize("algo_type", ("ns", "nsr"))
def test_nses_driver(algo_type, tmp_path):
    from dne_hip import nses_gpu

    def run(log_dir, iters, eng=None, **over):
        eng = eng or A.host_engine((), "relu", 16)
        return nses_gpu.main(str(log_dir), engine=eng, noise=D.shared_noise(), seed=4, max_iters=iters, **A.ns_exp(algo_type, **over)), eng

    st2, e2 = run(tmp_path / "two", 2)
    _finite_rows(tmp_path / "two", 2)
    assert st2.game == A.GAME and st2.model == "LinearClassifier" and st2.it == 2 and st2.num_params == 21
    assert st2.archive.shape == (3 + 2, 4) and np.isfinite(st2.archive).all()
    snap = pickle.load(open(tmp_path / "two" / "snapshot.pkl", "rb"))
    assert snap.game == A.GAME and snap.model == "LinearClassifier" and snap.algo_type == algo_type
    run(tmp_path / "one", 1)
    st1b, _ = run(tmp_path / "one", 1)
    assert st1b.it == 2 and A.same(st1b.archive, st2.archive) and all(A.same(a, b) for a, b in zip(st1b.thetas, st2.thetas))
    with pytest.raises(ValueError, match=r"holds game 'gym.Acrobot-v1', model 'LinearClassifier', P = 21.*this run is game 'gym.CartPole-v1', model 'LinearClassifier', P = 10"):
        nses_gpu.main(str(tmp_path / "two"), engine=_other_game_engine(), noise=D.shared_noise(), seed=4, max_iters=1,
                      **A.ns_exp(algo_type, game="gym.CartPole-v1"))
    # SimpleClassifier names the (16, 16) relu shape here, for the caller's engine too
    sts, es = run(tmp_path / "simple", 1, eng=A.host_engine((16, 16), "relu", 16), model="SimpleClassifier")
    assert sts.model == "SimpleClassifier" and sts.num_params == 435


# ---- 7. still refused, by name ----------------------------------------------------------------------------------------------------------------------------
def test_still_refused_by_name(tmp_path):
    from dne_hip import _lib, es_gpu, ga_gpu, nses_gpu
    for game in ("gym.MountainCar-v0", "gym.CartPole-v0", "gym.Acrobot-v0"):
        with pytest.raises(NotImplementedError, match=game):
            es_gpu.main(str(tmp_path / "x"), engine=None, noise=D.shared_noise(), seed=4, max_iters=1, **A.es_exp(game=game))
        with pytest.raises(NotImplementedError, match=game):
            es_gpu.main(str(tmp_path / "x"), engine=A.host_engine((), "relu", 16), noise=D.shared_noise(), seed=4, max_iters=1, **A.es_exp(game=game))
        with pytest.raises(NotImplementedError, match=game):
            ga_gpu.dense_main(str(tmp_path / "x"), engine=None, noise=D.shared_noise(), seed=4, max_iters=1, **A.ga_exp(game=game))
        with pytest.raises(NotImplementedError, match=game):
            ga_gpu.dense_ns_main(str(tmp_path / "x"), engine=None, noise=D.shared_noise(), seed=4, max_iters=1,
                                 **A.ga_exp(game=game, novelty_search={"k": 2, "archive_prob": 0.1}))
        with pytest.raises(NotImplementedError, match=game):
            nses_gpu.main(str(tmp_path / "x"), engine=None, noise=D.shared_noise(), seed=4, max_iters=1, **A.ns_exp(game=game))
    with pytest.raises(NotImplementedError, match="ModelVirtualBN.*gym.Acrobot-v1"):   # without an engine the two named shapes, nothing else
        es_gpu.main(str(tmp_path / "x"), engine=None, noise=D.shared_noise(), seed=4, max_iters=1, **A.es_exp("ModelVirtualBN"))
    # dne_create(policy_kind = 9): an environment id is no engine kind.  (No device is needed to see it refused: without one the refusal is
    # "no HIP device visible", with one "bad config"; either way no handle.)
    cfg = _lib.Config(device_id=0, policy_kind=_lib.ENV_ACROBOT, n_actions=3, max_members=4)
    h = __import__("ctypes").c_void_p()
    assert _lib.load().dne_create(__import__("ctypes").byref(cfg), __import__("ctypes").byref(h)) != 0 and not h.value
    assert _lib.load().dne_num_params(_lib.ENV_ACROBOT, 3) == -1
    # action 3 in a batch: refused for the whole batch, nothing moved
    batch = _lib.stepenv_reset_host(A.ENV, 3, [1, 2, 3])
    before = [a.copy() for a in batch]
    with pytest.raises(_lib.DneError, match="action 3 at position 1, Acrobot-v1 has actions 0, 1 and 2"):
        _lib.stepenv_step_host(A.ENV, [0, 3, 1], *batch)
    with pytest.raises(_lib.DneError, match="action -1 at position 2"):
        _lib.stepenv_step_host(A.ENV, [0, 2, -1], *batch)
    assert all(A.same(a, b) for a, b in zip(batch, before))
    with pytest.raises(_lib.DneError, match="action 3, Acrobot-v1 has actions 0, 1 and 2"):
        _lib.acrobot_actions_host(np.array([[0, 3]], np.int32), np.zeros((1, 4)))
    with pytest.raises(_lib.DneError, match="seeds is NULL"):
        _lib.stepenv_reset_host(A.ENV, 2, None)


# ---- 8. the headers under AddressSanitizer and UBSan, in a program of their own -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/acrobot_asan_main.cpp, built once: address, undefined and float-cast-overflow (a NaN or an infinity reaching a cast to int)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(ROOT, "tests", "acrobot_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("acrobot_asan") / "acrobot_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program):
    out = subprocess.run([sanitizer_program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = out.stdout.split()
    # 2 x 20 episodes of the named members + 4 shapes x 3 members x 3 limits; outside the contract 4 shapes x (6 fills + 6 states)
    assert tok[:3] == ["ok", "episodes", "76"] and tok[4] == "facts" and int(tok[5]) >= 150 and tok[6:8] == ["wild", "48"], out.stdout
