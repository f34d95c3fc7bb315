"""CPU: the maze, the cart-pole and the pendulum one step at a time outside the kernels -- csrc/step_env.h compiled for the host
(dne_stepenv_reset_host / _step_host / _observe_host, no GPU and no handle) against what the project already trusts, BIT FOR BIT: stepping one
action at a time equals dne_maze_actions_host / dne_cartpole_actions_host / dne_pendulum_actions_host over those tests' own sequences;
envs.rollout with the host forward twin as the policy equals dne_*_rollout_host in returns, lengths and final states; a done environment
stays as it is; subsets, the refusals, envs.make; the .so exports what the header declares; and the header under AddressSanitizer + UBSan in a
stand-alone program.  The Python classes run on stepenv_support.StepEnvHostEngine."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cartpole_support as CS
import maze_support as MS
import pendulum_support as PS
import stepenv_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the widths, the symbols ------------------------------------------------------------------------------------------------------------------
def test_dims_of_the_three_kinds_and_of_no_other():
    from dne_hip import _lib
    for kind in S.KINDS:
        assert _lib.stepenv_dims(S.kind_id(kind)) == S.DIMS[kind]
    assert _lib.STEPENV_KINDS == (4, 5, 6)
    for kind in (0, 1, 2, 3, 7, -1):
        assert _lib.load().dne_stepenv_dims(kind, None, None, None, None) == -1
        with pytest.raises(_lib.DneError, match="kind %d has no step-at-a-time environment" % kind):
            _lib.stepenv_dims(kind)
    assert _lib.load().dne_stepenv_dims(_lib.KIND_MAZE, None, None, None, None) == 0      # a NULL output is skipped


def test_library_exports_every_symbol_the_header_declares():
    from dne_hip import _lib
    text = open(os.path.join(ROOT, "include", "dne_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(dne_[a-z0-9_]+)\s*\(", text)))
    assert len(names) > 100 and {"dne_stepenv_dims", "dne_stepenv_reset", "dne_stepenv_step_f32", "dne_stepenv_step_i32", "dne_stepenv_observation",
                                 "dne_stepenv_get_state", "dne_stepenv_set_state", "dne_stepenv_reset_host", "dne_stepenv_step_host"} <= set(names)
    lib = _lib.load()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


# ---- 2. open loop: one action at a time equals the open-loop steppers ----------------------------------------------------------------------------
def test_maze_steps_equal_actions_host():
    from dne_hip import _lib
    header, lines = MS.fixture_maze()
    acts = np.load(MS.RECORDING)["actions"]                                  # [32][400][2]: test_maze_cpu.py's sequences
    rows, obs0 = _lib.maze_actions_host(acts, header, lines)
    n = acts.shape[0]
    for max_steps in (0, 50):
        limit = 400 if max_steps == 0 else max_steps
        st, steps, lim, done, obs = _lib.stepenv_reset_host(_lib.KIND_MAZE, n, None, max_steps, header, lines)
        assert S.same(obs, obs0) and np.all(steps == 0) and np.all(done == 0) and np.all(lim == limit)
        assert S.same(st, np.tile(np.array([header[2], header[3], 0, 0, 0, 0, 0], np.float64), (n, 1)))
        for t in range(limit):
            rew = _lib.stepenv_step_host(_lib.KIND_MAZE, acts[:, t], st, steps, lim, done, obs, header, lines)
            assert S.same(obs, rows[:, t, :11]), t
            assert S.same(st[:, :5], rows[:, t, 11:16].astype(np.float64)) and np.array_equal(st[:, 6], rows[:, t, 16]), t
            assert np.all(steps == t + 1) and np.all(done == (t + 1 == limit))
            # the reward: final_reward on step 400, 0 on every other step -- and 0 throughout under a smaller limit, as maze::rollout_host
            assert S.same(rew, rows[:, t, 17]) and (np.all(rew < 0) if t == 399 else np.all(rew == 0)), t
        frozen = [a.copy() for a in (st, steps, done, obs)]
        for t in range(3):
            rew = _lib.stepenv_step_host(_lib.KIND_MAZE, acts[:, t], st, steps, lim, done, obs, header, lines)
            assert S.same(rew, np.zeros(n, np.float32)) and all(S.same(a, b) for a, b in zip((st, steps, done, obs), frozen))


@pytest.mark.parametrize("name", ("zeros", "ones", "alternating", "random0"))
def test_cartpole_steps_equal_actions_host(name):
    from dne_hip import _lib
    a, init = next((a, init) for nm, a, init in CS.open_loop_cases() if nm == name)
    rows = _lib.cartpole_actions_host(a[None], init[None])[0]
    k = CS.first_done(rows)
    assert k < a.size and rows[k - 1, 4] == 1                                  # each of these sequences ends before it runs out
    e = S.host_engine("cartpole", 2)
    e.stepenv_set_state(init[None], indices=[1])
    assert S.same(e.stepenv_observation([1])[0], init.astype(np.float32))
    for t in range(a.size):
        rew, done = e.stepenv_step(a[t:t + 1], [1])
        st, steps, dn = e.stepenv_state([1])
        if t < k:                                                               # the episode: every double of every step, reward 1 the last step included
            assert S.same(st[0], rows[t, :4]) and steps[0] == t + 1 and rew[0] == 1.0
            assert done[0] == bool(rows[t, 4]) == (t == k - 1) and dn[0] == done[0]
            assert S.same(e.stepenv_observation([1])[0], rows[t, :4].astype(np.float32))
        else:                                                                   # past done actions_host steps on; the environment does not
            assert S.same(st[0], rows[k - 1, :4]) and steps[0] == k and rew[0] == 0.0 and done[0]


@pytest.mark.parametrize("name", ("plus2_0", "minus2_0", "zero_0", "random0"))
def test_pendulum_steps_equal_actions_host(name):
    from dne_hip import _lib
    a, init = next((a, init) for nm, a, init in PS.open_loop_cases() if nm == name)
    rows = _lib.pendulum_actions_host(a[None], init[None])[0]
    e = S.host_engine("pendulum", 2)
    e.stepenv_set_state(init[None], indices=[0])
    assert S.same(e.stepenv_observation([0])[0], PS.obs_py(init))
    for t in range(a.size):
        rew, done = e.stepenv_step(a[t:t + 1], [0])
        st, steps, _ = e.stepenv_state([0])
        assert S.same(st[0], rows[t, :2]) and S.same(rew[0], np.float32(rows[t, 2])) and steps[0] == t + 1 and done[0] == (t == 199), t
        if t % 37 == 0:
            assert S.same(e.stepenv_observation([0])[0], PS.obs_py(st[0]))
    assert a.size == 200
    rew, done = e.stepenv_step(a[:1], [0])
    assert rew[0] == 0 and done[0] and S.same(e.stepenv_state([0])[0][0], rows[-1, :2])


def test_reset_equals_the_reset_twins():
    from dne_hip import _lib
    seeds = S.mixed_seeds(6)
    st, steps, lim, done, obs = _lib.stepenv_reset_host(_lib.KIND_CARTPOLE, 6, seeds)
    assert S.same(st, np.stack([_lib.cartpole_reset_host(s) for s in seeds])) and S.same(obs, st.astype(np.float32)) and np.all(lim == 500)
    st, steps, lim, done, obs = _lib.stepenv_reset_host(_lib.KIND_PENDULUM, 6, seeds, 5000)
    assert S.same(st, np.stack([_lib.pendulum_reset_host(s) for s in seeds])) and np.all(lim == 200) and np.all(steps == 0) and not done.any()
    assert S.same(obs, np.stack([PS.obs_py(s) for s in st]))
    for max_steps, want in ((-1, 200), (0, 200), (1, 1), (199, 199), (200, 200), (201, 200)):
        assert np.all(_lib.stepenv_reset_host(_lib.KIND_PENDULUM, 2, seeds[:2], max_steps)[2] == want)
    # the observation of a given state: the same function
    assert S.same(_lib.stepenv_observe_host(_lib.KIND_PENDULUM, st), obs)


# ---- 3. closed loop: envs.rollout under the host forward twin equals the whole-episode twins --------------------------------------------------------
@pytest.mark.parametrize("kind,hidden,nonlin", (("maze", 0, ""), ("cartpole", 0, ""), ("pendulum", 64, "tanh"), ("pendulum", 256, "relu")))
def test_rollout_equals_rollout_host(kind, hidden, nonlin):
    from dne_hip import envs
    thetas = S.closed_loop_thetas(kind, hidden or 64)
    seeds = S.mixed_seeds(5)
    env = envs.make(S.GAMES[kind], 5, engine=S.host_engine(kind, 5))
    for max_frames, tslimit in ((None, 5000), (7, 7)):
        ret, ln = envs.rollout(env, S.policy(kind, thetas, hidden, nonlin), seeds=seeds, max_frames=max_frames)
        hret, hln, hfinal = S.rollout_host(kind, thetas, seeds, tslimit, hidden, nonlin)
        print(kind, "lengths", ln.tolist(), "returns", ret.tolist())
        assert ret.dtype == np.float32 and ln.dtype == np.int32
        assert S.same(ret, hret) and np.array_equal(ln, hln) and S.same(S.final_of(kind, env), hfinal), (kind, max_frames)
        assert env.state()[2].all() and np.array_equal(env.state()[1], hln)
    if kind == "cartpole":                                                       # theta = 0 ends at once, the episodes differ
        ret, ln = envs.rollout(env, S.policy(kind, thetas), seeds=seeds)
        assert ln[0] in (9, 10, 11) and len(set(ln.tolist())) >= 3 and ln.max() > 3 * ln[0]
        e = S.host_engine(kind, 1)
        e.stepenv_set_state(np.array([CS.BALANCE_INIT]))                        # the balanced case: 500 steps from BALANCE_INIT
        act, total = S.policy(kind, thetas[1:2]), 0.0
        for t in range(500):
            rew, done = e.stepenv_step(act(e.stepenv_observation(n=1)))
            total += float(rew[0])
            assert done[0] == (t == 499)
        assert total == 500.0 and e.stepenv_state(n=1)[0][0, 0] == CS.BALANCE_FINAL_X
    env.close()


# ---- 4. done, set_state, limits, subsets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_done_environments_keep_every_bit(kind):
    S.check_done_freezes(S.host_engine(kind), kind)


@pytest.mark.parametrize("kind", S.KINDS)
def test_set_state(kind):
    S.check_set_state(S.host_engine(kind), kind)


def test_maze_limits():
    S.check_maze_limits(S.host_engine("maze"))


@pytest.mark.parametrize("kind", S.KINDS)
def test_subsets_and_the_order_of_the_list(kind):
    S.check_subsets(S.host_engine(kind), kind)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_refusals_leave_the_batch_alone(kind):
    S.check_refusals(S.host_engine(kind), kind, lambda: S.StepEnvHostEngine(kind, 8))


def test_host_twins_refuse_by_name():
    from dne_hip import _lib
    header, lines = MS.fixture_maze()
    for kind in (0, 1, 2, 3, 7):
        with pytest.raises(_lib.DneError, match="kind %d has no step-at-a-time environment" % kind):
            _lib.stepenv_reset_host(kind, 1, [0])
    lib = _lib.load()
    assert lib.dne_stepenv_step_host(2, 1, None, None, None, 0, None, None, None, None, None, None) == -1
    assert b"dne_stepenv_step_host: kind 2" in lib.dne_last_error(None)
    with pytest.raises(_lib.DneError, match="seeds is NULL"):
        _lib.stepenv_reset_host(_lib.KIND_CARTPOLE, 2, None)
    with pytest.raises(_lib.DneError, match="seeds is NULL"):
        _lib.stepenv_reset_host(_lib.KIND_PENDULUM, 2, None)
    with pytest.raises(_lib.DneError, match="at least one environment"):
        _lib.stepenv_reset_host(_lib.KIND_PENDULUM, 0, None)
    with pytest.raises(_lib.DneError, match="65 walls"):
        _lib.stepenv_reset_host(_lib.KIND_MAZE, 1, None, 0, header, np.zeros((65, 4), np.float32))
    with pytest.raises(_lib.DneError, match="header and lines"):
        _lib.stepenv_reset_host(_lib.KIND_MAZE, 1, None)
    batch = _lib.stepenv_reset_host(_lib.KIND_CARTPOLE, 3, [1, 2, 3])
    before = [a.copy() for a in batch]
    with pytest.raises(_lib.DneError, match="action 2 at position 1, CartPole-v1 has actions 0 and 1"):
        _lib.stepenv_step_host(_lib.KIND_CARTPOLE, [0, 2, 1], *batch)
    assert all(S.same(a, b) for a, b in zip(batch, before))
    with pytest.raises(_lib.DneError, match="6 action values, 3 given"):
        _lib.stepenv_step_host(_lib.KIND_MAZE, np.zeros(3, np.float32), *_lib.stepenv_reset_host(_lib.KIND_MAZE, 3, None, 0, header, lines), header, lines)


# ---- 6. envs.py -----------------------------------------------------------------------------------------------------------------------------------------
def test_envs_surface_and_make_refusals():
    from dne_hip import _lib, envs
    for name in ("frostbite", "gym.CartPole-v0", "gym.MountainCar-v0", "Pendulum-v1"):
        with pytest.raises(NotImplementedError, match=re.escape(name)):
            envs.make(name, 4)
    with pytest.raises(ValueError, match="'maze'.*kind 5"):
        envs.make("maze", 4, engine=S.host_engine("cartpole", 8))
    with pytest.raises(ValueError, match="gym.CartPole-v1.*kind 6"):
        envs.make("gym.CartPole-v1", 4, engine=S.host_engine("pendulum", 8))
    with pytest.raises(ValueError, match="batch of 9 environments, the engine passed in holds 8"):
        envs.make("Pendulum-v0", 9, engine=S.host_engine("pendulum", 8))
    with pytest.raises(ValueError, match="batch of 0"):
        envs.make("Pendulum-v0", 0, engine=S.host_engine("pendulum", 8))
    want = {"maze": (envs.HipMazeEnv, (11,), 2, False, 400), "cartpole": (envs.HipCartPoleEnv, (4,), 2, True, 500),
            "pendulum": (envs.HipPendulumEnv, (3,), 1, False, 200)}
    for kind in S.KINDS:
        cls, ob, ac, disc, cutoff = want[kind]
        env = envs.make(S.GAMES[kind], 4, engine=S.host_engine(kind, 8), seed=11)
        assert type(env) is cls and env.batch_size == 4 and env.observation_space == ob and env.action_space == ac
        assert env.discrete_action is disc and env.env_default_timestep_cutoff == cutoff and env.unwrapped is env
        env.reset()                                                             # seeds=None: drawn from RandomState(seed)
        first = env.state()[0]
        assert env.observation().shape == (4,) + ob and env.observation().dtype == np.float32
        rew, done = env.step(S.scripted_actions(kind, 4, 1)[0])
        assert rew.dtype == np.float32 and rew.shape == (4,) and done.dtype == bool and not done.any()
        assert env.final_state().shape == (4, 2) and env.final_state().dtype == np.float32 and env.final_state([1, 3]).shape == (2, 2)
        if kind == "maze":
            assert S.same(env.final_state(), env.state()[0][:, :2].astype(np.float32)) and np.all(env.final_state() != 0)
        else:
            assert not env.final_state().any()                                  # PythonEnv.final_state: zeros
            again = envs.make(S.GAMES[kind], 4, engine=S.host_engine(kind, 8), seed=11)
            again.reset()
            assert S.same(again.state()[0], first) and len({tuple(r) for r in first.tolist()}) == 4
            again.reset(indices=[2], max_frames=3)
            assert not S.same(again.state()[0][2], first[2]) and S.same(again.state()[0][[0, 1, 3]], first[[0, 1, 3]])
        env.reset(indices=[0, 2], max_frames=1, seeds=[5, 6])
        rew, done = env.step(S.scripted_actions(kind, 4, 1)[0])
        assert done.tolist() == [True, False, True, False]
        env.close()
        assert env.engine is None
    # the maze file: the drivers' rule (maze_run.maze_file)
    eng = S.StepEnvHostEngine("maze", 4)
    env = envs.make("maze", 2, engine=eng, maze_file=MS.MAZE_FILE)
    assert eng.lines is not None and eng.lines.shape == MS.fixture_maze()[1].shape
    with pytest.raises(FileNotFoundError, match="no_such_maze"):
        envs.make("maze", 2, engine=eng, maze_file="no_such_maze.txt")
    assert _lib.KIND_MAZE == env.kind


def test_design_quotes_the_measurement():
    """profiles/r15_stepenv_time.json is what tools/stepenv_time.py wrote, and DESIGN.md section 15 carries its figures"""
    import json
    d = json.loads(open(os.path.join(ROOT, "profiles", "r15_stepenv_time.json")).read().strip().splitlines()[-1])
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    text = text[text.index("## 15. "):]
    assert d["tool"] == "stepenv_time" and d["batch"] == 1000 and d["reps"] == 30 and d["warmup"] == 3
    for kind in S.KINDS:
        r = d[kind]
        assert r["identical"] is True and r["step_ms_range"][0] <= r["step_ms"] <= r["step_ms_range"][1] and r["kernel_ms"] < r["step_ms"]
        assert "**%.1f µs** (%.1f … %.1f)" % (1e3 * r["step_ms"], 1e3 * r["step_ms_range"][0], 1e3 * r["step_ms_range"][1]) in text, kind
        assert "%.1f µs (%.1f … %.1f)" % (1e3 * r["kernel_ms"], 1e3 * r["kernel_ms_range"][0], 1e3 * r["kernel_ms_range"][1]) in text, kind
        assert "| %.1f µs |" % (1e3 * r["episode_ms_per_step"]) in text, kind


# ---- 7. the header under AddressSanitizer and UBSan, in a program of its own ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/stepenv_asan_main.cpp, built once from step_env.h alone: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(ROOT, "tests", "stepenv_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("stepenv_asan") / "stepenv_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program):
    out = subprocess.run([sanitizer_program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = out.stdout.split()
    # 3 limits x 3 kinds x 3 environments; outside the contract 2 kinds x 5 actions + 3 kinds x 6 states
    assert tok[:2] == ["ok", "27"] and tok[3] == "facts" and int(tok[4]) > 1000 and tok[5:] == ["wild", "28"], out.stdout
