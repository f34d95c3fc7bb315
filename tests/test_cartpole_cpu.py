"""CPU: gym.CartPole-v1 outside the kernel -- csrc/cartpole.h compiled for the host (dne_cartpole_reset_host / _actions_host / _forward_host /
_rollout_host, no GPU and no handle) against the contract restated in plain Python (tests/cartpole_support.py): the reset stream, the
open-loop step bit for bit, the facts of DESIGN.md section 13, the thresholds at equality, the closed loop, ties and NaN in the action
rule, the distance to a libm version of the step; P = 386, policies.flat_layout and simple_scale_by for the kind; the es_gpu.py driver with
exp['game'] = 'gym.CartPole-v1' on CartPoleHostEngine; and the header under AddressSanitizer + UBSan in a stand-alone program."""
import math
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import cartpole_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay():
    """{name: (actions, init, host rows, plain-Python rows)} of the open-loop sequences, once"""
    from dne_hip import _lib
    return {name: (a, init, _lib.cartpole_actions_host(a[None], init[None])[0], S.actions_py(a, init)) for name, a, init in S.open_loop_cases()}


# ---- 1. the reset ----------------------------------------------------------------------------------------------------------------------------
def test_reset_is_splitmix64_of_the_seed():
    from dne_hip import _lib
    assert tuple(S.splitmix_r(0)) == S.SEED0_R
    assert tuple(S.reset_py(0)) == S.SEED0_STATE
    assert tuple(_lib.cartpole_reset_host(0).tolist()) == S.SEED0_STATE
    seeds = [0, 1, 2 ** 31, 2 ** 32 - 1] + [int(s) for s in np.random.RandomState(9).randint(0, 2 ** 32, size=1000, dtype=np.uint64)]
    for seed in seeds:
        got = _lib.cartpole_reset_host(seed)
        assert np.array_equal(S.bits64(got), S.bits64(S.reset_py(seed))), seed
        assert np.all(got >= -0.05) and np.all(got < 0.05)
    # the episode entry point resets the same way: one step of theta = 0 (action 0) from each of a few seeds
    th = np.zeros((4, S.P), np.float32)
    _, ln, state = _lib.cartpole_rollout_host(th, seeds[:4], 1)
    assert np.all(ln == 1)
    for k in range(4):
        assert np.array_equal(S.bits64(state[k]), S.bits64(S.step_py(S.reset_py(seeds[k]), 0)[0]))


# ---- 2. the step, open loop --------------------------------------------------------------------------------------------------------------------
def test_open_loop_equals_the_plain_python_contract_bit_for_bit(replay):
    assert sorted(replay) == sorted(["zeros", "ones", "alternating", "random0", "random1", "random2", "balanced"])
    for name, (a, init, rows, py) in replay.items():
        assert rows.shape == (a.size, 5) and np.array_equal(rows[:, 4], py[:, 4]), name
        k = S.first_done(rows)
        # every step of the episode bit for bit; past done the stepping goes on, still the same doubles (NaN-free on these sequences up to there)
        assert np.array_equal(S.bits64(rows[:k]), S.bits64(py[:k])), name
        same = np.isnan(rows) == np.isnan(py)
        assert np.all(same) and np.array_equal(S.bits64(rows)[~np.isnan(rows)], S.bits64(py)[~np.isnan(py)]), name
    assert [a.size for a, _, _, _ in (replay["random0"], replay["random1"], replay["random2"], replay["balanced"])] == [500] * 4


def test_facts_of_the_contract(replay):
    ones, zeros, alt = replay["ones"][2], replay["zeros"][2], replay["alternating"][2]
    assert S.first_done(ones) == 9 and ones[8, 2] == -0.21518604988500967
    assert S.first_done(zeros) == 9 and zeros[8, 2] == 0.21518604988500967
    assert np.array_equal(zeros[:9, :4], -ones[:9, :4])                       # constant 0 mirrors constant 1
    assert replay["alternating"][0][0] == 0 and S.first_done(alt) == 33
    assert S.first_done(replay["balanced"][2]) == 500 and replay["balanced"][2][:, 4].sum() == 0


def test_thresholds_are_strict():
    from dne_hip import _lib
    cases = S.threshold_states()
    assert len(cases) == 8 and sum(d for _, d in cases) == 4
    assert math.nextafter(S.TH, 1.0) > S.TH and math.nextafter(S.X_TH, 3.0) > S.X_TH
    for init, done in cases:
        for a in (0, 1):
            row = _lib.cartpole_actions_host(np.array([[a]], np.int32), np.array([init]))[0, 0]
            assert row[0] == init[0] and row[2] == init[2]                  # x + 0.02 * 0 and theta + 0.02 * 0: the state stays ON (or beyond) the threshold
            assert bool(row[4]) == done, (init, a)
            assert S.step_py(init, a)[1] == done
        # closed loop from the same states: a theta that answers action 0 (all zeros) runs on or ends at step 1
        _, ln, _ = _lib.cartpole_rollout_host(np.zeros((1, S.P), np.float32), [0], 500, init=np.array([init]))
        assert (ln[0] == 1) == done


# ---- 3. the closed loop ------------------------------------------------------------------------------------------------------------------------
def test_closed_loop():
    from dne_hip import _lib
    zero = np.zeros((1, 4))
    ret, ln, state = _lib.cartpole_rollout_host(np.zeros((1, S.P), np.float32), [0], 5000, init=zero)     # equal logits: action 0 every step
    assert ln[0] == 9 and ret[0] == 9.0 and ret.dtype == np.float32 and state[0, 2] == 0.21518604988500967
    th = S.balancing_theta()
    init = np.array([S.BALANCE_INIT])
    ret, ln, state, trace = _lib.cartpole_rollout_host(th[None], [0], 500, init=init, want_trace=True)
    assert ln[0] == 500 and ret[0] == 500.0 and state[0, 0] == S.BALANCE_FINAL_X
    t_py, s_py = S.rollout_py(th, S.BALANCE_INIT)                               # the float32-forward run in plain Python
    assert t_py == 500 and s_py[0] == S.BALANCE_FINAL_X and np.array_equal(S.bits64(state[0]), S.bits64(s_py))
    # the trace: the state after every step, and its float32 cast as the observation the policy sees next
    rows = _lib.cartpole_actions_host(S.open_loop_cases()[-1][1][None], init)[0]
    assert np.array_equal(S.bits64(trace[0, :, 4:]), S.bits64(rows[:, :4]))
    assert np.array_equal(trace[0, :, :4], rows[:, :4].astype(np.float32).astype(np.float64))
    # a smaller tslimit is honoured; a larger one (the shipped 5000) leaves 500 in force
    for limit, want in ((7, 7), (1, 1), (499, 499), (5000, 500)):
        ret, ln, _ = _lib.cartpole_rollout_host(th[None], [0], limit, init=init)
        assert ln[0] == want and ret[0] == float(want)
    # from seeds: the episode is the plain-Python one
    noise = S.maze_noise()
    for seed, idx in ((3, 100), (2 ** 32 - 1, 7777)):
        th = S.perturbed(S.theta0(noise), noise, idx, 1.0)
        ret, ln, state = _lib.cartpole_rollout_host(th[None], [seed], 500)
        t_py, s_py = S.rollout_py(th, S.reset_py(seed))
        assert ln[0] == t_py and ret[0] == float(t_py) and np.array_equal(S.bits64(state[0]), S.bits64(s_py))
    with pytest.raises(_lib.DneError, match="dne_cartpole_rollout_host"):
        _lib.cartpole_rollout_host(th[None], [0], 0)
    with pytest.raises(_lib.DneError, match="action 2"):
        _lib.cartpole_actions_host(np.array([[0, 2]], np.int32), zero)


def test_forward_matches_the_fmaf_chains():
    from dne_hip import _lib
    noise = S.maze_noise()
    rs = np.random.RandomState(5)
    th = np.stack([S.perturbed(S.theta0(noise), noise, 50 * k, s) for k, s in enumerate((0.0, 0.02, 1.0, -1.0))])
    obs = rs.uniform(-1, 1, (4, 4)).astype(np.float32)
    h1, h2, out = _lib.cartpole_forward_host(th, obs)
    for k in range(4):
        for got, want in zip((h1[k], h2[k], out[k]), S.forward_np(th[k], obs[k])):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_ties_and_nan_in_the_action_rule():
    """every weight 0, the logits are the output biases: equal -> 0, one ulp apart either way, NaN in either -> 0 (one step from the zero state:
    action 1 pushes right, x_dot > 0)"""
    from dne_hip import _lib
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    cases = [((one, one), 0), ((one, up), 1), ((up, one), 0), ((np.float32(0.0), np.float32(-0.0)), 0), ((np.float32(-0.0), np.float32(0.0)), 0),
             ((np.float32(np.nan), one), 0), ((one, np.float32(np.nan)), 0), ((np.float32(np.nan), np.float32(np.nan)), 0),
             ((np.float32(-np.inf), np.float32(np.inf)), 1), ((np.float32(np.inf), np.float32(np.inf)), 0)]
    th = np.zeros((len(cases), S.P), np.float32)
    for k, ((b0, b1), _) in enumerate(cases):
        th[k, S.B3], th[k, S.B3 + 1] = b0, b1
    _, _, out = _lib.cartpole_forward_host(th, np.zeros((len(cases), 4), np.float32))
    _, ln, state = _lib.cartpole_rollout_host(th, np.zeros(len(cases), np.uint32), 1, init=np.zeros((len(cases), 4)))
    for k, (_, want) in enumerate(cases):
        assert S.pick_action(out[k]) == want
        assert ln[k] == 1 and (state[k, 1] > 0) == (want == 1), cases[k]


# ---- 4. against libm ---------------------------------------------------------------------------------------------------------------------------
def test_step_against_libm(replay):
    worst = 0.0
    for name, (a, init, rows, _) in replay.items():
        lm = S.actions_py(a, init, S.sincos_libm)
        k = S.first_done(rows)
        assert S.first_done(lm) == k, name                                      # the same lengths
        worst = max(worst, float(np.abs(rows[:k, :4] - lm[:k, :4]).max()))
    print("largest state difference to the libm step:", repr(worst))
    assert worst <= S.TOL_LIBM == 4 * S.MEASURED_LIBM


# ---- 5. P, the layout, scale_by ------------------------------------------------------------------------------------------------------------------
def test_scale_by_layout_and_num_params():
    from dne_hip import _lib, policies
    assert _lib.KIND_CARTPOLE == 5 and _lib.CARTPOLE_STEPS == 500
    assert _lib.num_params(_lib.KIND_CARTPOLE, 2) == 386 == S.P
    for nact in (1, 3, 18):
        assert _lib.num_params(_lib.KIND_CARTPOLE, nact) < 0
    spec, P = policies.flat_layout(_lib.KIND_CARTPOLE, 2)
    assert P == 386 and [(k, v[0]) for k, v in spec.items()] == [("fc1/w", 0), ("fc1/b", 64), ("fc2/w", 80), ("fc2/b", 336), ("out/w", 352), ("out/b", 384)]
    sb = policies.simple_scale_by(_lib.KIND_CARTPOLE)
    assert sb.dtype == np.float32 and sb.shape == (386,)
    assert np.all(sb[0:64] == np.float32(0.5)) and np.all(sb[80:336] == np.float32(0.25)) and np.all(sb[352:384] == np.float32(0.1 / 4))
    assert np.all(sb[64:80] == 0) and np.all(sb[336:352] == 0) and np.all(sb[384:] == 0)
    assert policies.simple_scale_by().shape == (498,)                           # the default stays the maze's
    with pytest.raises(ValueError, match="SimpleClassifier"):
        policies.simple_scale_by(_lib.KIND_ES)
    for call, args in ((_lib.debug_plan, (_lib.KIND_CARTPOLE, 2, 8, 2)), (_lib.debug_plan_act, (_lib.KIND_CARTPOLE, 2, 8))):
        with pytest.raises(_lib.DneError, match="DNE_KIND_CARTPOLE"):
            call(*args)


# ---- 6. the es_gpu.py driver on the host-function engine ------------------------------------------------------------------------------------
def _exp(**over):
    exp = {"game": S.GAME, "model": "SimpleClassifier", "num_test_episodes": 2, "population_size": 8, "timesteps": 10 ** 9,
           "episode_cutoff_mode": 5000, "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}
    exp.update(over)
    return exp


def _noise():
    from dne_hip import es
    noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    noise.noise = S.maze_noise()
    noise._engines = []
    return noise


def test_driver_on_the_cartpole(oracle, tmp_path):
    from maze_support import MazeHostEngine
    from oracle_engine import OracleEngine
    from dne_hip import _lib, es_gpu, policies
    noise = _noise()

    def run(log_dir, iters, eng=None, **over):
        eng = eng or S.CartPoleHostEngine(max_members=8)
        return es_gpu.main(str(log_dir), engine=eng, noise=noise, seed=4, max_iters=iters, **_exp(**over)), eng

    st0, e0 = run(tmp_path / "zero", 0)
    assert e0.P == 386 and st0.model == "SimpleClassifier" and st0.game == S.GAME and st0.it == 0 and st0.tslimit == 5000
    rs = np.random.RandomState(4)
    i0 = rs.randint(0, noise.noise.size - 386 + 1)                               # the first draw of the run's stream
    th0 = noise.get(i0, 386) * policies.simple_scale_by(_lib.KIND_CARTPOLE)
    assert th0.dtype == np.float32 and np.array_equal(st0.theta, th0)
    assert e0.calls == [("es_eval", 1)]                                          # the test episodes at power 0 ran (2 episodes = one pair)
    test_seeds = rs.randint(0, 2 ** 32, size=2, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(e0.seeds_seen[0], test_seeds)                          # ... each under its own seed of the stream

    st1, e1 = run(tmp_path / "one", 1)
    # the first update against the formulas (es.py:227-246): centered ranks of the 8 returns, g = sum (r+ - r-) eps / 8, Adam on -g + l2 * theta
    idx = np.array([rs.randint(0, noise.noise.size - 386 + 1) for _ in range(4)], np.int64)
    seeds = rs.randint(0, 2 ** 32, size=8, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(e1.seeds_seen[1], seeds)
    th = np.stack([S.perturbed(th0, noise.noise, i, s) for i in idx for s in (0.02, -0.02)])
    ret, ln, _ = _lib.cartpole_rollout_host(th, seeds, 500)
    steps1 = int(ln.sum())
    assert np.array_equal(ret, ln.astype(np.float32)) and np.all(ln >= 1) and np.all(ln <= 500)
    assert st1.timesteps_so_far == steps1 and st1.num_frames == steps1            # no frame skip: a step is a frame
    ranks = np.asarray(e1.centered_ranks(ret), np.float64).reshape(4, 2)         # (lengths tie: the ranks are the engine's, checked below)
    assert np.allclose(np.sort(ranks.reshape(-1)), np.arange(8) / 7 - 0.5, rtol=0, atol=1e-6)   # a permutation of the eight centered ranks ...
    assert np.all(np.diff(ret[np.argsort(ranks.reshape(-1), kind="stable")]) >= 0)                # ... in the order of the returns
    g = sum((ranks[k, 0] - ranks[k, 1]) * noise.noise[idx[k]:idx[k] + 386].astype(np.float64) for k in range(4)) / 8
    gg = -g + 0.005 * th0.astype(np.float64)
    m, v = 0.1 * gg, 0.001 * gg * gg
    want = th0 - 0.01 * np.sqrt(1 - 0.999) / (1 - 0.9) * m / (np.sqrt(v) + 1e-8)
    assert np.abs(st1.theta - want).max() <= 1e-6 and np.abs(st1.theta - th0).max() > 5e-3
    assert st1.optimizer[2] == 1 and np.allclose(st1.optimizer[0], m, rtol=1e-4, atol=1e-9)

    st2, _ = run(tmp_path / "two", 2)
    st1b, _ = run(tmp_path / "one", 1)                                           # resumes from the one-iteration run's snapshot.pkl
    assert st1b.it == st2.it == 2 and st1b.timesteps_so_far == st2.timesteps_so_far > steps1 and st1b.num_frames == st2.num_frames
    assert np.array_equal(st1b.theta, st2.theta) and not np.array_equal(st2.theta, st1.theta)
    for a, b in zip(st1b.optimizer[:2], st2.optimizer[:2]):
        assert np.array_equal(a, b)
    assert st1b.optimizer[2] == st2.optimizer[2] == 2
    snap = pickle.load(open(tmp_path / "two" / "snapshot.pkl", "rb"))
    assert snap.game == S.GAME and snap.model == "SimpleClassifier" and snap.num_params == 386 and snap.flat_layout == "native"

    # a cutoff below 500 is honoured (no reset state falls within three steps); 'env_default' means 500
    st, e = run(tmp_path / "short", 1, episode_cutoff_mode=3)
    assert st.timesteps_so_far == 8 * 3 and st.tslimit == 3
    st, e = run(tmp_path / "default", 0, episode_cutoff_mode="env_default")
    assert st.tslimit is None and es_gpu._env_limit(e) == 500

    # a resume across games names both, either way round
    with pytest.raises(ValueError, match=r"'gym.CartPole-v1'.*'maze'"):
        es_gpu.main(str(tmp_path / "two"), engine=MazeHostEngine(max_members=8), noise=noise, seed=4, max_iters=1,
                    **_exp(game="maze", episode_cutoff_mode="env_default"))
    with pytest.raises(ValueError, match=r"'gym.CartPole-v1'.*'frostbite'"):
        es_gpu.main(str(tmp_path / "two"), engine=OracleEngine(0, ref_count=8, max_members=8), noise=noise, seed=4, max_iters=1,
                    **_exp(game="frostbite", model="ModelVirtualBN"))
    # any other gym.* name is refused by name
    with pytest.raises(NotImplementedError, match="gym.MountainCar-v0"):
        run(tmp_path / "x", 1, game="gym.MountainCar-v0")
    with pytest.raises(NotImplementedError, match="gym.CartPole-v0"):
        es_gpu.main(str(tmp_path / "x"), engine=None, noise=noise, seed=4, max_iters=1, **_exp(game="gym.CartPole-v0"))
    # the game, the model and the engine have to agree
    with pytest.raises(NotImplementedError, match="ModelVirtualBN.*gym.CartPole-v1"):
        run(tmp_path / "x", 1, model="ModelVirtualBN")
    with pytest.raises(ValueError, match="frostbite.*gym.CartPole-v1"):
        run(tmp_path / "x", 1, game="frostbite")
    with pytest.raises(ValueError, match="'maze'.*gym.CartPole-v1"):
        run(tmp_path / "x", 1, game="maze")
    with pytest.raises(ValueError, match="KIND_CARTPOLE"):
        run(tmp_path / "x", 1, eng=OracleEngine(0, ref_count=8, max_members=8))
    with pytest.raises(ValueError, match="KIND_CARTPOLE"):
        run(tmp_path / "x", 1, eng=MazeHostEngine(max_members=8))
    with pytest.raises(ValueError, match="flat_layout"):
        run(tmp_path / "x", 1, flat_layout="es_distributed")
    # SimpleClassifier on an Atari game keeps its text
    with pytest.raises(NotImplementedError, match="it runs on game 'maze' only"):
        es_gpu.main(str(tmp_path / "x"), engine=OracleEngine(0, ref_count=8, max_members=8), noise=noise, seed=4, max_iters=1,
                    **_exp(game="frostbite"))


def test_the_other_drivers_keep_refusing_the_game(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import ga_gpu, nses_gpu
    noise = _noise()
    for main in (ga_gpu.main, nses_gpu.main):
        with pytest.raises(NotImplementedError, match="gym.CartPole-v1"):
            main(str(tmp_path / "x"), engine=OracleEngine(0, ref_count=8, max_members=8), noise=noise, seed=4, max_iters=1, **_exp())


# ---- 7. the header under AddressSanitizer and UBSan, in a program of its own ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/cartpole_asan_main.cpp, built once: address, undefined and float-cast-overflow (a NaN or an infinity reaching a cast to int)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(ROOT, "tests", "cartpole_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("cartpole_asan") / "cartpole_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program):
    out = subprocess.run([sanitizer_program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = out.stdout.split()
    # 3 closed-loop episodes of the facts + 12 generated ones; 50 facts; outside the contract 6 fills x 2 parts x 2 limits + 6 states
    assert tok[:2] == ["ok", "15"] and tok[3:5] == ["facts", "50"] and tok[5:7] == ["wild", "30"], out.stdout
    assert 30 <= int(tok[7]) <= 30 * 500
