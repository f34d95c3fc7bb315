"""The dense kind without a GPU (csrc/dense.h behind dne_dense_forward_host / dne_dense_rollout_host): the twin's
forward pass against a numpy restatement on every shape, non-finite parameters included; on (16, 16) relu the twin against the maze's and the
cart-pole's own twins; on the pendulum against envs.rollout under the twin's forward pass; P and scale_by against values written out by hand;
every refusal that needs no device; the policy behind the environments (stepenv_act / stepenv_run of DenseHostEngine) against the whole-episode
twin; the es_gpu.py driver with exp['model'] = 'LinearClassifier' on DenseHostEngine against a plain loop; and the header under
AddressSanitizer + UBSan in a stand-alone program."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import dense_support as D
import maze_support as MS
import stepenv_support as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [D.case_id(c) for c in D.CASES]


@pytest.fixture(scope="module", autouse=True)
def built():
    from dne_hip import _lib
    _lib.build()
    return _lib.load()


def observations(env, n, seed=3):
    """observations the environments give (a few steps off the reset) -- and for the last rows values they never give"""
    h = SS.host_engine(env, n)
    h.stepenv_reset(n=n, seeds=SS.mixed_seeds(n))
    for t in range(3):
        h.stepenv_step(SS.scripted_actions(env, n, 3)[t])
    obs = h.stepenv_observation(n=n)
    obs[-1] = np.random.RandomState(seed).uniform(-3, 3, obs.shape[1]).astype(np.float32)
    return obs


# ---- 1. the twin's forward pass against numpy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_forward_twin_equals_numpy(case):
    from dne_hip import _lib
    env, hidden, nl = case
    th = D.member_thetas(env, hidden)
    n, P = th.shape
    obs = observations(env, n)
    layers, out, act = _lib.dense_forward_host(th, obs, SS.kind_id(env), hidden, nl, D.N_OUT[env])
    want_layers, want_out = D.forward_np(env, hidden, nl, th, obs)
    assert D.same(out, want_out) and D.same(layers, want_layers)
    assert D.same(act, D.action_np(env, want_out)) and not np.isnan(out).any()
    assert layers.shape == (n, sum(hidden)) and out.shape == (n, D.N_OUT[env])
    # parameters no run gives: NaN, +-inf, +-0 and 1e30 strewn over theta, one kind a row (the payload and sign of a NaN are free: IEEE 754
    # does not say which operand's a fused operation hands on; everything that is not a NaN is compared bit for bit)
    wild = th[:6].copy()
    rs = np.random.RandomState(11)
    for row, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30)):
        wild[row, rs.choice(P, max(1, P // 7), replace=False)] = np.float32(v)
    layers, out, act = _lib.dense_forward_host(wild, obs[:6], SS.kind_id(env), hidden, nl, D.N_OUT[env])
    want_layers, want_out = D.forward_np(env, hidden, nl, wild, obs[:6])
    assert MS.same_nan(out, want_out) and MS.same_nan(layers, want_layers)
    assert D.same(act, D.action_np(env, want_out))                       # (a NaN logit never wins: action 0)
    assert not np.isfinite(out[:3]).all()


# ---- 2. (16, 16) relu is SimpleClassifier: the maze's and the cart-pole's own twins ----------------------------------------------------------------
@pytest.mark.parametrize("env", ("maze", "cartpole"))
def test_16_16_relu_equals_the_baked_twins(env):
    from dne_hip import _lib
    th = SS.closed_loop_thetas(env)
    seeds = SS.mixed_seeds(len(th))
    obs = observations(env, len(th))
    kind = SS.kind_id(env)
    layers, out, _ = _lib.dense_forward_host(th, obs, kind, (16, 16), "relu", 2)
    h1, h2, want = (_lib.maze_forward_host if env == "maze" else _lib.cartpole_forward_host)(th, obs)
    assert D.same(out, want) and D.same(layers[:, :16], h1) and D.same(layers[:, 16:], h2)
    hdr, lines = MS.fixture_maze()
    for tslimit in (1, 7, SS.OWN_LIMIT[env]):
        r = _lib.dense_rollout_host(th, kind, (16, 16), "relu", 2, seeds=seeds, tslimit=tslimit, header=hdr, lines=lines)
        if env == "maze":
            ret, ln, xy = _lib.maze_rollout_host(th, hdr, lines, tslimit=tslimit)
            assert D.same(r["state"][:, :2].astype(np.float32), xy) and D.same(r["signreturns"], np.sign(ret).astype(np.float32))
        else:
            ret, ln, st = _lib.cartpole_rollout_host(th, seeds, tslimit)[:3]
            assert D.same(r["state"], st) and D.same(r["signreturns"], ret)
        assert D.same(r["returns"], ret) and D.same(r["lengths"], ln)
    if env == "cartpole":
        assert len(set(ln.tolist())) >= 3                                 # the members end at different steps


# ---- 3. the pendulum: the whole-episode twin against the step-at-a-time loop under the twin's forward pass ----------------------------------------
@pytest.mark.parametrize("case", [c for c in D.CASES if c[0] == "pendulum"], ids=lambda c: D.case_id(c))
def test_pendulum_rollout_equals_the_stepped_loop(case):
    from dne_hip import _lib, envs
    env, hidden, nl = case
    th = D.member_thetas(env, hidden)
    n = len(th)
    seeds = SS.mixed_seeds(n)
    for tslimit in (1, 7, 200):
        r = _lib.dense_rollout_host(th, _lib.KIND_PENDULUM, hidden, nl, 1, seeds=seeds, tslimit=tslimit)
        e = envs.make("Pendulum-v0", n, engine=SS.StepEnvHostEngine("pendulum", n))
        ret, ln = envs.rollout(e, lambda obs: _lib.dense_forward_host(th, obs, _lib.KIND_PENDULUM, hidden, nl, 1)[2], seeds=seeds, max_frames=tslimit)
        assert D.same(r["returns"], ret) and D.same(r["lengths"], ln) and D.same(r["state"], e.state()[0])
        assert np.all(ln == tslimit) and np.all(r["signreturns"] == -tslimit)      # every reward of the swing-up is negative
    assert len(set(r["returns"].tolist())) == n


# ---- 4. P and scale_by by hand ---------------------------------------------------------------------------------------------------------------------
def test_num_params_and_scale_by():
    from dne_hip import _lib, policies
    K = {e: SS.kind_id(e) for e in SS.KINDS}
    assert _lib.dense_num_params(K["maze"], (), 2) == 11 * 2 + 2 == 24
    assert _lib.dense_num_params(K["cartpole"], (5, 33), 2) == 4 * 5 + 5 + 5 * 33 + 33 + 33 * 2 + 2 == 291
    assert _lib.dense_num_params(K["pendulum"], (64,), 1) == 3 * 64 + 64 + 64 + 1 == 321
    assert _lib.dense_num_params(K["maze"], (64, 64, 64), 2) == 9218
    assert _lib.dense_num_params(K["maze"], (16, 16), 2) == 498 == _lib.num_params(_lib.KIND_MAZE, 2)
    assert _lib.dense_num_params(K["cartpole"], (16, 16), 2) == 386 == _lib.num_params(_lib.KIND_CARTPOLE, 2)
    assert _lib.num_params(_lib.KIND_DENSE, 2) == -1
    for env, hidden, _ in D.CASES:
        assert _lib.dense_num_params(K[env], hidden, D.N_OUT[env]) == D.num_params(env, hidden)
    f = np.float32
    sb = policies.dense_scale_by(K["maze"], (), 2)                        # LinearClassifier: one layer at std 1.0
    assert sb.dtype == np.float32 and D.same(sb, np.concatenate([np.full(22, f(1.0 / np.sqrt(11))), np.zeros(2, f)]).astype(f))
    sb = policies.dense_scale_by(K["cartpole"], (5, 33), 2)
    want = np.concatenate([np.full(20, f(1.0 / np.sqrt(4))), np.zeros(5), np.full(165, f(1.0 / np.sqrt(5))), np.zeros(33), np.full(66, f(0.1 / np.sqrt(33))), np.zeros(2)]).astype(f)
    assert D.same(sb, want)
    sb = policies.dense_scale_by(K["pendulum"], (64,), 1)
    assert D.same(sb, np.concatenate([np.full(192, f(1.0 / np.sqrt(3))), np.zeros(64), np.full(64, f(0.1 / 8)), np.zeros(1)]).astype(f))
    assert D.same(policies.dense_scale_by(K["maze"], (16, 16), 2), policies.simple_scale_by())
    assert D.same(policies.dense_scale_by(K["cartpole"], (16, 16), 2), policies.simple_scale_by(_lib.KIND_CARTPOLE))


# ---- 5. refusals that need no device -----------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(built):
    from dne_hip import _lib
    K = {e: SS.kind_id(e) for e in SS.KINDS}
    for env_kind, hidden, n_out in ((0, (), 2), (7, (), 2), (8, (), 2), (K["maze"], (1, 2, 3, 4), 2), (K["maze"], (0,), 2), (K["maze"], (65,), 2),
                                    (K["maze"], (16, -1), 2), (K["maze"], (), 1), (K["maze"], (), 3), (K["cartpole"], (4,), 1), (K["pendulum"], (4,), 2)):
        assert _lib.dense_num_params(env_kind, hidden, n_out) == -1, (env_kind, hidden, n_out)
    obs, th = np.zeros((1, 11), np.float32), np.zeros(58, np.float32)     # (58: P of (4,) on the maze, the one refused shape that has a P)
    for match, args in ((r"environments DNE_KIND_MAZE \(4\), DNE_KIND_CARTPOLE \(5\) and DNE_KIND_PENDULUM \(6\); environment 7 is refused", (7, (), "relu", 2)),
                        (r"0\.\.3 hidden layers; 4 hidden layers are refused", (K["maze"], (1, 2, 3, 4), "relu", 2)),
                        (r"hidden widths 1\.\.64; width 65 of hidden layer 1 is refused", (K["maze"], (3, 65), "relu", 2)),
                        (r"hidden widths 1\.\.64; width 0 of hidden layer 0 is refused", (K["maze"], (0,), "relu", 2)),
                        (r"has 2 outputs on environment 5 .* n_actions 3 is refused", (K["cartpole"], (4,), "relu", 3)),
                        (r"has 1 outputs on environment 6 .* n_actions 2 is refused", (K["pendulum"], (4,), "relu", 2)),
                        (r"nonlinearities 0 \(tanh\) and 1 \(relu\); nonlinearity 2 is refused", (K["maze"], (4,), 2, 2))):
        for call in (lambda a: _lib.dense_forward_host(th, obs[:, :_lib.stepenv_dims(a[0])[0] if a[0] in _lib.STEPENV_KINDS else 1], *a),
                     lambda a: _lib.dense_rollout_host(th, *a, seeds=[1], **(dict(zip(("header", "lines"), MS.fixture_maze())) if a[0] == K["maze"] else {}))):
            with pytest.raises(_lib.DneError, match=match):
                call(args)
    P = _lib.dense_num_params(K["cartpole"], (), 2)
    with pytest.raises(_lib.DneError, match="seeds is NULL"):
        _lib.dense_rollout_host(np.zeros((1, P), np.float32), K["cartpole"], (), "relu", 2)
    with pytest.raises(_lib.DneError, match="maze: header or lines missing|needs header and lines"):
        _lib.dense_rollout_host(np.zeros((1, 24), np.float32), K["maze"], (), "relu", 2)
    lib = _lib.load()
    for name in ("dne_dense_num_params", "dne_dense_env_kind", "dne_dense_final_state", "dne_stepenv_act", "dne_stepenv_run", "dne_dense_forward_host", "dne_dense_rollout_host"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "dne_hip.h")).read()
    assert "#define DNE_KIND_DENSE 8" in text and _lib.KIND_DENSE == 8
    # the host engine refuses in the engine's words, the batch unchanged
    case = ("cartpole", (5, 33), "relu")
    e = D.host_engine(case, 8)
    e.stepenv_reset(n=4, seeds=SS.mixed_seeds(4))
    before = SS.snapshot(e, 4)
    with pytest.raises(_lib.DneError, match=D.REFUSED["members"]):
        e.stepenv_act(n=4)
    D.load_members(e, case)
    for what, fn in (("max_steps", lambda: e.stepenv_run(0, n=4)), ("max_steps", lambda: e.stepenv_run(-1, n=4)),
                     ("member", lambda: e.stepenv_run(1, n=2, members=[0, 7])), ("member", lambda: e.stepenv_act(n=2, members=[-1, 0]))):
        with pytest.raises(_lib.DneError, match=D.REFUSED[what]):
            fn()
    for what, fn in (("never", lambda: e.stepenv_run(1, n=5)), ("twice", lambda: e.stepenv_act(np.array([1, 1], np.int32))),
                     ("range", lambda: e.stepenv_run(3, np.array([8], np.int32), members=[0]))):
        with pytest.raises(_lib.DneError, match=SS.REFUSED[what]):
            fn()
    assert SS.same_snapshot(SS.snapshot(e, 4), before)


# ---- the policy behind the environments, on the twins -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("maze", (5, 33), "relu"), ("cartpole", (), "relu"), ("cartpole", (64,), "tanh"), ("pendulum", (5, 33), "relu")], ids=lambda c: D.case_id(c))
def test_run_in_pieces_equals_the_whole_episode_twin(case):
    """stepenv_run 7, then 1, then the rest: the state of one run to the end and of dne_dense_rollout_host; the members permuted against the
    environments, one member under two of them"""
    from dne_hip import _lib, envs
    env, hidden, nl = case
    n = 5
    members = np.array([3, 0, 6, 0, 2], np.int32)
    seeds = SS.mixed_seeds(n)
    a, b = D.host_engine(case, 8), D.host_engine(case, 8)
    th = D.load_members(a, case); D.load_members(b, case)
    want = _lib.dense_rollout_host(th[members], SS.kind_id(env), hidden, nl, D.N_OUT[env], seeds=seeds, **a.envs._maze())
    a.stepenv_reset(n=n, seeds=seeds); b.stepenv_reset(n=n, seeds=seeds)
    pieces = [a.stepenv_run(k, n=n, members=members) for k in (7, 1, 1000)]
    whole = b.stepenv_run(1000, n=n, members=members)
    assert SS.same_snapshot(SS.snapshot(a, n), SS.snapshot(b, n)) and whole[2].all() and pieces[2][2].all()
    assert D.same(whole[0], want["returns"]) and D.same(whole[1], want["lengths"]) and D.same(b.stepenv_state(n=n)[0], want["state"])
    assert np.array_equal(sum(p[1] for p in pieces), want["lengths"])
    if env != "pendulum":                                                  # every partial sum is an integer or holds one term: the split is exact
        assert D.same(sum(p[0].astype(np.float64) for p in pieces).astype(np.float32), want["returns"])
    e = envs.make(SS.GAMES[env], n, engine=b)
    ret, ln = envs.run(e, members=members, seeds=seeds)
    assert D.same(ret, want["returns"]) and D.same(ln, want["lengths"])


# ---- 6. es_gpu.main with LinearClassifier ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ("maze", "cartpole"))
def test_driver_with_linear_classifier(env, tmp_path):
    from dne_hip import _lib, es_gpu
    from maze_support import MazeHostEngine
    game = SS.GAMES[env]
    table = D.shared_noise()

    def run(log_dir, iters, eng=None, **over):
        eng = eng or D.host_engine((env, (), "relu"), 10)
        return es_gpu.main(str(log_dir), engine=eng, noise=table, seed=4, max_iters=iters, **D.exp(game, **over)), eng

    want = D.plain_loop(env, 3)
    st3, e3 = run(tmp_path / "three", 3)
    assert st3.model == "LinearClassifier" and st3.game == game and st3.it == 3 and st3.num_params == e3.P == D.num_params(env, ())
    assert D.same(st3.theta, want[2][0]) and D.same(st3.optimizer[0], want[2][1]) and D.same(st3.optimizer[1], want[2][2]) and st3.optimizer[2] == 3
    rows = D.log_rows(tmp_path / "three")
    assert len(rows) == 3
    for it, (row, w) in enumerate(zip(rows, want), 1):
        rets, lens = w[3].reshape(-1), w[4]
        assert row["Iteration"] == str(it) and row["PopulationEpCount"] == "10" and row["MutationPower"] == "0.02"
        assert row["PopulationEpRewMax"] == ("%-8.6g" % np.max(rets)).strip() and row["PopulationEpRewMean"] == ("%-8.6g" % np.mean(rets.astype(np.float64))).strip()
        assert row["PopulationEpRewMedian"] == ("%-8.6g" % np.median(rets)).strip()
        assert row["PopulationTimesteps"] == row["TimestepsThisIter"] == str(int(lens.sum()))
        assert row["TimestepsSoFar"] == row["TimestepsComputed"] == str(int(sum(x[4].sum() for x in want[:it])))
    st1, _ = run(tmp_path / "one", 1)
    assert D.same(st1.theta, want[0][0])
    st1b, _ = run(tmp_path / "one", 2)                                    # resumes from snapshot.pkl: two more iterations
    assert st1b.it == 3 and D.same(st1b.theta, st3.theta) and D.same(st1b.optimizer[0], st3.optimizer[0]) and D.same(st1b.optimizer[1], st3.optimizer[1])
    snap = pickle.load(open(tmp_path / "three" / "snapshot.pkl", "rb"))
    assert snap.model == "LinearClassifier" and snap.game == game and snap.flat_layout == "native"
    # a snapshot of SimpleClassifier is refused, naming both models
    simple = MazeHostEngine(max_members=10) if env == "maze" else __import__("cartpole_support").CartPoleHostEngine(max_members=10)
    es_gpu.main(str(tmp_path / "simple"), engine=simple, noise=table, seed=4, max_iters=1, **D.exp(game, model="SimpleClassifier"))
    with pytest.raises(ValueError, match="holds model 'SimpleClassifier'.*this run is model 'LinearClassifier'"):
        run(tmp_path / "simple", 1)
    # an engine of any shape on its environment's game; an engine of another environment is refused, naming both
    wide = D.host_engine((env, (5, 33), "relu"), 10)
    stw = es_gpu.main(str(tmp_path / "wide"), engine=wide, noise=table, seed=4, max_iters=1, **D.exp(game, model=None))
    assert stw.model == "Dense(5, 33; relu)" and stw.num_params == D.num_params(env, (5, 33))
    assert D.same(stw.theta, D.plain_loop(env, 1, hidden=(5, 33))[0][0])
    other = "cartpole" if env == "maze" else "maze"
    with pytest.raises(ValueError, match="game %r asked for.*runs %r" % (game, SS.GAMES[other])):
        run(tmp_path / "x", 1, eng=D.host_engine((other, (), "relu"), 10))
    with pytest.raises(ValueError, match="model 'SimpleClassifier' asked for"):
        run(tmp_path / "x", 1, model="SimpleClassifier")
    with pytest.raises(NotImplementedError, match="LinearClassifier"):
        es_gpu.main(str(tmp_path / "x"), engine=None, noise=table, seed=4, max_iters=1, **D.exp("frostbite"))
    with pytest.raises(NotImplementedError, match="LinearClassifier"):   # SimpleClassifier keeps its own kinds: their engines refuse the name
        run(tmp_path / "x", 1, eng=simple)


def test_the_other_drivers_keep_refusing_the_model(oracle, tmp_path):
    """ga_gpu, nses_gpu: out of scope; what they said to LinearClassifier before they still say"""
    from oracle_engine import OracleEngine
    from dne_hip import ga_gpu, nses_gpu
    table = D.shared_noise()
    for main in (ga_gpu.main, nses_gpu.main):
        with pytest.raises(NotImplementedError, match="LinearClassifier"):
            main(str(tmp_path / "x"), engine=MS.MazeHostEngine(max_members=10), noise=table, seed=4, max_iters=1, **D.exp("maze"))
    with pytest.raises(NotImplementedError, match="gym.CartPole-v1.*LinearClassifier"):
        nses_gpu.main(str(tmp_path / "x"), engine=OracleEngine(0, ref_count=8, max_members=10), noise=table, seed=4, max_iters=1, **D.exp("gym.CartPole-v1"))


# ---- 7. the header under AddressSanitizer and UBSan, in a program of its own ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/dense_asan_main.cpp, built once: address, undefined and float-cast-overflow (a NaN or an infinity reaching a cast to int)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(ROOT, "tests", "dense_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("dense_asan") / "dense_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program):
    out = subprocess.run([sanitizer_program], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = out.stdout.split()
    # 15 shapes, each: forward passes and 3 episodes x 3 limits on finite thetas, then 6 non-finite fills
    assert tok[0] == "ok" and tok[1:3] == ["shapes", "15"] and tok[3:5] == ["episodes", str(15 * 9)] and tok[5:7] == ["wild", str(15 * 6)], out.stdout
    assert tok[7] == "facts" and int(tok[8]) > 15 * 9
