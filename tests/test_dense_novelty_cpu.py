"""CPU: novelty over final states on the dense kind (csrc/dense_novelty.h through dne_dense_novelty_host / dne_dense_bc_host) against the
contract restated in numpy float64, bit for bit; D = 2 against dne_maze_novelty_host; the BCs against the final state records of the dense
twin and the maze's own rollout; every refusal of the host twins; the header's host side under sanitizers in a program of its own; and
dne_hip/nses_gpu.py's dense route on DenseNoveltyHostEngine against the loop written out."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import dense_novelty_support as S
import dense_support as D
import maze_support as MS
import stepenv_support as SS


def test_constants_agree_with_the_library():
    from dne_hip import _lib
    assert _lib.DENSE_NOVELTY_KMAX == _lib.MAZE_NOVELTY_KMAX == S.KMAX and _lib.MAZE_NOVELTY_TILE == S.TILE
    assert "#define DNE_DENSE_NOVELTY_KMAX DNE_MAZE_NOVELTY_KMAX" in open(os.path.join(MS.ROOT, "include", "dne_hip.h")).read()
    src = open(os.path.join(MS.ROOT, "deep-neuroevolution_amd", "csrc", "dense_novelty.h")).read()
    for name in ("sort_key", "key_value", "KMAX", "TILE", "KEY_NAN", "KEY_NONE"):      # used, not copied
        assert "using maze_novelty::%s;" % name in src
    assert "constexpr int KMAX" not in src and "constexpr int TILE" not in src
    assert [_lib.dense_bc_dim(SS.kind_id(env)) for env in ("maze", "cartpole", "pendulum")] == [2, 4, 2]


# ---- 1. the host twin against the restatement, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.DIMS)
@pytest.mark.parametrize("name", S.SETS)
def test_host_equals_the_restatement_on_every_shape(name, dim):
    from dne_hip import _lib
    cells = 0
    for narch in S.SIZES:
        mem, arch = S.point_set(name, dim, narch)
        assert mem.shape == (9, dim) and arch.shape == (narch, dim)
        for k in S.KS:
            want = S.contract_of(name, dim, narch, k)
            for n in S.COUNTS:
                got = _lib.dense_novelty_host(mem[:n], arch, k)
                assert got.dtype == np.float64 and S.same(got, want[:n]), (name, dim, narch, n, k, got, want[:n])
                cells += 1
    assert cells == len(S.SIZES) * len(S.KS) * len(S.COUNTS)


def test_the_point_sets_do_what_they_are_for():
    """held on the restatement alone"""
    for dim in S.DIMS:
        for narch in S.SIZES:
            if narch >= 63:     # the lattice: two archive points at equal distance on either side of position kk, so the slot decides
                assert S.tie_at_cut("lattice", dim, narch), (dim, narch)
        mem, arch = S.point_set("edge_few_nan", dim, 1025)
        assert int(np.isnan(arch).any(axis=1).sum()) == 3 and int(np.all(arch == mem[0], axis=1).sum()) == 2
        got = S.contract(mem, arch, 25)
        assert got[0] > 0.0 and S.contract(mem[:1], arch, 2)[0] == 0.0          # its own point, twice: two zero distances
        assert np.isnan(got[1]) and np.isposinf(got[2]) and np.isposinf(got[6])  # the NaN member; the members at +-inf (inf before every NaN)
        assert np.isfinite(got[3]) and np.isfinite(got[4]) and np.isfinite(got[5]) and np.isfinite(got[7])
        assert np.isnan(S.contract(mem[2:3], arch, 1025)[0])                    # ... until inf - inf is reached
        mem, arch = S.point_set("edge_mostly_nan", dim, 1025)
        assert int(np.isnan(arch).any(axis=1).sum()) > 1025 - 25
        assert np.isfinite(S.contract(mem[7:8], arch, 2)[0]) and np.isnan(S.contract(mem[7:8], arch, 25)[0])   # the sum reaches the NaNs
        signs = np.signbit(S.point_set("edge_few_nan", dim, 64)[0][4])
        assert signs.any() and not signs.all()                                     # +0.0 and -0.0


@pytest.mark.parametrize("name", S.SETS)
def test_two_coordinates_equal_the_maze_twin(name):
    from dne_hip import _lib
    for narch in S.SIZES:
        mem, arch = S.point_set(name, 2, narch)
        for k in S.KS:
            assert S.same(_lib.dense_novelty_host(mem, arch, k), _lib.maze_novelty_host(mem, arch, k)), (name, narch, k)


# ---- 2. the behaviour characterisations ----------------------------------------------------------------------------------------------------------------
BC_CASES = (("maze", (), "relu"), ("cartpole", (5, 33), "relu"), ("pendulum", (64,), "tanh"))


@pytest.mark.parametrize("case", BC_CASES, ids=D.case_id)
def test_bc_of_the_final_state_records(case):
    from dne_hip import _lib
    env, hidden, nl = case
    kind, dim = SS.kind_id(env), S.BC_DIM[env]
    th = D.member_thetas(env, hidden)
    maze = dict(zip(("header", "lines"), MS.fixture_maze())) if env == "maze" else {}
    rec = _lib.dense_rollout_host(th, kind, hidden, nl, D.N_OUT[env], seeds=SS.mixed_seeds(len(th)), **maze)["state"]
    bc = _lib.dense_bc_host(kind, rec)
    assert bc.dtype == np.float32 and bc.shape == (len(th), dim)
    assert np.array_equal(S.bits(bc), S.bits(rec[:, :dim].astype(np.float32)))
    if env != "maze":
        assert np.any(bc.astype(np.float64) != rec[:, :dim])           # the cast rounds: the records are doubles of their own
    odd = np.zeros((4, rec.shape[1]))
    odd[0, :dim] = np.nan; odd[1, :dim] = np.inf; odd[2, :dim] = -np.inf; odd[3, :dim] = 1.0 + 2.0 ** -24   # a tie: to even
    with np.errstate(all="ignore"):
        assert np.array_equal(S.bits(_lib.dense_bc_host(kind, odd)), S.bits(odd[:, :dim].astype(np.float32)))
    assert _lib.dense_bc_host(kind, odd)[3, 0] == np.float32(1.0)


def test_bc_of_the_maze_is_the_final_position_of_the_baked_rollout():
    from dne_hip import _lib
    header, lines = MS.fixture_maze()
    th = D.member_thetas("maze", (16, 16))
    rec = _lib.dense_rollout_host(th, _lib.KIND_MAZE, (16, 16), "relu", 2, header=header, lines=lines)["state"]
    xy = _lib.maze_rollout_host(th, header, lines, 400)[2]
    assert np.array_equal(S.bits(_lib.dense_bc_host(_lib.KIND_MAZE, rec)), S.bits(xy))


# ---- 3. what the host twins refuse ---------------------------------------------------------------------------------------------------------------------
def test_host_refusals():
    from dne_hip import _lib
    one = np.zeros((1, 2), np.float32)
    for bc, arch, k, dim, text in ((one[:0], one, 1, 2, "n = 0"), (one, one[:0], 1, 2, "the archive is empty"), (one, one, 0, 2, "k = 0"),
                                   (np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), 1, 3, "D = 3"), (one, one, 1, 1, "D = 1")):
        with pytest.raises(_lib.DneError, match="dne_dense_novelty_host: .*" + text):
            _lib.dense_novelty_host(bc, arch, k, D=dim)
    lib = _lib.load()
    import ctypes as C
    out = np.zeros(1, np.float64)
    fp, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for args in ((None, 1, fp(one), 1, 2, 1, dp(out)), (fp(one), 1, None, 1, 2, 1, dp(out)), (fp(one), 1, fp(one), 1, 2, 1, None)):
        assert lib.dne_dense_novelty_host(*args) == -1 and "dne_dense_novelty_host: a buffer is missing" in lib.dne_last_error(None).decode()
    rec = np.zeros((1, 4), np.float64)
    assert lib.dne_dense_bc_host(_lib.KIND_CARTPOLE, None, 1, fp(one)) == -1 and "dne_dense_bc_host: a buffer is missing" in lib.dne_last_error(None).decode()
    assert lib.dne_dense_bc_host(_lib.KIND_CARTPOLE, dp(rec), 1, None) == -1 and "dne_dense_bc_host: a buffer is missing" in lib.dne_last_error(None).decode()
    with pytest.raises(_lib.DneError, match="dne_dense_bc_host: n = 0"):
        _lib.dense_bc_host(_lib.KIND_CARTPOLE, np.zeros((0, 4)))
    with pytest.raises(_lib.DneError, match="dne_dense_bc_host: environment 7"):
        _lib.dense_bc_host(_lib.KIND_MJMAZE, np.zeros((1, 1)))


# ---- 4. the header's host side under sanitizers, in a program of its own ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/dense_novelty_asan_main.cpp, built once: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(MS.ROOT, "tests", "dense_novelty_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("dense_novelty_asan") / "dense_novelty_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(MS.ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def _tok(v):
    return "nan" if v != v else float(v).hex()


def _parse(line):
    return np.array([float("nan") if t == "nan" else float.fromhex(t) for t in line.split()])


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program, tmp_path):
    cases = [(name, dim, narch, n, k) for name in S.SETS for dim in S.DIMS for narch in (1, 2, 63, 65, 1025) for n, k in ((1, 1), (5, 25), (9, 40))]
    text = []
    for name, dim, narch, n, k in cases:
        mem, arch = S.point_set(name, dim, narch)
        text.append("%d %d %d %d\n%s\n%s\n" % (dim, n, narch, k, " ".join(_tok(v) for v in mem[:n].reshape(-1)), " ".join(_tok(v) for v in arch.reshape(-1))))
    path = tmp_path / "cases.txt"
    path.write_text("".join(text))
    out = subprocess.run([sanitizer_program, "novelty", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % len(cases) and len(lines) == len(cases) + 1
    for line, (name, dim, narch, n, k) in zip(lines, cases):
        assert S.same(_parse(line), S.contract_of(name, dim, narch, k)[:n]), (name, dim, narch, n, k)
    # the BCs: records of every environment with a NaN, the infinities and a value that rounds
    recs = []
    for env in ("maze", "cartpole", "pendulum"):
        Sw = {"maze": 7, "cartpole": 4, "pendulum": 2}[env]
        rec = np.random.RandomState(Sw).randn(3, Sw) * 3.0
        rec[1, 0], rec[1, 1], rec[2, 0], rec[2, 1] = np.nan, np.inf, -np.inf, 1.0 + 2.0 ** -30
        recs.append((env, rec))
    path = tmp_path / "recs.txt"
    path.write_text("".join("%d %d\n%s\n" % (SS.kind_id(env), len(rec), " ".join(_tok(v) for v in rec.reshape(-1))) for env, rec in recs))
    out = subprocess.run([sanitizer_program, "bc", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok 3" and len(lines) == 4
    for line, (env, rec) in zip(lines, recs):
        assert S.same(_parse(line), rec[:, :S.BC_DIM[env]].astype(np.float32).reshape(-1).astype(np.float64)), env


# ---- 5. the driver on the host-function engine ---------------------------------------------------------------------------------------------------------------
DRIVER_CASES = (
    ("maze", dict()),
    ("maze", dict(algo_type="nsr", return_proc_mode="centered_rank")),
    ("maze", dict(return_proc_mode="sign", ns={"selection_method": "novelty_prob"})),
    ("cartpole", dict()),
    ("cartpole", dict(algo_type="nsr", return_proc_mode="sign", ns={"num_rollouts": 3})),
    ("cartpole", dict(return_proc_mode="centered_rank", ns={"selection_method": "novelty_prob", "num_rollouts": 3})),
)


@pytest.mark.parametrize("env,over", DRIVER_CASES, ids=lambda v: v if isinstance(v, str) else "-".join("%s" % (x,) for x in list(v.values())[:2]) or "ns")
def test_driver_equals_the_loop_written_out_and_resumes(tmp_path, env, over):
    import copy
    want = S.plain_loop(env, 4, **copy.deepcopy(over))
    st4, e4 = S.run(tmp_path / "four", 4, env, **copy.deepcopy(over))
    assert st4.it == 4 and S.same_state(st4, want)
    R = over.get("ns", {}).get("num_rollouts", 1)
    assert st4.archive.shape == (3 + 4, S.BC_DIM[env]) and np.array_equal(S.bits(e4.dense_archive()), S.bits(st4.archive))
    assert (st4.game, st4.model, st4.num_params, st4.num_rollouts) == (S.GAMES[env], "LinearClassifier", e4.P, R)
    st2, _ = S.run(tmp_path / "resumed", 2, env, **copy.deepcopy(over))
    snap = pickle.load(open(tmp_path / "resumed" / "snapshot.pkl", "rb"))
    assert snap.it == 2 and snap.archive.shape == (5, S.BC_DIM[env]) and snap.num_rollouts == R
    st22, e22 = S.run(tmp_path / "resumed", 2, env, **copy.deepcopy(over))       # a fresh engine: the archive comes from the snapshot
    assert st2.it == 2 and S.same_state(st22, st4) and np.array_equal(S.bits(e22.dense_archive()), S.bits(st4.archive))
    if env == "cartpole":
        assert len({int(n) for n in e4.seeds_seen[-1]}) > 1                        # every episode under its own seed


def test_a_16_16_dense_engine_on_the_maze_is_the_simple_classifier_run(oracle, tmp_path):
    import maze_novelty_support as MN
    from dne_hip import nses_gpu
    for sub, over in (("rr", dict()), ("prob", dict(algo_type="nsr", ns={"selection_method": "novelty_prob"}))):
        ref = nses_gpu.main(str(tmp_path / sub / "maze"), engine=MN.MazeNoveltyHostEngine(max_members=8), noise=D.shared_noise(), seed=4, max_iters=3,
                            **S.exp("maze", model="SimpleClassifier", **dict(over)))
        got, eng = S.run(tmp_path / sub / "dense", 3, "maze", eng=S.host_engine("maze", (16, 16), "relu", 8), model=None, **dict(over))
        assert S.same_state(got, ref) and got.model == "Dense(16, 16; relu)" and ref.model == "SimpleClassifier"
        assert D.same_rows(D.log_rows(tmp_path / sub / "dense"), D.log_rows(tmp_path / sub / "maze"))


def test_routing_and_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import _lib, nses_gpu
    # the routing table: (engine, game, model) -> dense or the existing path
    dense_eng = S.host_engine("maze")
    for eng, game, model, dense in ((dense_eng, "maze", "LinearClassifier", True), (dense_eng, "frostbite", None, True),
                                    (None, "maze", "LinearClassifier", True), (None, "gym.CartPole-v1", "LinearClassifier", True),
                                    (None, "maze", "SimpleClassifier", False), (None, "gym.CartPole-v1", "SimpleClassifier", False),
                                    (None, "Pendulum-v0", "LinearClassifier", False), (None, "frostbite", "LinearClassifier", False),
                                    (MS.MazeHostEngine(max_members=8), "maze", "LinearClassifier", False),
                                    (OracleEngine(0, ref_count=8, max_members=8), "gym.CartPole-v1", "LinearClassifier", False)):
        assert nses_gpu._is_dense_run(eng, {"game": game, "model": model}) is dense
    # the existing refusals, through the calls of the pinned tests
    for main_exp in (D.exp("maze"),):
        with pytest.raises(NotImplementedError, match="LinearClassifier"):
            nses_gpu.main(str(tmp_path / "x"), engine=MS.MazeHostEngine(max_members=10), noise=D.shared_noise(), seed=4, max_iters=1, **main_exp)
    with pytest.raises(NotImplementedError, match="gym.CartPole-v1.*LinearClassifier"):
        nses_gpu.main(str(tmp_path / "x"), engine=OracleEngine(0, ref_count=8, max_members=10), noise=D.shared_noise(), seed=4, max_iters=1, **D.exp("gym.CartPole-v1"))
    with pytest.raises(NotImplementedError, match=r"game 'Pendulum-v0' with model 'LinearClassifier': this loop runs game 'maze' with model 'SimpleClassifier'"):
        nses_gpu.main(str(tmp_path / "x"), engine=None, noise=D.shared_noise(), seed=4, max_iters=1, **S.exp("pendulum"))
    # the dense route's own
    with pytest.raises(NotImplementedError, match="'Pendulum-v0': this loop runs a KIND_DENSE engine on 'maze' and 'gym.CartPole-v1'"):
        S.run(tmp_path / "x", 1, "pendulum", eng=S.host_engine("pendulum"))
    with pytest.raises(ValueError, match=r"game 'gym.CartPole-v1' asked for, the engine passed in \(kind 8 on environment kind 4\) runs 'maze'"):
        S.run(tmp_path / "x", 1, "cartpole", eng=S.host_engine("maze"))
    with pytest.raises(ValueError, match=r"model 'LinearClassifier' asked for, the engine passed in \(kind 8\) runs 'Dense\(5, 33; relu\)'"):
        S.run(tmp_path / "x", 1, "cartpole", eng=S.host_engine("cartpole", (5, 33)))
    with pytest.raises(ValueError, match="num_rollouts 2: the maze is deterministic"):
        S.run(tmp_path / "x", 1, "maze", ns={"num_rollouts": 2})
    with pytest.raises(ValueError, match="num_rollouts 0"):
        S.run(tmp_path / "x", 1, "cartpole", ns={"num_rollouts": 0})
    with pytest.raises(NotImplementedError, match="tournament"):
        S.run(tmp_path / "x", 1, "cartpole", ns={"selection_method": "tournament"})
    with pytest.raises(NotImplementedError, match="median"):
        S.run(tmp_path / "x", 1, "cartpole", return_proc_mode="median")
    with pytest.raises(ValueError, match="algo_type 'nsra'"):
        S.run(tmp_path / "x", 1, "cartpole", algo_type="nsra")
    with pytest.raises(ValueError, match=r"k 33 \(1 <= k <= 32\)"):
        S.run(tmp_path / "x", 1, "cartpole", ns={"k": 33})
    assert not os.path.exists(tmp_path / "x" / "snapshot.pkl")
    assert S.run(tmp_path / "shape", 1, "cartpole", eng=S.host_engine("cartpole", (5, 33)), model=None)[0].model == "Dense(5, 33; relu)"


def test_refused_resumes(oracle, tmp_path):
    import maze_novelty_support as MN
    from dne_hip import es_gpu, nses_gpu
    S.run(tmp_path / "cp", 1, "cartpole")
    with pytest.raises(ValueError, match=r"algo_type 'ns', population_size 3, k 2; this run is algo_type 'nsr', population_size 3, k 2"):
        S.run(tmp_path / "cp", 1, "cartpole", algo_type="nsr")
    with pytest.raises(ValueError, match=r"population_size 3, k 2; this run is algo_type 'ns', population_size 2, k 2"):
        S.run(tmp_path / "cp", 1, "cartpole", ns={"population_size": 2})
    with pytest.raises(ValueError, match=r"k 2; this run is algo_type 'ns', population_size 3, k 5"):
        S.run(tmp_path / "cp", 1, "cartpole", ns={"k": 5})
    with pytest.raises(ValueError, match=r"P = 10, num_rollouts 1; this run is game 'gym.CartPole-v1', model 'LinearClassifier', P = 10, num_rollouts 3"):
        S.run(tmp_path / "cp", 1, "cartpole", ns={"num_rollouts": 3})
    with pytest.raises(ValueError, match=r"model 'LinearClassifier', P = 10, num_rollouts 1; this run is game 'gym.CartPole-v1', model 'Dense\(5; relu\)', P = 37"):
        S.run(tmp_path / "cp", 1, "cartpole", eng=S.host_engine("cartpole", (5,)), model=None)
    with pytest.raises(ValueError, match=r"holds game 'gym.CartPole-v1', model 'LinearClassifier', P = 10, num_rollouts 1; this run is game 'maze', model 'LinearClassifier', P = 24"):
        S.run(tmp_path / "cp", 1, "maze")
    # the two maze runs do not take each other's snapshots: the model and P differ
    S.run(tmp_path / "dense16", 1, "maze", eng=S.host_engine("maze", (16, 16), "relu", 8), model=None)
    with pytest.raises(ValueError, match=r"holds game 'maze', model 'Dense\(16, 16; relu\)', P = 498, num_rollouts 1; this run is game 'maze', model 'SimpleClassifier', P = 498"):
        nses_gpu.main(str(tmp_path / "dense16"), engine=MN.MazeNoveltyHostEngine(max_members=8), noise=D.shared_noise(), seed=4, max_iters=1,
                      **S.exp("maze", model="SimpleClassifier"))
    plain = {k: v for k, v in S.exp("cartpole").items() if k not in ("algo_type", "novelty_search")}
    plain.update(num_test_episodes=2, return_proc_mode="centered_rank")
    es_gpu.main(str(tmp_path / "es"), engine=S.host_engine("cartpole"), noise=D.shared_noise(), seed=4, max_iters=1, **plain)
    with pytest.raises(ValueError, match=r"'es_gpu'.*'nses'"):
        S.run(tmp_path / "es", 1, "cartpole")
