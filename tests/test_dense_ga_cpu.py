"""CPU: Deep-GA on the dense kind (csrc/dense_ga.h).  The host twins (dne_dense_ga_theta_host,
dne_dense_ga_members_host) against the contract in float32 numpy with P a parameter (dense_ga_support.py) on the five shapes, and against
maze_ga's own twins at (16, 16); their refusals by text; the header's host side under sanitizers in a program of its own; ga_gpu.dense_main
on DenseGaHostEngine against the same algorithm written the reference's way (dense_ga_support.plain_loop) and, at (16, 16) on the maze,
against ga_gpu.maze_main; the routing of ga_gpu.main and the resumes it refuses.  Every comparison is bit for bit."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import dense_ga_support as S
import dense_support as D
import maze_ga_support as MG
import maze_support as M

CASE_IDS = [S.case_id(c) for c in S.CASES]


def _same(a, b):
    return M.same_nan(np.asarray(a, np.float32), np.asarray(b, np.float32))


# ---- 1. the host twins against the numpy statement, bit for bit ------------------------------------------------------------------------------------
def test_shapes_are_the_block_edges():
    assert tuple(S.num_params(c) for c in S.CASES) == S.PS == (24, 256, 291, 498, 9218)
    assert [(-(-p // 256), p % 256) for p in S.PS] == [(1, 24), (1, 0), (2, 35), (2, 242), (37, 2)]
    for c in S.CASES:
        assert S.scale_by(c).size == S.num_params(c)


@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_theta_host_equals_numpy(case):
    from dne_hip import _lib
    P, sb, table = S.num_params(case), S.scale_by(case), S.noise()
    genomes = S.genomes(P)
    assert sorted(len(g) for g in genomes) == sorted(2 * list(S.CHAIN_LENGTHS) + [1, 1])
    idx = [S.split(g)[0] for g in genomes] + [i for g in genomes for i, _ in S.split(g)[1]]
    assert 0 in idx and table.size - P in idx
    assert {np.float32(p) for g in genomes for _, p in S.split(g)[1]} == {np.float32(p) for p in S.POWERS}
    for genome in genomes:
        got = _lib.dense_ga_theta_host(table, sb, genome)
        assert got.dtype == np.float32 and got.shape == (P, ) and _same(got, S.genome_theta(table, sb, genome)), (genome, )
        if len(genome) > 1:                                                                       # the chain IS the child form applied in order
            parent = _lib.dense_ga_theta_host(table, sb, genome[:-1])
            assert _same(got, S.perturbed(parent, table, *genome[-1]))


@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_members_host_equals_numpy_on_every_form(case):
    from dne_hip import _lib
    P, sb, table = S.num_params(case), S.scale_by(case), S.noise()
    forms = set()
    for T in S.BANKS:
        bank = np.stack([S.genome_theta(table, sb, g) for g in S.bank_genomes(P, T)]) if T else None
        for n in S.COUNTS:
            for kept in (False, True):
                parent, idx, power = S.descriptors(P, T, n, seed=n, kept=kept and T > 0)
                got = _lib.dense_ga_members_host(table, sb, bank, parent, idx, power)
                assert got.shape == (n, P) and _same(got, S.members_theta(table, sb, bank, parent, idx, power)), (T, n, kept)
                forms |= {"root" if a < 0 else "kept" if b < 0 else "again" if (b == 0 and c == 0) else "child" for a, b, c in zip(parent, idx, power)}
        if T:
            parent, idx, power = S.descriptors(P, T, 9, seed=9, kept=True)
            assert parent[-1] == parent[-2] and idx[-1] < 0 and idx[-2] < 0                        # one source named twice
            assert T == 1 or any(j != a for j, (a, b) in enumerate(zip(parent, idx)) if b < 0)    # kept to another index than its own
            assert {0, table.size - P} <= set(int(b) for b in idx if b >= 0)
    assert forms == {"root", "kept", "again", "child"}


@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_kept_is_bit_for_bit_and_power_zero_is_the_child_formula(case):
    from dne_hip import _lib
    P, sb = S.num_params(case), S.scale_by(case)
    table = S.signed_zero_noise(P)
    root = _lib.dense_ga_members_host(table, sb, None, [-1], [0], [0.5])[0]
    assert _same(root, S.root_theta(table, sb, 0))
    biases = S.bias_positions(case)
    assert biases.size == sum(D.dims_of(case[0], case[1])[1:]) and np.all(M.bits(root[biases]) == 0x80000000)   # every bias of this root is -0.0
    kept, again_same_sign, again_other_sign = _lib.dense_ga_members_host(table, sb, root[None], [0, 0, 0], [-1, 0, P], [9.0, 0.0, 0.0])
    assert np.array_equal(M.bits(kept), M.bits(root))                                             # kept: the bits, the power unread
    assert np.array_equal(M.bits(again_same_sign), M.bits(root))                                  # -0.0 + fl(0 * negative) = -0.0
    assert np.all(M.bits(again_other_sign[biases]) == 0) and np.array_equal(again_other_sign, root)   # -0.0 + (+0.0) = +0.0: the child formula
    assert _same(again_other_sign, S.perturbed(root, table, P, 0.0))


def test_twins_equal_maze_ga_at_16_16():
    """the witness: at (16, 16) on the maze the P-generic twins and maze_ga.h's own are the same function"""
    from dne_hip import _lib
    case = S.CASES[3]
    sb, table = S.scale_by(case), S.noise()
    assert S.num_params(case) == MG.P and np.array_equal(M.bits(sb), M.bits(MG.scale_by()))
    for genome in MG.genomes():
        assert np.array_equal(M.bits(_lib.dense_ga_theta_host(table, sb, genome)), M.bits(_lib.maze_ga_theta_host(table, sb, genome)))
    for T in (0, ) + MG.BANKS:
        bank = np.stack([MG.genome_theta(table, g) for g in MG.bank_genomes(T)]) if T else None
        for n in MG.COUNTS:
            parent, idx, power = MG.descriptors(T, n, seed=n, kept=T > 0)
            a = _lib.dense_ga_members_host(table, sb, bank, parent, idx, power)
            b = _lib.maze_ga_members_host(table, sb, bank, parent, idx, power)
            assert M.same_nan(a, b), (T, n)


def test_host_refusals():
    from dne_hip import _lib
    for case in (S.CASES[0], S.CASES[2], S.CASES[4]):
        P, sb, table = S.num_params(case), S.scale_by(case), S.noise()
        last = table.size - P
        bank = np.zeros((3, P), np.float32)
        for genome, text in (((), "dne_dense_ga_theta_host: genome 0: empty chain"),
                             ((last + 1, ), r"genome 0: noise index %d \+ P = %d outside the table of %d" % (last + 1, P, table.size)),
                             ((-1, ), r"noise index -1 \+ P = %d outside the table" % P),
                             ((0, (last + 1, 0.1)), r"noise index %d \+ P = %d outside the table of %d" % (last + 1, P, table.size))):
            with pytest.raises(_lib.DneError, match=text):
                _lib.dense_ga_theta_host(table, sb, genome)
        with pytest.raises(_lib.DneError, match="a table of %d floats holds no P = %d parameters" % (P - 1, P)):
            _lib.dense_ga_theta_host(table[:P - 1], sb, (0, ))
        for T, parent, idx, text in ((3, [3], [0], "member 0: parent 3, the bank holds 3"), (0, [0], [0], "member 0: parent 0 on an empty bank"),
                                     (3, [-2], [0], r"member 0: parent -2 \(-1 is a root"), (3, [-1], [-1], "member 0: a root needs a noise index, got -1"),
                                     (3, [1], [last + 1], r"member 0: noise index %d \+ P = %d outside the table of %d" % (last + 1, P, table.size)),
                                     (3, [-1], [last + 1], r"\+ P = %d outside the table" % P), (3, [0, 1, 5], [0, 0, 0], "member 2: parent 5, the bank holds 3")):
            with pytest.raises(_lib.DneError, match=text):
                _lib.dense_ga_members_host(table, sb, bank[:T] if T else None, parent, idx, np.zeros(len(parent), np.float32))
        with pytest.raises(_lib.DneError, match="n = 0, at least one member is needed"):
            _lib.dense_ga_members_host(table, sb, bank, [], [], [])
        with pytest.raises(_lib.DneError, match="3 parents, 2 indices"):
            _lib.dense_ga_members_host(table, sb, bank, [0, 1, 2], [0, 0], 0.0)
    table = S.noise()
    with pytest.raises(_lib.DneError, match=r"dne_dense_ga_theta_host: P = 0 outside \[1, 9218\]"):
        _lib.dense_ga_theta_host(table, np.zeros(0, np.float32), (0, ))
    with pytest.raises(_lib.DneError, match=r"dne_dense_ga_members_host: P = 9219 outside \[1, 9218\]"):
        _lib.dense_ga_members_host(table, np.zeros(9219, np.float32), None, [-1], [0], 0.0)
    # the C entry points' own argument checks
    import ctypes as C
    lib, f = _lib.load(), np.zeros(24, np.float32)
    i64, i32 = np.zeros(1, np.int64), np.zeros(1, np.int32)
    fp, lp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    assert lib.dne_dense_ga_theta_host(None, C.c_size_t(24), fp(f), 24, lp(i64), fp(f), 1, fp(f)) == -1
    assert b"dne_dense_ga_theta_host: a buffer is missing" in lib.dne_last_error(None)
    assert lib.dne_dense_ga_theta_host(fp(f), C.c_size_t(24), fp(f), 24, lp(i64), fp(f), 1, None) == -1
    assert b"dne_dense_ga_theta_host: a buffer is missing" in lib.dne_last_error(None)
    assert lib.dne_dense_ga_members_host(fp(f), C.c_size_t(24), fp(f), 24, None, 1, ip(i32), lp(i64), fp(f), 1, fp(f)) == -1
    assert b"dne_dense_ga_members_host: T = 1 parents without a bank" in lib.dne_last_error(None)
    assert lib.dne_dense_ga_members_host(fp(f), C.c_size_t(24), fp(f), 24, None, 0, None, lp(i64), fp(f), 1, fp(f)) == -1
    assert b"dne_dense_ga_members_host: a buffer is missing" in lib.dne_last_error(None)


# ---- 2. the header's host side under sanitizers, in a program of its own ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/dense_ga_asan_main.cpp, built once: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(M.ROOT, "tests", "dense_ga_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("dense_ga_asan") / "dense_ga_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(M.ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program, tmp_path, case):
    """a table of P + 1000 floats in an exactly sized buffer: index 1000 reads its last float; every form, the aliasing promotions included"""
    P, sb = S.num_params(case), S.scale_by(case)
    count = P + 1000
    table, last = S.noise()[:count], 1000
    hexes = lambda v: " ".join(float(x).hex() for x in np.asarray(v, np.float32).reshape(-1))
    rs = np.random.RandomState(3)
    cases, want = [], []
    for n in S.CHAIN_LENGTHS:
        idx = [int(v) for v in rs.randint(0, last + 1, size=n)]
        idx[-1] = last; idx[0] = 0 if n > 1 else last
        genome = (idx[0], ) + tuple((idx[j], S.POWERS[j % len(S.POWERS)]) for j in range(1, n))
        cases.append("G %d %s" % (n, " ".join("%d %s" % (i, float(np.float32(p)).hex()) for i, p in [(idx[0], 0.0)] + list(genome[1:]))))
        want.append(S.genome_theta(table, sb, genome))
    for T in S.BANKS:
        bank = np.stack([S.genome_theta(table, sb, (int(rs.randint(0, last + 1)), (last, 0.005))) for _ in range(T)]) if T else np.zeros((0, P), np.float32)
        parent, idx, power = S.descriptors(P, T, 9, seed=T, kept=T > 0, count=count)
        idx[0] = last
        assert T == 0 or (np.any(idx < 0) and parent[-1] == parent[-2])
        cases.append("M %d 9 %s %s" % (T, hexes(bank), " ".join("%d %d %s" % (a, b, float(c).hex()) for a, b, c in zip(parent, idx, power))))
        want.append(S.members_theta(table, sb, bank, parent, idx, power).reshape(-1))
    refused = ["G 0", "G 1 %d 0x0p+0" % (last + 1), "G 2 0 0x0p+0 -1 0x1p-3", "M 0 1 0 0 0x0p+0", "M 0 1 -1 %d 0x0p+0" % (last + 1),
               "M 1 2 %s 0 -1 0x0p+0 1 0 0x0p+0" % hexes(np.zeros(P)), "M 1 1 %s -1 -1 0x0p+0" % hexes(np.zeros(P))]
    path = tmp_path / "cases.txt"
    path.write_text("%d %d\n%s\n%s\n%s\n" % (count, P, hexes(table), hexes(sb), "\n".join(cases + refused)))
    out = subprocess.run([sanitizer_program, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % (len(cases) + len(refused)) and len(lines) == len(cases) + len(refused) + 1
    for line, w in zip(lines, want):
        got = np.array([float("nan") if t == "nan" else float.fromhex(t) for t in line.split()], np.float32)
        assert _same(got, w)
    assert all(line.startswith("refused ") for line in lines[len(cases):-1]), lines[len(cases):-1]
    assert ("+ P = %d outside the table of %d" % (P, count)) in lines[len(cases) + 1]


# ---- 3. the driver on the host engine ----------------------------------------------------------------------------------------------------------------
SEED = 4
LINEAR = {"maze": ("maze", (), "relu"), "gym.CartPole-v1": ("cartpole", (), "relu")}
GAMES = sorted(LINEAR)
CONFIGS = {"plain": {}, "no_parents": {"selection_threshold": 0}}


def _run(log_dir, iters, game, eng=None, case=None, **over):
    from dne_hip import ga_gpu
    eng = eng or S.host_engine(case or LINEAR[game], max_members=10)
    return ga_gpu.main(str(log_dir), engine=eng, noise=S.shared_noise(), seed=SEED, max_iters=iters, **S.exp(game, **over)), eng


def _assert_generation(state, eng, rec, exp):
    """the driver after g generations against record g of the plain loop"""
    from dne_hip import ga_gpu
    parents = ga_gpu.parents_of(state, exp["selection_threshold"])
    assert parents == rec["parents"] and eng.dense_ga_parents() == len(parents)
    for j, th in enumerate(rec["thetas"]):
        assert np.array_equal(M.bits(eng.dense_ga_get_parent(j)), M.bits(th)), j                  # the promoted bank = every parent from its whole genome
    assert state.elite.seeds == rec["elite"] and [o.seeds for o in state.population] == rec["top"]
    assert state.curr_solution == rec["curr_solution"] and state.timesteps_so_far == rec["timesteps_so_far"]
    assert (state.curr_solution_val, state.curr_solution_test) == (rec["curr_solution_val"], rec["curr_solution_test"])
    assert len(state.population) == max(exp["selection_threshold"], exp["validation_threshold"])   # lazy: genomes for the survivors only


def _generation_returns(eng, n):
    return [e[2] for e in eng.evals if len(e[2]) == n]


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("game", GAMES)
def test_driver_equals_the_plain_loop_generation_by_generation(oracle, tmp_path, game, config):
    exp = S.exp(game, **CONFIGS[config])
    records = S.plain_loop(LINEAR[game], exp, SEED, 3)
    for g in (1, 2, 3):
        (test, val, state), eng = _run(tmp_path / ("g%d" % g), g, game, **CONFIGS[config])
        assert state.it == g and (test, val["val"]) == (state.curr_solution_test, state.curr_solution_val)
        _assert_generation(state, eng, records[g - 1], exp)
        rets = _generation_returns(eng, exp["population_size"])
        assert len(rets) == g and all(np.array_equal(M.bits(a), M.bits(r["returns"])) for a, r in zip(rets, records))
        builds = [c for c in eng.calls if c[0] == "dense_ga_build"]
        promotes = [c for c in eng.calls if c[0] == "dense_ga_promote"]
        T = exp["selection_threshold"]
        assert builds == ([("dense_ga_build", T)] if T else []) and promotes == [("dense_ga_promote", T)] * (g - 1 if T else 0)   # one build per call
    assert state.num_frames == sum(int(e[3].sum()) for e in eng.evals if len(e[3]) == exp["population_size"])   # steps, no frame-skip factor
    if config == "no_parents":                                                                    # random search: roots every generation, an empty bank
        assert all(len(o.seeds) == 1 for o in state.population) and eng.dense_ga_parents() == 0
        assert all(np.all(e[0] == -1) for e in eng.evals)
    if game == "maze":
        assert all(e[4] is None for e in eng.evals)                                               # no environment seed is drawn
    else:                                                                                         # every call under its own seeds: no episode twice
        seeds = np.concatenate([e[4] for e in eng.evals])
        assert len(eng.evals) == 3 * 3 and np.unique(seeds).size == seeds.size == 3 * (10 + 4 + 2)
        assert len({int(l) for e in eng.evals for l in e[3]}) >= 3                                # the episodes end at different steps


@pytest.mark.parametrize("game", GAMES)
def test_driver_keeps_an_elite_by_the_kept_form(oracle, tmp_path, game):
    """over enough generations an elite survives a generation; its bank entry then moves by the kept form, and the run still equals the
    plain loop"""
    exp = S.exp(game)
    records = S.plain_loop(LINEAR[game], exp, SEED, 6)
    retained = [g for g in range(1, 6) if records[g]["elite"] == records[g - 1]["elite"]]
    assert retained, [r["elite"] for r in records]
    seen = []

    class Recording(S.DenseGaHostEngine):
        def dense_ga_promote(self, parent, idx, power):
            seen.append((np.array(parent), np.array(idx)))
            super().dense_ga_promote(parent, idx, power)

    env, hidden, nl = LINEAR[game]
    eng = Recording(env, hidden, nl, 10)
    (_, _, state), eng = _run(tmp_path / "six", 6, game, eng=eng)
    _assert_generation(state, eng, records[5], exp)
    assert len(seen) == 5 and any(np.any(idx < 0) for _, idx in seen)
    for g in retained:                                                                            # promotion g - 1 follows generation g (0-based)
        parent, idx = seen[g - 1]
        assert np.sum(idx < 0) == 1 and records[g]["parents"][int(np.argmax(idx < 0))] == records[g]["elite"]


@pytest.mark.parametrize("game", GAMES)
def test_driver_resume_and_load_population(oracle, tmp_path, game):
    exp = S.exp(game)
    records = S.plain_loop(LINEAR[game], exp, SEED, 4)
    (_, _, four), e4 = _run(tmp_path / "straight", 4, game)
    _assert_generation(four, e4, records[3], exp)
    (_, _, two), e2 = _run(tmp_path / "resumed", 2, game)
    snap = pickle.load(open(tmp_path / "resumed" / "snapshot.pkl", "rb"))
    assert (snap.game, snap.model, snap.algo, snap.it, snap.num_params) == (game, "LinearClassifier", "ga", 2, e2.P) and snap.stream is not None
    (_, _, again), e22 = _run(tmp_path / "resumed", 2, game)                                       # a fresh engine: the bank is rebuilt from the genomes
    assert again.it == 4
    _assert_generation(again, e22, records[3], exp)
    assert [c for c in e22.calls if c[0] == "dense_ga_build"] == [("dense_ga_build", 3)]
    assert e22.calls.index(("dense_ga_build", 3)) < e22.calls.index(("dense_ga_eval", 10))
    assert [c for c in e22.calls if c[0] == "dense_ga_promote"] == [("dense_ga_promote", 3)] * 2
    assert all(np.array_equal(M.bits(a), M.bits(b)) for a, b in zip(_generation_returns(e22, 10), _generation_returns(e4, 10)[2:]))
    assert [o.seeds for o in again.population] == [o.seeds for o in four.population] and again.num_frames == four.num_frames
    assert again.validation_timesteps_so_far == four.validation_timesteps_so_far
    assert D.log_rows(tmp_path / "resumed")[-2:] == D.log_rows(tmp_path / "straight")[-2:]
    # load_population: another run's snapshot as the first parents (ga.py:143-144), elite and counters fresh
    (_, _, loaded), el = _run(tmp_path / "loaded", 1, game, load_population=str(tmp_path / "resumed" / "snapshot.pkl"))
    assert el.calls.index(("dense_ga_build", 3)) < el.calls.index(("dense_ga_eval", 10)) and loaded.it == 1
    parents = [o.seeds for o in again.population[:3]]
    assert all(o.seeds[:-1] in parents for o in loaded.population)
    pop = [S.Individual(o.seeds, o.fitness, 0) for o in again.population]
    _assert_generation(loaded, el, S.plain_loop(LINEAR[game], exp, SEED, 1, population=pop)[0], exp)


def test_driver_equals_maze_main_at_16_16(oracle, tmp_path):
    """the second witness: dense_main on a (16, 16) relu maze engine and maze_main on MazeGaHostEngine write the same rows and the same
    parents from the same seed (no environment seed is drawn on the maze, so the two streams are one)"""
    from dne_hip import ga_gpu
    case = S.CASES[3]
    exp = S.exp("maze", model="SimpleClassifier")
    dense_exp = {k: v for k, v in exp.items() if k != "model"}
    me = MG.MazeGaHostEngine(max_members=10)
    _, _, ms = ga_gpu.main(str(tmp_path / "maze"), engine=me, noise=S.shared_noise(), seed=SEED, max_iters=4, **exp)
    de = S.host_engine(case, max_members=10)
    _, _, ds = ga_gpu.main(str(tmp_path / "dense"), engine=de, noise=S.shared_noise(), seed=SEED, max_iters=4, **dense_exp)
    rows = D.log_rows(tmp_path / "dense")
    assert len(rows) == 4 and rows == D.log_rows(tmp_path / "maze")
    assert de.dense_ga_parents() == me.maze_ga_parents() == 3
    for j in range(3):
        assert np.array_equal(M.bits(de.dense_ga_get_parent(j)), M.bits(me.maze_ga_get_parent(j)))
    assert [o.seeds for o in ds.population] == [o.seeds for o in ms.population] and ds.elite.seeds == ms.elite.seeds
    assert ds.stream[1].tolist() == ms.stream[1].tolist() and ds.stream[2] == ms.stream[2]
    assert (ds.model, ms.model, ds.num_params) == ("Dense(16, 16; relu)", "SimpleClassifier", 498)
    assert [(c[0].replace("dense_ga", "maze_ga"), ) + tuple(c[1:]) for c in de.calls if c[0].startswith("dense_ga")] == \
        [c for c in me.calls if c[0].startswith("maze_ga")]


# ---- 4. the routing of ga_gpu.main, and the resumes it refuses -------------------------------------------------------------------------------------------
def test_routing_without_an_engine(oracle, tmp_path, monkeypatch):
    """LinearClassifier on the two games and SimpleClassifier on the cart-pole open a KIND_DENSE engine of the right shape"""
    from dne_hip import _lib, ga_gpu
    made = []

    def fake_engine(kind, n_actions, max_members=0, env=None, hidden=(), nonlin=None, **kw):
        assert kind == _lib.KIND_DENSE and n_actions == 2 and nonlin == "relu"
        e = S.DenseGaHostEngine({_lib.KIND_MAZE: "maze", _lib.KIND_CARTPOLE: "cartpole"}[env], hidden, nonlin, max_members)
        made.append(e)
        return e

    monkeypatch.setattr(_lib, "Engine", fake_engine)
    for game, model, hidden, P in (("maze", "LinearClassifier", (), 24), ("gym.CartPole-v1", "LinearClassifier", (), 10),
                                   ("gym.CartPole-v1", "SimpleClassifier", (16, 16), 386)):
        log = tmp_path / ("%s-%s" % (game, model))
        _, _, state = ga_gpu.main(str(log), noise=S.shared_noise(), seed=SEED, max_iters=2, **S.exp(game, model=model))
        e = made[-1]
        assert (e.hidden, e.P, e.max_members) == (hidden, P, 10) and state.it == 2
        assert (state.game, state.model, state.algo, state.num_params) == (game, model, "ga", P)
        assert ("dense_ga_build", 3) in e.calls and ("dense_ga_promote", 3) in e.calls
        from dne_hip import policies
        assert np.array_equal(e.scale, policies.dense_scale_by(e.env_kind, hidden, 2))
    assert np.array_equal(made[-1].scale, __import__("dne_hip").policies.simple_scale_by(_lib.KIND_CARTPOLE))   # cartpole.h's layout
    # the same SimpleClassifier run written out: the plain loop on the (16, 16) cart-pole shape
    rec = S.plain_loop(("cartpole", (16, 16), "relu"), S.exp("gym.CartPole-v1", model="SimpleClassifier"), SEED, 2)[1]
    _assert_generation(state, made[-1], rec, S.exp("gym.CartPole-v1"))


def test_routing_with_an_engine_and_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import ga_gpu
    x = str(tmp_path / "x")
    maze16 = S.host_engine(S.CASES[3], max_members=10)
    with pytest.raises(ValueError, match=r"game 'gym.CartPole-v1' asked for, the engine passed in \(kind 8 on environment kind 4\) runs 'maze'"):
        _run(x, 1, "gym.CartPole-v1", eng=maze16)
    with pytest.raises(ValueError, match=r"model 'LinearClassifier' asked for, the engine passed in \(kind 8\) runs 'Dense\(16, 16; relu\)'"):
        _run(x, 1, "maze", eng=maze16)
    with pytest.raises(ValueError, match=r"model 'SimpleClassifier' asked for, the engine passed in \(kind 8\) runs 'Dense\(16, 16; relu\)'"):
        _run(x, 1, "maze", eng=maze16, model="SimpleClassifier")
    with pytest.raises(NotImplementedError, match="Pendulum-v0"):
        ga_gpu.main(x, engine=S.host_engine(S.CASES[1], 10), noise=S.shared_noise(), max_iters=1, **S.exp("Pendulum-v0", model="Dense(51; tanh)"))
    with pytest.raises(NotImplementedError, match="novelty_search"):
        _run(x, 1, "maze", novelty_search={"k": 2, "archive_prob": 0.1})
    with pytest.raises(NotImplementedError, match="novelty_search"):
        _run(x, 1, "gym.CartPole-v1", novelty_search={"k": 2, "archive_prob": 0.1})
    # every other kind: refused as before
    with pytest.raises(NotImplementedError, match="LinearClassifier"):
        ga_gpu.main(x, engine=M.MazeHostEngine(max_members=10), noise=S.shared_noise(), max_iters=1, **S.exp("maze"))
    with pytest.raises(NotImplementedError, match="gym.CartPole-v1"):
        ga_gpu.main(x, engine=OracleEngine(0, ref_count=8, max_members=10), noise=S.shared_noise(), max_iters=1,
                    **S.exp("gym.CartPole-v1", model="SimpleClassifier"))
    with pytest.raises(NotImplementedError, match=r"'SimpleClassifier' on game 'frostbite'"):
        ga_gpu.main(x, engine=MG.MazeGaHostEngine(), noise=S.shared_noise(), max_iters=1, **S.exp("frostbite", model="SimpleClassifier"))
    with pytest.raises(NotImplementedError, match=r"'LinearClassifier' on game 'frostbite'"):
        ga_gpu.dense_main(x, noise=S.shared_noise(), max_iters=1, **S.exp("frostbite"))
    assert not os.path.exists(tmp_path / "x" / "snapshot.pkl")
    # a model name that is the engine's is accepted
    (_, _, state), _ = _run(tmp_path / "named", 1, "maze", eng=maze16, model="Dense(16, 16; relu)")
    assert state.model == "Dense(16, 16; relu)"


def test_resumes_that_do_not_fit_name_both_sides(oracle, tmp_path):
    from dne_hip import es_gpu, ga_gpu
    _run(tmp_path / "lin", 1, "maze")
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'LinearClassifier'; this run is game 'maze' under model 'Dense\(16, 16; relu\)'"):
        _run(tmp_path / "lin", 1, "maze", case=S.CASES[3], model="Dense(16, 16; relu)")
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'LinearClassifier'; this run is game 'gym.CartPole-v1' under model 'LinearClassifier'"):
        _run(tmp_path / "lin", 1, "gym.CartPole-v1")
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'LinearClassifier'; this run is game 'maze' under model 'SimpleClassifier'"):
        ga_gpu.main(str(tmp_path / "lin"), engine=MG.MazeGaHostEngine(max_members=10), noise=S.shared_noise(), max_iters=1, **S.exp("maze", model="SimpleClassifier"))
    # maze_main's snapshot under dense_main, and an Atari GA snapshot
    ga_gpu.main(str(tmp_path / "mz"), engine=MG.MazeGaHostEngine(max_members=10), noise=S.shared_noise(), max_iters=1, **S.exp("maze", model="SimpleClassifier"))
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'SimpleClassifier'; this run is game 'maze' under model 'Dense\(16, 16; relu\)'"):
        _run(tmp_path / "mz", 1, "maze", case=S.CASES[3], model=None)
    os.makedirs(tmp_path / "atari")
    with open(tmp_path / "atari" / "snapshot.pkl", "wb") as f:
        pickle.dump(ga_gpu.TrainingState(S.exp("maze")), f)
    with pytest.raises(ValueError, match=r"game 'an Atari game' under model 'Model'; this run is game 'maze' under model 'LinearClassifier'"):
        _run(tmp_path / "atari", 1, "maze")
    # the same game and model name under another P
    snap = pickle.load(open(tmp_path / "lin" / "snapshot.pkl", "rb"))
    snap.num_params = 25
    os.makedirs(tmp_path / "p")
    with open(tmp_path / "p" / "snapshot.pkl", "wb") as f:
        pickle.dump(snap, f)
    with pytest.raises(ValueError, match=r"holds model 'LinearClassifier' with P = 25; this run is model 'LinearClassifier' with P = 24"):
        _run(tmp_path / "p", 1, "maze")
    # another driver's snapshot
    es_exp = dict(D.exp("maze"), maze_file=M.MAZE_FILE)
    es_gpu.main(str(tmp_path / "es"), engine=D.host_engine(("maze", (), "relu"), 10), noise=S.shared_noise(), seed=SEED, max_iters=1, **es_exp)
    with pytest.raises(ValueError, match=r"'es_gpu'.*'ga'"):
        _run(tmp_path / "es", 1, "maze")
