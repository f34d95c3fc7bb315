"""CPU: Deep-GA on the hard maze.  The host twins of csrc/maze_ga.h (dne_maze_ga_theta_host, dne_maze_ga_members_host) against the contract
stated in float32 numpy (maze_ga_support.py), bit for bit; the header's host side under sanitizers in a program of its own; and
dne_hip/ga_gpu.py's maze loop on MazeGaHostEngine against the same algorithm written the reference's way (maze_ga_support.plain_loop)."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import maze_ga_support as S
import maze_support as M


def _same(a, b):
    return M.same_nan(np.asarray(a, np.float32), np.asarray(b, np.float32))


# ---- 1. the host twins against the numpy statement, bit for bit ------------------------------------------------------------------------------------
def test_genomes_cover_what_they_are_for():
    lengths = sorted(len(g) for g in S.genomes())
    assert lengths == sorted(2 * list(S.CHAIN_LENGTHS) + [1, 1])
    idx = [S.split(g)[0] for g in S.genomes()] + [i for g in S.genomes() for i, _ in S.split(g)[1]]
    assert 0 in idx and S.noise().size - S.P in idx
    powers = {np.float32(p) for g in S.genomes() for _, p in S.split(g)[1]}
    assert powers == {np.float32(p) for p in S.POWERS}
    assert np.all(np.isfinite(S.genome_thetas())) and np.abs(S.genome_thetas()).max() > 1e29      # 1e30 * noise stays a float


@pytest.mark.parametrize("g", range(len(S.genomes())))
def test_theta_host_equals_numpy(g):
    from dne_hip import _lib
    genome = S.genomes()[g]
    got = _lib.maze_ga_theta_host(S.noise(), S.scale_by(), genome)
    assert got.dtype == np.float32 and _same(got, S.genome_thetas()[g]), (genome, )
    if len(genome) > 1:                                                                           # the chain IS the child form applied in order
        parent = _lib.maze_ga_theta_host(S.noise(), S.scale_by(), genome[:-1])
        assert _same(got, M.perturbed(parent, S.noise(), *genome[-1]))


@pytest.mark.parametrize("T", (0, ) + S.BANKS)
def test_members_host_equals_numpy_on_every_form(T):
    from dne_hip import _lib
    bank = np.stack([S.genome_theta(S.noise(), g) for g in S.bank_genomes(T)]) if T else None
    for n in S.COUNTS:
        for kept in (False, True):
            parent, idx, power = S.descriptors(T, n, seed=n, kept=kept and T > 0)
            got = _lib.maze_ga_members_host(S.noise(), S.scale_by(), bank, parent, idx, power)
            assert got.shape == (n, S.P) and _same(got, S.members_theta(S.noise(), bank, parent, idx, power)), (T, n, kept)


def test_descriptors_cover_what_they_are_for():
    forms = set()
    for T in S.BANKS:
        parent, idx, power = S.descriptors(T, 9, seed=9, kept=True)
        forms |= {"root" if a < 0 else "kept" if b < 0 else "again" if (b == 0 and c == 0) else "child" for a, b, c in zip(parent, idx, power)}
        assert parent[-1] == parent[-2] and idx[-1] < 0 and idx[-2] < 0                            # one source named twice
        kept = [(j, a) for j, (a, b) in enumerate(zip(parent, idx)) if b < 0]
        assert T == 1 or any(j != a for j, a in kept)                                             # kept to another index than its own
        assert {0, S.noise().size - S.P} <= set(int(b) for b in idx if b >= 0)
    assert forms == {"root", "kept", "again", "child"}


def test_kept_is_bit_for_bit_and_power_zero_is_the_child_formula():
    from dne_hip import _lib
    noise = S.signed_zero_noise()
    root = _lib.maze_ga_members_host(noise, S.scale_by(), None, [-1], [0], [0.5])[0]
    assert _same(root, S.root_theta(noise, 0))
    biases = np.r_[M.B1:M.W2, M.B2:M.W3, M.B3:S.P]
    assert np.all(M.bits(root[biases]) == 0x80000000)                                             # every bias of this root is -0.0
    kept, again_same_sign, again_other_sign = _lib.maze_ga_members_host(noise, S.scale_by(), root[None], [0, 0, 0], [-1, 0, S.P], [9.0, 0.0, 0.0])
    assert np.array_equal(M.bits(kept), M.bits(root))                                             # kept: the bits, the power unread
    assert np.array_equal(M.bits(again_same_sign), M.bits(root))                                  # -0.0 + fl(0 * negative) = -0.0
    assert np.all(M.bits(again_other_sign[biases]) == 0) and np.array_equal(again_other_sign, root)   # -0.0 + (+0.0) = +0.0: the child formula, nothing else
    assert _same(again_other_sign, M.perturbed(root, noise, S.P, 0.0))


def test_host_refusals():
    from dne_hip import _lib
    noise, sb, last = S.noise(), S.scale_by(), S.noise().size - S.P
    bank = S.genome_thetas()[:3]
    for genome, text in (((), "empty chain"), ((last + 1, ), r"outside the table"), ((-1, ), r"outside the table"),
                         ((0, (last + 1, 0.1)), r"noise index %d \+ 498 outside the table of %d" % (last + 1, noise.size))):
        with pytest.raises(_lib.DneError, match=text):
            _lib.maze_ga_theta_host(noise, sb, genome)
    with pytest.raises(_lib.DneError, match="holds no 498 parameters"):
        _lib.maze_ga_theta_host(noise[:497], sb, (0, ))
    with pytest.raises(_lib.DneError, match="498 expected"):
        _lib.maze_ga_theta_host(noise, sb[:100], (0, ))
    for T, parent, idx, text in ((3, [3], [0], "parent 3, the bank holds 3"), (0, [0], [0], "parent 0 on an empty bank"), (3, [-2], [0], "parent -2"),
                                 (3, [-1], [-1], "a root needs a noise index"), (3, [1], [last + 1], "outside the table"),
                                 (3, [-1], [last + 1], "outside the table"), (3, [0, 1, 5], [0, 0, 0], "member 2: parent 5")):
        with pytest.raises(_lib.DneError, match=text):
            _lib.maze_ga_members_host(noise, sb, bank[:T] if T else None, parent, idx, np.zeros(len(parent), np.float32))
    with pytest.raises(_lib.DneError, match="n = 0"):
        _lib.maze_ga_members_host(noise, sb, bank, [], [], [])
    with pytest.raises(_lib.DneError, match="3 parents, 2 indices"):
        _lib.maze_ga_members_host(noise, sb, bank, [0, 1, 2], [0, 0], 0.0)


# ---- 2. the header's host side under sanitizers, in a program of its own ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/maze_ga_asan_main.cpp, built once: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(M.ROOT, "tests", "maze_ga_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("maze_ga_asan") / "maze_ga_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(M.ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program, tmp_path):
    """a table of 4096 floats in an exactly sized buffer: index 4096 - 498 reads its last float"""
    count = 4096
    noise, last = S.noise()[:count], count - S.P
    hexes = lambda v: " ".join(float(x).hex() for x in np.asarray(v, np.float32).reshape(-1))
    rs = np.random.RandomState(3)
    cases, want = [], []
    for n in S.CHAIN_LENGTHS:
        idx = [int(v) for v in rs.randint(0, last + 1, size=n)]
        idx[-1] = last; idx[0] = 0 if n > 1 else last
        genome = (idx[0], ) + tuple((idx[j], S.POWERS[j % len(S.POWERS)]) for j in range(1, n))
        cases.append("G %d %s" % (n, " ".join("%d %s" % (i, float(np.float32(p)).hex()) for i, p in [(idx[0], 0.0)] + list(genome[1:]))))
        want.append(S.genome_theta(noise, genome))
    for T in (0, ) + S.BANKS:
        bank = np.stack([S.genome_theta(noise, (int(rs.randint(0, last + 1)), (last, 0.005))) for _ in range(T)]) if T else np.zeros((0, S.P), np.float32)
        parent, idx, power = S.descriptors(T, 9, seed=T, kept=T > 0)
        idx = np.where(idx >= 0, np.minimum(idx, last), idx)
        idx[0] = last
        cases.append("M %d 9 %s %s" % (T, hexes(bank), " ".join("%d %d %s" % (a, b, float(c).hex()) for a, b, c in zip(parent, idx, power))))
        want.append(S.members_theta(noise, bank, parent, idx, power).reshape(-1))
    refused = ["G 0", "G 1 %d 0x0p+0" % (last + 1), "G 2 0 0x0p+0 -1 0x1p-3", "M 0 1 0 0 0x0p+0", "M 0 1 -1 %d 0x0p+0" % (last + 1),
               "M 1 2 %s 0 -1 0x0p+0 1 0 0x0p+0" % hexes(np.zeros(S.P)), "M 1 1 %s -1 -1 0x0p+0" % hexes(np.zeros(S.P))]
    path = tmp_path / "cases.txt"
    path.write_text("%d\n%s\n%s\n%s\n" % (count, hexes(noise), hexes(S.scale_by()), "\n".join(cases + refused)))
    out = subprocess.run([sanitizer_program, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % (len(cases) + len(refused)) and len(lines) == len(cases) + len(refused) + 1
    for line, w in zip(lines, want):
        got = np.array([float("nan") if t == "nan" else float.fromhex(t) for t in line.split()], np.float32)
        assert _same(got, w)
    assert all(line.startswith("refused ") for line in lines[len(cases):-1]), lines[len(cases):-1]


# ---- 3. the driver on the host engine ----------------------------------------------------------------------------------------------------------------
SEED = 4


def _exp(**over):
    exp = {"game": "maze", "model": "SimpleClassifier", "population_size": 10, "selection_threshold": 3, "validation_threshold": 2,
           "num_validation_episodes": 2, "num_test_episodes": 2, "episode_cutoff_mode": 40, "mutation_power": 0.005, "timesteps": 10 ** 9,
           "maze_file": M.MAZE_FILE}
    exp.update(over)
    return exp


CONFIGS = {"plain": {}, "no_parents": {"selection_threshold": 0}, "wide_validation": {"validation_threshold": 4, "episode_cutoff_mode": 400}}


def _noise():
    from dne_hip import es
    noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    noise.noise = S.noise()
    noise._engines = []
    return noise


def _run(log_dir, iters, eng=None, **over):
    from dne_hip import ga_gpu
    eng = eng or S.MazeGaHostEngine(max_members=10)
    return ga_gpu.main(str(log_dir), engine=eng, noise=_noise(), seed=SEED, max_iters=iters, **_exp(**over)), eng


def _maze_of(exp):
    from dne_hip import _lib
    return _lib.load_maze(exp["maze_file"])


def _assert_generation(state, eng, rec, exp):
    """the driver after g generations against record g of the plain loop"""
    from dne_hip import ga_gpu
    parents = ga_gpu.parents_of(state, exp["selection_threshold"])
    assert parents == rec["parents"] and eng.maze_ga_parents() == len(parents)
    for j, th in enumerate(rec["thetas"]):
        assert np.array_equal(M.bits(eng.maze_ga_get_parent(j)), M.bits(th)), j                   # the promoted bank = every parent from its whole genome
    assert state.elite.seeds == rec["elite"] and [o.seeds for o in state.population] == rec["top"]
    assert state.curr_solution == rec["curr_solution"] and state.timesteps_so_far == rec["timesteps_so_far"]
    assert (state.curr_solution_val, state.curr_solution_test) == (rec["curr_solution_val"], rec["curr_solution_test"])
    assert len(state.population) == max(exp["selection_threshold"], exp["validation_threshold"])   # lazy: genomes for the survivors only


def _generation_returns(eng, n):
    """the returns of every whole-population evaluation the engine ran, in order"""
    return [e[2] for e in eng.evals if len(e[2]) == n]


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_driver_equals_the_plain_loop_generation_by_generation(oracle, tmp_path, config):
    exp = _exp(**CONFIGS[config])
    records = S.plain_loop(S.noise(), _maze_of(exp), exp, SEED, 3)
    for g in (1, 2, 3):
        (test, val, state), eng = _run(tmp_path / ("g%d" % g), g, **CONFIGS[config])
        assert state.it == g and (test, val["val"]) == (state.curr_solution_test, state.curr_solution_val)
        _assert_generation(state, eng, records[g - 1], exp)
        rets = _generation_returns(eng, exp["population_size"])
        assert len(rets) == g and all(np.array_equal(M.bits(a), M.bits(r["returns"])) for a, r in zip(rets, records))
        builds = [c for c in eng.calls if c[0] == "maze_ga_build"]
        promotes = [c for c in eng.calls if c[0] == "maze_ga_promote"]
        T = exp["selection_threshold"]
        assert builds == ([("maze_ga_build", T)] if T else []) and promotes == [("maze_ga_promote", T)] * (g - 1 if T else 0)
    assert state.num_frames == sum(int(e[3].sum()) for e in eng.evals if len(e[3]) == exp["population_size"])   # steps, no frame-skip factor
    if config == "no_parents":
        assert all(len(o.seeds) == 1 for o in state.population) and eng.maze_ga_parents() == 0


def test_driver_keeps_an_elite_by_the_kept_form(oracle, tmp_path):
    """over enough generations of the plain configuration an elite survives a generation; its bank entry then moves by the kept form, and
    the run still equals the plain loop"""
    exp = _exp()
    records = S.plain_loop(S.noise(), _maze_of(exp), exp, SEED, 6)
    retained = [g for g in range(1, 6) if records[g]["elite"] == records[g - 1]["elite"]]
    assert retained, [r["elite"] for r in records]
    seen = []

    class Recording(S.MazeGaHostEngine):
        def maze_ga_promote(self, parent, idx, power):
            seen.append((np.array(parent), np.array(idx)))
            super().maze_ga_promote(parent, idx, power)

    (_, _, state), eng = _run(tmp_path / "six", 6, eng=Recording(max_members=10))
    _assert_generation(state, eng, records[5], exp)
    assert len(seen) == 5 and any(np.any(idx < 0) for _, idx in seen)
    for g in retained:                                                                            # promotion g - 1 follows generation g (0-based)
        parent, idx = seen[g - 1]
        assert np.sum(idx < 0) == 1 and records[g]["parents"][int(np.argmax(idx < 0))] == records[g]["elite"]


def test_driver_ties_keep_arrival_order(oracle, tmp_path):
    """a maze whose goal is not a number: every 400-step episode ends at distance NaN, which the environment reports as -500 -- the whole
    generation ties, and the stable order makes the first arrivals the parents"""
    text = open(M.MAZE_FILE).read().split()
    text[6], text[7] = "nan", "nan"
    maze_file = tmp_path / "nowhere.txt"
    maze_file.write_text(" ".join(text))
    over = dict(maze_file=str(maze_file), episode_cutoff_mode=400)
    (_, _, state), eng = _run(tmp_path / "ties", 2, **over)
    rets = _generation_returns(eng, 10)
    assert len(rets) == 2 and all(np.all(r == -500.0) for r in rets)
    idx0, (of1, idx1) = eng.evals[0][1], next((e[0], e[1]) for e in eng.evals[1:] if len(e[0]) == 10)
    assert np.all(eng.evals[0][0] == -1)
    first = [(int(i), ) for i in idx0[:3]]                                                        # generation 0: the first three roots are the parents
    assert [state.population[j].seeds for j in range(3)] == [first[of1[j]] + ((int(idx1[j]), 0.005), ) for j in range(3)]
    exp = _exp(**over)
    _assert_generation(state, eng, S.plain_loop(S.noise(), _maze_of(exp), exp, SEED, 2)[1], exp)


def test_driver_resume_and_load_population(oracle, tmp_path):
    exp = _exp()
    records = S.plain_loop(S.noise(), _maze_of(exp), exp, SEED, 4)
    (_, _, four), e4 = _run(tmp_path / "straight", 4)
    _assert_generation(four, e4, records[3], exp)
    (_, _, two), e2 = _run(tmp_path / "resumed", 2)
    snap = pickle.load(open(tmp_path / "resumed" / "snapshot.pkl", "rb"))
    assert (snap.game, snap.model, snap.algo, snap.it) == ("maze", "SimpleClassifier", "ga", 2)
    (_, _, again), e22 = _run(tmp_path / "resumed", 2)                                            # a fresh engine: the bank is rebuilt from the genomes
    assert again.it == 4
    _assert_generation(again, e22, records[3], exp)
    assert [c for c in e22.calls if c[0] == "maze_ga_build"] == [("maze_ga_build", 3)] and e22.calls.index(("maze_ga_build", 3)) < e22.calls.index(("maze_ga_eval", 10))
    assert [c for c in e22.calls if c[0] == "maze_ga_promote"] == [("maze_ga_promote", 3)] * 2
    assert all(np.array_equal(M.bits(a), M.bits(b)) for a, b in zip(_generation_returns(e22, 10), _generation_returns(e4, 10)[2:]))
    assert [o.seeds for o in again.population] == [o.seeds for o in four.population] and again.num_frames == four.num_frames
    assert again.validation_timesteps_so_far == four.validation_timesteps_so_far
    # load_population: another run's snapshot as the first parents (ga.py:143-144), elite and counters fresh
    (_, _, loaded), el = _run(tmp_path / "loaded", 1, load_population=str(tmp_path / "resumed" / "snapshot.pkl"))
    assert el.calls.index(("maze_ga_build", 3)) < el.calls.index(("maze_ga_eval", 10)) and loaded.it == 1
    parents = [o.seeds for o in again.population[:3]]
    assert all(o.seeds[:-1] in parents for o in loaded.population)
    pop = [S.Individual(o.seeds, o.fitness, 0) for o in again.population]
    rec = S.plain_loop(S.noise(), _maze_of(exp), exp, SEED, 1, population=pop)[0]
    _assert_generation(loaded, el, rec, exp)


def test_driver_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import es_gpu, ga_gpu, nses_gpu
    with pytest.raises(NotImplementedError, match=r"'SimpleClassifier' on game 'frostbite'"):
        _run(tmp_path / "x", 1, game="frostbite")
    with pytest.raises(NotImplementedError, match=r"'LargeModel' on game 'maze'"):
        _run(tmp_path / "x", 1, model="LargeModel")
    with pytest.raises(NotImplementedError, match=r"'Model' on game 'maze'"):
        ga_gpu.main(str(tmp_path / "x"), engine=S.MazeGaHostEngine(), noise=_noise(), max_iters=1, **{k: v for k, v in _exp().items() if k != "model"})
    with pytest.raises(ValueError, match="KIND_MAZE"):
        _run(tmp_path / "x", 1, eng=OracleEngine(1, max_members=10))
    assert not os.path.exists(tmp_path / "x" / "snapshot.pkl")
    # resumes that do not fit name both sides
    plain = dict(_exp(), population_size=8, return_proc_mode="centered_rank", l2coeff=0.005, optimizer={"args": {"stepsize": 0.01}, "type": "adam"},
                 episode_cutoff_mode="env_default")
    es_gpu.main(str(tmp_path / "es"), engine=M.MazeHostEngine(max_members=8), noise=_noise(), seed=SEED, max_iters=1, **plain)
    with pytest.raises(ValueError, match=r"'es_gpu'.*'ga'"):
        _run(tmp_path / "es", 1)
    import maze_novelty_support as N
    ns = dict(plain, algo_type="ns", return_proc_mode="centered_sign_rank",
              novelty_search={"k": 2, "population_size": 3, "num_rollouts": 1, "selection_method": "round_robin"})
    nses_gpu.main(str(tmp_path / "ns"), engine=N.MazeNoveltyHostEngine(max_members=8), noise=_noise(), seed=SEED, max_iters=1, **ns)
    with pytest.raises(ValueError, match=r"'nses'.*'ga'"):
        _run(tmp_path / "ns", 1)
    os.makedirs(tmp_path / "atari")
    with open(tmp_path / "atari" / "snapshot.pkl", "wb") as f:                                     # what ga_gpu.main writes on an Atari game: no game, no model
        pickle.dump(ga_gpu.TrainingState(_exp()), f)
    with pytest.raises(ValueError, match=r"game 'an Atari game' under model 'Model'; this run is game 'maze' under model 'SimpleClassifier'"):
        _run(tmp_path / "atari", 1)
    _run(tmp_path / "maze", 1)
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'SimpleClassifier'; this run is game 'frostbite' under model 'Model'"):
        ga_gpu.main(str(tmp_path / "maze"), engine=OracleEngine(1, max_members=10), noise=_noise(), max_iters=1,
                    **dict(_exp(), game="frostbite", model="Model"))
