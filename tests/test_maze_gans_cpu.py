"""CPU: GA-NS on the hard maze.  The pool novelty of csrc/maze_novelty.h (dne_maze_novelty_pool_host) against the contract stated in plain
Python (maze_gans_support.py), bit for bit; the contract against a dense numpy formulation within maze_novelty_support.py's derived bound; the
header's host side under sanitizers in a program of its own; dne_hip/ga_gpu.py's GA-NS loop on MazeGaNsHostEngine against the same
algorithm written the long way (maze_gans_support.plain_loop); and the wrong-but-plausible forms these inputs tell from the contract."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import maze_ga_support as G
import maze_gans_support as S
import maze_support as M


# ---- 1. the host twin against the contract, bit for bit ------------------------------------------------------------------------------------------
def test_shapes_are_the_ones_asked_for():
    from dne_hip import _lib
    assert S.ARCHIVES == (0, 1, 2, 63, 64, 65, 1020, 1023, 1024, 1025) and S.COUNTS == (1, 2, 3, 4, 5, 9) and S.KS == (1, 2, 25, 32)
    assert (_lib.MAZE_NOVELTY_KMAX, _lib.MAZE_NOVELTY_TILE) == (S.KMAX, S.TILE)
    assert len(S.shapes()) == len(S.ARCHIVES) * len(S.COUNTS) - 1 and (0, 1) not in S.shapes()
    xy = S.members()
    assert np.array_equal(xy[0], S.archive(1)[0]) and np.array_equal(xy[6], xy[2]) and np.array_equal(xy[7], S.archive(2)[1])


@pytest.mark.parametrize("A", S.ARCHIVES)
def test_host_equals_the_contract_on_every_shape(A):
    from dne_hip import _lib
    archive = S.archive(A)
    for n in S.COUNTS:
        if A + n - 1 < 1:
            continue
        for k in S.KS:
            got, want = _lib.maze_novelty_pool_host(S.members()[:n], archive, k), S.contract(S.members()[:n], archive, k)
            assert got.dtype == np.float64 and got.shape == (n, ) and S.same(got, want), (A, n, k, got, want)
            if A >= 1 and k == 1:
                assert got[0] == 0.0                                              # the member on archive slot 0: that point counts, at distance 0
            if n == 9 and k == 1:
                assert got[2] == 0.0 and got[6] == 0.0                            # two members at one point see each other


@pytest.mark.parametrize("name", sorted(S.edge_cases()))
def test_host_equals_the_contract_on_the_edge_inputs(name):
    from dne_hip import _lib
    xy, archive, ks = S.edge_cases()[name]
    for k in ks:
        for n in sorted(set(min(n, len(xy)) for n in S.COUNTS)):
            if len(archive) + n - 1 < 1:
                continue
            got, want = _lib.maze_novelty_pool_host(xy[:n], archive, k), S.contract(xy[:n], archive, k)
            assert S.same(got, want), (name, k, n, got, want)


def test_edge_inputs_do_what_they_are_for():
    """held on the contract alone: exclusion by index, ties, kk, the NaN order"""
    E = S.edge_cases()
    c = lambda name, k: S.contract(E[name][0], E[name][1], k)
    assert S.same(c("k_above_pool", 32), c("k_above_pool", 4)) and not S.same(c("k_above_pool", 4), c("k_above_pool", 3))
    assert S.same(c("k_above_pool_no_archive", 32), c("k_above_pool_no_archive", 2))
    on = c("member_on_an_archive_point", 1)
    assert on[1] == 0.0 and np.all(on[[0, 2, 3, 4]] > 0)                          # the archive point under member 1 counts, the member itself does not
    tw = c("two_members_at_one_point", 1)
    assert tw[0] == 0.0 and tw[3] == 0.0 and np.all(tw[[1, 2, 4]] > 0)
    assert np.all(c("two_members_at_one_point", 2)[[0, 3]] > 0)                   # ... once: the second neighbour is elsewhere
    for k in (1, 3, 4, 32):
        assert np.array_equal(c("all_members_at_one_point", k), np.zeros(5))
    for chosen, kk in S.neighbours(*E["all_members_on_one_archive_point"][:2], 6):
        assert kk == 6 and [s for s, _ in chosen][:2] == [0, 1] and [s for s, _ in chosen] == sorted(s for s, _ in chosen)   # ties by slot, the archive first
    xy, arch, _ = E["lattice"]
    r2 = np.sqrt(2.0)
    origin = [S.contract(xy, arch, k)[0] for k in (1, 4, 5, 8, 9)]
    assert origin == [1.0, 1.0, (4 + r2) / 5, ((((4 + r2) + r2) + r2) + r2) / 8, (((((4 + r2) + r2) + r2) + r2) + 2) / 9]
    chosen = [s for s, _ in S.neighbours(xy, arch, 8)[0][0]]
    assert sum(s < len(arch) for s in chosen[:4]) == 2 and chosen[:4] == sorted(chosen[:4])       # a four-way tie: two in the archive, two members,
    assert sum(s < len(arch) for s in chosen[4:]) == 2 and chosen[4:] == sorted(chosen[4:])       # the archive's first; likewise the ring at sqrt 2
    nan = {k: c("nan_member", k) for k in (1, 8, 9)}
    assert all(np.isnan(v[2]) for v in nan.values())                              # the NaN member's own novelty
    assert np.all(np.isfinite(np.delete(nan[8], 2))) and np.all(np.isnan(nan[9]))  # the others: eight numbers, then the NaN
    clean = np.delete(E["nan_member"][0], 2, axis=0)
    assert S.same(np.delete(nan[8], 2), S.contract(clean, E["nan_member"][1], 8))  # short of the NaNs the others are unchanged
    assert np.all(np.isfinite(c("nan_archive_entries", 13))) and np.all(np.isnan(c("nan_archive_entries", 14)))
    inf = c("inf", 8)
    assert np.isnan(inf[0]) and np.isnan(inf[1]) and np.isposinf(inf[2])           # inf - inf is a NaN distance and sorts last
    assert np.all(np.isfinite(c("tiny_and_huge", 1)))


def test_host_refusals():
    from dne_hip import _lib
    one = np.zeros((1, 2), np.float32)
    two = np.zeros((2, 2), np.float32)
    for xy, archive, k, text in ((one[:0], one, 1, "n = 0"), (one, one[:0], 1, "the pool is empty"), (one, None, 1, "the pool is empty"),
                                 (two, one, 0, "k = 0"), (two, one, -1, "k = -1")):
        with pytest.raises(_lib.DneError, match="dne_maze_novelty_pool_host: .*" + text):
            _lib.maze_novelty_pool_host(xy, archive, k)
    assert np.array_equal(_lib.maze_novelty_pool_host(two, None, 1000), [0.0, 0.0])                 # any k >= 1, no archive
    assert np.array_equal(_lib.maze_novelty_pool_host(one, one + 3, 5), [np.sqrt(18.0)])


# ---- 2. the contract against a dense numpy formulation, within the derived bound -------------------------------------------------------------------
def test_contract_against_the_dense_formulation_within_the_derived_bound():
    """maze_novelty_support.reference_bound, reused: (2 kk + 6) * 2**-53 relative.  Its derivation holds here term for term -- the dense form's
    distance is sqrt(dx**2 + dy**2) in double with at most the roundings counted there, a masked diagonal removes the same entry the contract
    skips, and numpy's mean over kk sorted values is a sum of kk non-negative terms and one division.
    Measured here: 3267 novelties, worst 4.53 * 2**-53 relative (the bound: 8 at kk = 1, 70 at kk = 32); 822 differ from numpy in the last bits."""
    import maze_novelty_support as N
    worst, differ, total = 0.0, 0, 0
    for xy, archive in S.dense_cases():
        for k in (1, 10, 32):
            got, ref = S.contract(xy, archive, k), S.dense_np(xy, archive, k)
            kk = min(k, len(archive) + len(xy) - 1)
            err = np.abs(got - ref) / np.where(ref == 0, 1.0, ref)
            worst = max(worst, float(err.max())); differ += int(np.sum(got != ref)); total += got.size
            assert np.all(np.abs(got - ref) <= N.reference_bound(kk) * np.abs(ref)), (len(archive), k, err.max() * 2.0 ** 53)
    print("dense comparison: %d novelties, %d differ from numpy, worst %.2f * 2**-53" % (total, differ, worst * 2.0 ** 53))
    assert total == 121 * 3 * 9


# ---- 3. the header's host side under sanitizers, in a program of its own ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/maze_novelty_asan_main.cpp, built once: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(M.ROOT, "tests", "maze_novelty_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("maze_gans_asan") / "maze_gans_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(M.ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def _case_text(xy, archive, k):
    tok = lambda v: "nan" if v != v else float(v).hex()
    return "%d %d %d\n%s\n%s\n" % (len(xy), len(archive), k, " ".join(tok(v) for v in np.asarray(xy).reshape(-1)),
                                   " ".join(tok(v) for v in np.asarray(archive).reshape(-1)))


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program, tmp_path):
    cases = [(xy, archive, k) for _, (xy, archive, ks) in sorted(S.edge_cases().items()) for k in ks]
    cases += [(S.members()[:n], S.archive(A), k) for A in (0, 1, 64, S.TILE + 1) for n in (2, 9) for k in (1, 25, 32)]
    cases.append((S.members()[:1], S.archive(1), 1))                                             # the smallest pool there is
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case_text(*c) for c in cases))
    out = subprocess.run([sanitizer_program, "pool", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % len(cases) and len(lines) == len(cases) + 1
    for line, (xy, archive, k) in zip(lines, cases):
        got = np.array([float("nan") if t == "nan" else float.fromhex(t) for t in line.split()])
        assert S.same(got, S.contract(xy, archive, k)), (k, archive.shape)


# ---- 4. the driver on the host engine ----------------------------------------------------------------------------------------------------------------
SEED, N_POP = 4, 10


def _exp(ns=None, **over):
    exp = {"game": "maze", "model": "SimpleClassifier", "population_size": N_POP, "selection_threshold": 3, "validation_threshold": 2,
           "num_validation_episodes": 2, "num_test_episodes": 2, "episode_cutoff_mode": 400, "mutation_power": 0.005, "timesteps": 10 ** 9,
           "maze_file": M.MAZE_FILE, "novelty_search": {"k": 3, "archive_prob": 0.3}}
    exp.update(over)
    exp["novelty_search"] = dict(exp["novelty_search"], **(ns or {}))
    return exp


CONFIGS = {
    "prob_0": dict(ns={"archive_prob": 0.0}),
    "prob_1": dict(ns={"archive_prob": 1.0}),
    "prob_0.3": dict(),
    "no_parents": dict(selection_threshold=0),
    "wide_selection_short_episodes": dict(selection_threshold=4, validation_threshold=3, episode_cutoff_mode=40, ns={"k": 25}),
}


def _noise():
    from dne_hip import es
    noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    noise.noise = G.noise()
    noise._engines = []
    return noise


def _run(log_dir, iters, eng=None, ns=None, **over):
    from dne_hip import ga_gpu
    eng = eng or S.MazeGaNsHostEngine(max_members=N_POP)
    return ga_gpu.main(str(log_dir), engine=eng, noise=_noise(), seed=SEED, max_iters=iters, **_exp(ns=ns, **over)), eng


def _maze_of(exp):
    from dne_hip import _lib
    return _lib.load_maze(exp["maze_file"])


def _assert_generation(state, eng, rec, exp):
    """the driver after g generations against record g of the plain loop"""
    T, V = exp["selection_threshold"], exp["validation_threshold"]
    assert [o.seeds for o in state.population[:T]] == rec["parents"] and eng.maze_ga_parents() == len(rec["parents"])
    for j, th in enumerate(rec["thetas"]):
        assert np.array_equal(M.bits(eng.maze_ga_get_parent(j)), M.bits(th)), j                   # the promoted bank = every parent from its whole genome
    assert np.array_equal(M.bits(state.archive), M.bits(rec["archive"])) and np.array_equal(M.bits(eng.maze_archive()), M.bits(rec["archive"]))
    assert S.same(eng.novelties[-1], rec["raw"])
    assert state.elite.seeds == rec["elite"] and state.curr_solution == rec["curr_solution"] and state.timesteps_so_far == rec["timesteps_so_far"]
    assert (state.curr_solution_val, state.curr_solution_test) == (rec["curr_solution_val"], rec["curr_solution_test"])
    union = list(rec["by_novelty"][:T]) + [i for i in rec["by_reward"][:V] if i not in rec["by_novelty"][:T]]
    assert len(state.population) == len(union)                                                     # lazy: genomes for the top T by novelty and the top V by reward
    assert [o.novelty for o in state.population] == [float(rec["novelty"][i]) for i in union]
    assert [o.seeds for o in state.population] == [rec["tasks"][i] for i in union]


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_driver_equals_the_plain_loop_generation_by_generation(oracle, tmp_path, config):
    exp = _exp(**CONFIGS[config])
    records = S.plain_loop(G.noise(), _maze_of(exp), exp, SEED, 3)
    T, prob = exp["selection_threshold"], exp["novelty_search"]["archive_prob"]
    for g in (1, 2, 3):
        (test, val, state), eng = _run(tmp_path / ("g%d" % g), g, **CONFIGS[config])
        assert state.it == g and (test, val["val"]) == (state.curr_solution_test, state.curr_solution_val)
        _assert_generation(state, eng, records[g - 1], exp)
        assert len(eng.novelties) == g and all(S.same(a, r["raw"]) for a, r in zip(eng.novelties, records))
        rets = [e[2] for e in eng.evals if len(e[2]) == N_POP]
        assert len(rets) == g and all(np.array_equal(M.bits(a), M.bits(r["returns"])) for a, r in zip(rets, records))
        builds = [c for c in eng.calls if c[0] == "maze_ga_build"]
        promotes = [c for c in eng.calls if c[0] == "maze_ga_promote"]
        assert builds == ([("maze_ga_build", T)] if T else []) and promotes == [("maze_ga_promote", T)] * (g - 1 if T else 0)
        assert [c for c in eng.calls if c[0] == "maze_novelty_pool"] == [("maze_novelty_pool", exp["novelty_search"]["k"])] * g
        assert not any(c[0] in ("maze_final_state", "maze_novelty") for c in eng.calls)            # the points stay where the rollout left them
    assert (state.algo, state.k, state.archive_prob) == ("ga_ns", exp["novelty_search"]["k"], prob)
    sizes = [len(r["archive"]) for r in records]
    if prob == 0.0:
        assert sizes == [0, 0, 0] and not any(c[0] == "maze_archive_append_members" for c in eng.calls)   # the pool is the population alone
    elif prob == 1.0:
        assert sizes == [N_POP, 2 * N_POP, 3 * N_POP] and np.array_equal(M.bits(records[0]["archive"]), M.bits(records[0]["xy"]))   # arrival order
    else:
        assert 0 < sizes[0] <= sizes[1] <= sizes[2] < 3 * N_POP and sizes[0] < sizes[2]     # (one generation of this seed archives nobody)
    if config == "no_parents":                                                                     # random search, with an archive that still fills
        assert all(len(o.seeds) == 1 for o in state.population) and eng.maze_ga_parents() == 0 and sizes[2] > 0
    if T:
        by_reward = [list(r["by_reward"][:T]) for r in records]
        assert any(list(r["by_novelty"][:T]) != b for r, b in zip(records, by_reward))            # novelty selects others than the reward would


def _boxed_in(tmp_path):
    """a maze with four more walls inside the navigator's radius around its start: it collides at every step and never moves"""
    tok = open(M.MAZE_FILE).read().split()
    sx, sy = float(tok[3]), float(tok[4])
    box = [(sx - 5, sy - 5, sx + 5, sy - 5), (sx + 5, sy - 5, sx + 5, sy + 5), (sx + 5, sy + 5, sx - 5, sy + 5), (sx - 5, sy + 5, sx - 5, sy - 5)]
    tok[2] = str(int(tok[2]) + 4)
    path = tmp_path / "boxed_in.txt"
    path.write_text(" ".join(tok + ["%g" % v for wall in box for v in wall]))
    return str(path)


def test_driver_all_at_one_point_follows_arrival_order(oracle, tmp_path):
    over = dict(maze_file=_boxed_in(tmp_path), ns={"archive_prob": 1.0})
    (_, _, state), eng = _run(tmp_path / "boxed", 2, **over)
    assert len(eng.novelties) == 2 and all(np.array_equal(v, np.zeros(N_POP)) for v in eng.novelties)
    assert len(np.unique(eng.maze_archive(), axis=0)) == 1 and eng.maze_archive_size() == 2 * N_POP
    idx0, (of1, idx1) = eng.evals[0][1], next((e[0], e[1]) for e in eng.evals[1:] if len(e[0]) == N_POP)
    first = [(int(i), ) for i in idx0[:3]]                                                        # generation 0: the first three roots are the parents
    assert [o.seeds for o in state.population[:3]] == [first[of1[j]] + ((int(idx1[j]), 0.005), ) for j in range(3)]
    exp = _exp(**over)
    _assert_generation(state, eng, S.plain_loop(G.noise(), _maze_of(exp), exp, SEED, 2)[1], exp)


def test_driver_never_selects_a_nan_policy(oracle, tmp_path):
    """member 0 of generation 1 runs a policy of NaNs: its final position, and so its novelty, is NaN; it counts as 0.0 and is not among the parents"""
    nan_theta = np.full(S.P, np.nan, np.float32)

    class Poisoned(S.MazeGaNsHostEngine):
        full = 0

        def _run(self, thetas, tslimit):
            if len(thetas) == N_POP:
                self.full += 1
                if self.full == 2:
                    thetas = [nan_theta] + list(thetas[1:])
            return super()._run(thetas, tslimit)

    over = dict(ns={"archive_prob": 0.0, "k": 9})                                                  # kk = 9 reaches the NaN in everybody's pool
    (_, _, state), eng = _run(tmp_path / "nan", 2, eng=Poisoned(max_members=N_POP), **over)
    assert np.all(np.isnan(eng.novelties[1])) and np.all(np.isfinite(eng.novelties[0]))
    exp = _exp(**over)
    rec = S.plain_loop(G.noise(), _maze_of(exp), exp, SEED, 2, poison=(1, 0, nan_theta))[1]
    assert np.array_equal(rec["novelty"], np.zeros(N_POP)) and list(rec["by_novelty"][:3]) == [0, 1, 2]   # all 0.0: arrival order (a tie, not a preference)
    over = dict(ns={"archive_prob": 0.0, "k": 3})                                                  # kk = 3 stays short of it: only the NaN member is 0.0
    (_, _, state), eng = _run(tmp_path / "nan3", 2, eng=Poisoned(max_members=N_POP), **over)
    exp = _exp(**over)
    rec = S.plain_loop(G.noise(), _maze_of(exp), exp, SEED, 2, poison=(1, 0, nan_theta))[1]
    assert np.isnan(eng.novelties[1][0]) and np.all(np.isfinite(eng.novelties[1][1:])) and np.all(eng.novelties[1][1:] > 0)
    assert 0 not in rec["by_novelty"][:3] and rec["by_novelty"][-1] == 0
    assert S.same(eng.novelties[1], rec["raw"]) and [o.seeds for o in state.population[:3]] == rec["parents"]
    assert all(o.novelty > 0 for o in state.population[:3])


def test_driver_resume_equals_a_straight_run(oracle, tmp_path):
    exp = _exp()
    records = S.plain_loop(G.noise(), _maze_of(exp), exp, SEED, 4)
    (_, _, four), e4 = _run(tmp_path / "straight", 4)
    _assert_generation(four, e4, records[3], exp)
    assert [c for c in e4.calls if c[0] == "maze_ga_build"] == [("maze_ga_build", 3)]             # once per call: after generation 0
    (_, _, two), e2 = _run(tmp_path / "resumed", 2)
    snap = pickle.load(open(tmp_path / "resumed" / "snapshot.pkl", "rb"))
    assert (snap.game, snap.model, snap.algo, snap.it, snap.k, snap.archive_prob) == ("maze", "SimpleClassifier", "ga_ns", 2, 3, 0.3)
    assert np.array_equal(M.bits(snap.archive), M.bits(records[1]["archive"])) and snap.stream is not None
    (_, _, again), e22 = _run(tmp_path / "resumed", 2)                                            # a fresh engine: bank and archive come from the snapshot
    assert again.it == 4
    _assert_generation(again, e22, records[3], exp)
    assert [c for c in e22.calls if c[0] == "maze_ga_build"] == [("maze_ga_build", 3)] and e22.calls.index(("maze_ga_build", 3)) < e22.calls.index(("maze_ga_eval", N_POP))
    assert [c for c in e22.calls if c[0] == "maze_ga_promote"] == [("maze_ga_promote", 3)] * 2
    assert all(S.same(a, b) for a, b in zip(e22.novelties, e4.novelties[2:])) and len(e22.novelties) == 2
    assert [o.seeds for o in again.population] == [o.seeds for o in four.population] and again.num_frames == four.num_frames
    assert again.validation_timesteps_so_far == four.validation_timesteps_so_far
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(again.stream, four.stream))   # down to the stream's position


def test_run_without_the_key_is_maze_main_as_it_is(oracle, tmp_path):
    """the same engine class, no novelty_search key: maze_ga_support.plain_loop's run (the Deep GA), no scoring, no archive, and the stream
    where two whole-array draws per generation leave it"""
    from dne_hip import ga_gpu
    exp = {k: v for k, v in _exp().items() if k != "novelty_search"}
    eng = S.MazeGaNsHostEngine(max_members=N_POP)
    _, _, state = ga_gpu.main(str(tmp_path / "ga"), engine=eng, noise=_noise(), seed=SEED, max_iters=3, **exp)
    rec = G.plain_loop(G.noise(), _maze_of(exp), exp, SEED, 3)[2]
    assert state.algo == "ga" and ga_gpu.parents_of(state, 3) == rec["parents"] and [o.seeds for o in state.population] == rec["top"]
    assert state.elite.seeds == rec["elite"] and state.timesteps_so_far == rec["timesteps_so_far"] and state.curr_solution == rec["curr_solution"]
    assert not any(c[0] in ("maze_novelty_pool", "maze_archive_append_members") for c in eng.calls) and eng.maze_archive_size() == 0
    assert not hasattr(state, "archive") and not hasattr(state, "k")
    rs = np.random.RandomState(SEED)
    rs.randint(0, G.noise().size - S.P + 1, size=N_POP)
    for _ in range(2):
        rs.randint(3, size=N_POP); rs.randint(0, G.noise().size - S.P + 1, size=N_POP)
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(state.stream, rs.get_state()))


def test_driver_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import es_gpu, ga_gpu, nses_gpu
    import maze_novelty_support as N
    atari = dict(_exp(), game="frostbite", model="Model")
    with pytest.raises(NotImplementedError, match=r"'frostbite'.*'novelty_search'"):
        ga_gpu.main(str(tmp_path / "x"), engine=OracleEngine(1, max_members=N_POP), noise=_noise(), max_iters=1, **atari)
    with pytest.raises(ValueError, match="KIND_MAZE"):
        _run(tmp_path / "x", 1, eng=OracleEngine(1, max_members=N_POP))
    with pytest.raises(ValueError, match=r"k = 33.*MAZE_NOVELTY_KMAX = 32"):
        _run(tmp_path / "x", 1, ns={"k": 33})
    with pytest.raises(ValueError, match=r"k = 0"):
        _run(tmp_path / "x", 1, ns={"k": 0})
    with pytest.raises(ValueError, match=r"archive_prob = 1.5"):
        _run(tmp_path / "x", 1, ns={"archive_prob": 1.5})
    assert not os.path.exists(tmp_path / "x" / "snapshot.pkl")
    # resumes that do not fit name both sides
    plain = {k: v for k, v in _exp().items() if k != "novelty_search"}
    ga_gpu.main(str(tmp_path / "ga"), engine=S.MazeGaNsHostEngine(max_members=N_POP), noise=_noise(), seed=SEED, max_iters=1, **plain)
    with pytest.raises(ValueError, match=r"'ga'.*'ga_ns'"):
        _run(tmp_path / "ga", 1)
    _run(tmp_path / "gans", 1)
    with pytest.raises(ValueError, match=r"'ga_ns'.*'ga'"):
        ga_gpu.main(str(tmp_path / "gans"), engine=S.MazeGaNsHostEngine(max_members=N_POP), noise=_noise(), seed=SEED, max_iters=1, **plain)
    with pytest.raises(ValueError, match=r"holds k 3, archive_prob 0.3; this run is k 5, archive_prob 0.3"):
        _run(tmp_path / "gans", 1, ns={"k": 5})
    with pytest.raises(ValueError, match=r"holds k 3, archive_prob 0.3; this run is k 3, archive_prob 0.5"):
        _run(tmp_path / "gans", 1, ns={"archive_prob": 0.5})
    es_exp = dict(plain, population_size=8, return_proc_mode="centered_rank", l2coeff=0.005, optimizer={"args": {"stepsize": 0.01}, "type": "adam"},
                  episode_cutoff_mode="env_default")
    es_gpu.main(str(tmp_path / "es"), engine=M.MazeHostEngine(max_members=8), noise=_noise(), seed=SEED, max_iters=1, **es_exp)
    with pytest.raises(ValueError, match=r"'es_gpu'.*'ga_ns'"):
        _run(tmp_path / "es", 1)
    ns = dict(es_exp, algo_type="ns", return_proc_mode="centered_sign_rank",
              novelty_search={"k": 2, "population_size": 3, "num_rollouts": 1, "selection_method": "round_robin"})
    nses_gpu.main(str(tmp_path / "ns"), engine=N.MazeNoveltyHostEngine(max_members=8), noise=_noise(), seed=SEED, max_iters=1, **ns)
    with pytest.raises(ValueError, match=r"'nses'.*'ga_ns'"):
        _run(tmp_path / "ns", 1)
    os.makedirs(tmp_path / "atari")
    with open(tmp_path / "atari" / "snapshot.pkl", "wb") as f:                                     # what ga_gpu.main writes on an Atari game
        pickle.dump(ga_gpu.TrainingState(_exp()), f)
    with pytest.raises(ValueError, match=r"'ga'.*'ga_ns'"):
        _run(tmp_path / "atari", 1)


# ---- 5. the wrong-but-plausible forms ------------------------------------------------------------------------------------------------------------------
def _all_inputs():
    for A, n in S.shapes():
        for k in S.KS:
            yield ("shape", A, n), S.members()[:n], S.archive(A), k
    for name, (xy, archive, ks) in sorted(S.edge_cases().items()):
        for k in ks:
            yield name, xy, archive, k


@pytest.mark.parametrize("form", sorted(S.WRONG_FORMS))
def test_inputs_tell_the_wrong_forms_from_the_contract(form):
    """Each wrong form gives another novelty than the contract on inputs the tests above (and the GPU file) run -- so a host twin or a kernel
    of that form fails them.  One form cannot show in any novelty: which of two EQUAL distances comes first changes neither the kk values that
    are added nor their order, so "the population before the archive in ties" is told apart where it can be, in the neighbours the contract
    names (their combined slots), and its novelties are checked to be the contract's."""
    from dne_hip import _lib
    wrong = S.WRONG_FORMS[form]
    caught = []
    for name, xy, archive, k in _all_inputs():
        want, other = S.contract(xy, archive, k), S.contract(xy, archive, k, **wrong)
        if form == "population_before_archive_in_ties":
            assert S.same(want, other), name
            slots = lambda **kw: [[s for s, _ in chosen] for chosen, _ in S.neighbours(xy, archive, k, **kw)]
            if slots() != slots(**wrong):
                caught.append((name, k))
        elif not S.same(want, other):
            assert S.same(_lib.maze_novelty_pool_host(xy, archive, k), want)                       # the library is on the contract's side
            caught.append((name, k))
    names = {c[0] for c in caught}
    print("%s: told apart on %d inputs" % (form, len(caught)))
    assert len(names) >= 3, names
    need = {"self_not_excluded": "k_above_pool_no_archive", "self_excluded_by_value": "two_members_at_one_point_no_archive",
            "everything_at_distance_zero_excluded": "member_on_an_archive_point", "population_before_archive_in_ties": "lattice",
            "kk_counts_self": "k_above_pool"}[form]
    assert need in names, (need, names)
