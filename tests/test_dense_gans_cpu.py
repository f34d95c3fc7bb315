"""CPU: GA-NS on the dense kind.  The pool novelty of csrc/dense_novelty.h (dne_dense_novelty_pool_host) against the
contract restated in plain Python / numpy (dense_gans_support.py) on the grid, the lattice, random and edge sets, and for D = 2 against
dne_maze_novelty_pool_host; the wrong-but-plausible forms these inputs tell from the contract; the host refusals by text; the header's host
side under sanitizers in a program of its own; ga_gpu.dense_ns_main on DenseGaNsHostEngine against the same algorithm written the long way
(dense_gans_support.plain_loop) and, at (16, 16) on the maze, against ga_gpu.maze_ns_main; the resumes it refuses.  Bit for bit throughout."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import dense_ga_support as G
import dense_gans_support as S
import dense_novelty_support as N
import maze_gans_support as MS
import maze_support as M


# ---- 1. the host twin against the restatement, bit for bit ----------------------------------------------------------------------------------------
def test_shapes_are_the_ones_asked_for():
    from dne_hip import _lib
    assert S.DIMS == (2, 4) and S.ARCHIVES == (0, 1, 2, 63, 64, 65, 1020, 1023, 1024, 1025) and S.COUNTS == (1, 2, 3, 4, 5, 9) and S.KS == (1, 2, 25, 32)
    assert (_lib.DENSE_NOVELTY_KMAX, _lib.MAZE_NOVELTY_TILE) == (S.KMAX, S.TILE)
    assert len(S.shapes()) == len(S.ARCHIVES) * len(S.COUNTS) - 1 and (0, 1) not in S.shapes()
    for dim in S.DIMS:
        mem, arch = S.point_set("lattice", dim)
        assert np.all(np.abs(mem) <= 3) and np.all(np.abs(arch) <= 3) and np.all(mem == np.round(mem)) and np.all(arch == np.round(arch))
        assert not (arch == 0).all(1).any() and np.array_equal(mem[6], mem[4]) and np.array_equal(mem[7], arch[1])
        mem, arch = S.point_set("random", dim)
        assert np.array_equal(mem[0], arch[0]) and np.array_equal(mem[6], mem[2]) and np.array_equal(mem[7], arch[1])


@pytest.mark.parametrize("dim", S.DIMS)
@pytest.mark.parametrize("name", S.SETS)
def test_host_equals_the_restatement_on_every_shape(name, dim):
    from dne_hip import _lib
    for A, n in S.shapes():
        bc, archive = S.cell(name, dim, A, n)
        for k in S.KS:
            got, want = _lib.dense_novelty_pool_host(bc, archive, k), S.contract_cell(name, dim, A, n, k)
            assert got.dtype == np.float64 and got.shape == (n, ) and S.same(got, want), (name, dim, A, n, k, got, want)
            if name == "random" and A >= 1 and k == 1:
                assert got[0] == 0.0                                              # the member on archive slot 0: that point counts, at distance 0
            if name == "random" and n == 9 and k == 1:
                assert got[2] == 0.0 and got[6] == 0.0                            # two members at one BC see each other


@pytest.mark.parametrize("dim", S.DIMS)
def test_lattice_has_ties_across_the_cut_in_archive_and_population(dim):
    """on the restatement alone: in every (D, A >= 63, n = 9) cell some member has equal distances on both sides of position kk, and the points
    at that distance are in the archive and in the population -- which of them is named depends on the combined slots' order"""
    for A in S.ARCHIVES:
        if A >= 63:
            assert S.tie_across_the_cut("lattice", dim, A, 9), (dim, A)
    origin = S.ordered_cell("lattice", dim, 63, 9)[0]
    ring = [c for c, d in origin if d == 1.0]
    assert origin[0] == (0, 1.0) and ring == sorted(ring) and {0, 64, 65, 66} <= set(ring)        # by combined slot: the archive's first, then members 1, 2, 3


@pytest.mark.parametrize("dim", S.DIMS)
def test_host_equals_the_restatement_on_the_edge_inputs(dim):
    from dne_hip import _lib
    for name, (bc, archive, ks) in sorted(S.edge_cases(dim).items()):
        for k in ks:
            for n in sorted(set(min(n, len(bc)) for n in S.COUNTS)):
                if len(archive) + n - 1 < 1:
                    continue
                got, want = _lib.dense_novelty_pool_host(bc[:n], archive, k), S.contract(bc[:n], archive, k)
                assert S.same(got, want), (name, dim, k, n, got, want)


@pytest.mark.parametrize("dim", S.DIMS)
def test_edge_inputs_do_what_they_are_for(dim):
    """held on the restatement alone: exclusion by index, ties, kk, the NaN order"""
    E = S.edge_cases(dim)
    c = lambda name, k: S.contract(E[name][0], E[name][1], k)
    assert S.same(c("k_above_pool", 32), c("k_above_pool", 4)) and not S.same(c("k_above_pool", 4), c("k_above_pool", 3))
    assert S.same(c("k_above_pool_no_archive", 32), c("k_above_pool_no_archive", 2))
    on = c("member_on_an_archive_point", 1)
    assert on[1] == 0.0 and np.all(on[[0, 2, 3, 4]] > 0)                          # the archive point under member 1 counts, the member itself does not
    tw = c("two_members_at_one_bc", 1)
    assert tw[0] == 0.0 and tw[3] == 0.0 and np.all(tw[[1, 2, 4]] > 0)
    assert np.all(c("two_members_at_one_bc", 2)[[0, 3]] > 0)                       # ... once: the second neighbour is elsewhere
    for k in (1, 3, 4, 32):
        assert np.array_equal(c("all_members_at_one_bc", k), np.zeros(5))
    for chosen, kk in S.neighbours(*E["all_members_on_one_archive_point"][:2], 6):
        assert kk == 6 and [s for s, _ in chosen][:2] == [0, 1] and [s for s, _ in chosen] == sorted(s for s, _ in chosen)   # ties by slot, the archive first
    assert np.array_equal(c("signed_zeros", 4), np.zeros(4)) and np.all(c("signed_zeros", 5) > 0)   # +0.0 and -0.0 are one point: 3 members and 1 archive point at 0
    nan = {k: c("nan_member", k) for k in (1, 8, 9)}
    assert all(np.isnan(v[2]) for v in nan.values())                              # the NaN member's own novelty
    assert np.all(np.isfinite(np.delete(nan[8], 2))) and np.all(np.isnan(nan[9]))  # the others: short of kk eight numbers, within kk the NaN
    clean = np.delete(E["nan_member"][0], 2, axis=0)
    assert S.same(np.delete(nan[8], 2), S.contract(clean, E["nan_member"][1], 8))  # short of the NaN the others are unchanged
    assert np.all(np.isfinite(c("nan_archive_points", 13))) and np.all(np.isnan(c("nan_archive_points", 14)))
    inf = c("inf", 8)
    assert np.isnan(inf[0]) and np.isnan(inf[1]) and np.isposinf(inf[2])           # inf - inf is a NaN distance and sorts last
    th = c("tiny_and_huge", 1)
    assert np.all(np.isfinite(th)) and 0.0 < th[1] < 1e-39 and th[2] == 0.0       # a float32 subnormal apart; 1e30 sits on an archive point


@pytest.mark.parametrize("name", S.SETS)
def test_two_floats_a_point_is_the_maze_pool_twin(name):
    from dne_hip import _lib
    for A, n in S.shapes():
        bc, archive = S.cell(name, 2, A, n)
        for k in S.KS:
            assert S.same(_lib.dense_novelty_pool_host(bc, archive, k), _lib.maze_novelty_pool_host(bc, archive, k)), (name, A, n, k)
    for case, (bc, archive, ks) in sorted(S.edge_cases(2).items()):
        for k in ks:
            assert S.same(_lib.dense_novelty_pool_host(bc, archive, k), _lib.maze_novelty_pool_host(bc, archive, k)), (case, k)
    for case, (xy, archive, ks) in sorted(MS.edge_cases().items()):               # and on the maze's own edge inputs
        for k in ks:
            assert S.same(_lib.dense_novelty_pool_host(xy, archive, k, D=2), _lib.maze_novelty_pool_host(xy, archive, k)), (case, k)


def test_archive_form_is_unchanged():
    """dne_dense_novelty_host still gives 17b's restatement (the pool form stands beside it)"""
    from dne_hip import _lib
    for dim in S.DIMS:
        mem, arch = N.point_set("edge_few_nan", dim, 65)
        for k in (1, 25, 40):
            assert S.same(_lib.dense_novelty_host(mem, arch, k), N.contract(mem, arch, k))


# ---- 2. the wrong-but-plausible forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.DIMS)
@pytest.mark.parametrize("form", sorted(S.WRONG_FORMS))
def test_inputs_tell_the_wrong_forms_from_the_contract(form, dim):
    """Each wrong form gives another novelty than the contract on inputs the tests above (and the GPU file) run, so a twin or a kernel of
    that form fails them.  One form cannot show in any novelty: which of two EQUAL distances comes first changes neither the kk values that are
    added nor their order, so "the population before the archive in ties" is told apart where it can be, in the neighbours the contract names
    (their combined slots), and its novelties are checked to be the contract's."""
    from dne_hip import _lib
    wrong = S.WRONG_FORMS[form]
    inputs = [(name, bc, archive, k) for name, bc, archive, k in S.all_inputs(dim, archives=(0, 1, 2, 63, 65)) if not (isinstance(name, tuple) and name[0] == "random" and name[1] > 2)]
    caught = []
    for name, bc, archive, k in inputs:
        want, other = S.contract(bc, archive, k), S.contract(bc, archive, k, **wrong)
        if form == "population_before_archive_in_ties":
            assert S.same(want, other), name
            slots = lambda **kw: [[s for s, _ in chosen] for chosen, _ in S.neighbours(bc, archive, k, **kw)]
            if slots() != slots(**wrong):
                caught.append((name, k))
        elif not S.same(want, other):
            assert S.same(_lib.dense_novelty_pool_host(bc, archive, k), want)                       # the library is on the contract's side
            caught.append((name, k))
    names = {c[0] if isinstance(c[0], str) else c[0][0] for c in caught}
    print("%s, D = %d: told apart on %d inputs" % (form, dim, len(caught)))
    need = {"self_not_excluded": "k_above_pool_no_archive", "self_excluded_by_value": "two_members_at_one_bc_no_archive",
            "population_before_archive_in_ties": "lattice", "kk_counts_self": "k_above_pool"}[form]
    assert need in names and len(names) >= 3, (need, names)


# ---- 3. the host refusals, by text -----------------------------------------------------------------------------------------------------------------------
def test_host_refusals():
    from dne_hip import _lib
    import ctypes as C
    for dim in S.DIMS:
        one, two = np.zeros((1, dim), np.float32), np.zeros((2, dim), np.float32)
        for bc, archive, k, text in ((one[:0], one, 1, "n = 0, at least one point is needed"), (one, one[:0], 1, "the pool is empty \\(one member, no archive point\\)"),
                                     (one, None, 1, "the pool is empty"), (two, one, 0, "k = 0, at least one neighbour is needed"), (two, one, -1, "k = -1")):
            with pytest.raises(_lib.DneError, match="dne_dense_novelty_pool_host: " + text):
                _lib.dense_novelty_pool_host(bc, archive, k, D=dim)
        assert np.array_equal(_lib.dense_novelty_pool_host(two, None, 1000), [0.0, 0.0])            # any k >= 1, no archive
        assert np.array_equal(_lib.dense_novelty_pool_host(one, one + 3, 5), [np.sqrt(9.0 * dim)])
    for dim in (0, 1, 3, 5):
        with pytest.raises(_lib.DneError, match="dne_dense_novelty_pool_host: D = %d, a behaviour characterisation has 2 or 4 values" % dim):
            _lib.dense_novelty_pool_host(np.zeros((2, max(dim, 1)), np.float32), None, 1, D=dim)
    lib, f, d = _lib.load(), C.POINTER(C.c_float), C.POINTER(C.c_double)
    pts, out = np.zeros((2, 2), np.float32), np.zeros(2, np.float64)
    p, o = pts.ctypes.data_as(f), out.ctypes.data_as(d)
    for args in ((None, 2, p, 2, 2, 1, o), (p, 2, None, 2, 2, 1, o), (p, 2, p, 2, 2, 1, None)):     # members, an archive that narch says exists, results
        assert lib.dne_dense_novelty_pool_host(*args) == -1
        assert lib.dne_last_error(None).decode() == "dne_dense_novelty_pool_host: a buffer is missing"
    assert lib.dne_dense_novelty_pool_host(p, 2, p, -1, 2, 1, o) == -1 and lib.dne_last_error(None).decode() == "dne_dense_novelty_pool_host: narch = -1"
    assert lib.dne_dense_novelty_pool_host(p, 2, None, 0, 2, 1, o) == 0                             # no archive buffer at all at narch 0


# ---- 4. the header's host side under sanitizers, in a program of its own ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/dense_gans_asan_main.cpp, built once: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(M.ROOT, "tests", "dense_gans_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("dense_gans_asan") / "dense_gans_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(M.ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def _case_text(bc, archive, k):
    tok = lambda v: "nan" if v != v else float(v).hex()
    return "%d %d %d %d\n%s\n%s\n" % (bc.shape[1], len(bc), len(archive), k, " ".join(tok(v) for v in np.asarray(bc).reshape(-1)),
                                      " ".join(tok(v) for v in np.asarray(archive).reshape(-1)))


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program, tmp_path):
    cases = []
    for dim in S.DIMS:
        cases += [(bc, archive, k) for _, (bc, archive, ks) in sorted(S.edge_cases(dim).items()) for k in ks]
        cases += [S.cell(name, dim, A, n) + (k, ) for name in S.SETS for A in (0, 1, 64, S.TILE + 1) for n in (2, 9) for k in (1, 25, 32)]
        cases.append(S.cell("random", dim, 1, 1) + (1, ))                                          # the smallest pool there is
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case_text(*c) for c in cases))
    out = subprocess.run([sanitizer_program, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % len(cases) and len(lines) == len(cases) + 1
    for line, (bc, archive, k) in zip(lines, cases):
        got = np.array([float("nan") if t == "nan" else float.fromhex(t) for t in line.split()])
        assert S.same(got, S.contract(bc, archive, k)), (k, bc.shape, archive.shape)


# ---- 5. the driver on the host engine ------------------------------------------------------------------------------------------------------------------
SEED, N_POP = 4, 10
CASES = {"maze-linear": ("maze", (), "relu"), "cartpole-linear": ("cartpole", (), "relu"), "cartpole-5-33": ("cartpole", (5, 33), "relu")}
GAME = {"maze": "maze", "cartpole": "gym.CartPole-v1"}
CONFIGS = {
    "prob_0": dict(ns={"archive_prob": 0.0}),
    "prob_1": dict(ns={"archive_prob": 1.0}),
    "prob_0.3": dict(),
    "no_parents": dict(selection_threshold=0),
}


def _exp(case, ns=None, **over):
    over.setdefault("model", None if case[1] else "LinearClassifier")
    return S.exp(GAME[case[0]], ns=ns, **over)


def _run(log_dir, iters, case, eng=None, ns=None, **over):
    from dne_hip import ga_gpu
    eng = eng or S.host_engine(case, N_POP)
    return ga_gpu.dense_ns_main(str(log_dir), engine=eng, noise=S.shared_noise(), seed=SEED, max_iters=iters, **_exp(case, ns=ns, **over)), eng


def _assert_generation(state, eng, rec, exp):
    """the driver after g generations against record g of the plain loop"""
    T, V = exp["selection_threshold"], exp["validation_threshold"]
    assert [o.seeds for o in state.population[:T]] == rec["parents"] and eng.dense_ga_parents() == len(rec["parents"])
    for j, th in enumerate(rec["thetas"]):
        assert np.array_equal(M.bits(eng.dense_ga_get_parent(j)), M.bits(th)), j                   # the promoted bank = every parent from its whole genome
    assert state.archive.shape == rec["archive"].shape and np.array_equal(S.bits(state.archive), S.bits(rec["archive"]))   # contents and order
    assert np.array_equal(S.bits(eng.dense_archive()), S.bits(rec["archive"]))
    assert S.same(eng.novelties[-1], rec["raw"])
    assert state.elite.seeds == rec["elite"] and state.curr_solution == rec["curr_solution"] and state.timesteps_so_far == rec["timesteps_so_far"]
    assert (state.curr_solution_val, state.curr_solution_test) == (rec["curr_solution_val"], rec["curr_solution_test"])
    union = list(rec["by_novelty"][:T]) + [i for i in rec["by_reward"][:V] if i not in rec["by_novelty"][:T]]
    assert len(state.population) == len(union)                                                     # lazy: genomes for the top T by novelty and the top V by reward
    assert [o.novelty for o in state.population] == [float(rec["novelty"][i]) for i in union]
    assert [o.seeds for o in state.population] == [rec["tasks"][i] for i in union]
    assert S.same_stream(state.stream, rec["stream"])                                              # the stream's position


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_driver_equals_the_plain_loop_generation_by_generation(oracle, tmp_path, name, config):
    case = CASES[name]
    exp = _exp(case, **CONFIGS[config])
    records = S.plain_loop(case, exp, SEED, 3)
    T, prob, k = exp["selection_threshold"], exp["novelty_search"]["archive_prob"], exp["novelty_search"]["k"]
    for g in (1, 2, 3):
        (test, val, state), eng = _run(tmp_path / ("g%d" % g), g, case, **CONFIGS[config])
        assert state.it == g and (test, val["val"]) == (state.curr_solution_test, state.curr_solution_val)
        _assert_generation(state, eng, records[g - 1], exp)
        assert len(eng.novelties) == g and all(S.same(a, r["raw"]) for a, r in zip(eng.novelties, records))
        rets = [e[2] for e in eng.evals if len(e[2]) == N_POP]
        assert len(rets) == g and all(np.array_equal(M.bits(a), M.bits(r["returns"])) for a, r in zip(rets, records))
        builds = [c for c in eng.calls if c[0] == "dense_ga_build"]
        promotes = [c for c in eng.calls if c[0] == "dense_ga_promote"]
        assert builds == ([("dense_ga_build", T)] if T else []) and promotes == [("dense_ga_promote", T)] * (g - 1 if T else 0)   # one build per call
        assert [c for c in eng.calls if c[0] == "dense_novelty_pool"] == [("dense_novelty_pool", k)] * g
        assert not any(c[0] in ("dense_final_state", "dense_novelty") for c in eng.calls)          # the records stay where the rollout left them
    assert (state.algo, state.game, state.model, state.num_params, state.k, state.archive_prob) == \
        ("ga_ns", GAME[case[0]], "LinearClassifier" if not case[1] else "Dense(5, 33; relu)", eng.P, k, prob)
    assert state.archive.shape[1] == N.BC_DIM[case[0]] and state.archive.dtype == np.float32
    sizes = [len(r["archive"]) for r in records]
    if prob == 0.0:
        assert sizes == [0, 0, 0] and not any(c[0] == "dense_archive_append_members" for c in eng.calls)   # the pool is the population alone
    elif prob == 1.0:
        assert sizes == [N_POP, 2 * N_POP, 3 * N_POP] and np.array_equal(S.bits(records[0]["archive"]), S.bits(records[0]["bc"]))   # arrival order
    else:
        assert sizes[0] <= sizes[1] <= sizes[2] < 3 * N_POP and 0 < sizes[2]
    if config == "no_parents":                                                                     # random search, with an archive that still fills
        assert all(len(o.seeds) == 1 for o in state.population) and eng.dense_ga_parents() == 0 and sizes[2] > 0
    if case[0] == "maze":
        assert all(e[4] is None for e in eng.evals)                                               # no environment seed is drawn
    else:                                                                                         # every call under its own seeds: no episode twice
        seeds = np.concatenate([e[4] for e in eng.evals])
        assert len(eng.evals) == 3 * 3 and np.unique(seeds).size == seeds.size == 3 * (10 + 4 + 2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_driver_with_a_nan_theta_member(oracle, tmp_path, name):
    """member 0 of generation 1 runs a policy of NaNs; whatever BC that leaves, the run equals the plain loop's.  On the maze the BC and so the
    novelty are NaN: it counts as 0.0 and is not among the parents"""
    case = CASES[name]
    nan_theta = np.full(G.num_params(case), np.nan, np.float32)

    class Poisoned(S.DenseGaNsHostEngine):
        full = 0

        def _run(self, thetas, tslimit, seeds):
            if len(thetas) == N_POP:
                self.full += 1
                if self.full == 2:
                    thetas = [nan_theta] + list(thetas[1:])
            return super()._run(thetas, tslimit, seeds)

    for k in (3, 9):                                                                               # kk = 9 reaches a NaN in everybody's pool
        over = dict(ns={"archive_prob": 0.0, "k": k})
        (_, _, state), eng = _run(tmp_path / ("nan%d" % k), 2, case, eng=S.host_engine(case, N_POP, cls=Poisoned), **over)
        exp = _exp(case, **over)
        rec = S.plain_loop(case, exp, SEED, 2, poison=(1, 0, nan_theta))[1]
        assert S.same(eng.novelties[1], rec["raw"]) and [o.seeds for o in state.population[:3]] == rec["parents"]
        assert state.timesteps_so_far == rec["timesteps_so_far"] and S.same_stream(state.stream, rec["stream"])
        if case[0] == "maze":
            assert np.isnan(eng.novelties[1][0]) and rec["novelty"][0] == 0.0
            if k == 9:
                assert np.all(np.isnan(eng.novelties[1])) and list(rec["by_novelty"][:3]) == [0, 1, 2]   # all 0.0: arrival order (a tie, not a preference)
            else:
                assert np.all(np.isfinite(eng.novelties[1][1:])) and 0 not in rec["by_novelty"][:3] and all(o.novelty > 0 for o in state.population[:3])


@pytest.mark.parametrize("name", sorted(CASES))
def test_driver_resume_equals_a_straight_run(oracle, tmp_path, name):
    case = CASES[name]
    exp = _exp(case)
    records = S.plain_loop(case, exp, SEED, 4)
    (_, _, four), e4 = _run(tmp_path / "straight", 4, case)
    _assert_generation(four, e4, records[3], exp)
    assert [c for c in e4.calls if c[0] == "dense_ga_build"] == [("dense_ga_build", 3)]            # once per call: after generation 0
    (_, _, two), e2 = _run(tmp_path / "resumed", 2, case)
    snap = pickle.load(open(tmp_path / "resumed" / "snapshot.pkl", "rb"))
    assert (snap.game, snap.algo, snap.it, snap.k, snap.archive_prob, snap.num_params) == (GAME[case[0]], "ga_ns", 2, 3, 0.3, e2.P)
    assert np.array_equal(S.bits(snap.archive), S.bits(records[1]["archive"])) and snap.stream is not None
    (_, _, again), e22 = _run(tmp_path / "resumed", 2, case)                                       # a fresh engine: bank and archive come from the snapshot
    assert again.it == 4
    _assert_generation(again, e22, records[3], exp)
    assert [c for c in e22.calls if c[0] == "dense_ga_build"] == [("dense_ga_build", 3)] and e22.calls.index(("dense_ga_build", 3)) < e22.calls.index(("dense_ga_eval", N_POP))
    assert [c for c in e22.calls if c[0] == "dense_ga_promote"] == [("dense_ga_promote", 3)] * 2
    assert all(S.same(a, b) for a, b in zip(e22.novelties, e4.novelties[2:])) and len(e22.novelties) == 2
    assert [o.seeds for o in again.population] == [o.seeds for o in four.population] and again.num_frames == four.num_frames
    assert again.validation_timesteps_so_far == four.validation_timesteps_so_far
    assert S.same_stream(again.stream, four.stream)                                                # down to the stream's position
    assert S.log_rows(tmp_path / "resumed")[-2:] == S.log_rows(tmp_path / "straight")[-2:]


def test_driver_equals_maze_ns_main_at_16_16(oracle, tmp_path):
    """the second witness: dense_ns_main on a (16, 16) relu maze engine and maze_ns_main on MazeGaNsHostEngine write the same rows, parents and
    archive from the same seed, and leave the stream at the same position (nothing but the three draws is drawn on the maze)"""
    from dne_hip import ga_gpu
    case = G.CASES[3]
    exp = S.exp("maze", model="SimpleClassifier", episode_cutoff_mode=400)
    dense_exp = {k: v for k, v in exp.items() if k != "model"}
    me = MS.MazeGaNsHostEngine(max_members=N_POP)
    _, _, ms = ga_gpu.main(str(tmp_path / "maze"), engine=me, noise=S.shared_noise(), seed=SEED, max_iters=4, **exp)
    de = S.host_engine(case, N_POP)
    _, _, ds = ga_gpu.dense_ns_main(str(tmp_path / "dense"), engine=de, noise=S.shared_noise(), seed=SEED, max_iters=4, **dense_exp)
    rows = S.log_rows(tmp_path / "dense")
    assert len(rows) == 4 and rows == S.log_rows(tmp_path / "maze") and "NoveltyMean" in rows[0] and "ArchiveSize" in rows[0]
    assert de.dense_ga_parents() == me.maze_ga_parents() == 3
    for j in range(3):
        assert np.array_equal(M.bits(de.dense_ga_get_parent(j)), M.bits(me.maze_ga_get_parent(j)))
    assert [o.seeds for o in ds.population] == [o.seeds for o in ms.population] and ds.elite.seeds == ms.elite.seeds
    assert len(ds.archive) > 0 and np.array_equal(S.bits(ds.archive), S.bits(ms.archive)) and np.array_equal(S.bits(de.dense_archive()), S.bits(me.maze_archive()))
    assert all(S.same(a, b) for a, b in zip(de.novelties, me.novelties)) and len(de.novelties) == 4
    assert S.same_stream(ds.stream, ms.stream)
    assert (ds.model, ms.model, ds.num_params, ds.algo, ms.algo) == ("Dense(16, 16; relu)", "SimpleClassifier", 498, "ga_ns", "ga_ns")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_driver_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import ga_gpu
    lin, x = CASES["maze-linear"], tmp_path / "x"
    with pytest.raises(ValueError, match=r"k = 33.*DENSE_NOVELTY_KMAX = 32"):
        _run(x, 1, lin, ns={"k": 33})
    with pytest.raises(ValueError, match=r"k = 0"):
        _run(x, 1, lin, ns={"k": 0})
    with pytest.raises(ValueError, match=r"archive_prob = 1.5"):
        _run(x, 1, lin, ns={"archive_prob": 1.5})
    # the engine is checked as dense_main checks it
    with pytest.raises(ValueError, match=r"dense_ns_main needs an engine of kind KIND_DENSE \(8\), the engine passed in is of kind 1"):
        _run(x, 1, lin, eng=OracleEngine(1, max_members=N_POP))
    maze16 = S.host_engine(G.CASES[3], N_POP)
    with pytest.raises(ValueError, match=r"game 'gym.CartPole-v1' asked for, the engine passed in \(kind 8 on environment kind 4\) runs 'maze'"):
        _run(x, 1, CASES["cartpole-linear"], eng=maze16)
    with pytest.raises(ValueError, match=r"model 'LinearClassifier' asked for, the engine passed in \(kind 8\) runs 'Dense\(16, 16; relu\)'"):
        _run(x, 1, lin, eng=maze16)
    with pytest.raises(NotImplementedError, match="Pendulum-v0"):
        ga_gpu.dense_ns_main(str(x), engine=S.host_engine(G.CASES[1], N_POP), noise=S.shared_noise(), max_iters=1,
                             **S.exp("Pendulum-v0", model="Dense(51; tanh)"))
    with pytest.raises(NotImplementedError, match=r"'LinearClassifier' on game 'frostbite'"):
        ga_gpu.dense_ns_main(str(x), noise=S.shared_noise(), max_iters=1, **S.exp("frostbite"))
    assert not os.path.exists(x / "snapshot.pkl")
    # main and dense_main keep refusing the key on a dense run
    for game, case in (("maze", lin), ("gym.CartPole-v1", CASES["cartpole-linear"])):
        for entry in (ga_gpu.main, ga_gpu.dense_main):
            with pytest.raises(NotImplementedError, match="novelty_search"):
                entry(str(x), engine=S.host_engine(case, N_POP), noise=S.shared_noise(), max_iters=1, **S.exp(game))
    assert not os.path.exists(x / "snapshot.pkl")


def test_resumes_that_do_not_fit_name_both_sides(oracle, tmp_path):
    from dne_hip import es_gpu, ga_gpu, nses_gpu
    import dense_support as D
    lin, cart = CASES["maze-linear"], CASES["cartpole-linear"]
    plain = lambda game: {k: v for k, v in S.exp(game).items() if k != "novelty_search"}
    _run(tmp_path / "gans", 1, lin)
    with pytest.raises(ValueError, match=r"holds k 3, archive_prob 0.3; this run is k 5, archive_prob 0.3"):
        _run(tmp_path / "gans", 1, lin, ns={"k": 5})
    with pytest.raises(ValueError, match=r"holds k 3, archive_prob 0.3; this run is k 3, archive_prob 0.5"):
        _run(tmp_path / "gans", 1, lin, ns={"archive_prob": 0.5})
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'LinearClassifier'; this run is game 'gym.CartPole-v1' under model 'LinearClassifier'"):
        _run(tmp_path / "gans", 1, cart)
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'LinearClassifier'; this run is game 'maze' under model 'Dense\(16, 16; relu\)'"):
        _run(tmp_path / "gans", 1, G.CASES[3], eng=S.host_engine(G.CASES[3], N_POP))
    snap = pickle.load(open(tmp_path / "gans" / "snapshot.pkl", "rb"))
    snap.num_params = 25
    os.makedirs(tmp_path / "p")
    with open(tmp_path / "p" / "snapshot.pkl", "wb") as f:
        pickle.dump(snap, f)
    with pytest.raises(ValueError, match=r"holds model 'LinearClassifier' with P = 25; this run is model 'LinearClassifier' with P = 24"):
        _run(tmp_path / "p", 1, lin)
    # another algo's snapshot under dense_ns_main
    ga_gpu.main(str(tmp_path / "ga"), engine=S.host_engine(lin, N_POP), noise=S.shared_noise(), seed=SEED, max_iters=1, **plain("maze"))
    with pytest.raises(ValueError, match=r"'ga'.*'ga_ns'"):
        _run(tmp_path / "ga", 1, lin)
    es_exp = dict(D.exp("maze"), maze_file=M.MAZE_FILE)
    es_gpu.main(str(tmp_path / "es"), engine=D.host_engine(lin, 10), noise=S.shared_noise(), seed=SEED, max_iters=1, **es_exp)
    with pytest.raises(ValueError, match=r"'es_gpu'.*'ga_ns'"):
        _run(tmp_path / "es", 1, lin)
    N.run(tmp_path / "ns", 1, "maze")
    with pytest.raises(ValueError, match=r"'nses'.*'ga_ns'"):
        _run(tmp_path / "ns", 1, lin)
    ga_gpu.main(str(tmp_path / "mzns"), engine=MS.MazeGaNsHostEngine(max_members=N_POP), noise=S.shared_noise(), seed=SEED, max_iters=1,
                **S.exp("maze", model="SimpleClassifier", episode_cutoff_mode=400))
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'SimpleClassifier'; this run is game 'maze' under model 'LinearClassifier'"):
        _run(tmp_path / "mzns", 1, lin)                                                            # maze_ns_main's snapshot: the same algo, another model
    # this driver's snapshot under the others
    with pytest.raises(ValueError, match=r"'ga_ns'.*'ga'"):
        ga_gpu.dense_main(str(tmp_path / "gans"), engine=S.host_engine(lin, N_POP), noise=S.shared_noise(), seed=SEED, max_iters=1, **plain("maze"))
    with pytest.raises(ValueError, match=r"'ga_ns'.*'ga'"):
        ga_gpu.maze_main(str(tmp_path / "gans"), engine=MS.MazeGaNsHostEngine(max_members=N_POP), noise=S.shared_noise(), seed=SEED, max_iters=1,
                         **dict(plain("maze"), model="SimpleClassifier"))
    with pytest.raises(ValueError, match=r"holds game 'maze' under model 'LinearClassifier'; this run is game 'maze' under model 'SimpleClassifier'"):
        ga_gpu.maze_main(str(tmp_path / "gans"), engine=MS.MazeGaNsHostEngine(max_members=N_POP), noise=S.shared_noise(), seed=SEED, max_iters=1,
                         **S.exp("maze", model="SimpleClassifier"))                                # (with the key: maze_ns_main)
    with pytest.raises(ValueError, match=r"'ga_ns'"):
        N.run(tmp_path / "gans", 1, "maze")
    assert pickle.load(open(tmp_path / "gans" / "snapshot.pkl", "rb")).it == 1                     # the refused resumes left it alone
