"""CPU: GA-NS on Atari (csrc/ram_novelty.h).  dne_ram_novelty_pool_host against the contract restated in
tests/atari_gans_support.py, novelty and neighbours bit for bit, on every shape of the grid and on the edge inputs; the wrong forms told from the
contract; the n = 1 pool against the oracle's novelty; the contract against the dense numpy formulation within a derived bound; the header's
host side under sanitizers in a program of its own; ga_gpu.atari_ns_main on AtariGaNsHostEngine against the same algorithm written the long
way, its resume, its refusals."""
import ctypes as C
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import atari_gans_support as S
import dense_support as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twin(bc, archive, k):
    from dne_hip import _lib
    return _lib.ram_novelty_pool_host(bc, archive, k, neighbours=True)


# ---- 1. the twin against the contract --------------------------------------------------------------------------------------------------------------
def test_shapes_are_the_ones_asked_for():
    from dne_hip import _lib
    assert (_lib.RAM_NOVELTY_KMAX, _lib.RAM_NOVELTY_TILE, _lib.RAM_NOVELTY_MEMBERS, _lib.RAM_BYTES) == (S.KMAX, S.TILE, S.MEMBERS, S.RAM)
    assert S.ARCHIVES == (0, 1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025) and S.COUNTS == (1, 2, 3, 5, 9, 33, 65) and S.KS == (1, 2, 25, 32)
    assert (0, 1) not in S.shapes() and len(S.shapes()) == 12 * 7 - 1


@pytest.mark.parametrize("A", S.ARCHIVES)
@pytest.mark.parametrize("name", S.SETS)
def test_twin_equals_the_contract_on_every_shape(oracle, name, A):
    for n in S.COUNTS:
        if A + n - 1 < 1:
            continue
        bc, arch = S.cell(name, A, n)
        for k in S.KS:
            want_nov, want_nb = S.contract_cell(name, A, n, k)
            nov, nb = _twin(bc, arch, k)
            assert nb.shape == (n, min(k, A + n - 1)) and np.array_equal(nb, want_nb), (n, k)
            assert S.same(nov, want_nov), (n, k)


def test_twin_equals_the_contract_on_the_edge_inputs(oracle):
    for name, (bc, arch, ks) in sorted(S.edge_cases().items()):
        for k in ks:
            want_nov, want_nb = S.contract(bc, arch, k)
            nov, nb = _twin(bc, arch, k)
            assert np.array_equal(nb, want_nb) and S.same(nov, want_nov), (name, k)


def test_edge_inputs_do_what_they_are_for(oracle):
    e = S.edge_cases()
    bc, arch, _ = e["extremes"]
    assert S.squared(bc[0], arch[:1]) == [S.S_MAX] and S.distance(bc[0], arch[0]) == np.sqrt(np.sqrt(float(S.S_MAX)) ** 2 + 0.0) < S.D_MAX
    nov, nb = _twin(bc[:2], None, 1)
    assert nov.tolist() == [S.distance(bc[0], bc[1])] * 2 and nb.tolist() == [[1], [0]]                # the largest S there is
    bc, arch, _ = e["member_on_an_archive_point"]
    nov, nb = _twin(bc, arch, 1)
    assert nov[1] == 0.0 and nb[1, 0] == 3                                                              # stays in the pool at distance 0
    bc, arch, _ = e["two_members_equal"]
    nov, nb = _twin(bc, arch, 1)
    assert nov[0] == nov[3] == 0.0 and nb[0, 0] == len(arch) + 3 and nb[3, 0] == len(arch) + 0        # each other's nearest: left out by index only
    bc, arch, _ = e["all_members_equal"]
    nov, nb = _twin(bc, arch, 32)
    assert np.all(nov == 0.0) and nb.tolist() == [[c for c in range(5) if c != m] for m in range(5)]  # ties in slot order, self passed over
    bc, arch, _ = e["all_members_on_one_archive_point"]
    nov, nb = _twin(bc, arch, 6)
    assert np.all(nov == 0.0) and nb[2].tolist() == [0, 1, 2, 3, 5, 6]                                  # the archive first, then the others
    mem, arch = S.point_set("lattice")
    assert S.squared(mem[0], [mem[1], arch[0]]) == [1, 1]                                              # a tie across the seam at every A >= 1


# ---- 2. the wrong forms ------------------------------------------------------------------------------------------------------------------------------
def _small_inputs():
    for name in S.SETS:
        for A, n in S.shapes((0, 1, 2, 31), (2, 3, 5, 9)):
            for k in S.KS:
                yield S.cell(name, A, n) + (k, S.contract_cell(name, A, n, k))
    for name, (bc, arch, ks) in sorted(S.edge_cases().items()):
        for k in ks:
            yield bc, arch, k, S.contract(bc, arch, k)


@pytest.mark.parametrize("form", sorted(S.WRONG_FORMS))
def test_inputs_tell_the_wrong_forms_from_the_contract(oracle, form):
    told_by_novelty = told_by_neighbours = 0
    for bc, arch, k, (nov, nb) in _small_inputs():
        wnov, wnb = S.contract(bc, arch, k, **S.WRONG_FORMS[form])
        told_by_novelty += not S.same(nov, wnov)
        told_by_neighbours += wnb.shape != nb.shape or not np.array_equal(wnb, nb)
    if form == "population_before_archive_in_ties":
        assert told_by_neighbours > 0                                                                  # the tie rule shows in the neighbours
    else:
        assert told_by_novelty > 0


# ---- 3. the second witness: with one member the pool is the archive -----------------------------------------------------------------------------------
def test_one_member_pool_is_the_oracles_novelty(oracle):
    from oracle_engine import OracleEngine
    eng = OracleEngine(1)
    for name in S.SETS:
        mem, arch = S.point_set(name)
        for A in (1, 2, 31, 33, 65):
            entries = [arch[a:a + 1] for a in range(A)]
            for m in (0, 1, 7):
                for k in S.KS:
                    want = eng.novelty(entries, mem[m:m + 1], k)
                    assert S.same(_twin(mem[m:m + 1], arch[:A], k)[0], [want]), (name, A, m, k)
                    assert S.same(S.contract(mem[m:m + 1], arch[:A], k)[0], [want]), (name, A, m, k)


# ---- 4. the contract against the dense numpy formulation -----------------------------------------------------------------------------------------------
def test_contract_against_dense_numpy_within_the_derived_bound(oracle):
    """measured worst case of |contract - dense numpy| / (dense_bound(kk) * D_MAX) over these inputs: see DESIGN.md section 18"""
    worst = 0.0
    for name in S.SETS:
        for A, n in S.shapes((0, 1, 33, 1025), (2, 9, 65)):
            bc, arch = S.cell(name, A, n)
            for k in S.KS:
                kk = min(k, A + n - 1)
                err = np.abs(S.contract_cell(name, A, n, k)[0] - S.dense_numpy(bc, arch, k)).max()
                bound = S.dense_bound(kk) * S.D_MAX
                worst = max(worst, err / bound)
                assert err <= bound, (name, A, n, k, err, bound)
    for name, (bc, arch, ks) in sorted(S.edge_cases().items()):
        for k in ks:
            kk = min(k, len(arch) + len(bc) - 1)
            err = np.abs(S.contract(bc, arch, k)[0] - S.dense_numpy(bc, arch, k)).max()
            worst = max(worst, err / (S.dense_bound(kk) * S.D_MAX))
            assert err <= S.dense_bound(kk) * S.D_MAX, (name, k, err)
    print("worst |contract - dense numpy| / bound = %.4f" % worst)
    assert S.dense_bound(25) == (2 * 25 + 4) * 2.0 ** -53 * (1 + 2.0 ** -20)


# ---- 5. the host refusals ----------------------------------------------------------------------------------------------------------------------------
def test_host_refusals():
    from dne_hip import _lib
    bc = S.point_set("random")[0]
    with pytest.raises(_lib.DneError, match="the pool is empty"):
        _lib.ram_novelty_pool_host(bc[:1], None, 1)
    with pytest.raises(_lib.DneError, match="k = 0"):
        _lib.ram_novelty_pool_host(bc[:2], None, 0)
    with pytest.raises(_lib.DneError, match="n = 0"):
        _lib.ram_novelty_pool_host(bc[:0], bc[:2], 1)
    assert _lib.ram_novelty_pool_host(bc[:2], None, 40).shape == (2, )                                 # any k >= 1 on the host
    lib = _lib.load()
    p = bc[:2].ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.zeros(2)
    o = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.dne_ram_novelty_pool_host(p, 2, None, 3, 1, o, None) != 0 and b"a buffer is missing" in lib.dne_last_error(None)
    assert lib.dne_ram_novelty_pool_host(None, 2, None, 0, 1, o, None) != 0 and b"a buffer is missing" in lib.dne_last_error(None)
    assert lib.dne_ram_novelty_pool_host(p, 2, None, -1, 1, o, None) != 0 and b"narch = -1" in lib.dne_last_error(None)
    assert lib.dne_ram_novelty_pool_host(p, 2 ** 31 - 1, p, 1, 1, o, None) != 0 and b"slot field" in lib.dne_last_error(None)   # refused before anything is read
    assert lib.dne_ram_novelty_pool_host(p, 2, None, 0, 1, o, None) == 0                                # no archive buffer at all at narch 0


# ---- 6. the header's host side under sanitizers, in a program of its own -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/atari_gans_asan_main.cpp, built once with address and undefined"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(ROOT, "tests", "atari_gans_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("atari_gans_asan") / "atari_gans_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(oracle, sanitizer_program, tmp_path):
    cases = [(bc, archive, k) for _, (bc, archive, ks) in sorted(S.edge_cases().items()) for k in ks]
    cases += [S.cell(name, A, n) + (k, ) for name in S.SETS for A in (0, 1, 33, 1025) for n in (2, 9) for k in (1, 25, 32)]
    cases.append(S.cell("random", 1, 1) + (1, ))                                                      # the smallest pool there is
    text = lambda bc, arch, k: "%d %d %d\n%s\n%s\n" % (len(bc), len(arch), k, " ".join(map(str, np.asarray(bc).reshape(-1))),
                                                       " ".join(map(str, np.asarray(arch).reshape(-1))))
    path = tmp_path / "cases.txt"
    path.write_text("".join(text(*c) for c in cases))
    out = subprocess.run([sanitizer_program, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % len(cases) and len(lines) == len(cases) + 1
    for line, (bc, archive, k) in zip(lines, cases):
        tok, n = line.split(), len(bc)
        nov, nb = S.contract(bc, archive, k)
        assert S.same([float.fromhex(t) for t in tok[:n]], nov) and [int(t) for t in tok[n:]] == nb.reshape(-1).tolist(), (k, bc.shape, archive.shape)


# ---- 7. the driver on the host engine --------------------------------------------------------------------------------------------------------------------
SEED, N_POP = 4, 6
CONFIGS = {
    "prob_0": dict(ns={"archive_prob": 0.0}),
    "prob_1": dict(ns={"archive_prob": 1.0}),
    "prob_0.3": dict(),
    "no_parents": dict(selection_threshold=0),
}


def _run(log_dir, iters, eng=None, ns=None, **over):
    from dne_hip import ga_gpu
    eng = eng or S.AtariGaNsHostEngine(max_members=N_POP)
    return ga_gpu.atari_ns_main(str(log_dir), engine=eng, noise=S.shared_noise(), seed=SEED, max_iters=iters, **S.exp(ns=ns, **over)), eng


def _assert_generation(state, eng, rec, exp):
    """the driver after g generations against record g of the plain loop"""
    T = exp["selection_threshold"]
    assert [o.seeds for o in state.population[:T]] == rec["parents"]                                  # the genomes of the parents
    assert state.archive.dtype == np.uint8 and state.archive.shape == rec["archive"].shape and np.array_equal(state.archive, rec["archive"])   # contents and order
    assert np.array_equal(eng._arch, rec["archive"])
    assert S.same(eng.novelties[-1], rec["raw"])
    assert [o.novelty for o in state.population[:T]] == sorted(rec["novelty"].tolist(), reverse=True)[:T]
    assert state.elite.seeds == rec["elite"] and state.curr_solution == rec["curr_solution"] and state.timesteps_so_far == rec["timesteps_so_far"]
    assert (state.curr_solution_val, state.curr_solution_test) == (rec["curr_solution_val"], rec["curr_solution_test"])
    assert S.same_stream(state.stream, rec["stream"])                                                  # the stream's position


@pytest.fixture(scope="module")
def plain_records(oracle):
    """the plain loop of each configuration, four generations, computed once"""
    return {name: S.plain_loop(S.shared_noise().noise, S.exp(**over), SEED, 4, max_members=N_POP) for name, over in CONFIGS.items()}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_driver_equals_the_plain_loop(oracle, tmp_path, plain_records, config):
    exp = S.exp(**CONFIGS[config])
    records = plain_records[config]
    prob, k = exp["novelty_search"]["archive_prob"], exp["novelty_search"]["k"]
    for g in (2, 4):
        (test, val, state), eng = _run(tmp_path / ("g%d" % g), g, **CONFIGS[config])
        assert state.it == g and (test, val["val"]) == (state.curr_solution_test, state.curr_solution_val)
        _assert_generation(state, eng, records[g - 1], exp)
        assert len(eng.novelties) == g and all(S.same(a, r["raw"]) for a, r in zip(eng.novelties, records))
        assert [c for c in eng.calls if c[0] == "ram_novelty_pool"] == [("ram_novelty_pool", k)] * g
        assert [c for c in eng.calls if c[0] == "ga_eval_powers"][::3] == [("ga_eval_powers", N_POP)] * g   # a generation is ONE evaluation
    assert (state.algo, state.game, state.model, state.num_params, state.k, state.archive_prob) == ("ga_ns", "frostbite", "Model", eng.P, k, prob)
    sizes = [len(r["archive"]) for r in records]
    if prob == 0.0:
        assert sizes == [0] * 4 and not any(c[0] == "archive_append_members" for c in eng.calls)      # the pool is the population alone
    elif prob == 1.0:
        assert sizes == [N_POP * g for g in (1, 2, 3, 4)] and np.array_equal(records[0]["archive"], records[0]["bc"])   # arrival order
    else:
        assert sizes[0] <= sizes[1] <= sizes[2] <= sizes[3] < 4 * N_POP and 0 < sizes[3]
    if config == "no_parents":                                                                         # random search, with an archive that still fills
        assert all(len(o.seeds) == 1 for o in state.population) and sizes[3] > 0
    rows = D.log_rows(tmp_path / "g4")
    assert len(rows) == 4 and all(key in rows[0] for key in ("NoveltyMean", "NoveltyMax", "ArchiveSize")) and rows[3]["ArchiveSize"] == str(sizes[3])


def test_driver_resume_equals_a_straight_run(oracle, tmp_path, plain_records):
    exp, records = S.exp(), plain_records["prob_0.3"]
    (_, _, four), e4 = _run(tmp_path / "straight", 4)
    _assert_generation(four, e4, records[3], exp)
    (_, _, two), e2 = _run(tmp_path / "resumed", 2)
    snap = pickle.load(open(tmp_path / "resumed" / "snapshot.pkl", "rb"))
    assert (snap.game, snap.model, snap.algo, snap.it, snap.k, snap.archive_prob, snap.num_params) == ("frostbite", "Model", "ga_ns", 2, 3, 0.3, e2.P)
    assert np.array_equal(snap.archive, records[1]["archive"]) and snap.stream is not None
    (_, _, again), e22 = _run(tmp_path / "resumed", 2)                                                # a fresh engine: the archive comes from the snapshot
    assert again.it == 4
    _assert_generation(again, e22, records[3], exp)
    if len(records[1]["archive"]):
        assert e22.calls.index(("archive_append_points", len(records[1]["archive"]))) < e22.calls.index(("ga_eval_powers", N_POP))
    assert all(S.same(a, b) for a, b in zip(e22.novelties, e4.novelties[2:])) and len(e22.novelties) == 2
    assert [o.seeds for o in again.population] == [o.seeds for o in four.population] and again.num_frames == four.num_frames
    assert again.validation_timesteps_so_far == four.validation_timesteps_so_far
    assert S.same_stream(again.stream, four.stream)                                                    # down to the stream's position
    assert D.log_rows(tmp_path / "resumed")[-2:] == D.log_rows(tmp_path / "straight")[-2:]


def test_driver_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import ga_gpu
    x = tmp_path / "x"
    with pytest.raises(ValueError, match=r"k = 33.*RAM_NOVELTY_KMAX = 32"):
        _run(x, 1, ns={"k": 33})
    with pytest.raises(ValueError, match=r"k = 0"):
        _run(x, 1, ns={"k": 0})
    with pytest.raises(ValueError, match=r"archive_prob = 1.5"):
        _run(x, 1, ns={"archive_prob": 1.5})
    with pytest.raises(ValueError, match=r"population_size 6 exceeds the engine's max_members 5"):
        _run(x, 1, eng=S.AtariGaNsHostEngine(max_members=5))
    with pytest.raises(ValueError, match=r"record_bc"):
        _run(x, 1, eng=S.AtariGaNsHostEngine(max_members=N_POP, record_bc=False))
    with pytest.raises(ValueError, match=r"record_bc"):
        _run(x, 1, eng=OracleEngine(1, max_members=N_POP))                                              # an engine that never heard of it
    with pytest.raises(ValueError, match=r"model 'LargeModel' asked for \(engine kind 2\), the engine passed in is of kind 1"):
        _run(x, 1, model="LargeModel")
    with pytest.raises(NotImplementedError, match=r"'SimpleClassifier' on game 'maze'"):
        _run(x, 1, game="maze", model="SimpleClassifier")
    with pytest.raises(NotImplementedError, match=r"'Model' on game 'maze'"):
        _run(x, 1, game="maze")
    assert not os.path.exists(x / "snapshot.pkl")
    # main keeps refusing the key under an Atari game
    with pytest.raises(NotImplementedError, match=r"game 'frostbite' with exp\['novelty_search'\]: GA-NS runs on game 'maze' only"):
        ga_gpu.main(str(x), engine=S.AtariGaNsHostEngine(max_members=N_POP), noise=S.shared_noise(), max_iters=1, **S.exp())
    assert not os.path.exists(x / "snapshot.pkl")


def test_resumes_that_do_not_fit_name_both_sides(oracle, tmp_path):
    from dne_hip import ga_gpu
    plain = {k: v for k, v in S.exp().items() if k != "novelty_search"}
    _run(tmp_path / "gans", 1)
    with pytest.raises(ValueError, match=r"holds k 3, archive_prob 0.3; this run is k 5, archive_prob 0.3"):
        _run(tmp_path / "gans", 1, ns={"k": 5})
    with pytest.raises(ValueError, match=r"holds k 3, archive_prob 0.3; this run is k 3, archive_prob 0.5"):
        _run(tmp_path / "gans", 1, ns={"archive_prob": 0.5})
    with pytest.raises(ValueError, match=r"holds game 'frostbite' under model 'Model'; this run is game 'pong' under model 'Model'"):
        _run(tmp_path / "gans", 1, game="pong")
    snap = pickle.load(open(tmp_path / "gans" / "snapshot.pkl", "rb"))
    for attr, value, text in (("num_params", 25, r"holds model 'Model' with P = 25; this run is model 'Model' with P = 1008450"),
                              ("model", "LargeModel", r"holds game 'frostbite' under model 'LargeModel'; this run is game 'frostbite' under model 'Model'")):
        other = pickle.loads(pickle.dumps(snap))
        setattr(other, attr, value)
        os.makedirs(tmp_path / attr)
        with open(tmp_path / attr / "snapshot.pkl", "wb") as f:
            pickle.dump(other, f)
        with pytest.raises(ValueError, match=text):
            _run(tmp_path / attr, 1)
    # the plain GA's snapshot under this driver, and this driver's under the plain GA
    ga_gpu.main(str(tmp_path / "ga"), engine=S.AtariGaNsHostEngine(max_members=N_POP), noise=S.shared_noise(), seed=SEED, max_iters=1, **plain)
    with pytest.raises(ValueError, match=r"'ga'.*'ga_ns'"):
        _run(tmp_path / "ga", 1)
