"""CPU: novelty on the hard maze (csrc/maze_novelty.h through dne_maze_novelty_host) against the contract stated in plain Python, bit for bit;
against the reference's formula in numpy within the bound derived in maze_novelty_support.py; the header's host side under sanitizers in a
program of its own; and dne_hip/nses_gpu.py -- the NS-ES / NSR-ES loop -- on MazeNoveltyHostEngine."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import maze_novelty_support as S
import maze_support as M


def test_constants_agree_with_the_library():
    from dne_hip import _lib
    assert (_lib.MAZE_NOVELTY_KMAX, _lib.MAZE_NOVELTY_TILE) == (S.KMAX, S.TILE)
    src = open(os.path.join(M.ROOT, "deep-neuroevolution_amd", "csrc", "maze_novelty.h")).read()
    assert "KMAX = %d;" % S.KMAX in src and "TILE = %d;" % S.TILE in src
    assert "#define DNE_MAZE_NOVELTY_KMAX %d" % S.KMAX in open(os.path.join(M.ROOT, "include", "dne_hip.h")).read()


# ---- 1. the host twin against the contract, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narch", S.SIZES)
def test_host_equals_the_contract_on_every_archive_size(narch):
    from dne_hip import _lib
    xy, archive = S.members(), S.sized_archive(narch)
    assert archive.shape == (narch, 2)
    for k in S.KS:
        got, want = _lib.maze_novelty_host(xy, archive, k), S.contract(xy, archive, k)
        assert got.dtype == np.float64 and S.same(got, want), (narch, k, got, want)
        assert got[0] == 0.0 if k == 1 else got[0] > 0.0 or narch == 1       # the member on slot 0: its nearest distance is 0


@pytest.mark.parametrize("name", sorted(S.edge_cases()))
def test_host_equals_the_contract_on_the_edge_inputs(name):
    from dne_hip import _lib
    xy, archive, ks = S.edge_cases()[name]
    for k in ks:
        got, want = _lib.maze_novelty_host(xy, archive, k), S.contract(xy, archive, k)
        assert S.same(got, want), (name, k, got, want)


def test_edge_inputs_do_what_they_are_for():
    """held on the contract alone: the ties, the NaN order and the infinities behave as the issue states them"""
    E = S.edge_cases()
    xy, archive, _ = E["lattice"]
    c = lambda k: S.contract(xy[:1], archive, k)[0]
    r2 = np.sqrt(2.0)
    assert c(1) == 0.0 and c(5) == 4 / 5 and c(9) == ((1.0 + 1 + 1 + 1) + r2 + r2 + r2 + r2) / 9       # the member's own point, 4 at 1, 4 at sqrt 2
    assert c(13) == (((((1.0 + 1 + 1 + 1) + r2 + r2 + r2 + r2) + 2) + 2) + 2 + 2) / 13 and c(32) > c(13)
    xy, archive, _ = E["nan_archive_short_and_reached"]
    assert np.all(np.isfinite(S.contract(xy, archive, 9))) and np.all(np.isnan(S.contract(xy, archive, 10)))   # nine numbers, then the NaNs
    xy, archive, _ = E["nan_member"]
    assert np.array_equal(np.isnan(S.contract(xy, archive, 1)), [True, True, True, False])
    xy, archive, _ = E["inf_in_archive"]
    assert np.all(np.isfinite(S.contract(xy, archive, 5))) and np.all(np.isposinf(S.contract(xy, archive, 6)))   # +inf sorts behind every finite number
    xy, archive, _ = E["inf_member"]
    got = S.contract(xy, archive, 6)
    assert np.isnan(got[0]) and np.isnan(got[1]) and np.isposinf(got[2])           # inf - inf is a NaN distance and sorts last
    assert np.isposinf(S.contract(xy, archive, 4)[0])                              # ... so four infinities come first for the member at (inf, 0)
    xy, archive, _ = E["mostly_nan"]
    assert np.all(np.isfinite(S.contract(xy, archive, 3))) and np.all(np.isnan(S.contract(xy, archive, 4)))
    xy, archive, _ = E["k_above_narch"]
    assert S.same(S.contract(xy, archive, 32), S.contract(xy, archive, 3))


def test_host_refusals():
    from dne_hip import _lib
    one = np.zeros((1, 2), np.float32)
    for xy, archive, k, text in ((one[:0], one, 1, "n = 0"), (one, one[:0], 1, "archive is empty"), (one, one, 0, "k = 0")):
        with pytest.raises(_lib.DneError, match=text):
            _lib.maze_novelty_host(xy, archive, k)


# ---- 2. against the reference's formula, within the derived bound -------------------------------------------------------------------------------
def test_host_against_the_reference_formula_within_the_derived_bound():
    """Measured here: 5400 novelties, worst 4.36 * 2**-53 relative; 1365 differ from numpy in the last bits, so bit equality is not the target."""
    from dne_hip import _lib
    worst, differ, total = 0.0, 0, 0
    for xy, archive in S.reference_cases():
        refs = S.reference_np(xy, archive, S.REFERENCE_KS)
        for k in S.REFERENCE_KS:
            got, ref = _lib.maze_novelty_host(xy, archive, k), refs[k]
            kk = min(k, archive.shape[0])
            err = np.abs(got - ref) / np.where(ref == 0, 1.0, ref)
            worst = max(worst, float(err.max())); differ += int(np.sum(got != ref)); total += got.size
            assert np.all(np.abs(got - ref) <= S.reference_bound(kk) * np.abs(ref)), (archive.shape[0], k, err.max() * 2.0 ** 53)
    print("reference comparison: %d novelties, %d differ from numpy, worst %.2f * 2**-53" % (total, differ, worst * 2.0 ** 53))
    assert total == 5400


# ---- 3. the header's host side under sanitizers, in a program of its own --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/maze_novelty_asan_main.cpp, built once: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(M.ROOT, "tests", "maze_novelty_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("maze_novelty_asan") / "maze_novelty_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(M.ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def _case_text(xy, archive, k):
    tok = lambda v: "nan" if v != v else float(v).hex()
    return "%d %d %d\n%s\n%s\n" % (len(xy), len(archive), k, " ".join(tok(v) for v in np.asarray(xy).reshape(-1)),
                                   " ".join(tok(v) for v in np.asarray(archive).reshape(-1)))


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program, tmp_path):
    cases = [(xy, archive, k) for _, (xy, archive, ks) in sorted(S.edge_cases().items()) for k in ks]
    cases += [(S.members(), S.sized_archive(n), k) for n in (1, 2, 63, 64, 65, S.TILE + 1) for k in (1, 10, 32)]
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case_text(*c) for c in cases))
    out = subprocess.run([sanitizer_program, "archive", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % len(cases) and len(lines) == len(cases) + 1
    for line, (xy, archive, k) in zip(lines, cases):
        got = np.array([float("nan") if t == "nan" else float.fromhex(t) for t in line.split()])
        assert S.same(got, S.contract(xy, archive, k)), (k, archive.shape)


# ---- 4. the driver on the host-function engine -----------------------------------------------------------------------------------------------------
def _exp(**over):
    exp = {"game": "maze", "model": "SimpleClassifier", "algo_type": "ns", "population_size": 8, "timesteps": 10 ** 9,
           "novelty_search": {"k": 2, "population_size": 3, "num_rollouts": 1, "selection_method": "round_robin"},
           "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_sign_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "maze_file": M.MAZE_FILE}
    ns = dict(exp["novelty_search"]); ns.update(over.pop("ns", {}))
    exp.update(over); exp["novelty_search"] = ns
    return exp


def _noise():
    from dne_hip import es
    noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    noise.noise = M.maze_noise()
    noise._engines = []
    return noise


def _run(log_dir, iters, eng=None, **over):
    from dne_hip import nses_gpu
    eng = eng or S.MazeNoveltyHostEngine(max_members=8)
    return nses_gpu.main(str(log_dir), engine=eng, noise=_noise(), seed=4, max_iters=iters, **_exp(**over)), eng


def _same_state(a, b):
    ok = len(a.thetas) == len(b.thetas) and a.parents == b.parents and a.curr_parent == b.curr_parent and a.it == b.it
    ok = ok and all(np.array_equal(M.bits(x), M.bits(y)) for x, y in zip(a.thetas, b.thetas))
    ok = ok and all(np.array_equal(M.bits(x[0]), M.bits(y[0])) and np.array_equal(M.bits(x[1]), M.bits(y[1])) and x[2] == y[2]
                    for x, y in zip(a.optimizers, b.optimizers))
    return bool(ok and np.array_equal(M.bits(a.archive), M.bits(b.archive)) and a.novelty_log == b.novelty_log)


@pytest.mark.parametrize("pop", (2, 3))
def test_driver_archive_order_resume_and_algo_types(oracle, tmp_path, pop):
    from dne_hip import _lib, policies
    noise = _noise()
    header, lines = M.fixture_maze()
    final_xy = lambda theta: _lib.maze_rollout_host(theta, header, lines, 400)[2][0]

    st0, e0 = _run(tmp_path / "zero", 0, ns={"population_size": pop})
    rs = np.random.RandomState(4)
    for m in range(pop):                                                            # every theta from its own draw, in order
        th = noise.get(rs.randint(0, noise.noise.size - 498 + 1), 498) * policies.simple_scale_by()
        rs.randint(0, 2 ** 32, size=2, dtype=np.uint64)                             # (its episode's seeds)
        assert np.array_equal(st0.thetas[m], th) and st0.optimizers[m][2] == 0 and not np.any(st0.optimizers[m][0])
        assert np.array_equal(st0.archive[m], final_xy(th))
    assert st0.archive.shape == (pop, 2) and st0.it == 0 and st0.algo == "nses" and e0.maze_archive_size() == pop

    st3, e3 = _run(tmp_path / "three", 3, ns={"population_size": pop})
    assert st3.it == 3 and st3.archive.shape == (pop + 3, 2) and st3.parents == [i % pop for i in range(3)] and st3.curr_parent == 3 % pop
    assert np.array_equal(st3.archive[:pop], st0.archive) and np.array_equal(e3.maze_archive(), st3.archive)
    last = {p: i for i, p in enumerate(st3.parents)}                                # the entry appended after a parent's last update is where its theta ends
    for p, i in last.items():
        assert np.array_equal(st3.archive[pop + i], final_xy(st3.thetas[p])) and st3.optimizers[p][2] == st3.parents.count(p)
        assert not np.array_equal(st3.thetas[p], st0.thetas[p])
    assert st3.timesteps_so_far == 3 * 8 * 400 and len(st3.novelty_log) == 3 and all(0 < a <= b for a, b in st3.novelty_log)

    st1, _ = _run(tmp_path / "resumed", 1, ns={"population_size": pop})
    snap = pickle.load(open(tmp_path / "resumed" / "snapshot.pkl", "rb"))
    assert snap.algo == "nses" and snap.it == 1 and snap.archive.shape == (pop + 1, 2) and (snap.algo_type, snap.pop_size, snap.k) == ("ns", pop, 2)
    st12, e12 = _run(tmp_path / "resumed", 2, ns={"population_size": pop})          # a fresh engine: the archive comes from the snapshot
    assert st1.it == 1 and _same_state(st12, st3) and np.array_equal(e12.maze_archive(), st3.archive)

    nsr, _ = _run(tmp_path / "nsr", 3, algo_type="nsr", ns={"population_size": pop})
    assert np.array_equal(nsr.archive[:pop], st3.archive[:pop]) and not _same_state(nsr, st3)
    assert all(not np.array_equal(a, b) for a, b in zip(nsr.thetas, st3.thetas))


def test_driver_novelty_prob_and_the_two_decisions(oracle, tmp_path):
    from dne_hip import nses_gpu
    st, eng = _run(tmp_path / "prob", 3, ns={"selection_method": "novelty_prob"})
    assert st.it == 3 and st.archive.shape == (6, 2) and st.parents[0] == 0 and all(0 <= p < 3 for p in st.parents + [st.curr_parent])
    again, _ = _run(tmp_path / "prob2", 3, ns={"selection_method": "novelty_prob"})
    assert _same_state(st, again)
    one, _ = _run(tmp_path / "prob3", 1, ns={"selection_method": "novelty_prob"})
    resumed, _ = _run(tmp_path / "prob3", 2, ns={"selection_method": "novelty_prob"})
    assert _same_state(resumed, st)
    # the selection itself: all M thetas in one evaluation, probabilities = normalised novelties
    rs = np.random.RandomState(99)
    before = list(eng.calls)
    got = nses_gpu.select_parent(eng, st, "novelty_prob", 2, 400, rs)
    nov = eng.maze_novelty(2, n=3)
    rs2 = np.random.RandomState(99); rs2.randint(0, 2 ** 32, size=3, dtype=np.uint64)
    assert got == rs2.choice(range(3), 1, p=nov / nov.sum())[0] and eng.calls == before     # (eval_members, not es_eval)
    assert np.array_equal(nov, S.contract(np.stack([eng.maze_final_state(3)[m] for m in range(3)]), st.archive, 2))

    class Flat(S.MazeNoveltyHostEngine):                                            # novelties whose sum is 0, then not finite: uniform
        value = 0.0

        def maze_novelty(self, k, xy=None, n=None):
            return np.full(3, self.value)

    flat = Flat(max_members=8)
    flat.noise_upload(M.maze_noise()); flat.maze_set_walls(*M.fixture_maze())
    for value in (0.0, np.nan, np.inf):
        flat.value = value
        rs, rs2 = np.random.RandomState(5), np.random.RandomState(5)
        rs2.randint(0, 2 ** 32, size=3, dtype=np.uint64)
        assert nses_gpu.select_parent(flat, st, "novelty_prob", 2, 400, rs) == rs2.choice(range(3), 1, p=np.full(3, 1 / 3))[0]
    # a non-finite novelty counts as 0.0 before any rank
    assert np.array_equal(nses_gpu.sanitized([1.5, np.nan, np.inf, -np.inf, 0.0]), [1.5, 0.0, 0.0, 0.0, 0.0])


def test_driver_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import es_gpu
    with pytest.raises(NotImplementedError, match=r"'frostbite'.*'SimpleClassifier'"):
        _run(tmp_path / "x", 1, game="frostbite")
    with pytest.raises(NotImplementedError, match=r"'maze'.*'ModelVirtualBN'"):
        _run(tmp_path / "x", 1, model="ModelVirtualBN")
    with pytest.raises(ValueError, match="KIND_MAZE"):
        _run(tmp_path / "x", 1, eng=OracleEngine(0, ref_count=8, max_members=8))
    with pytest.raises(ValueError, match="num_rollouts 2"):
        _run(tmp_path / "x", 1, ns={"num_rollouts": 2})
    with pytest.raises(NotImplementedError, match="tournament"):
        _run(tmp_path / "x", 1, ns={"selection_method": "tournament"})
    with pytest.raises(NotImplementedError, match="median"):
        _run(tmp_path / "x", 1, return_proc_mode="median")
    with pytest.raises(ValueError, match="algo_type 'nsra'"):
        _run(tmp_path / "x", 1, algo_type="nsra")
    assert not os.path.exists(tmp_path / "x" / "snapshot.pkl")
    for mode in ("centered_rank", "sign"):                                          # the other two modes of nses.py:217-228 run
        assert _run(tmp_path / mode, 1, return_proc_mode=mode)[0].it == 1
    # resumes that do not fit name both sides
    _run(tmp_path / "ns", 1)
    with pytest.raises(ValueError, match=r"algo_type 'ns', population_size 3, k 2; this run is algo_type 'nsr', population_size 3, k 2"):
        _run(tmp_path / "ns", 1, algo_type="nsr")
    with pytest.raises(ValueError, match=r"population_size 3, k 2; this run is algo_type 'ns', population_size 2, k 2"):
        _run(tmp_path / "ns", 1, ns={"population_size": 2})
    with pytest.raises(ValueError, match=r"k 2; this run is algo_type 'ns', population_size 3, k 5"):
        _run(tmp_path / "ns", 1, ns={"k": 5})
    plain = {k: v for k, v in _exp().items() if k not in ("algo_type", "novelty_search")}
    plain.update(num_test_episodes=2, return_proc_mode="centered_rank")
    es_gpu.main(str(tmp_path / "es"), engine=M.MazeHostEngine(max_members=8), noise=_noise(), seed=4, max_iters=1, **plain)
    with pytest.raises(ValueError, match=r"'es_gpu'.*'nses'"):
        _run(tmp_path / "es", 1)
