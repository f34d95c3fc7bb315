"""The Deep GA with MujocoPolicy without a GPU (csrc/mujoco_ga.h's host twins, policies.MujocoPolicy, dne_hip/ga_mujoco.py):
the column scale against numpy's own expression bit for bit on every built shape, roots, genomes as a root followed by promotions, the
policy's reinitialize / set_from_seeds, the refusals by their words, three iterations of the drivers on the host engines of both kinds, and the
header under the sanitizers in a program of its own."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mujoco_ga_support as S   # noqa: E402

KINDS = (S.KIND_PENDULUM, S.KIND_MJMAZE)
SHAPES = [(k, H, O) for k in KINDS for H in S.HS for O in S.OUTS[k]]
U = 2.0 ** -24


def test_symbols_and_module_exist():
    from dne_hip import _lib, ga_mujoco
    lib = _lib.load()
    for name in ("reserve", "build", "eval", "promote", "parents", "get_parent", "theta_host", "members_host", "colscale_host"):
        assert getattr(lib, "dne_mujoco_ga_" + name).argtypes is not None
    assert all(callable(getattr(ga_mujoco, f)) for f in ("setup", "run_master", "run_worker"))
    assert all(d in ga_mujoco.__doc__ for d in ("(a)", "(b)", "(c)", "(d)", "(e)"))


# ---- 1. the column scale -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_column_scale_is_numpys_bit_for_bit_on_every_built_shape(kind):
    """K in {3 | 11, 64, 128, 256}, C = H in {64, 128, 256} and O = every output count of the kind (C = 1: numpy's pairwise order), at the
    table's start, at its end and in between"""
    from dne_hip import _lib
    tab = S.table()
    for H in S.HS:
        for O in S.OUTS[kind]:
            P = S.num_params(kind, H, O)
            assert P == (_lib.pendulum_num_params(H, O) if kind == S.KIND_PENDULUM else _lib.mjmaze_num_params(H, O))
            for idx in (0, tab.size - P, 4099 + 17 * O):
                got = _lib.mujoco_ga_colscale_host(tab, kind, H, O, idx)
                want = S.colscale_np(tab[idx:idx + P], kind, H, O)
                assert got.shape == want.shape == (2 * H + O, )
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, H, O, idx)


def test_a_sequential_sum_of_the_one_column_layer_would_be_reported():
    """out/w [H][1] of the pendulum's continuous action: numpy sums the contiguous run pairwise.  The twin equals numpy on every one of 40
    slices a width; a k-ordered float32 sum differs from numpy on some of them at every width, so the comparison above would catch it"""
    from dne_hip import _lib
    tab = S.table()
    for H in S.HS:
        (_, _, _, _), (_, _, _, _), (w0, K, C, _) = S.blocks(S.KIND_PENDULUM, H, 1)[0]
        assert (K, C) == (H, 1)
        differs = 0
        for t in range(40):
            idx = 1000 * t + 3
            x = tab[idx + w0:idx + w0 + K]
            want = (1.0 / np.sqrt(np.square(x.reshape(K, 1)).sum(axis=0, keepdims=True))).astype(np.float32)[0, 0]
            assert _lib.mujoco_ga_colscale_host(tab, S.KIND_PENDULUM, H, 1, idx)[-1].view(np.uint32) == want.view(np.uint32)
            ss = np.float32(0)
            for v in x:
                ss = np.float32(ss + np.float32(v * v))
            differs += int(np.float32(1.0) / np.sqrt(ss) != want)
        assert differs >= 5, (H, differs)


# ---- 2. roots ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,O", [(S.KIND_PENDULUM, 64, 1), (S.KIND_PENDULUM, 128, 7), (S.KIND_MJMAZE, 64, 2), (S.KIND_MJMAZE, 256, 16)])
def test_roots_have_zero_biases_and_unit_columns_out_included(kind, H, O):
    """a column's norm: ss carries at most (K + 1) roundings and sc a square root and a division, each element one more -- the norm of the
    float32 column is within ((K + 1) / 2 + 3) * 2^-24 of 1 (relative; first order), the float64 check itself adding nothing of that size"""
    from dne_hip import _lib
    tab = S.table()
    P = S.num_params(kind, H, O)
    for idx in (0, tab.size - P):
        th = _lib.mujoco_ga_theta_host(tab, kind, H, O, (idx, ))
        assert S.same(th, S.root_np(tab, kind, H, O, idx))
        for w0, K, C, b0 in S.blocks(kind, H, O)[0]:
            assert np.array_equal(th[b0:b0 + C].view(np.uint32), np.zeros(C, np.uint32))          # +0.0, not -0.0
            norms = np.sqrt(np.square(th[w0:b0].reshape(K, C).astype(np.float64)).sum(axis=0))
            assert np.all(np.abs(norms - 1.0) <= ((K + 1) / 2 + 3) * U * 1.01), (K, C, np.abs(norms - 1.0).max())
        w0, K, C, b0 = S.blocks(kind, H, O)[0][2]
        assert abs(np.linalg.norm(th[w0:b0].reshape(K, C)[:, 0].astype(np.float64)) - 0.01) > 0.9                # `out` at 1, not 0.01


def test_a_zero_column_is_nan_on_both_sides_at_the_same_places():
    from dne_hip import _lib
    kind, H, O = S.KIND_MJMAZE, 64, 4
    tab = S.zero_column_table(kind, H, O, 777, 2, 3)
    th = _lib.mujoco_ga_theta_host(tab, kind, H, O, (777, (5, 0.02)))
    w0, K, C, _ = S.blocks(kind, H, O)[0][2]
    want = np.zeros(th.size, bool)
    want[w0 + 3 + C * np.arange(K)] = True
    assert np.array_equal(np.isnan(th), want) and S.same(th, S.genome_np(tab, kind, H, O, (777, (5, 0.02))))


# ---- 3. genomes and promotions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,O", [(S.KIND_PENDULUM, 64, 1), (S.KIND_PENDULUM, 64, 16), (S.KIND_MJMAZE, 64, 2), (S.KIND_MJMAZE, 128, 4)])
def test_a_genome_is_its_root_followed_by_promotions(kind, H, O):
    """chains of 1..4 seeds built at once (theta_host, build) equal the numpy statement, and equal the same chains grown one seed a promotion:
    kept parents that move, two descriptors naming one source, a root among the descriptors, T from 1 to T_max"""
    from dne_hip import _lib
    tab, sigma, T_max = S.table(), 0.02, 5
    P = S.num_params(kind, H, O)
    rs = np.random.RandomState(5 + O)
    seeds = [int(v) for v in rs.randint(0, tab.size - P + 1, size=12)] + [0, tab.size - P]
    chains = [tuple(seeds[j:j + n]) for j, n in ((0, 1), (1, 2), (3, 3), (6, 4), (12, 2))]
    for c in chains:
        assert S.same(_lib.mujoco_ga_theta_host(tab, kind, H, O, S.chain_genome(c, sigma)), S.genome_np(tab, kind, H, O, S.chain_genome(c, sigma)))
    e = S.host_engine(kind, H, O, ac_mode="continuous" if O in (1, 2) and (kind, O) != (S.KIND_PENDULUM, 2) else "uniform")
    e.mujoco_ga_reserve(T_max)
    for T in range(1, T_max + 1):
        e.mujoco_ga_build([S.chain_genome(c, sigma) for c in chains[:T]])
        assert e.mujoco_ga_parents() == T
        for j in range(T):
            assert S.same(e.mujoco_ga_get_parent(j), S.genome_np(tab, kind, H, O, S.chain_genome(chains[j], sigma)))
    # generation by generation from one-seed roots: bank = [a], then [a, a+b, a+c, r], then moved and doubled, then grown again
    a, b, c, d, r = seeds[0], seeds[1], seeds[2], seeds[3], seeds[13]
    e.mujoco_ga_build([(a, )])
    e.mujoco_ga_promote([0, 0, 0, -1], [-1, b, c, r], [0.0, sigma, sigma, 9.0])
    want = [(a, ), (a, b), (a, c), (r, )]
    e.mujoco_ga_promote([2, 1, 1, 3, 0], [-1, -5, d, b, -1], [0.0, 0.0, sigma, sigma, 0.0])   # kept parents move; source 1 named twice
    want = [want[2], want[1], want[1] + (d, ), want[3] + (b, ), want[0]]
    e.mujoco_ga_promote([2], [c], [sigma])                                                       # T back to 1, a chain of four
    want = [want[2] + (c, )]
    assert e.mujoco_ga_parents() == 1 and len(want[0]) == 4
    assert S.same(e.mujoco_ga_get_parent(0), _lib.mujoco_ga_theta_host(tab, kind, H, O, S.chain_genome(want[0], sigma)))
    assert S.same(e.mujoco_ga_get_parent(0), S.genome_np(tab, kind, H, O, S.chain_genome(want[0], sigma)))
    # the descriptors against numpy, the kept form bit for bit
    bank = np.stack([S.genome_np(tab, kind, H, O, S.chain_genome(ch, sigma)) for ch in chains[:3]])
    parent, idx, power = np.array([-1, 0, 2, 1, 1], np.int32), np.array([tab.size - P, 0, tab.size - P, -1, -77], np.int64), np.array([3.0, 0.0, -0.02, 1.0, 0.0], np.float32)
    got = _lib.mujoco_ga_members_host(tab, kind, H, O, bank, parent, idx, power)
    assert S.same(got, S.members_np(tab, kind, H, O, bank, parent, idx, power))
    assert np.array_equal(got[3].view(np.uint32), bank[1].view(np.uint32)) and np.array_equal(got[4].view(np.uint32), bank[1].view(np.uint32))


# ---- 4. the policy ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_policy_reinitialize_and_set_from_seeds_are_the_twin(kind):
    from dne_hip import _lib, es, ga_mujoco
    exp = S.ga_exp(kind)
    e = S.host_engine(kind)
    config, env, policy = ga_mujoco.setup(exp, engine=e)
    tab = S.table()
    P = policy.num_params
    policy.set_trainable_flat(tab[31:31 + P])
    policy.reinitialize()
    assert S.same(policy.get_trainable_flat(), _lib.mujoco_ga_theta_host(tab, kind, 64, policy.n_out, (31, )))
    assert S.same(policy.get_trainable_flat(), S.root_np(tab, kind, 64, policy.n_out, 31))
    chain = [31, 4000, tab.size - P, 9]
    got = policy.set_from_seeds(chain, 0.02, tab)
    # ga.py:152-158 in numpy: reinitialise on the first slice, then v += noise_stdev * noise.get(seed) per further seed
    v = S.root_np(tab, kind, 64, policy.n_out, 31)
    for s in chain[1:]:
        v = (v + np.float32(0.02) * tab[s:s + P]).astype(np.float32)
    assert S.same(got, v) and S.same(policy.get_trainable_flat(), v) and S.same(e.theta, v)
    nt = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    nt.noise = tab
    assert S.same(policy.set_from_seeds(chain[:1], 0.02, nt), S.root_np(tab, kind, 64, policy.n_out, 31))
    with pytest.raises(TypeError):                      # the table is a required argument: a policy holds none
        policy.set_from_seeds(chain, 0.02)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_host_refusals_by_their_words():
    from dne_hip import _lib
    tab = S.table(70000)
    kind, H, O = S.KIND_PENDULUM, 64, 1
    P = S.num_params(kind, H, O)
    bank = np.zeros((2, P), np.float32)

    def refused(f, *a):
        with pytest.raises(_lib.DneError) as ei:
            f(*a)
        return str(ei.value)
    m = _lib.mujoco_ga_members_host
    assert refused(m, tab, kind, H, O, bank, [2], [0], 0.1) == "dne_mujoco_ga_members_host: member 0: parent 2, the bank holds 2"
    assert refused(m, tab, kind, H, O, None, [0], [0], 0.1) == "dne_mujoco_ga_members_host: member 0: parent 0 on an empty bank"
    assert refused(m, tab, kind, H, O, bank, [0, -1], [0, tab.size - P + 1], 0.1) == \
        "dne_mujoco_ga_members_host: member 1: noise index %d + P = %d outside the table of %d" % (tab.size - P + 1, P, tab.size)
    assert refused(m, tab, kind, H, O, bank, [-1], [-1], 0.1) == "dne_mujoco_ga_members_host: member 0: a root needs a noise index, got -1"
    assert refused(m, tab, kind, H, O, bank, [-2], [0], 0.1) == "dne_mujoco_ga_members_host: member 0: parent -2 (-1 is a root, 0 .. T - 1 a parent)"
    t = _lib.mujoco_ga_theta_host
    assert refused(t, tab, kind, H, O, ()) == "dne_mujoco_ga_theta_host: genome 0: empty chain"
    assert refused(t, tab, kind, H, O, (0, (tab.size, 0.1))) == \
        "dne_mujoco_ga_theta_host: genome 0: noise index %d + P = %d outside the table of %d" % (tab.size, P, tab.size)
    assert refused(t, tab[:P - 1], kind, H, O, (0, )) == "dne_mujoco_ga_theta_host: a table of %d floats holds no P = %d parameters" % (P - 1, P)
    assert refused(_lib.mujoco_ga_colscale_host, tab, kind, H, O, -1) == \
        "dne_mujoco_ga_colscale_host: noise index -1 + P = %d outside the table of %d" % (P, tab.size)
    # another kind, a shape the headers do not build: the C side's words
    lib, buf = _lib.load(), np.zeros(4, np.float32)
    ptr = _lib._ptr(tab, _lib.C.c_float)
    assert lib.dne_mujoco_ga_colscale_host(ptr, tab.size, _lib.KIND_MAZE, 64, 2, 0, _lib._ptr(buf, _lib.C.c_float)) == -1
    assert lib.dne_last_error(None).decode() == "dne_mujoco_ga_colscale_host: kind 4 runs no MujocoPolicy (DNE_KIND_PENDULUM (6) and DNE_KIND_MJMAZE (7) do)"
    assert lib.dne_mujoco_ga_colscale_host(ptr, tab.size, _lib.KIND_MJMAZE, 64, 3, 0, _lib._ptr(buf, _lib.C.c_float)) == -1
    assert lib.dne_last_error(None).decode() == "dne_mujoco_ga_colscale_host: hidden width 64 with 3 outputs is not a shape csrc/mjmaze.h builds"
    assert "is not a MujocoPolicy shape" in refused(t, tab, _lib.KIND_MAZE, H, O, (0, ))
    # the host engine: before reserve, T > T_max, the kept form in an evaluation, no walls, statistics unset
    e = S.host_engine(S.KIND_MJMAZE)
    assert refused(e.mujoco_ga_build, [(0, )]) == "dne_mujoco_ga_build: no bank (dne_mujoco_ga_reserve comes first)"
    e.mujoco_ga_reserve(2)
    assert refused(e.mujoco_ga_build, [(0, ), (1, ), (2, )]) == "dne_mujoco_ga_build: T = 3 outside [1, T_max = 2]"
    e.mujoco_ga_build([(0, )])
    assert "the kept form is for promotion only" in refused(e.mujoco_ga_eval, [0], [-1], [0.0], 20)
    assert "the observation statistics of a DNE_KIND_MJMAZE engine are NaN" in refused(e.mujoco_ga_eval, [0], [5], [0.02], 20)
    e.maze = None
    assert "no maze loaded" in refused(e.mujoco_ga_eval, [0], [5], [0.02], 20)
    p = S.host_engine(S.KIND_PENDULUM)
    p.mujoco_ga_reserve(1)
    S.set_stat(p, S.KIND_PENDULUM)
    assert "env_seed is NULL" in refused(p.mujoco_ga_eval, [-1], [5], [0.0], 20)


@pytest.mark.parametrize("kind", KINDS)
def test_ga_setup_still_refuses_the_policy_and_points_to_the_module(kind):
    from dne_hip import ga
    with pytest.raises(NotImplementedError, match="ga with MujocoPolicy is not built") as ei:
        ga.setup(S.ga_exp(kind))
    assert "dne_hip.ga_mujoco" in str(ei.value)


# ---- 6. the drivers --------------------------------------------------------------------------------------------------------------------------------------
_runs = {}


def driver_run(kind, tmp_path_factory, bank_reuse=True):
    from dne_hip import es
    key = (kind, bank_reuse)
    if key not in _runs:
        noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
        noise.noise, noise._engines = S.table(), []
        exp = S.ga_exp(kind, pop=8, population_size=4, num_elites=2, calc_obstat_prob=0.5)
        me, we = S.host_engine(kind, count=0), S.host_engine(kind, count=0)
        run = S.run_ga(exp, me, we, noise, tmp_path_factory.mktemp("ga_mujoco"), 3, bank_reuse=bank_reuse)
        _runs[key] = (exp, we, run)
    return _runs[key]


@pytest.mark.parametrize("kind", KINDS)
def test_three_iterations_of_the_drivers_on_the_host_engine(kind, tmp_path_factory):
    from dne_hip import _lib, es
    exp, we, run = driver_run(kind, tmp_path_factory)
    tab, sigma, n_out = S.table(), exp["config"]["noise_stdev"], 1 if kind == S.KIND_PENDULUM else 2
    steps, n_obs = (200, 3) if kind == S.KIND_PENDULUM else (400, 11)
    shards = [(t, r) for t, r in run["pushed"] if r.eval_length is None]
    evals = [(t, r) for t, r in run["pushed"] if r.eval_length is not None]
    assert [t for t, _ in shards] == [0, 1, 2] and len(evals) == 3 and len(we.evals) == 3
    # decision (a): every task carries mean 0 and std 1; decision (d): the eval episode runs the environment's own limit
    for task in run["tasks"]:
        assert np.array_equal(task.ob_mean, np.zeros(n_obs, np.float32)) and np.array_equal(task.ob_std, np.ones(n_obs, np.float32))
        assert task.timestep_limit is None
    assert all(r.eval_length == steps for _, r in evals)
    assert run["tasks"][0].population == [] and all(len(t.population) == 4 for t in run["tasks"][1:])
    # every pushed Result: the chains extend a member of the task's population by one index, theta is the chain's genome, the returns and
    # lengths are the evaluation's, the statistics the flagged episodes' sums in member order
    flagged = 0
    for (tid, r), ev, task in zip(shards, we.evals, run["tasks"]):
        pop = [list(c) for c in task.population]
        assert len(r.noise_inds_n) == 8 and r.returns_n2.dtype == np.float32 and r.lengths_n2.dtype == np.int32
        for i, chain in enumerate(r.noise_inds_n):
            assert (chain[:-1] in pop) if pop else len(chain) == 1
            assert S.same(ev["thetas"][i], S.genome_np(tab, kind, 64, n_out, S.chain_genome(chain, sigma)))
        assert np.array_equal(r.returns_n2, ev["returns"]) and np.array_equal(r.lengths_n2, ev["lengths"]) and (r.lengths_n2 == steps).all()
        n, std, off, flag = ev["options"]
        assert n == 8 and std == 0.01 and off is not None and (off + steps * (1 if kind == S.KIND_PENDULUM else 2) <= tab.size).all()
        if flag.any():
            s, q, c = es.flagged_ob_stats(ev["ob"], flag.astype(bool))
            assert r.ob_count == steps * int(flag.sum()) == c and np.array_equal(r.ob_sum, s) and np.array_equal(r.ob_sumsq, q) and r.ob_sum.dtype == np.float32
            flagged += 1
        else:
            assert r.ob_count == 0 and r.ob_sum is None and r.ob_sumsq is None
    assert flagged > 0, "no coin landed: choose another worker seed"
    # the population order is truncate's: (-return, arrival) over the elites with their old scores, then the children
    pop, score = [], np.zeros(0, np.float32)
    for k, (tid, r) in enumerate(shards):
        cand = [list(c) for c in pop[:2]] + [list(c) for c in r.noise_inds_n]
        ret = np.concatenate([score[:2], r.returns_n2]).astype(np.float32)
        order = np.argsort(-ret, kind="stable")[:4]
        pop, score = [cand[i] for i in order], ret[order]
        later = run["tasks"][k + 1].population if k + 1 < len(run["tasks"]) else run["population"]
        assert [list(c) for c in later] == pop
    assert np.array_equal(run["scores"], score)
    # the elite's theta
    assert S.same(run["theta"], _lib.mujoco_ga_theta_host(tab, kind, 64, n_out, S.chain_genome(run["population"][0], sigma)))
    assert S.same(run["tasks"][2].params, _lib.mujoco_ga_theta_host(tab, kind, 64, n_out, S.chain_genome(run["tasks"][2].population[0], sigma)))
    # the bank was reused: built once (the first population), promoted afterwards
    assert [c[0] for c in we.ga_calls] == ["reserve", "eval", "build", "eval", "promote", "eval"]


@pytest.mark.parametrize("kind", KINDS)
def test_the_bank_route_equals_rebuilding_every_parent_from_its_genome(kind, tmp_path_factory):
    _, we, run = driver_run(kind, tmp_path_factory)
    _, we2, run2 = driver_run(kind, tmp_path_factory, bank_reuse=False)
    assert [c[0] for c in we2.ga_calls] == ["reserve", "eval", "build", "eval", "build", "eval"]
    S.assert_same_ga_runs(run, run2, "bank reuse against rebuilding")
    for a, b in zip(we.evals, we2.evals):
        assert S.same(a["thetas"], b["thetas"])
    assert S.same(we.bank, we2.bank)


# ---- 7. the header under AddressSanitizer and UBSan, in a program of its own ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/mujoco_ga_asan_main.cpp, built once: address, undefined and float-cast-overflow"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(ROOT, "tests", "mujoco_ga_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("mujoco_ga_asan") / "mujoco_ga_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program):
    out = subprocess.run([sanitizer_program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    # 3 widths x (16 + 8) output counts
    assert out.stdout.split()[:2] == ["ok", "72"] and int(out.stdout.split()[2]) > 100000, out.stdout
