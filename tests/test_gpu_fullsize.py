"""GPU, BASELINE.json full sizes (pop 5000 = 2500 antithetic pairs, the 250M-entry noise table, P = 1 009 058):
size-independent properties + spot checks against the oracle, where a full oracle run would take hours."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PAIRS, NACT = 2500, 18
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def full(oracle, noise_table):
    from dne_hip import _lib, es, policies
    noise = noise_table                                              # es.py:51-61, 250M entries
    e = _lib.Engine(_lib.KIND_ES, NACT, max_members=2 * N_PAIRS, ref_count=128)
    noise.attach(e)
    th = policies.xavier_flat(NACT, 0)
    e.set_theta(th)
    ref = oracle.get_ref_batch(seed=0, batch_size=128, nact=NACT)
    e.set_ref_batch(ref)
    yield e, noise, th, ref
    e.close()


def test_noise_table_golden(full, golden):
    _, noise, _, _ = full
    assert noise.noise.size == 250_000_000
    assert noise.noise[:8].view(np.uint32).tolist() == [3213555186, 1065308680, 1049682575, 3217083972, 3205766949,
                                                        1070817862, 3223015094, 3202062960]
    assert noise.noise[-3:].view(np.uint32).tolist() == [3158718917, 3219242230, 1075127793]
    if "noise_full_sha256" in golden.files:
        import hashlib
        assert hashlib.sha256(noise.noise.tobytes()).digest() == golden["noise_full_sha256"].tobytes()


def test_aggregate_properties_full_size(full, oracle):
    e, noise, th, _ = full
    P = e.P
    srs = np.random.RandomState(0)
    idx = np.array([noise.sample_index(srs, P) for _ in range(N_PAIRS)], np.int64)
    assert idx[:4].tolist() == [209652396, 130329135, 118924917, 136432832]
    rets = (10 * np.random.RandomState(1).poisson(20, (N_PAIRS, 2))).astype(np.float32)               # SURVEY 8d aggregate micro-benchmark
    proc = e.centered_ranks(rets)
    assert np.array_equal(proc, oracle.centered_ranks(rets.reshape(-1)).reshape(rets.shape))
    assert proc.min() == -0.5 and proc.max() == 0.5 and abs(float(proc.sum())) < 1e-3
    w = proc[:, 0] - proc[:, 1]
    g = e.weighted_sum(idx, w, rets.size)
    assert g.shape == (P,) and g.dtype == np.float32                                                   # es.py:297
    # one-hot weights select exactly one slice; homogeneity; antisymmetry; additivity within fp32 round-off
    onehot = np.zeros(N_PAIRS, np.float32); onehot[1234] = 1.0
    assert np.array_equal(e.weighted_sum(idx, onehot, 1.0), noise.get(idx[1234], P))
    assert np.array_equal(e.weighted_sum(idx, -w, rets.size), -g)
    assert np.array_equal(e.weighted_sum(idx, 2 * w, rets.size), 2 * g)
    half = w.copy(); half[N_PAIRS // 2:] = 0
    rest = w - half
    gs = e.weighted_sum(idx, half, rets.size) + e.weighted_sum(idx, rest, rets.size)
    assert np.abs(gs - g).max() < 1e-5 * max(1.0, np.abs(g).max())
    # spot check 4096 parameters against the reference formulation in float64
    ps = np.random.RandomState(2).randint(0, P, 4096)
    ref = np.zeros(4096)
    for i in range(N_PAIRS):
        ref += float(w[i]) * noise.noise[idx[i] + ps].astype(np.float64)
    assert np.abs(g[ps] - ref / rets.size).max() < 1e-5
    # full update vs the oracle's Adam on the same g
    e.optimizer_reset(); e.set_theta(th)
    e.es_update(idx, rets, None, "centered_rank", "adam", 0.005, 0.01)
    opt = oracle.Adam(th, 0.01)
    _, oth = opt.update(g, 0.005)
    assert np.array_equal(e.get_theta(), oth)
    e.set_theta(th)


def test_materialize_full_table(full):
    e, noise, th, _ = full
    idx = np.array([0, 248_990_942, 125_000_001], np.int64)          # first, last legal and an odd-aligned index
    out = e.materialize(idx, 0.02)
    for i, ix in enumerate(idx):
        v = np.float32(0.02) * noise.get(ix, e.P)
        assert np.array_equal(out[i, 0], th + v) and np.array_equal(out[i, 1], th - v)
    assert np.abs((out[:, 0] + out[:, 1]) / 2 - th).max() < 1e-5     # gpu_implementation/es.py:182-183
    with pytest.raises(Exception):
        e.materialize(np.array([248_990_943], np.int64), 0.02)        # one past the last legal index


def test_population_eval_properties(full, oracle):
    from dne_hip import es
    e, noise, th, ref = full
    L = oracle.layout(oracle.KIND_ES, NACT)
    tslimit = 40
    _, idx, seeds = es.generation_inputs(noise.noise.size, e.P, N_PAIRS, 0, 0, 1)
    ret, sg, ln = e.es_eval(idx, 0.02, tslimit, seeds)
    assert ret.shape == sg.shape == ln.shape == (N_PAIRS, 2) and ret.dtype == np.float32 and ln.dtype == np.int32
    assert ln.min() >= 1 and ln.max() <= tslimit
    assert np.all(ret >= 0) and np.all(np.mod(ret, 10) == 0)         # SynthAtari rewards are multiples of 10
    assert np.all(sg <= ret / 10 + 1e-6) and np.all((sg > 0) == (ret > 0))
    ret2, sg2, ln2 = e.es_eval(idx, 0.02, tslimit, seeds)            # idempotent: no hidden state between evaluations
    assert np.array_equal(ret, ret2) and np.array_equal(sg, sg2) and np.array_equal(ln, ln2)
    # permutation equivariance: a member's result does not depend on its slot or on which sub-batch stream ran it
    perm = np.random.RandomState(3).permutation(N_PAIRS)
    retp, sgp, lnp = e.es_eval(idx[perm], 0.02, tslimit, seeds.reshape(-1, 2)[perm].reshape(-1))
    assert np.array_equal(retp, ret[perm]) and np.array_equal(lnp, ln[perm]) and np.array_equal(sgp, sg[perm])
    # spot-check pairs against the oracle
    for i in (0, 1249, 1250, 2499, 777):
        oret, osg, oln = oracle.es_eval(L, th, noise.noise, idx[i:i + 1], 0.02, tslimit, ref, seeds[2 * i:2 * i + 2])
        assert np.array_equal(oret[0], ret[i]) and np.array_equal(oln[0], ln[i]) and np.array_equal(osg[0], sg[i]), i


BENCH_CONFIG = dict(l2coeff=0.005, noise_stdev=0.02, episodes_per_batch=5000, timesteps_per_batch=10000, calc_obstat_prob=0.0,
                    eval_prob=0.0, snapshot_freq=0, return_proc_mode="centered_rank", episode_cutoff_mode=5000)
BENCH_OPT = {"type": "adam", "args": {"stepsize": 0.01}}


def test_bench_config_soak(full):
    """bench.py's exact path (pop 5000, tslimit 5000, events on, device-resident exchange + update) for six consecutive
    generations in one process: the profile's invariants hold, no kernel writes outside its buffer, and generation 0 equals
    the same generation on the engine without events (the profiled and unprofiled launch sequences give the same bits)."""
    from dne_hip import _lib, es
    e0, noise, th, ref = full
    cfg = es.Config(**BENCH_CONFIG)
    e = _lib.Engine(_lib.KIND_ES, NACT, max_members=2 * N_PAIRS, ref_count=128, profile_events=True)
    try:
        noise.attach(e)
        assert np.array_equal(e.noise_get(249_000_000, 4096), noise.noise[249_000_000:249_004_096])   # staged upload, far end
        e.set_theta(th); e.set_ref_batch(ref); e.optimizer_reset()
        first = None
        for gen in range(6):
            rec, ratio = es.es_generation(e, noise.noise.size, cfg, N_PAIRS, gen, 5000, BENCH_OPT)
            p = e.profile()
            assert rec["len"].min() >= 1 and rec["len"].max() <= 5000
            assert p["env_steps"] == rec["len"].sum()
            assert 0 < p["fc_full_units"] <= p["env_steps"]                        # profiled launches cover a subset of the steps
            assert 0 < p["fc_full_union_ms"] <= p["eval_ms"] * 1.001 and p["fc_full_union_ms"] <= p["fc_full_ms"] * 1.001
            assert 0 < p["ref_ms"] < p["eval_ms"] and p["fc_full_kind"] == 5      # the table-ordered streaming kernel (k_fc_ring)
            assert p["fc_full_launches"] >= 3 and np.isfinite(ratio) and ratio > 0
            if first is None:
                first = rec.copy()
        assert np.isfinite(e.get_theta()).all()
        assert e.check_redzones() == 0
        # generation 0 again on the unprofiled engine, through the host-array update entry point
        e0.set_theta(th); e0.optimizer_reset()
        _, idx, seeds = es.generation_inputs(noise.noise.size, e0.P, N_PAIRS, 0, 0, 1)
        ret, sg, ln = e0.es_eval(idx, 0.02, 5000, seeds)
        assert np.array_equal(first["noise_idx"], idx) and np.array_equal(first["ret"], ret)
        assert np.array_equal(first["len"], ln) and np.array_equal(first["aux"], sg)
        e0.set_theta(th)
        assert e0.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.slow
@pytest.mark.timeout(1500)
def test_full_generation_bit_exact(full, oracle, oracle_es_gen0):
    """Generation 0 of config 2 in full -- all 2500 x 2 returns, sign-returns and lengths, and theta after the update --
    against the CPU oracle run over every usable host core (conftest.oracle_es_gen0, shared with the NS-ES test;
    es.py:246-248, 297)."""
    from dne_hip import es
    e, noise, th, ref = full
    _, idx, seeds = es.generation_inputs(noise.noise.size, e.P, N_PAIRS, 0, 0, 1)
    o = oracle_es_gen0
    assert np.array_equal(o["idx"], idx) and np.array_equal(o["seeds"], seeds) and np.array_equal(o["ref"], ref)
    e.set_theta(th); e.optimizer_reset()
    ret, sg, ln = e.es_eval(idx, 0.02, 5000, seeds)
    rec = e.allgather_results(N_PAIRS, N_PAIRS)
    assert np.array_equal(rec["noise_idx"], idx) and np.array_equal(rec["ret"], ret) and np.array_equal(rec["len"], ln)
    e.es_update_gathered("centered_rank", "adam", 0.005, 0.01)
    theta_gpu = e.get_theta()
    e.set_theta(th); e.optimizer_reset()
    assert np.array_equal(ln, o["ln"]), np.flatnonzero((ln != o["ln"]).any(axis=1))[:8]
    assert np.array_equal(ret, o["ret"]) and np.array_equal(sg, o["sg"])
    assert ret.shape == ln.shape == (N_PAIRS, 2) and ret.dtype == np.float32                      # es.py:246-248
    g = oracle.es_gradient(noise.noise, idx, o["ret"], e.P)
    assert g.shape == (e.P,) and g.dtype == np.float32                                              # es.py:297
    _, oth = oracle.Adam(th, 0.01).update(g, 0.005)
    assert np.array_equal(theta_gpu, oth)


@pytest.mark.slow
@pytest.mark.timeout(2400)
def test_generations_past_zero_bit_exact(full, oracle, oracle_es_gen0):
    """Parity past generation 0 (es.py:193-353 runs generation after generation on an evolving theta and a carried Adam state,
    optimizers.py:36-50).  Generations 0, 1, 2 of config 2 through es.es_generation -- the bench's path: device-resident exchange +
    update -- with the CPU oracle over every host core per generation: all 2500 x 2 returns / sign-returns / lengths of every
    generation, theta after every update, Adam's m, v, t after generation 2.  Then the GPU alone runs on to the end of the bench's
    warm-up (generations 3, 4) and generation 5 -- the first one bench.py times -- is checked again, the oracle starting from the
    engine's theta and optimizer state at that point: the episode-length mix, the 451 .. 799-pair k_fc_duo launches and the 32-step
    compaction of the timed region, value by value."""
    import hashlib
    import oracle_pool
    from dne_hip import es
    e, noise, th, ref = full
    cfg = es.Config(**BENCH_CONFIG)
    e.set_theta(th); e.optimizer_reset()
    try:
        opt = oracle.Adam(th, BENCH_OPT["args"]["stepsize"])
        oth = th

        def check(gen, oret, osg, oln):
            nonlocal oth
            _, idx, _ = es.generation_inputs(noise.noise.size, e.P, N_PAIRS, gen, 0, 1)
            rec, ratio = es.es_generation(e, noise.noise.size, cfg, N_PAIRS, gen, 5000, BENCH_OPT)
            assert np.array_equal(rec["noise_idx"], idx)
            assert np.array_equal(rec["len"], oln), (gen, np.flatnonzero((rec["len"] != oln).any(axis=1))[:8])
            assert np.array_equal(rec["ret"], oret) and np.array_equal(rec["aux"], osg), gen
            g = oracle.es_gradient(noise.noise, idx, oret, e.P)
            oratio, t2 = opt.update(g, cfg.l2coeff)
            oth = t2.copy()
            assert np.array_equal(e.get_theta(), oth), gen
            assert np.isfinite(ratio) and abs(ratio - oratio) <= 1e-4 * abs(oratio)
            return int(rec["len"].sum())

        o = oracle_es_gen0
        assert np.array_equal(o["ref"], ref)
        steps = [check(0, o["ret"], o["sg"], o["ln"])]
        for gen in (1, 2):
            _, idx, seeds = es.generation_inputs(noise.noise.size, e.P, N_PAIRS, gen, 0, 1)
            oret, osg, oln, _ = oracle_pool.es_generation(noise.noise, oth, ref, idx, seeds, cfg.noise_stdev, 5000, NACT)
            steps.append(check(gen, oret, osg, oln))
        m, v, t = e.optimizer_get_state()
        assert t == 3 == opt.t and np.array_equal(m, opt.m) and np.array_equal(v, opt.v)
        # the rest of bench.py's warm-up on the GPU alone, then its first timed generation against the oracle
        for gen in (3, 4):
            es.es_generation(e, noise.noise.size, cfg, N_PAIRS, gen, 5000, BENCH_OPT)
        oth = e.get_theta()
        m, v, t = e.optimizer_get_state()
        assert t == 5
        opt = oracle.Adam(oth, BENCH_OPT["args"]["stepsize"]); opt.m[:] = m; opt.v[:] = v; opt.t = t
        print("theta after 5 warm-up generations sha256", hashlib.sha256(oth.tobytes()).hexdigest())
        _, idx, seeds = es.generation_inputs(noise.noise.size, e.P, N_PAIRS, 5, 0, 1)
        oret, osg, oln, _ = oracle_pool.es_generation(noise.noise, oth, ref, idx, seeds, cfg.noise_stdev, 5000, NACT)
        steps.append(check(5, oret, osg, oln))
        m, v, t = e.optimizer_get_state()
        assert t == 6 and np.array_equal(m, opt.m) and np.array_equal(v, opt.v)
        print("env-steps per generation (0, 1, 2, 5):", steps)
        assert e.check_redzones() == 0
    finally:
        e.set_theta(th); e.optimizer_reset()


def test_ga_full_size_properties(oracle, noise_table):
    """Config 3 at full size: 1000 children, top-20 truncation, 250M table (ga.py:136-149, 251-271).  Generation 0 (every
    child its own normc genome) and a generation of children of 20 cached parents: idempotent, independent of the slot a
    child is evaluated in, spot-checked against the oracle; selection equals the oracle's on the full return vector; the
    parent cache rebuilds nothing it already holds."""
    from dne_hip import _lib, es, ga
    n, T, sigma, tslimit = 1000, 20, 0.005, 60
    noise = noise_table
    e = _lib.Engine(_lib.KIND_GA, NACT, max_members=n)
    try:
        noise.attach(e)
        L = oracle.layout(oracle.KIND_GA, NACT)
        pop, score = [], np.array([], np.float32)
        for gen in range(2):
            pop, score, ln = ga.ga_generation(e, noise.noise.size, sigma, pop, score, n, T, 1, gen, tslimit)
            assert len(pop) == T and np.all(np.diff(score) <= 0) and ln.min() >= 1 and ln.max() <= tslimit
            assert all(len(c) == gen + 1 for c in pop[1 if gen else 0:])          # children of generation g carry g + 1 seeds
        # generation 1 again, by hand: results do not depend on the slot or on the parent cache
        mine, parent, fresh, env_seeds = ga.ga_generation_inputs(noise.noise.size, e.P, n, T, 5, 0, 1)
        chains = [list(pop[p]) + [int(f)] for p, f in zip(parent, fresh)]
        ret, sg, ln = e.ga_eval(chains, sigma, tslimit, env_seeds)
        ret2, sg2, ln2 = e.ga_eval(chains, sigma, tslimit, env_seeds)
        assert np.array_equal(ret, ret2) and np.array_equal(ln, ln2) and np.array_equal(sg, sg2)
        perm = np.random.RandomState(4).permutation(n)
        retp, _, lnp = e.ga_eval([chains[i] for i in perm], sigma, tslimit, env_seeds[perm])
        assert np.array_equal(retp, ret[perm]) and np.array_equal(lnp, ln[perm])
        for i in (0, 499, 999):
            r = oracle.rollout(L, oracle.ga_rebuild(L, noise.noise, chains[i], sigma), None, env_seeds[i], tslimit)
            assert (ret[i], sg[i], ln[i]) == r[:3], i
        sel = e.ga_select(ret, T)
        assert np.array_equal(sel, oracle.ga_select(ret, T)) and len(set(sel.tolist())) == T
        assert e.check_redzones() == 0
    finally:
        e.close()


def _oracle_child(i):
    import oracle as O
    noise, chains, seeds, sigma = _ORACLE_GA
    L = O.layout(O.KIND_GA, NACT)
    return O.rollout(L, O.ga_rebuild(L, noise, chains[i], sigma), None, seeds[i], 5000)[:3]


@pytest.mark.slow
@pytest.mark.timeout(1800)
def test_ga_full_generation_bit_exact(oracle, noise_table):
    """Config 3 in full: generations 0 and 1 of the Deep GA at 1000 children, tslimit 5000, 250M table -- every child's
    return, sign-return and length, and the 20 survivors of the truncation with their scores, against the CPU oracle run over
    every host core (ga.py:136-149, 251-271; about half a minute per generation on the GPU box's host)."""
    import multiprocessing as mp
    from dne_hip import _lib, es, ga
    global _ORACLE_GA
    n, T, sigma = 1000, 20, 0.005
    noise = noise_table
    e = _lib.Engine(_lib.KIND_GA, NACT, max_members=n)
    try:
        noise.attach(e)
        import oracle_pool
        cores = oracle_pool.workers()
        pop, score = [], np.array([], np.float32)
        for gen in range(2):
            mine, parent, fresh, env_seeds = ga.ga_generation_inputs(noise.noise.size, e.P, n, len(pop), gen, 0, 1)
            chains = [(list(pop[p]) if p >= 0 else []) + [int(f)] for p, f in zip(parent, fresh)]
            ret, sg, ln = e.ga_eval(chains, sigma, 5000, env_seeds)
            _ORACLE_GA = (noise.noise, chains, env_seeds, sigma)
            with mp.get_context("fork").Pool(cores) as pool:
                out = pool.map(_oracle_child, range(n), chunksize=1)
            oret = np.array([o[0] for o in out], np.float32); osg = np.array([o[1] for o in out], np.float32)
            oln = np.array([o[2] for o in out], np.int32)
            assert np.array_equal(ln, oln), (gen, np.flatnonzero(ln != oln)[:8])
            assert np.array_equal(ret, oret) and np.array_equal(sg, osg), gen
            assert ln.max() <= 5000 and ln.min() >= 1
            # the driver's generation (same inputs) and the oracle's truncation of the same candidates: elite first (old score,
            # ga.py:136-137), then the children in arrival order; survivors ordered by (-return, arrival)
            new_pop, new_score, ln2 = ga.ga_generation(e, noise.noise.size, sigma, pop, score, n, T, 1, gen, 5000)
            assert np.array_equal(ln2, ln)
            cand = [list(c) for c in pop[:1]] + chains
            cand_ret = np.concatenate([score[:1], oret]).astype(np.float32)
            osel = oracle.ga_select(cand_ret, T)
            assert [cand[i] for i in osel] == [list(c) for c in new_pop] and np.array_equal(cand_ret[osel], new_score)
            assert new_score[0] == cand_ret.max()                                                  # ga.py:149
            pop, score = new_pop, new_score
        assert e.check_redzones() == 0
    finally:
        e.close()


def _bench(argv, timeout=800):
    import subprocess
    import sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    import json
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                         # ONE JSON line, from rank 0
    return json.loads(lines[0]), r.stderr


SMALL = ["--steps", "2", "--warmup", "1", "--pop", "96", "--tslimit", "40", "--noise-count", "4000000", "--no-cpu-baseline"]


@pytest.mark.timeout(900)
def test_two_ranks_one_gpu_bit_identical_theta():
    """bench.py's N > 1 path through its OWN launcher (python bench.py --gpus 2, no wrapper) with two ranks sharing this box's
    one GPU (records exchanged over gloo, since RCCL refuses two ranks on one device): the population is sharded round-robin,
    every rank runs the redundant update, and theta ends bit-identical on both ranks.  The same through an external launcher
    (torch.distributed.run), and the one-rank run's plumbing (supervised child, JSON line)."""
    import re
    import sys
    b = os.path.join(ROOT, "bench.py")
    d2, err = _bench([sys.executable, b, "--gpus", "2", "--transport", "gloo", "--single-device", "--extra", "none"] + SMALL)
    shas = re.findall(r"\[bench r(\d) .*theta sha256 ([0-9a-f]{64})", err)
    assert sorted(r for r, _ in shas) == ["0", "1"] and len({h for _, h in shas}) == 1, shas
    assert d2["n_gpus"] == 2 and d2["config"]["pairs_per_gpu"] == 24 and d2["value"] > 0
    assert d2["comm"]["carrier"] == "gloo" and d2["comm"]["launcher"] == "self" and "gloo" in d2["config"]["parallelism"]
    port = str(29600 + os.getpid() % 300)
    d2x, errx = _bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", port, b, "--gpus", "2", "--transport", "gloo", "--single-device", "--extra", "none"] + SMALL)
    shasx = re.findall(r"\[bench r(\d) .*theta sha256 ([0-9a-f]{64})", errx)
    assert {h for _, h in shasx} == {h for _, h in shas}             # same generations, same theta whoever launched the ranks
    assert d2x["comm"]["launcher"].startswith("external")
    d1, err1 = _bench([sys.executable, b, "--gpus", "1", "--extra", "none"] + SMALL)
    sha1 = re.findall(r"theta sha256 ([0-9a-f]{64})", err1)
    # one rank draws the whole population's indices from one stream, two ranks from two: the records differ, so theta does too --
    # what must agree is the rank-to-rank digest above; here only the plumbing (supervised child, JSON line) is checked
    assert len(sha1) == 1 and d1["n_gpus"] == 1 and "roofline" in d1 and d1["comm"]["carrier"].startswith("none")


def test_plain_run_dumps_the_last_generation(tmp_path):
    """A plain run (no --full) times the headline alone: no CPU baseline, no extra workloads.  --dump-outputs writes what the last
    timed generation computed -- theta after its update (the digest the run prints) and the generation's records in pair order --
    and a second run with the same arguments writes the same arrays, bit for bit."""
    import hashlib
    import re
    import sys
    b = os.path.join(ROOT, "bench.py")
    small = [a for a in SMALL if a != "--no-cpu-baseline"]
    got = []
    for run in ("a", "b"):
        d, err = _bench([sys.executable, b, "--dump-outputs", str(tmp_path / run)] + small)
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
        assert "cpu_baseline" not in d and "extra" not in d and "extra:" not in err and "cpu baseline" not in err
        arrays = {n: np.load(str(tmp_path / run / (n + ".npy"))) for n in ("theta", "noise_idx", "returns", "sign_returns", "lengths", "update_ratio")}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["theta"].dtype == np.float32 and arrays["theta"].size == 1009058
        assert arrays["noise_idx"].shape == (48,) and arrays["returns"].shape == arrays["lengths"].shape == (48, 2)
        assert arrays["lengths"].min() >= 1 and arrays["lengths"].max() <= 40 and np.array_equal(arrays["lengths"], np.rint(arrays["lengths"]))
        sha = re.findall(r"theta sha256 ([0-9a-f]{64})", err)
        assert sha == [hashlib.sha256(arrays["theta"].tobytes()).hexdigest()], sha
        got.append(arrays)
    for n in got[0]:
        assert np.array_equal(got[0][n], got[1][n]), n


def test_rccl_needs_one_device_per_rank():
    """python bench.py --gpus 2 on this one-GPU box: a clear refusal (RCCL takes one rank per device), not a hang"""
    import subprocess
    import sys
    from dne_hip import _lib
    if _lib.device_count() >= 2:
        pytest.skip("two devices are visible: the launch would be legitimate")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "needs 2 HIP devices" in r.stderr and not r.stdout.strip()


@pytest.mark.timeout(1500)
def test_extra_workloads_plumbing():
    """The `extra` block (BASELINE configs 1, 3, 4, 5 through tools/workloads.py) at reduced size: one rank with every leg and
    its CPU baselines, and two ranks (gloo, one GPU) with the sharded legs -- every leg reports a value and a roofline, none an error."""
    import sys
    b = os.path.join(ROOT, "bench.py")
    small = ["--steps", "1", "--warmup", "0", "--pop", "96", "--tslimit", "40", "--noise-count", "8000000", "--extra-small"]
    d1, _ = _bench([sys.executable, b, "--full", "--extra", "all"] + small, timeout=1400)
    ex = d1["extra"]
    assert sorted(ex) == ["config1", "ga", "ga_large", "nses", "predicted_n2", "shares", "sweep"], ex
    # an N = 2 launch rehearsed on this GPU (tools/workloads.py:simulate_ranks): the sharded generations end on the theta of the one-rank
    # evaluation of the same pairs, and rank 0's share sits in the line beside the headline's own
    pn = ex["predicted_n2"]
    assert "error" not in pn and pn["theta_matches_one_rank_evaluation"] is True and pn["verified_generations"] == 1 and pn["pairs_per_rank"] == 24, pn
    assert pn["value"] > 0 and len(pn["rank_eval_ms_mean"]) == 2 and sorted(ex["shares"]) == ["pairs_24", "pairs_48"], (pn, ex["shares"])
    for k in ("ga", "ga_large", "nses", "sweep"):
        assert "error" not in ex[k] and ex[k]["value"] > 0 and 0 < ex[k]["roofline"]["frac"] < 2, (k, ex[k])
    assert ex["ga"]["cpu_baseline"]["value"] > 0 and ex["config1"]["cores"] == 2 and ex["config1"]["value"] > 0
    assert [g["n_actions"] for g in ex["sweep"]["games"]] == [18, 14]
    assert "cpu_baseline" in d1 and d1["cpu_baseline"]["kind"] == "port"
    d2, _ = _bench([sys.executable, b, "--full", "--gpus", "2", "--single-device", "--transport", "gloo", "--extra", "ga,nses,sweep",
                    "--no-cpu-baseline"] + small, timeout=1400)
    ex2 = d2["extra"]
    assert sorted(ex2) == ["ga", "nses", "sweep"] and all("error" not in v and v["n_gpus"] == 2 for v in ex2.values()), ex2
    # the sharded GA draws its children from two streams instead of one, so the numbers differ from the one-rank run; the
    # bit-identity of the redundant selection across ranks is what tests/test_distributed_gloo.py pins
