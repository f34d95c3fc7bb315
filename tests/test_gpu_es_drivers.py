"""GPU: the ES master/worker drivers (dne_hip/es.py, dne_hip/es_modified.py) and the gym-style Policy surface (HipAtariEnv,
Policy.rollout, Policy.save / Load) on the HIP engine.  Every scenario runs twice in the test -- on tests/oracle_engine.py:OracleEngine
(the float32 CPU oracle behind the engine surface: the reference) and on _lib.Engine -- with the same experiment, noise table and
seeds, and everything that crosses a seam is compared: each pushed Result field by field, each declared Task, the logged
UpdateRatio, theta bit for bit (es_driver_support.assert_same_run)."""
import os
import pickle

import numpy as np
import pytest

import es_driver_support as S
from es_driver_support import NACT, NREF

pytestmark = pytest.mark.gpu

OPTIMIZERS = {
    "centered_rank": S.ADAM,
    "centered_sign_rank": {"type": "sgd", "args": {"stepsize": 0.02, "momentum": 0.8}},
    "sign": {"type": "adam", "args": {"stepsize": 0.01, "beta1": 0.8, "beta2": 0.99, "epsilon": 1e-6}},
}


@pytest.fixture(scope="module")
def hip():
    from dne_hip import _lib
    return _lib


@pytest.fixture(scope="module")
def noise(small_noise):
    from dne_hip import es
    t = es.SharedNoiseTable(count=small_noise.size)
    assert np.array_equal(t.noise, small_noise)
    return t


@pytest.fixture
def engines(hip, oracle):
    """make("hip" | "oracle", kind, **kw) -> an engine with 8 members and 16 reference frames, closed when the test ends"""
    from oracle_engine import OracleEngine
    made = []

    def make(backend, kind=0, **kw):
        cls = hip.Engine if backend == "hip" else OracleEngine
        e = cls(kind, NACT, max_members=8, ref_count=NREF, **kw)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


def _es_scenario(engines, noise, log_dir, backend, exp, iters, **kw):
    from dne_hip import es
    return S.run_driver(es, exp, engines(backend), engines(backend), noise, os.path.join(str(log_dir), backend), iters, **kw)


@pytest.fixture(scope="module")
def rank_runs():
    """scenario 1 at centered_rank, shared by its own test and the Redis one: {"oracle": DriverRun, "hip": DriverRun}"""
    return {}


def _scenario1(engines, noise, log_dir, mode, backend, **kw):
    return _es_scenario(engines, noise, log_dir, backend, S.es_exp(pop=8, cutoff=24, mode=mode, optimizer=OPTIMIZERS[mode], eval_prob=1.0),
                        3, **kw)


# ---------------------------------------------------------------------------------------------- 1: es.run_master + es.run_worker
@pytest.mark.parametrize("mode", list(OPTIMIZERS))
def test_es_driver_with_evaluation_episodes(engines, oracle, hip, noise, tmp_path, rank_runs, mode):
    """Three generations with eval_prob 1.0: every worker iteration runs the unlimited evaluation episode (one member, groups of one,
    virtual batch norm, ends at game over only) and then its shard on the same engine; the master's update takes the concatenated
    Results through sign / centered_sign_rank / centered_rank and SGD / Adam with the experiment's own constants."""
    want = _scenario1(engines, noise, tmp_path, mode, "oracle")
    got = _scenario1(engines, noise, tmp_path, mode, "hip")
    if mode == "centered_rank":
        rank_runs.update(oracle=want, hip=got)
    assert [t for t, _ in want.pushed] == [0, 0, 1, 1, 2, 2] and len(want.tasks) == 3
    assert [r.eval_length is not None for _, r in want.pushed] == [True, False] * 3          # the evaluation goes first (es.py:398-412)
    assert all(c[0] == 1 and c[1] == hip.ENV_MAX_EPISODE_STEPS for c in want.evals + got.evals)
    over = S.episodes_ended_by_game_over(oracle, want)
    assert over and all(n < hip.ENV_MAX_EPISODE_STEPS for _, n in over), over              # game over, not a limit, ended them
    assert not np.array_equal(want.tasks[0].params, want.tasks[2].params)
    S.assert_same_run(want, got, "es " + mode)


# ---------------------------------------------------------------------------------------------- 2: adaptive cutoff
def test_es_driver_adaptive_cutoff(engines, oracle, noise, tmp_path):
    """episode_cutoff_mode adaptive:12,0.5,1.5,40 (es.py:308-311): the limit of es_eval changes between generations on one engine."""
    exp = S.es_exp(pop=8, cutoff="adaptive:12,0.5,1.5,40", eval_prob=0.0)
    want = _es_scenario(engines, noise, tmp_path, "oracle", exp, 4)
    assert [t.timestep_limit for t in want.tasks] == [12, 18, 27, 40]                     # three changes of limit were crossed
    got = _es_scenario(engines, noise, tmp_path, "hip", exp, 4)
    assert [t.timestep_limit for t in got.tasks] == [12, 18, 27, 40]
    S.assert_same_run(want, got, "es adaptive")


# ---------------------------------------------------------------------------------------------- 3: odd episodes_per_batch
def test_es_driver_reevaluates_for_an_odd_batch(engines, oracle, small_noise, noise, tmp_path):
    """episodes_per_batch 9: one shard of 2 * (9 // 2) episodes is not enough, the worker (max_tasks=None, like a reference worker)
    delivers a second shard of the SAME task with fresh indices and the master updates from both.  The worker's draws are its seeded
    stream, so both shards are replayed by the oracle; theta after the update = the oracle's update from the Results the HIP worker
    actually pushed."""
    from oracle_engine import OracleEngine
    from dne_hip import es, policies
    exp = S.es_exp(pop=9, cutoff=6, eval_prob=0.0)
    got = _es_scenario(engines, noise, tmp_path, "hip", exp, 1, max_tasks=None, reeval_after=0.05,
                       master_cfg={"host": "127.0.0.1", "port": 1, "transport": "inprocess"},
                       relay_cfg={"unix_socket_path": "/tmp/dne_relay_y.sock"})
    assert len(got.pushed) >= 2 and all(t == 0 for t, _ in got.pushed) and len(got.tasks) == 1
    used = [r for _, r in got.pushed[:2]]                       # 16 episodes >= 9: the master stops collecting after the second
    cat = {f: np.concatenate([getattr(r, f) for r in used]) for f in S.RESULT_ARRAYS}
    assert len(got.updates) == 1 and np.array_equal(got.updates[0][0], cat["noise_inds_n"]) and cat["noise_inds_n"].shape == (8,)
    assert not np.array_equal(used[0].noise_inds_n, used[1].noise_inds_n)
    # the two shards against the oracle: same stream as the worker's (es.py:382-383, 406-408)
    L, th0, ref = oracle.layout(0, NACT), policies.xavier_flat(NACT, 0), got.tasks[0].ref_batch
    rs = np.random.RandomState(7); rs.randint(2 ** 31)
    for k, r in enumerate(used):
        rs.rand()
        idx = np.sort(np.array([noise.sample_index(rs, L.P) for _ in range(4)], np.int64))
        seeds = rs.randint(0, 2 ** 32, size=8, dtype=np.uint64).astype(np.uint32)
        oret, osg, oln = oracle.es_eval(L, th0, small_noise, idx, 0.02, 6, ref, seeds)
        for f, w in zip(S.RESULT_ARRAYS, (idx, oret, osg, oln)):
            S._same_array(w, getattr(r, f), "shard %d, %s" % (k, f))
    rep = OracleEngine(0, ref_count=NREF)
    rep.noise_upload(small_noise); rep.set_theta(th0)
    ratio = rep.es_update(cat["noise_inds_n"], cat["returns_n2"], cat["signreturns_n2"], "centered_rank", "adam", 0.005, 0.01)
    assert np.array_equal(got.theta, rep.get_theta())
    assert len(got.ratios) == 1 and abs(got.ratios[0] - ratio) <= 1e-9 * ratio


# ---------------------------------------------------------------------------------------------- 4: the Redis carrier
def test_es_driver_over_the_redis_protocol(engines, oracle, noise, tmp_path, rank_runs):
    """Scenario 1 at centered_rank with Task and (task_id, Result) pickled through a Redis-protocol server on loopback (resp.py against
    tests/fake_redis.py): Results and theta equal those of the in-process run on the same engine kind, and so the oracle's."""
    from fake_redis import FakeRedis
    if not rank_runs:
        rank_runs.update(oracle=_scenario1(engines, noise, tmp_path, "centered_rank", "oracle"),
                         hip=_scenario1(engines, noise, tmp_path / "inprocess", "centered_rank", "hip"))
    srv = FakeRedis()
    try:
        cfg = dict(srv.cfg, transport="redis")
        got = _scenario1(engines, noise, tmp_path / "redis", "centered_rank", "hip", master_cfg=cfg, worker_master_cfg=cfg,
                         relay_cfg={"unix_socket_path": "/tmp/dne_no_such_relay.sock"})
        assert {b"MSET", b"PUBLISH", b"BLPOP", b"RPUSH", b"MGET", b"SET"} <= set(srv.commands)
        task = pickle.loads(srv.kv[b"es:task_data"])
        assert int(srv.kv[b"es:task_id"]) == 2 and np.array_equal(task.params, got.tasks[2].params)
    finally:
        srv.close()
    S.assert_same_run(rank_runs["hip"], got, "es over redis vs in-process")
    S.assert_same_run(rank_runs["oracle"], got, "es over redis vs oracle")


# ---------------------------------------------------------------------------------------------- 5: es_modified
def test_es_modified_driver_and_its_dumps(engines, oracle, hip, noise, tmp_path):
    """es_modified master + worker on engines as es_modified.make_engine builds them (record_bc, bc_final_only), two generations with an
    evaluation episode each: Results with every bc_vectors entry, theta, and the .dat rows written from device results."""
    from dne_hip import es_modified, policies
    exp = S.es_exp(pop=8, cutoff=24, eval_prob=1.0)
    runs = {}
    for backend in ("oracle", "hip"):
        if backend == "hip":
            mk = lambda: es_modified.make_engine(exp, 4, n_actions=NACT, ref_count=NREF)     # noqa: E731
            me, we = mk(), mk()
            assert (me.record_bc, me.bc_final_only, me.max_members, me.ref_count) == (True, True, 8, NREF)
        else:
            me, we = engines("oracle", bc_final_only=True), engines("oracle", bc_final_only=True)
        root = str(tmp_path / backend / "snapshots")
        try:
            runs[backend] = S.run_driver(es_modified, exp, me, we, noise, tmp_path / backend, 2, master_kw={"snapshot_root": root}), root
        finally:
            if backend == "hip":
                me.close(); we.close()
    (want, wroot), (got, groot) = runs["oracle"], runs["hip"]
    assert [len(r.bc_vectors) for _, r in want.pushed] == [1, 8, 1, 8]
    S.assert_same_run(want, got, "es_modified")
    ext = policies.snapshot_extension()
    for gen in range(2):
        d = "snapshot_gen_%04d" % gen
        for name in ("snapshot_offspring_%04d.dat" % gen, "snapshot_parent_%04d.dat" % gen):
            w, g = (open(os.path.join(r, d, name), "rb").read() for r in (wroot, groot))
            assert w == g and len(w) > 128, (gen, name)
        assert np.loadtxt(os.path.join(groot, d, "snapshot_offspring_%04d.dat" % gen)).shape == (8, 128 + 5)
        # the parent snapshot was written before the update: it holds the theta of this generation's Task, moving moments included
        snaps = [policies.ESAtariPolicy.Load(os.path.join(r, d, "snapshot_parent_%04d" % gen + ext), engine=engines(b))
                 for r, b in ((wroot, "oracle"), (groot, "hip"))]
        for p in snaps:
            assert np.array_equal(p.get_trainable_flat(), got.tasks[gen].params), gen
        arrays = [policies.Policy._read_snapshot(os.path.join(r, d, "snapshot_parent_%04d" % gen + ext))[3] for r in (wroot, groot)]
        assert sorted(arrays[0]) == sorted(arrays[1]) and len(arrays[0]) == 20
        for k in arrays[0]:
            S._same_array(arrays[0][k], arrays[1][k], "generation %d snapshot, %s" % (gen, k))
        for r in (wroot, groot):
            S._same_array(pickle.load(open(os.path.join(r, d, "snapshot_parent_%04d_rb.p" % gen), "rb")), got.tasks[gen].ref_batch, "rb.p")


# ---------------------------------------------------------------------------------------------- 6: Policy.rollout
def _policy(backend, kind, engines, oracle, small_noise, env_seed=3):
    """(policy, env, theta, ref) of the ES policy (xavier seed 0, 16 reference frames) or the GA policy (a chain of three table indices)"""
    from dne_hip import policies
    e = engines(backend, kind)
    e.noise_upload(small_noise)
    env = policies.HipAtariEnv(e, seed=env_seed)
    if kind == 0:
        pol = policies.ESAtariPolicy(env.observation_space, env.action_space, engine=e)
        pol.initialize(0)
        ref = oracle.get_ref_batch(seed=0, batch_size=NREF, nact=NACT)
        pol.set_ref_batch(ref)
    else:
        pol = policies.GAAtariPolicy(env.observation_space, env.action_space, nonlin_type="relu", engine=e)
        pol.set_from_seeds([5, 77_777, 1_000_001], 0.005)
        ref = None
    return pol, env, pol.get_trainable_flat(), ref


def _check_rollout(oracle, hip, kind, theta, ref, seed, T, got, want=None, what=""):
    """One Policy.rollout result against oracle.rollout of the same episode -- return, length, novelty vector -- and, step by step,
    against the same rollout of the OracleEngine policy (`want`: per-step rewards, and the observations of the save_obs form)."""
    limit = hip.ENV_MAX_EPISODE_STEPS if T is None else T
    r, s, l, bc = oracle.rollout(oracle.layout(kind, NACT), theta, ref, seed, limit, want_bc=True)
    rews, t, nov = got[0], got[1], got[-1]
    assert t == l and len(rews) == l and rews.dtype == np.float32 and rews.sum() == r, (what, seed, T, t, l, rews.sum(), r)
    S._same_array(bc, nov, "%s seed %d T %s: novelty vector" % (what, seed, T))
    assert nov.shape == ((l, 128) if kind == 0 else (128,))
    if want is not None:
        assert len(want) == len(got) and want[1] == t
        for k, (w, g) in enumerate(zip(want, got)):
            if k != 1:
                S._same_array(w, g, "%s seed %d T %s: rollout()[%d]" % (what, seed, T, k))
    return l, bc


@pytest.mark.parametrize("kind", [0, 1], ids=["ESAtariPolicy", "GAAtariPolicy"])
def test_policy_rollout_on_device(engines, oracle, hip, small_noise, kind):
    """Policy.rollout drives a whole episode one step at a time through env_reset / ref_pass(1) / act(1) / env_step / env_ram on the
    live env slot.  Limits 1, 15 and none, then a second full episode on the same HipAtariEnv (the episode seed advances; nothing of the
    first episode may leak into the second), then the save_obs form."""
    pol, env, theta, ref = _policy("hip", kind, engines, oracle, small_noise)
    opol, oenv, otheta, _ = _policy("oracle", kind, engines, oracle, small_noise)
    assert np.array_equal(theta, otheta)
    lengths = []
    for ep, T in enumerate((1, 15, None, None)):
        got, want = pol.rollout(env, timestep_limit=T), opol.rollout(oenv, timestep_limit=T)
        l, bc = _check_rollout(oracle, hip, kind, theta, ref, 3 + ep, T, got, want, pol.__class__.__name__)
        lengths.append(l)
    assert lengths[:2] == [1, 15] and 15 < min(lengths[2:]) and max(lengths[2:]) < 1000, lengths
    assert (bc[-1] if kind == 0 else bc)[9]                                         # the unlimited episodes ended by game over
    got, want = pol.rollout(env, timestep_limit=15, save_obs=True), opol.rollout(oenv, timestep_limit=15, save_obs=True)
    assert got[2].shape == (15, 84, 84, 4) and got[2].dtype == np.float32
    _check_rollout(oracle, hip, kind, theta, ref, 7, 15, got, want, "save_obs")
    got, want = pol.rollout(env, save_obs=True, policy_seed=11), opol.rollout(oenv, save_obs=True, policy_seed=11)   # policies.py:392-396
    _check_rollout(oracle, hip, kind, theta, ref, 11, None, got, want, "save_obs policy_seed")


def test_policy_rollout_after_batched_evaluations(engines, oracle, hip, small_noise):
    """One es_eval and one eval_members on the engine, then Policy.rollout on it: the step-by-step episode must see nothing of the
    batched evaluations -- their done flags, episode lengths, members or tail table."""
    pol, env, theta, ref = _policy("hip", 0, engines, oracle, small_noise)
    e, L = pol.engine, oracle.layout(0, NACT)
    idx = np.array([5, 77_777, 1_000_001, 1_490_000], np.int64)
    seeds = np.arange(8, dtype=np.uint32) + 1000
    ret, sg, ln = e.es_eval(idx, 0.02, 24, seeds)
    oret, osg, oln = oracle.es_eval(L, theta, small_noise, idx, 0.02, 24, ref, seeds)
    assert np.array_equal(ret, oret) and np.array_equal(sg, osg) and np.array_equal(ln, oln)
    e.set_members(np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float32))
    r1, s1, l1 = e.eval_members(1, hip.ENV_MAX_EPISODE_STEPS, np.array([3], np.uint32))      # runs to game over: slot 0 is left done
    full = oracle.rollout(L, theta, ref, 3, hip.ENV_MAX_EPISODE_STEPS)
    assert (r1[0], s1[0], l1[0]) == full[:3] and l1[0] < 1000
    for ep, T in enumerate((None, 15)):
        _check_rollout(oracle, hip, 0, theta, ref, 3 + ep, T, pol.rollout(env, timestep_limit=T), None, "after es_eval + eval_members")
    # and the other way round: a batched evaluation after the step-by-step episodes
    ret, sg, ln = e.es_eval(idx, 0.02, 24, seeds)
    assert np.array_equal(ret, oret) and np.array_equal(sg, osg) and np.array_equal(ln, oln)
    assert np.array_equal(pol.get_trainable_flat(), theta)


# ---------------------------------------------------------------------------------------------- 7: Policy.save -> Load
def test_policy_save_and_load_on_device(engines, oracle, hip, small_noise, tmp_path):
    """After a rollout the snapshot's variables -- the six moving_mean / moving_variance arrays from dne_get_bn_moments included -- equal
    the OracleEngine policy's; saved and loaded into a fresh HIP engine, the policy is the same vector and plays the same episode."""
    from dne_hip import policies
    pol, env, theta, ref = _policy("hip", 0, engines, oracle, small_noise)
    opol, oenv, _, _ = _policy("oracle", 0, engines, oracle, small_noise)
    first = pol.rollout(env, timestep_limit=20)
    _check_rollout(oracle, hip, 0, theta, ref, 3, 20, first, opol.rollout(oenv, timestep_limit=20), "before save")
    arrays, want = pol.variable_arrays(), opol.variable_arrays()
    assert list(arrays) == list(want) and len(arrays) == 20 and sum("moving_" in k for k in arrays) == 6
    for k in want:
        S._same_array(want[k], arrays[k], k)
    _, mom = oracle.es_ref_pass_moments(oracle.layout(0, NACT), theta, ref)
    assert np.array_equal(arrays["ESAtariPolicy/BatchNorm_2/moving_mean:0"], mom[96:352])
    exts = [".npz"] + ([".h5"] if policies.snapshot_extension() == ".h5" else [])
    for ext in exts:
        fn = str(tmp_path / ("snap" + ext))
        pol.save(fn)
        saved = policies.Policy._read_snapshot(fn)[3]
        for k in want:
            S._same_array(want[k], saved[k], ext + " " + k)
        e2 = engines("hip")
        e2.noise_upload(small_noise)
        pol2 = policies.ESAtariPolicy.Load(fn, engine=e2)
        assert np.array_equal(pol2.get_trainable_flat(), theta) and np.array_equal(e2.get_theta(), theta)
        pol2.set_ref_batch(ref)
        again = pol2.rollout(policies.HipAtariEnv(e2, seed=3), timestep_limit=20)
        for k, (w, g) in enumerate(zip(first, again)):
            S._same_array(np.asarray(w), np.asarray(g), "%s: rollout()[%d] of the loaded policy" % (ext, k))
        loaded = pol2.variable_arrays()
        for k in want:
            S._same_array(want[k], loaded[k], ext + " loaded " + k)
