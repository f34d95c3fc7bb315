"""CPU: MujocoPolicy on the pendulum outside the kernel -- csrc/pendulum.h compiled for the host (dne_pendulum_reset_host / _actions_host /
_forward_host / _rollout_host / _math_host, no GPU and no handle) against the contract restated in plain Python (tests/pendulum_support.py): the
reset stream, the open-loop step bit for bit, the facts of DESIGN.md section 14, the distance to gym's own form one step at a time, the return
summation against numpy's pairwise sum, tanh_f against libm to one ulp, the forward pass in the four-chain association, the observation
statistics, RunningStat; es.run_master / run_worker with configurations/humanoid.json's shape on PendulumHostEngine; an Atari run's worker
stream against a recording made before this kind existed; the snapshot round trip; the refusals; and the header under AddressSanitizer + UBSan
in a stand-alone program.

Measured (glibc 2.35) over the 11 sequences of pendulum_support.open_loop_cases(), 2200 steps: against gym's form, step by step, the state
differs by at most 5.329070518200751e-15 and no float32 reward differs; the contract's return differs from numpy's pairwise float32 sum by at
most 0.0001220703125 (one ulp).  tanh_f: 0 ulp from float32(math.tanh) on all 1 047 832 values tried."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pendulum_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = np.array([0.1, -0.2, 0.3], np.float32), np.array([0.7, 0.6, 3.0], np.float32)


@pytest.fixture(scope="module")
def replay():
    """{name: (actions, init, host rows, plain-Python rows)} of the open-loop sequences, once"""
    from dne_hip import _lib
    return {name: (a, init, _lib.pendulum_actions_host(a[None], init[None])[0], S.actions_py(a, init)) for name, a, init in S.open_loop_cases()}


def _theta(H, O, seed=3, scale=1.0):
    from dne_hip import policies
    return (policies.normc_flat(H, O, seed) * np.float32(scale)).astype(np.float32)


# ---- 1. the reset and the step -------------------------------------------------------------------------------------------------------------------
def test_reset_is_splitmix64_of_the_seed():
    from dne_hip import _lib
    for seed in (0, 1, 2 ** 31, 2 ** 32 - 1):
        got, want = _lib.pendulum_reset_host(seed), np.array(S.reset_py(seed))
        assert np.array_equal(S.bits(got), S.bits(want)), (seed, got, want)
        assert -S.PI <= got[0] < S.PI and -1.0 <= got[1] < 1.0
    assert S.splitmix_r(0)[0] == 0xe220a8397b1dcdaf      # the generator of cartpole.h: its first output from seed 0


def test_open_loop_equals_the_plain_python_contract_bit_for_bit(replay):
    for name, (a, init, rows, py) in replay.items():
        assert np.array_equal(S.bits(rows), S.bits(py)), name
    # single steps: the first row of every sequence is one step from its reset
    from dne_hip import _lib
    for name, (a, init, rows, _) in replay.items():
        one = _lib.pendulum_actions_host(a[:1][None], init[None])[0, 0]
        assert np.array_equal(S.bits(one), S.bits(rows[0])), name


def test_facts_of_the_contract():
    from dne_hip import _lib
    z = np.zeros((1, S.STEPS), np.float32)
    up = _lib.pendulum_actions_host(z, [[math.pi, 0.0]])[0]           # upright is theta = 0; pi hangs down, where the cost is largest
    assert np.abs(up[:, 0] - math.pi).max() <= 4 * np.spacing(math.pi) and np.abs(up[:, 1]).max() < 1e-14
    assert (up[:, 2] == float(np.float32(-math.pi ** 2))).all()
    rest = _lib.pendulum_actions_host(z, [[0.0, 0.0]])[0]
    assert not rest.any()                                             # theta, theta_dot and every reward exactly 0
    r = _lib.pendulum_rollout_host(np.zeros((1, _lib.pendulum_num_params(64, 1)), np.float32), [5], 64, [0, 0, 0], [1, 1, 1], init=[[0.0, 0.0]])
    assert r['returns'][0] == 0 and r['signreturns'][0] == 0 and r['lengths'][0] == S.STEPS and not r['state'].any()
    three, two = (_lib.pendulum_actions_host(np.full((1, 5), v, np.float32), [[0.3, 0.1]])[0] for v in (3.0, 2.0))
    assert np.array_equal(S.bits(three), S.bits(two))                 # an action of 3.0 acts as 2.0
    clamp = _lib.pendulum_actions_host(np.full((1, 1), 2.0, np.float32), [[math.pi / 2, 7.9]])[0, 0]
    assert clamp[1] == 8.0                                            # 7.9 + (15 + 6) * 0.05 = 8.95 is clamped ...
    assert clamp[0] == math.pi / 2 + (7.9 + (15.0 * 1.0 + 3.0 * 2.0) * 0.05) * 0.05   # ... after theta has moved by the unclamped speed
    # the step limit: min(tslimit, 200)
    th = _theta(64, 1)[None]
    assert _lib.pendulum_rollout_host(th, [1], 64, MEAN, STD, tslimit=7)['lengths'][0] == 7
    assert _lib.pendulum_rollout_host(th, [1], 64, MEAN, STD, tslimit=1000)['lengths'][0] == S.STEPS


def test_each_step_against_gyms_own_form(replay):
    """step_gym on the twin's PREVIOUS state against the twin's next state and reward, so that the distance does not accumulate through the
    dynamics (near the upright position a one-ulp difference grows); the bounds are four times the largest distances measured"""
    worst_s = worst_r = 0.0
    for name, (a, init, rows, _) in replay.items():
        prev = [float(init[0]), float(init[1])]
        for t in range(len(a)):
            (nth, nd), rew = S.step_gym(prev, a[t])
            worst_s = max(worst_s, abs(nth - rows[t, 0]), abs(nd - rows[t, 1]))
            worst_r = max(worst_r, abs(float(np.float32(rew)) - rows[t, 2]))
            prev = [rows[t, 0], rows[t, 1]]
    print("largest distance to gym's form: state %r, float32 reward %r" % (worst_s, worst_r))
    assert worst_s <= S.TOL_GYM_STATE and worst_r <= S.TOL_GYM_REWARD, (worst_s, worst_r)


def test_return_summation(replay):
    from dne_hip import _lib
    worst = 0.0
    for name, (a, init, rows, _) in replay.items():
        rews = rows[:, 2].astype(np.float32)
        assert np.array_equal(rews.astype(np.float64), rows[:, 2])    # the rewards are floats
        ret, sg = S.return_py(rews)
        worst = max(worst, abs(float(ret) - float(rews.sum())))
        assert sg == -np.count_nonzero(rews)
    print("largest distance to numpy's pairwise float32 sum: %r" % worst)
    assert worst <= S.TOL_SUM
    # the closed loop returns exactly return_py of its trace's rewards
    th = _theta(64, 1)[None]
    r = _lib.pendulum_rollout_host(th, [11], 64, MEAN, STD, want_trace=True)
    ret, sg = S.return_py(r['trace'][0, :, 5].astype(np.float32))
    assert r['returns'][0] == ret and r['signreturns'][0] == sg


# ---- 2. tanh_f and norm ---------------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def test_tanh_f_is_within_one_ulp_of_libm():
    from dne_hip import _lib
    seam = []
    for v in (np.float32(2.0 ** -12), np.float32(10.0), np.float32(1.17549435e-38), np.float32(1e-45), np.float32(1.0), np.float32(19.0)):
        seam += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))]
    seam = np.array(seam + [0.0], np.float32)
    xs = np.concatenate([np.arange(0, 2 ** 32, 4099, dtype=np.uint64).astype(np.uint32).view(np.float32), seam, -seam,
                         np.array([np.inf, -np.inf], np.float32)])
    got = _lib.pendulum_math_host('tanh', xs.astype(np.float64)).astype(np.float32)
    want = np.array([math.tanh(float(v)) if v == v else np.nan for v in xs], np.float64).astype(np.float32)
    fin = ~np.isnan(want)
    assert np.isnan(got[~fin]).all() and (~fin).sum() > 1000          # NaN returns NaN
    d = _ulps(got[fin], want[fin])
    print("tanh_f: %d values, largest distance %d ulp, %d values differ" % (fin.sum(), d.max(), np.count_nonzero(d)))
    assert d.max() <= 1                                              # derived (csrc/pendulum.h), not measured: 2 would be a bug in the polynomial
    assert np.array_equal(np.signbit(got[fin]), np.signbit(xs[fin]))  # odd, -0 included
    t = lambda v: _lib.pendulum_math_host('tanh', np.asarray(v, np.float64))
    assert t([0.0])[0] == 0 and np.signbit(t([-0.0])[0]) and t([np.inf])[0] == 1 and t([-np.inf])[0] == -1 and np.isnan(t([np.nan])[0])
    assert t([1e-45])[0] == float(np.float32(1e-45))                  # a denormal returns itself
    for s in (np.float32(2.0 ** -12), np.float32(10.0)):              # monotone across the two seams
        run = [s]
        for _ in range(6):
            run = [np.nextafter(run[0], np.float32(0))] + run + [np.nextafter(run[-1], np.float32(np.inf))]
        y = t(np.array(run, np.float32))
        assert (np.diff(y) >= 0).all(), (s, y)


def test_norm_angle():
    from dne_hip import _lib
    xs = np.random.RandomState(3).uniform(-90, 90, 200_000)
    got = _lib.pendulum_math_host('norm', xs)
    want = np.array([S.norm_py(float(v)) for v in xs[:2000]])
    assert np.array_equal(S.bits(got[:2000]), S.bits(want))
    assert np.abs(got - (((xs + math.pi) % (2 * math.pi)) - math.pi)).max() <= 2e-14    # the issue's 1.1e-14 over +-90
    assert got.min() >= -math.pi - 1e-14 and got.max() <= math.pi + 1e-14


# ---- 3. the forward pass ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonlin", ["tanh", "relu"])
@pytest.mark.parametrize("ac_bins", ["continuous:", "uniform:2", "uniform:5", "uniform:16"])
def test_forward_matches_the_four_chain_restatement(nonlin, ac_bins):
    from dne_hip import _lib, policies
    H, O, mode, _ = policies.mujoco_shape(ac_bins, nonlin, [64, 64], 'ff')
    assert _lib.pendulum_num_params(H, O) == S.offsets(H, O)[6] == 5 * H + H * H + H * O + O
    assert _lib.pendulum_num_params(256, 1) == 67073
    theta = _theta(H, O, seed=11, scale=3.0)
    theta[S.offsets(H, O)[5]:] = np.float32(0.01) * np.arange(O, dtype=np.float32)        # biases that are not zero
    theta[S.offsets(H, O)[1]:S.offsets(H, O)[2]] = np.linspace(-0.5, 0.5, H).astype(np.float32)
    obs = np.array([[1.0, 0.0, 0.0], [-0.3, 0.95, -7.5], [0.5, -0.86, 3.25], [0.0, 1.0, 100.0]], np.float32)   # the last: beyond +-5 deviations
    x, h1, h2, out, act = _lib.pendulum_forward_host(np.tile(theta, (len(obs), 1)), obs, H, MEAN, STD, n_out=O, ac_mode=mode, nonlin=nonlin)
    for i, ob in enumerate(obs):
        want = S.forward_np(theta, ob, H, O, mode, nonlin, MEAN, STD)
        for g, w, what in zip((x[i], h1[i], h2[i], out[i], act[i]), want, ("x", "h1", "h2", "out", "action")):
            assert np.array_equal(S.bits(np.asarray(g, np.float32)), S.bits(np.asarray(w, np.float32))), (i, what)
    assert x[3, 2] == 5.0                                            # (100 - 0.3) / 3 is clipped
    if mode == 'uniform':
        assert set(np.round((act + 2) / 4 * (O - 1), 4)) <= set(float(k) for k in range(O))


def test_the_action_rule_on_ties_zeros_and_nan():
    from dne_hip import _lib
    H = 64
    for O in (2, 5, 16):
        L = S.offsets(H, O)
        zero = np.zeros(L[6], np.float32)
        act = _lib.pendulum_forward_host(zero[None], [[1, 0, 0]], H, MEAN, STD, n_out=O, ac_mode='uniform')[4]
        assert act[0] == -2.0                                         # theta = 0: every score 0, the first maximum is bin 0
        th = zero.copy(); th[L[5] + 1] = th[L[5] + O - 1] = 3.0       # two equal maximal scores: the first
        out, act = _lib.pendulum_forward_host(th[None], [[1, 0, 0]], H, MEAN, STD, n_out=O, ac_mode='uniform')[3:5]
        assert out[0, 1] == out[0, O - 1] == 3.0 and act[0] == S.pick_action_np(out[0], 'uniform') == np.float32(np.float32(1.0) / np.float32(O - 1)) * 4 - 2
        th = zero.copy(); th[L[5]] = np.nan                            # a NaN never wins ...
        assert _lib.pendulum_forward_host(th[None], [[1, 0, 0]], H, MEAN, STD, n_out=O, ac_mode='uniform')[4][0] == \
            (np.float32(np.float32(1.0) / np.float32(O - 1)) * 4 - 2 if O > 1 else -2.0)
        th[L[5]:] = np.nan                                             # ... and all NaN gives bin 0
        assert _lib.pendulum_forward_host(th[None], [[1, 0, 0]], H, MEAN, STD, n_out=O, ac_mode='uniform')[4][0] == -2.0
    assert _lib.pendulum_forward_host(np.zeros((1, S.offsets(H, 16)[6]), np.float32), [[1, 0, 0]], H, MEAN, STD, n_out=16, ac_mode='uniform')[3].shape == (1, 16)


# ---- 4. observation statistics --------------------------------------------------------------------------------------------------------------------
def test_statistics_of_flagged_members_and_action_noise():
    from dne_hip import _lib
    H, n = 64, 5
    noise = S.maze_noise()
    thetas = np.stack([_theta(H, 1, seed=k) for k in range(n)])
    seeds = np.arange(n, dtype=np.uint32) + 40
    flags, ac_off = np.array([1, 0, 1, 1, 0], np.uint8), np.array([0, 17, -1, noise.size - S.STEPS, 500], np.int64)
    r = _lib.pendulum_rollout_host(thetas, seeds, H, MEAN, STD, ac_noise_std=0.05, table=noise, ac_off=ac_off, stat_flag=flags, want_trace=True)
    for i in range(n):
        tr = r['trace'][i]
        if flags[i]:
            s, q = np.zeros(3), np.zeros(3)
            for row in tr:                                            # float64, in step order; the squares are exact
                s += row[:3]
                q += row[:3] * row[:3]
            assert np.array_equal(S.bits(r['ob_sum'][i]), S.bits(s)) and np.array_equal(S.bits(r['ob_sumsq'][i]), S.bits(q)) and r['ob_count'][i] == S.STEPS
        else:
            assert not r['ob_sum'][i].any() and not r['ob_sumsq'][i].any() and r['ob_count'][i] == 0
        want = tr[:, 3].astype(np.float32) if ac_off[i] < 0 else \
            (tr[:, 3].astype(np.float32) + np.float32(0.05) * noise[ac_off[i]:ac_off[i] + S.STEPS]).astype(np.float32)
        assert np.array_equal(tr[:, 4].astype(np.float32), want), i   # a += fl(ac_noise_std * table[ac_off + t])
        # the observation acted on is the state before the step
        assert np.array_equal(tr[0, :3].astype(np.float32), S.obs_py(S.reset_py(seeds[i])))
        assert np.array_equal(tr[1, :3].astype(np.float32), S.obs_py(tr[0, 6:8]))
    with pytest.raises(_lib.DneError, match="past the noise table"):
        _lib.pendulum_rollout_host(thetas[:1], seeds[:1], H, MEAN, STD, table=noise, ac_off=[noise.size - S.STEPS + 1])


def test_running_stat_is_the_references():
    from dne_hip import es
    st = es.RunningStat((3,), eps=1e-2)
    assert st.sum.dtype == st.sumsq.dtype == np.float32
    assert np.array_equal(st.mean, np.zeros(3, np.float32)) and np.array_equal(st.std, np.ones(3, np.float32))   # the eps state: mean 0, std 1
    s, q = np.array([10.0, -4.0, 0.5], np.float32), np.array([30.0, 9.0, 0.05], np.float32)
    st.increment(s, q, 5)
    cnt = 1e-2 + 5
    mean = s / cnt
    assert st.count == cnt and np.array_equal(st.mean, mean)
    want = np.sqrt(np.maximum((np.float32(1e-2) + q) / cnt - np.square(mean), 1e-2))
    assert np.array_equal(st.std, want) and st.std[2] == np.sqrt(np.float32(1e-2))          # the 1e-2 floor on the variance
    st.set_from_init(np.float32(2.0), np.float32(3.0), 1e5)
    assert st.count == 1e5 and np.allclose(st.mean, 2.0) and np.allclose(st.std, 3.0)


# ---- 5. the drivers ---------------------------------------------------------------------------------------------------------------------------------
WORKER_SEED = 1234


def _mine(pushed):
    """the Results this test's worker pushed: the wire spy is installed on the class, so a worker thread an earlier test of the session left
    looping (they run with seed 7) shows up in it too"""
    wid = np.random.RandomState(WORKER_SEED).randint(2 ** 31)
    return [(t, r) for t, r in pushed if r.worker_id == wid]


@pytest.mark.parametrize("prob, ac_std", [(0.5, 0.01), (0.0, 0.0)])
def test_run_master_and_run_worker_on_the_host_twin(oracle, tmp_path, prob, ac_std):
    import es_driver_support as D
    from dne_hip import es
    noise = es.SharedNoiseTable(count=400_000)
    exp = S.humanoid_exp(pop=8, calc_obstat_prob=prob, ac_noise_std=ac_std, eval_prob=1.0)
    me, we = S.PendulumHostEngine(), S.PendulumHostEngine()
    run = D.run_driver(es, exp, me, we, noise, tmp_path, 2, worker_seed=WORKER_SEED)
    assert len(run.tasks) == 2 and [t.timestep_limit for t in run.tasks] == [None, None]
    t0, t1 = run.tasks
    pushed = _mine(run.pushed)
    assert np.array_equal(t0.ob_mean, np.zeros(3, np.float32)) and np.array_equal(t0.ob_std, np.ones(3, np.float32))   # RunningStat's eps state
    shards = [(t, r) for t, r in pushed if r.eval_length is None]
    evals = [(t, r) for t, r in pushed if r.eval_length is not None]
    assert len(shards) == 2 and len(evals) == 2
    # the worker's engine saw the task's statistics before every evaluation, and the evaluation episode ran without options
    assert np.array_equal(we.ob_stats_seen[0][0], t0.ob_mean) and np.array_equal(we.ob_stats_seen[1][1], t1.ob_std)
    assert all(r.eval_length == S.STEPS and r.ob_count is None for _, r in evals)
    # the shard: one coin per episode, offsets only with action noise, ob_count = the flagged lengths' sum
    st = es.RunningStat((3,), eps=1e-2)
    for k, ((tid, r), (n, std, off, flag)) in enumerate(zip(shards, we.options_seen)):
        assert tid == k and n == 8 and r.lengths_n2.shape == (4, 2) and (r.lengths_n2 == S.STEPS).all()
        assert (off is None) == (ac_std == 0) and std == np.float32(ac_std)
        assert r.ob_count == S.STEPS * int(flag.sum())
        if prob == 0:
            assert not flag.any() and r.ob_sum is None and r.ob_sumsq is None and r.ob_count == 0
        elif flag.any():
            assert r.ob_sum.dtype == r.ob_sumsq.dtype == np.float32 and r.ob_sum.shape == (3,)
            if k == 0:
                st.increment(r.ob_sum, r.ob_sumsq, r.ob_count)
    if prob:
        assert sum(int(f.sum()) for _, _, _, f in we.options_seen) > 0, "no coin landed: choose another worker seed"
    # the second task's statistics follow from the first's results by RunningStat; the master's policy holds the last ones
    assert np.array_equal(t1.ob_mean, st.mean) and np.array_equal(t1.ob_std, st.std)
    assert np.array_equal(run.policy.ob_mean, me.ob_stats_seen[-1][0]) and len(me.ob_stats_seen) == 2
    assert run.theta.shape == (me.P,) and not np.array_equal(t0.params, t1.params)
    # the worker's stream: indices, seeds, then coins, then offsets
    rs = np.random.RandomState(WORKER_SEED)
    rs.randint(2 ** 31); rs.rand(); rs.randint(0, 2 ** 32, size=1, dtype=np.uint64)
    idx = np.sort(np.array([noise.sample_index(rs, me.P) for _ in range(4)], dtype=np.int64))
    seeds = rs.randint(0, 2 ** 32, size=8, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(shards[0][1].noise_inds_n, idx) and np.array_equal(we.seeds_seen[1], seeds)
    if prob:
        assert np.array_equal(we.options_seen[0][3], (rs.rand(8) < prob).astype(np.uint8))
    if ac_std:
        assert np.array_equal(we.options_seen[0][2], rs.randint(0, len(noise.noise) - S.STEPS + 1, size=8))


def test_an_atari_runs_stream_and_tasks_are_what_they_were(oracle, tmp_path):
    """tests/golden/pendulum_atari_stream.npz was recorded on the commit before DNE_KIND_PENDULUM existed, from this very scenario: the noise
    indices, the environment seeds of the shards and of the evaluation episodes, the worker id and the Results' ob_count"""
    import es_driver_support as D
    from oracle_engine import OracleEngine
    from dne_hip import es
    want = np.load(os.path.join(ROOT, "tests", "golden", "pendulum_atari_stream.npz"))
    noise = es.SharedNoiseTable(count=2_500_000)
    we = OracleEngine(0, ref_count=16)
    es_evals = D.record_calls(we, "es_eval")
    run = D.run_driver(es, D.es_exp(pop=8, cutoff=12, eval_prob=1.0), OracleEngine(0, ref_count=16), we, noise, tmp_path, 2, worker_seed=WORKER_SEED)
    pushed = _mine(run.pushed)
    assert all(t.ob_mean is None and t.ob_std is None for t in run.tasks)
    assert np.array_equal(np.stack([r.noise_inds_n for _, r in pushed if r.noise_inds_n is not None]), want["noise_inds"])
    assert np.array_equal(np.stack([c[3] for c in es_evals]), want["es_seeds"])
    assert np.array_equal(np.array([int(c[2][0]) for c in run.evals], np.uint32), want["eval_seeds"])
    assert np.array_equal(np.array([r.worker_id for _, r in pushed], np.int64), want["worker_ids"])
    assert np.array_equal(np.array([-1 if r.ob_count is None else r.ob_count for _, r in pushed], np.int64), want["ob_counts"])
    assert all(r.ob_sum is None and r.ob_sumsq is None for _, r in pushed)
    assert float(run.theta.astype(np.float64).sum()) == float(want["theta_sum"])


# ---- 6. the policy surface and snapshots ---------------------------------------------------------------------------------------------------------
def _policy(**over):
    from dne_hip import policies
    env = policies.PendulumEnv()
    args = S.humanoid_exp(**over)["policy"]["args"]
    return policies.MujocoPolicy(env.observation_space, env.action_space, **args), env


def test_policy_surface():
    from dne_hip import _lib
    pol, env = _policy(hidden=64)
    assert pol.needs_ob_stat and not pol.needs_ref_batch and pol.num_params == _lib.pendulum_num_params(64, 1) == 4481
    assert np.isnan(pol.ob_mean).all() and np.isnan(pol.ob_std).all()          # policies.py:138-141
    pol.initialize(5)
    th = pol.get_trainable_flat()
    L = S.offsets(64, 1)
    w0, w1, wo = th[L[0]:L[1]].reshape(3, 64), th[L[2]:L[3]].reshape(64, 64), th[L[4]:L[5]].reshape(64, 1)
    assert np.allclose(np.square(w0).sum(0), 1, atol=1e-6) and np.allclose(np.square(w1).sum(0), 1, atol=1e-5)   # normc_initializer(1.0), per column
    assert np.allclose(np.square(wo).sum(0), 1e-4, rtol=1e-5) and not th[L[1]:L[2]].any() and not th[L[3]:L[4]].any() and not th[L[5]:].any()
    pol.set_ob_stat(MEAN, STD)
    ob = np.array([[0.5, -0.86, 3.25], [1.0, 0.0, 0.0]], np.float32)
    a = pol.act(ob)
    assert a.shape == (2, 1) and a[0, 0] == S.forward_np(th, ob[0], 64, 1, 'continuous', 'tanh', MEAN, STD)[4]
    noisy = pol.act(ob, random_stream=np.random.RandomState(1))
    assert np.array_equal(noisy, a + (np.random.RandomState(1).randn(2, 1) * 0.01).astype(np.float32))
    env.seed(9)
    rews, t, obs = pol.rollout(env, save_obs=True)
    assert t == S.STEPS and rews.dtype == np.float32 and rews.shape == (S.STEPS,) and obs.shape == (S.STEPS, 3)
    want = _lib.pendulum_rollout_host(th[None], [9], 64, MEAN, STD)
    assert S.return_py(rews)[0] == want['returns'][0] and np.array_equal(obs[0], S.obs_py(S.reset_py(9)))
    rews2, t2 = pol.rollout(env, timestep_limit=13, random_stream=np.random.RandomState(2))
    assert t2 == 13 and rews2.shape == (13,)


def test_snapshot_round_trip(tmp_path):
    from dne_hip import policies
    pol, _ = _policy(hidden=64, ac_bins="uniform:5", nonlin="relu")
    pol.initialize(2)
    pol.set_ob_stat(MEAN, STD)
    arrays = pol.variable_arrays()
    assert list(arrays) == ["MujocoPolicy/%s:0" % n for n in ("l0/w", "l0/b", "l1/w", "l1/b", "out/w", "out/b", "ob_mean", "ob_std")]
    assert [a.shape for a in arrays.values()] == [(3, 64), (64,), (64, 64), (64,), (64, 5), (5,), (3,), (3,)]
    for ext in (".npz", policies.snapshot_extension()):
        fn = str(tmp_path / ("snap" + ext))
        pol.save(fn)
        back = policies.MujocoPolicy.Load(fn)
        assert np.array_equal(back.get_trainable_flat(), pol.get_trainable_flat())
        assert np.array_equal(back.ob_mean, MEAN) and np.array_equal(back.ob_std, STD)
        assert back.kwargs == pol.kwargs and (back.hidden, back.n_out, back.ac_mode, back.nonlin) == (64, 5, 'uniform', 'relu')
    with pytest.raises(NotImplementedError, match="376"):
        pol.initialize_from("whatever.h5")


# ---- 7. refusals, by name ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle, tmp_path):
    from dne_hip import _lib, es, ga, nses, policies
    env = policies.PendulumEnv()
    base = S.humanoid_exp()["policy"]["args"]
    for over, word in ((dict(ac_bins="custom:-1,0,1"), "custom"), (dict(nonlin_type="lrelu"), "lrelu"), (dict(nonlin_type="elu"), "elu"),
                       (dict(hidden_dims=[64, 64, 64]), "two hidden layers"), (dict(hidden_dims=[64, 128]), "one width"),
                       (dict(hidden_dims=[96, 96]), "96"), (dict(ac_bins="uniform:17"), "uniform:17"), (dict(ac_bins="uniform:1"), "uniform:1"),
                       (dict(connection_type="rnn"), "rnn")):
        with pytest.raises(NotImplementedError, match=word):
            policies.MujocoPolicy(env.observation_space, env.action_space, **dict(base, **over))
    for env_id, word in (("Humanoid-v1", "MuJoCo"), ("CartPole-v1", "CartPole-v1"), (None, "None")):
        with pytest.raises(NotImplementedError, match=word):
            es.setup(S.humanoid_exp(env_id=env_id), engine=S.PendulumHostEngine())
    with pytest.raises(ValueError, match="KIND_PENDULUM"):
        es.setup(S.humanoid_exp(), engine=type("E", (), {"kind": 0})())
    with pytest.raises(NotImplementedError, match="nses with MujocoPolicy"):
        nses.run_master({}, str(tmp_path), dict(S.humanoid_exp(), algo_type="nses", novelty_search={}), engine=S.PendulumHostEngine())
    with pytest.raises(NotImplementedError, match="ga with MujocoPolicy"):
        ga.setup(S.humanoid_exp(), engine=S.PendulumHostEngine())
    # the C ABI without a GPU
    assert _lib.pendulum_num_params(96, 1) == -1 and _lib.pendulum_num_params(64, 17) == -1 and _lib.pendulum_num_params(64, 0) == -1
    assert _lib.num_params(_lib.KIND_PENDULUM, 1) == -1               # dne_num_params cannot know the width
    th = np.zeros((1, 4481), np.float32)
    with pytest.raises(_lib.DneError, match="not a shape"):
        _lib.pendulum_rollout_host(th, [1], 64, MEAN, STD, n_out=1, ac_mode='uniform')
    with pytest.raises(_lib.DneError, match="DNE_KIND_PENDULUM"):
        _lib.debug_plan(_lib.KIND_PENDULUM, 1, 8, 2)
    with pytest.raises(_lib.DneError, match="DNE_KIND_PENDULUM"):
        _lib.debug_plan_act(_lib.KIND_PENDULUM, 1, 8)
    # evaluation before set_ob_stat, and an offset past the table's end, on the host-twin engine (the device's: tests/test_gpu_pendulum.py)
    e = S.PendulumHostEngine()
    e.noise_upload(S.maze_noise())
    with pytest.raises(_lib.DneError, match="set_ob_stat"):
        e.es_eval(np.array([5], np.int64), 0.02, 200, np.array([1, 2], np.uint32))
    with pytest.raises(_lib.DneError, match="past the noise table"):
        e.pendulum_set_rollout_options(2, 0.01, np.array([0, e.noise.size - S.STEPS + 1], np.int64), None)


# ---- 8. the header under AddressSanitizer and UBSan, in a program of its own ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitizer_program(tmp_path_factory):
    """tests/pendulum_asan_main.cpp, built once: address, undefined and float-cast-overflow (a NaN or an infinity reaching a cast to int)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = os.path.join(ROOT, "tests", "pendulum_asan_main.cpp")
    exe = str(tmp_path_factory.mktemp("pendulum_asan") / "pendulum_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "deep-neuroevolution_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def test_header_under_sanitizers_in_a_stand_alone_program(sanitizer_program):
    out = subprocess.run([sanitizer_program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    # 3 widths x 4 output counts x 2 nonlinearities (8 of 200 steps, 16 of 37); 3 facts each + 4; outside the contract 6 fills x 3 deviations x 2
    assert out.stdout.split() == ["ok", "24", "2192", "facts", "76", "wild", "36", "900"], out.stdout


def test_host_refusals_word_for_word():
    """the whole text of what dne_pendulum_rollout_host / dne_pendulum_forward_host refuse: a shape the header does not build, an action-noise
    offset whose 200 values end past the table"""
    from dne_hip import _lib
    th = np.zeros((2, _lib.pendulum_num_params(64, 4)), np.float32)
    shape = "dne_pendulum_%s_host: hidden width 64, 4 outputs, action mode 0, nonlinearity 0 is not a shape csrc/pendulum.h builds"
    with pytest.raises(_lib.DneError) as ei:
        _lib.pendulum_rollout_host(th, [1, 2], 64, MEAN, STD, n_out=4, ac_mode='continuous')
    assert str(ei.value) == shape % "rollout"
    with pytest.raises(_lib.DneError) as ei:
        _lib.pendulum_forward_host(th, np.zeros((2, 3), np.float32), 64, MEAN, STD, n_out=4, ac_mode='continuous')
    assert str(ei.value) == shape % "forward"
    with pytest.raises(_lib.DneError) as ei:
        _lib.pendulum_rollout_host(th, [1, 2], 64, MEAN, STD, n_out=4, ac_mode='uniform', table=np.zeros(1000, np.float32), ac_off=[-1, 801])
    assert str(ei.value) == "dne_pendulum_rollout_host: member 1 reads its action noise from offset 801, past the noise table's 1000 values"
    with pytest.raises(_lib.DneError) as ei:
        _lib.pendulum_rollout_host(th, [1, 2], 64, MEAN, STD, n_out=4, ac_mode='uniform', tslimit=0)
    assert str(ei.value) == "dne_pendulum_rollout_host: bad arguments"
