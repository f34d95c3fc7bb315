"""TEST-ONLY support for MujocoPolicy on the hard maze (DNE_KIND_MJMAZE, csrc/mjmaze.h): the forward pass restated in numpy
(pendulum_support's four-chain dense layer and normalisation; tanh from _lib.pendulum_math_host, the function the header calls), the shipped
humanoid_nses / humanoid_nsres / humanoid experiments at a test's size, the mazes the tests run in, and MjMazeHostEngine --
dne_mjmaze_rollout_host (the same header compiled for the CPU) behind the Engine method surface."""
import numpy as np

from maze_support import EDGE_MAZES, edge_maze, fixture_maze, maze_noise, synthetic_maze   # noqa: F401
from oracle_engine import OracleEngine
from pendulum_support import bits, dense4_np, normalise_np, perturbed, tanh_header   # noqa: F401

ENV_ID = "HardMaze-v0"
OBS, ADIM, STEPS, TRACE_W, AC_NOISE = 11, 2, 400, 20, 800
HS, NONLINS = (64, 128, 256), ("tanh", "relu")
MODES = (("continuous", 2), ("uniform", 4), ("uniform", 16))      # (action mode, outputs): continuous:, uniform:2, uniform:8
MEAN = np.array([0.9, 0.3, 0.25, 0.4, 0.2, 0.35, 0.5, 0.1, 0.4, 0.3, 0.2], np.float32)   # (the bias input 1 deviates from its mean by 0.1)
STD = np.array([1.0, 0.2, 0.15, 0.3, 0.1, 0.25, 0.3, 0.3, 0.5, 0.45, 0.4], np.float32)


def offsets(H, O):
    w1, b1 = 0, OBS * H
    w2 = b1 + H
    b2 = w2 + H * H
    w3 = b2 + H
    b3 = w3 + H * O
    return w1, b1, w2, b2, w3, b3, b3 + O


def pick_dim_np(out, i, mode):
    """dimension i of the action: out[i], or the first maximum of the dimension's B bins under a strict > scan from -inf, then
    ((1 / (B - 1)) * aidx) * 1 + (-0.5), every operation in float32"""
    if mode == 'continuous':
        return np.float32(out[i])
    B = len(out) // ADIM
    aidx, best = 0, np.float32(-np.inf)
    for b in range(B):
        if out[i * B + b] > best:
            best, aidx = out[i * B + b], b
    f = np.float32
    return f(f(f(f(1.0) / f(f(B) - f(1.0))) * f(aidx)) * f(1.0) + f(-0.5))


def forward_np(theta, ob, H, O, mode, nonlin, mean, std):
    """-> (x, h1, h2, out, action [2]) as dne_mjmaze_forward_host"""
    th = np.asarray(theta, np.float32)
    w1, b1, w2, b2, w3, b3, P = offsets(H, O)
    nl = tanh_header if nonlin == 'tanh' else (lambda v: np.where(v > 0, v, np.float32(0.0)).astype(np.float32))
    x = normalise_np(ob, mean, std)
    with np.errstate(all="ignore"):
        h1 = nl(dense4_np(x, th[w1:b1].reshape(OBS, H), th[b1:w2]))
        h2 = nl(dense4_np(h1, th[w2:b2].reshape(H, H), th[b2:w3]))
        out = dense4_np(h2, th[w3:b3].reshape(H, O), th[b3:P])
    return x, h1, h2, out, np.array([pick_dim_np(out, i, mode) for i in range(ADIM)], np.float32)


def random_theta(H, O, seed, scale=0.3):
    return (np.random.RandomState(seed).randn(offsets(H, O)[6]) * scale).astype(np.float32)


# ---- the mazes ---------------------------------------------------------------------------------------------------------------------------------
def one_wall_maze():
    return synthetic_maze(1)


def full_maze():
    """MAX_WALLS = 64 walls: the fixture's, then short walls far away from everything (x >= 1000) up to the count at which a loop that deals
    walls over 64 lanes has its edge"""
    header, lines = fixture_maze()
    extra = [[1000.0 + 10 * k, 1000.0, 1004.0 + 10 * k, 1003.0] for k in range(64 - len(lines))]
    return header, np.concatenate([lines, np.array(extra, np.float32).reshape(-1, 4)]).astype(np.float32)


def mazes():
    """{name: (header, lines)}: the fixture, every edge maze, one wall, 64 walls"""
    out = {"fixture": fixture_maze(), "one_wall": one_wall_maze(), "full": full_maze()}
    out.update({"edge_" + n: edge_maze(n) for n in EDGE_MAZES})
    return out


# ---- the experiments ---------------------------------------------------------------------------------------------------------------------------
def _exp(prefix, pop, calc_obstat_prob, ac_noise_std, eval_prob, hidden, ac_bins, nonlin, env_id, mode="centered_rank"):
    return {"config": {"calc_obstat_prob": calc_obstat_prob, "episodes_per_batch": pop, "eval_prob": eval_prob, "l2coeff": 0.005, "noise_stdev": 0.02,
                       "snapshot_freq": 0, "timesteps_per_batch": 10, "return_proc_mode": mode, "episode_cutoff_mode": "env_default"},
            "env_id": env_id, "exp_prefix": prefix, "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"},
            "policy": {"args": {"ac_bins": ac_bins, "ac_noise_std": ac_noise_std, "connection_type": "ff", "hidden_dims": [hidden, hidden],
                                "nonlin_type": nonlin}, "type": "MujocoPolicy"}}


def humanoid_exp(pop=8, calc_obstat_prob=0.5, ac_noise_std=0.01, eval_prob=1.0, hidden=64, ac_bins="continuous:", nonlin="tanh", env_id=ENV_ID):
    """configurations/humanoid.json with "env_id": "HardMaze-v0", at a test's size"""
    return _exp("humanoid", pop, calc_obstat_prob, ac_noise_std, eval_prob, hidden, ac_bins, nonlin, env_id)


def humanoid_nses_exp(pop=8, calc_obstat_prob=0.5, ac_noise_std=0.01, hidden=64, ac_bins="continuous:", nonlin="tanh", env_id=ENV_ID, algo_type="ns"):
    """configurations/humanoid_nses.json with "env_id": "HardMaze-v0": algo_type ns, centered_sign_rank, k 10, population 5,
    num_rollouts 5, novelty_prob; a small episodes_per_batch"""
    exp = _exp("humanoid", pop, calc_obstat_prob, ac_noise_std, 0.0, hidden, ac_bins, nonlin, env_id, "centered_sign_rank")
    exp["algo_type"] = algo_type
    exp["novelty_search"] = {"k": 10, "population_size": 5, "num_rollouts": 5, "selection_method": "novelty_prob"}
    return exp


def humanoid_nsres_exp(**kw):
    """configurations/humanoid_nsres.json likewise: algo_type nsr"""
    return humanoid_nses_exp(algo_type="nsr", **kw)


# ---- dne_mjmaze_rollout_host behind the Engine surface -------------------------------------------------------------------------------------------
class MjMazeHostEngine(OracleEngine):
    """The kind without a GPU: evaluations are dne_mjmaze_rollout_host on thetas perturbed in numpy, with the options, statistics, archive and
    novelty calls of the device engine (novelty: dne_maze_novelty_host); ranks, the weighted sum and the optimizer are the oracle's."""

    def __init__(self, hidden=64, n_out=2, ac_mode='continuous', nonlin='tanh', max_members=64, **kw):
        from dne_hip import _lib
        self.kind, self.n_actions, self.max_members, self.ref_count = _lib.KIND_MJMAZE, n_out, max_members, 0
        self.hidden, self.ac_mode, self.nonlin = hidden, ac_mode, nonlin
        self.P = _lib.mjmaze_num_params(hidden, n_out)
        self.bc_max_steps, self.bc_final_only = 0, False
        self.theta = np.zeros(self.P, np.float32)
        self.slots = {}
        self.noise = self.opt = self.members = self.maze = None
        self.mean = self.std = None
        self.options = None
        self.archive = np.zeros((0, 2), np.float32)
        self.calls, self.options_seen, self.ob_stats_seen, self.appends_seen = [], [], [], []

    def set_theta(self, theta, slot=0):
        if slot == 0:
            self.theta = np.array(theta, np.float32)
        self.slots[slot] = np.array(theta, np.float32)

    def maze_set_walls(self, header, lines):
        self.maze = (np.array(header, np.float32), np.array(lines, np.float32).reshape(-1, 4))

    def mjmaze_set_ob_stat(self, mean, std):
        self.mean, self.std = np.array(mean, np.float32), np.array(std, np.float32)
        self.ob_stats_seen.append((self.mean.copy(), self.std.copy()))

    def mjmaze_set_rollout_options(self, n, ac_noise_std=0.0, ac_off=None, stat_flag=None):
        from dne_hip import _lib
        if ac_off is not None and (np.asarray(ac_off) + AC_NOISE > self.noise.size).any():
            raise _lib.DneError("dne_mjmaze_set_rollout_options: an action-noise offset reaches past the noise table")
        self.options = (int(n), float(ac_noise_std), None if ac_off is None else np.array(ac_off, np.int64),
                        None if stat_flag is None else np.array(stat_flag, np.uint8))
        self.options_seen.append(self.options)

    def _run(self, thetas, tslimit):
        from dne_hip import _lib
        if self.maze is None:
            raise _lib.DneError("DNE_KIND_MJMAZE: no maze loaded (dne_maze_set_walls comes before an evaluation)")
        if self.mean is None:
            raise _lib.DneError("the observation statistics of a DNE_KIND_MJMAZE engine are NaN until dne_mjmaze_set_ob_stat is called")
        n, std, off, flag = self.options or (len(thetas), 0.0, None, None)
        assert n == len(thetas), "the rollout options were given for %d members, the evaluation runs %d" % (n, len(thetas))
        self.options = None                      # for the next evaluation only
        r = _lib.mjmaze_rollout_host(np.stack(thetas), self.maze[0], self.maze[1], self.hidden, self.mean, self.std, n_out=self.n_actions,
                                     ac_mode=self.ac_mode, nonlin=self.nonlin, tslimit=tslimit, ac_noise_std=std,
                                     table=self.noise if off is not None else None, ac_off=off, stat_flag=flag)
        self._last_run = r
        return r['returns'], r['signreturns'], r['lengths']

    def es_eval(self, idx, sigma, tslimit, seeds, want_bc=False):
        self.calls.append(("es_eval", len(idx)))
        th = [perturbed(self.theta, self.noise, int(i), s) for i in idx for s in (sigma, -sigma)]
        ret, sg, ln = self._run(th, tslimit)
        out = ret.reshape(-1, 2), sg.reshape(-1, 2), ln.reshape(-1, 2)
        self._last = (np.asarray(idx, np.int64),) + out
        return out

    def eval_members(self, n, tslimit, seeds, want_bc=False):
        slot, off, scale = self.members
        base = dict(self.slots); base[0] = self.theta
        return self._run([perturbed(base[int(slot[i])], self.noise, int(off[i]), scale[i]) for i in range(n)], tslimit)

    def mjmaze_ob_stats(self, n):
        r = self._last_run
        return r['ob_sum'][:n].copy(), r['ob_sumsq'][:n].copy(), r['ob_count'][:n].copy()

    def maze_final_state(self, n):
        return self._last_run['xy'][:n].copy()

    def maze_archive_clear(self):
        self.archive = np.zeros((0, 2), np.float32)

    def maze_archive_size(self):
        return len(self.archive)

    def maze_archive_append(self, xy=None, n=None):
        pts = self.maze_final_state(n) if xy is None else np.asarray(xy, np.float32).reshape(-1, 2)
        self.appends_seen.append(len(pts))
        self.archive = np.concatenate([self.archive, pts]).astype(np.float32)

    def maze_archive(self):
        return self.archive.copy()

    def maze_novelty(self, k, xy=None, n=None):
        from dne_hip import _lib
        if len(self.archive) < 1:
            raise _lib.DneError("dne_maze_novelty: the archive is empty (dne_maze_archive_append)")
        pts = self.maze_final_state(len(self._last_run['xy']) if n is None else n) if xy is None else np.asarray(xy, np.float32).reshape(-1, 2)
        return _lib.maze_novelty_host(pts, self.archive, k)


# ---- the drivers, shared by the CPU and the GPU tests --------------------------------------------------------------------------------------------
def run_nses(exp, me, we, noise, log_dir, iters=2, worker_seed=1234, master_seed=0, timeout=300):
    """nses.run_master on engine `me` and nses.run_worker on engine `we` for `iters` iterations, in this process, with the wire spied on.
    -> dict(theta_dict, archive, obstat_dict, optimizer_dict, pushed, tasks, ratios, parents)"""
    import threading
    import es_driver_support as D
    from dne_hip import dist, nses
    dist.reset_brokers()
    cfg = {"unix_socket_path": "/tmp/test_mjmaze_ns.sock", "transport": "inprocess"}
    out = {}

    declared = threading.Event()

    def master():
        try:
            out["r"] = nses.run_master(cfg, str(log_dir), exp, engine=me, noise=noise, max_iters=iters, seed=master_seed)
        except BaseException as e:   # noqa: B902
            out["error"] = e
            declared.set()

    def worker():
        try:
            nses.run_worker(cfg, cfg, noise, engine=we, max_tasks=iters, seed=worker_seed, reeval_after=1e9)
        except BaseException as e:   # noqa: B902
            out.setdefault("error", e)
    from dne_hip import tabular_logger
    parents = []
    with D.wire_spies(None, declared) as (pushed, tasks, ratios):
        record = tabular_logger.record_tabular
        tabular_logger.record_tabular = lambda key, val: (parents.append(int(val)) if key == "ParentId" else None, record(key, val))[1]
        tm, tw = threading.Thread(target=master, daemon=True), threading.Thread(target=worker, daemon=True)
        tm.start()
        assert declared.wait(timeout), "the master declared no task"
        if "error" in out:
            raise out["error"]
        tw.start()
        tm.join(timeout=timeout)
        tw.join(timeout=timeout if not tm.is_alive() else 1.0)
        if "error" in out:
            raise out["error"]
        assert not tm.is_alive() and not tw.is_alive(), "a driver thread did not return"
    theta_dict, archive, obstat_dict, optimizer_dict = out["r"]
    # the wire spy sits on the class: a worker thread an earlier test of the session left looping shows up in it too, under its own id
    wid = np.random.RandomState(worker_seed).randint(2 ** 31)
    pushed = [(t, r) for t, r in pushed if r.worker_id == wid]
    return dict(theta_dict=theta_dict, archive=np.asarray(archive, np.float32), obstat_dict=obstat_dict, optimizer_dict=optimizer_dict, pushed=list(pushed), tasks=list(tasks),
                ratios=list(ratios), parents=parents)


def check_nses_run(run, exp, noise, we_novelty):
    """what two iterations of nses / nsr must have left, whichever engine ran them"""
    import update_support as U
    from dne_hip import _lib, es, policies
    iters, pop, k = len(run['tasks']), exp['novelty_search']['population_size'], exp['novelty_search']['k']
    archive = run['archive']
    assert iters == 2 and archive.shape == (pop + iters, 2) and archive.dtype == np.float32       # the initial 5, then one point an iteration
    assert run['parents'][0] == 0 and len(run['parents']) == iters
    # the per-parent statistics advance only for the chosen parent
    shards = [r for _, r in run['pushed']]
    fresh = es.RunningStat((11,), eps=1e-2)
    want = {p: es.RunningStat((11,), eps=1e-2) for p in range(pop)}
    for p, r in zip(run['parents'], shards):
        if r.ob_count > 0:
            want[p].increment(r.ob_sum, r.ob_sumsq, r.ob_count)
    assert sum(r.ob_count for r in shards) > 0, "no coin landed: choose another worker seed"
    for p in range(pop):
        st = run['obstat_dict'][p]
        assert st.count == want[p].count and np.array_equal(st.sum, want[p].sum) and np.array_equal(st.sumsq, want[p].sumsq)
        if p not in run['parents']:
            assert st.count == fresh.count and not st.sum.any()
    assert np.array_equal(run['tasks'][0].ob_mean, fresh.mean) and np.array_equal(run['tasks'][0].ob_std, fresh.std)
    # the novelty in the Results is maze_novelty_host of the points, against the archive as it stood
    for i, (r, (pts, arch, kk, out)) in enumerate(zip(shards, we_novelty)):
        assert kk == k and len(arch) == pop + i and np.array_equal(arch, archive[:pop + i])
        assert r.signreturns_n2.dtype == np.float32 and (r.lengths_n2 == STEPS).all()
        assert np.array_equal(r.signreturns_n2, _lib.maze_novelty_host(pts, arch, k).astype(np.float32).reshape(-1, 2))
    # the first update: parent 0 from normc_flat(seed 0), by the numpy formulas of update_support
    r0 = shards[0]
    theta0 = policies.normc_flat(64, 2, 0, 11)
    assert np.array_equal(run['tasks'][0].params, theta0)
    proc = U.proc_np(r0.returns_n2, r0.signreturns_n2, exp['config']['return_proc_mode'])
    if exp['algo_type'] == 'nsr':
        proc = ((U.ranks_np(r0.returns_n2) + proc) / 2.0).astype(np.float32)
    g = U.weighted_sum_np(noise.noise, r0.noise_inds_n, U.pair_weights_np(proc), theta0.size, float(r0.returns_n2.size))
    new, m, v, ratio = U.adam_np(theta0, np.zeros_like(theta0), np.zeros_like(theta0), g, 1, 0.005, 0.01)
    after = run['theta_dict'][0] if run['parents'][1] != 0 else run['tasks'][1].params
    assert U.same_bits(after, new)
    assert abs(run['ratios'][0] - ratio) <= 1e-9 * ratio


def spy_novelty(we):
    """record (points, archive, k, result) of every maze_novelty call of engine `we`"""
    seen, inner = [], we.maze_novelty

    def spy(k, xy=None, n=None):
        out = inner(k, xy, n)
        seen.append((we.maze_final_state(n), we.maze_archive(), k, np.array(out)))
        return out
    we.maze_novelty = spy
    return seen
