"""TEST-ONLY support for the Deep GA with MujocoPolicy (csrc/mujoco_ga.h, dne_hip/ga_mujoco.py): the contract in float32
numpy in the test's own words -- a root is the noise slice with every weight column divided by numpy's OWN np.sqrt(np.square(w).sum(axis=0)) of
its [K][C] view and every bias +0, a mutation is two unfused roundings --, the shapes both test files share, the host engines of the two
kinds with the mujoco_ga_* surface over the host twins (so that ga_mujoco's drivers run without a GPU), and the driver runner.  Every
comparison is bit for bit; a NaN (a column whose squares sum to 0) has to stand at the same places."""
import threading

import numpy as np

import mjmaze_support as MS
import pendulum_support as PS

KIND_PENDULUM, KIND_MJMAZE = 6, 7
OBS = {KIND_PENDULUM: 3, KIND_MJMAZE: 11}
HS = (64, 128, 256)
OUTS = {KIND_PENDULUM: tuple(range(1, 17)), KIND_MJMAZE: tuple(range(2, 17, 2))}
TABLE = 1 << 18                                   # the GPU tests' noise table


def blocks(kind, H, O):
    """[(weights at, K, C, biases at)] of l0, l1, out in the flat vector, and P"""
    out, o = [], 0
    for K, C in ((OBS[kind], H), (H, H), (H, O)):
        out.append((o, K, C, o + K * C))
        o += K * C + C
    return out, o


def num_params(kind, H, O):
    return blocks(kind, H, O)[1]


def noise(count=TABLE, seed=11):
    n = np.random.RandomState(seed).randn(count).astype(np.float32)
    n.setflags(write=False)
    return n


_noise = {}


def table(count=TABLE):
    if count not in _noise:
        _noise[count] = noise(count)
    return _noise[count]


# ---- the contract --------------------------------------------------------------------------------------------------------------------------------
def colscale_np(x, kind, H, O, std=1.0):
    """numpy's own statement (tf_util.py:125): std / np.sqrt(np.square(w).sum(axis=0, keepdims=True)) on every [K][C] view of the slice x [P]"""
    out = []
    with np.errstate(all="ignore"):
        for w0, K, C, _ in blocks(kind, H, O)[0]:
            w = np.array(x[w0:w0 + K * C], np.float32).reshape(K, C)
            out.append((std / np.sqrt(np.square(w).sum(axis=0, keepdims=True))).astype(np.float32).reshape(-1))
    return np.concatenate(out)


def root_np(tab, kind, H, O, idx):
    """tf_util.py:149-158 on the slice: weights *= the column scale, biases = 0"""
    bl, P = blocks(kind, H, O)
    x = np.array(tab[idx:idx + P], np.float32)
    th = np.zeros(P, np.float32)
    with np.errstate(all="ignore"):
        for w0, K, C, _ in bl:
            w = x[w0:w0 + K * C].reshape(K, C).copy()
            w *= 1.0 / np.sqrt(np.square(w).sum(axis=0, keepdims=True))
            th[w0:w0 + K * C] = w.reshape(-1)
    return th


def perturbed(base, tab, off, scale):
    with np.errstate(all="ignore"):
        return (np.asarray(base, np.float32) + np.float32(scale) * tab[off:off + len(base)]).astype(np.float32)


def genome_np(tab, kind, H, O, genome):
    th = root_np(tab, kind, H, O, int(genome[0][0] if isinstance(genome[0], (tuple, list)) else genome[0]))
    for idx, power in genome[1:]:
        th = perturbed(th, tab, int(idx), power)
    return th


def member_np(tab, kind, H, O, bank, parent, idx, power):
    if parent < 0:
        return root_np(tab, kind, H, O, idx)
    if idx < 0:
        return np.array(bank[parent], np.float32)
    return perturbed(bank[parent], tab, idx, power)


def members_np(tab, kind, H, O, bank, parent, idx, power):
    power = np.broadcast_to(np.asarray(power, np.float32), np.shape(parent))
    return np.stack([member_np(tab, kind, H, O, bank, int(a), int(b), c) for a, b, c in zip(parent, idx, power)])


def chain_genome(chain, sigma):
    return (int(chain[0]), ) + tuple((int(s), float(sigma)) for s in chain[1:])


def same(a, b):
    """bit for bit where neither is a NaN, NaN at the same places"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def zero_column_table(kind, H, O, idx, layer, col, count=TABLE):
    """the table with column `col` of weight block `layer` of the slice at idx set to +-0"""
    n = table(count).copy()
    w0, K, C, _ = blocks(kind, H, O)[0][layer]
    n[idx + w0 + col + C * np.arange(K)] = np.where(np.arange(K) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    n.setflags(write=False)
    return n


# ---- the two kinds without a GPU ---------------------------------------------------------------------------------------------------------------------
class _GaHost(object):
    """mujoco_ga_* over dne_mujoco_ga_theta_host / _members_host and the kind's rollout twin; the words of the refusals are the engine's"""
    ga_kind = None

    def _ga_init(self):
        self.T_max, self.bank, self.ga_calls, self.evals = None, np.zeros((0, self.P), np.float32), [], []

    def _shape(self):
        return self.ga_kind, self.hidden, self.n_actions

    def _need(self, call):
        from dne_hip import _lib
        if self.T_max is None:
            raise _lib.DneError("dne_%s: no bank (dne_mujoco_ga_reserve comes first)" % call)
        if self.noise is None:
            raise _lib.DneError("dne_%s: noise table not uploaded (dne_noise_upload)" % call)

    def _count(self, call, T):
        from dne_hip import _lib
        if not 1 <= T <= self.T_max:
            raise _lib.DneError("dne_%s: T = %d outside [1, T_max = %d]" % (call, T, self.T_max))

    def mujoco_ga_reserve(self, T_max):
        self._ga_init()
        self.T_max = int(T_max)
        self.ga_calls.append(("reserve", int(T_max)))

    def mujoco_ga_build(self, genomes):
        from dne_hip import _lib
        self._need("mujoco_ga_build")
        self._count("mujoco_ga_build", len(genomes))
        self.ga_calls.append(("build", len(genomes)))
        self.bank = np.stack([_lib.mujoco_ga_theta_host(self.noise, *self._shape(), g) for g in genomes])

    def mujoco_ga_promote(self, parent, idx, power):
        from dne_hip import _lib
        self._need("mujoco_ga_promote")
        parent = np.asarray(parent, np.int32).reshape(-1)
        self._count("mujoco_ga_promote", len(parent))
        self.ga_calls.append(("promote", len(parent)))
        self.bank = _lib.mujoco_ga_members_host(self.noise, *self._shape(), self.bank if len(self.bank) else None, parent, idx, power)

    def mujoco_ga_eval(self, parent, idx, power, tslimit, env_seed=None):
        from dne_hip import _lib
        self._need("mujoco_ga_eval")
        parent, idx = np.asarray(parent, np.int32).reshape(-1), np.asarray(idx, np.int64).reshape(-1)
        if not 1 <= len(parent) <= self.max_members:
            raise _lib.DneError("dne_mujoco_ga_eval: n = %d outside [1, max_members = %d]" % (len(parent), self.max_members))
        if np.any((idx < 0) & (parent >= 0)):
            raise _lib.DneError("dne_mujoco_ga_eval: the kept form is for promotion only")
        self.ga_calls.append(("eval", len(parent)))
        th = _lib.mujoco_ga_members_host(self.noise, *self._shape(), self.bank if len(self.bank) else None, parent, idx, power)
        out = self._ga_run(list(th), tslimit, env_seed)
        self.evals.append(dict(parent=parent.copy(), idx=idx.copy(), power=np.array(power, np.float32), thetas=th, tslimit=tslimit,
                               seeds=None if env_seed is None else np.array(env_seed, np.uint32), returns=out[0].copy(), lengths=out[2].copy(),
                               options=self.options_seen[-1] if self.options_seen else None,
                               ob=tuple(self._last_run[k].copy() for k in ("ob_sum", "ob_sumsq", "ob_count"))))
        return out

    def mujoco_ga_parents(self):
        return len(self.bank)

    def mujoco_ga_get_parent(self, j):
        return self.bank[j].copy()


class PendulumGaHostEngine(_GaHost, PS.PendulumHostEngine):
    ga_kind = KIND_PENDULUM

    def __init__(self, *a, **kw):
        PS.PendulumHostEngine.__init__(self, *a, **kw)
        self._ga_init()

    def _ga_run(self, thetas, tslimit, env_seed):
        from dne_hip import _lib
        if env_seed is None:
            raise _lib.DneError("dne_mujoco_ga_eval: a DNE_KIND_PENDULUM engine resets every member from its environment seed, env_seed is NULL")
        return self._run(thetas, tslimit, env_seed)


class MjMazeGaHostEngine(_GaHost, MS.MjMazeHostEngine):
    ga_kind = KIND_MJMAZE

    def __init__(self, *a, **kw):
        MS.MjMazeHostEngine.__init__(self, *a, **kw)
        self._ga_init()

    def _ga_run(self, thetas, tslimit, env_seed):
        return self._run(thetas, tslimit)


def host_engine(kind, hidden=64, n_out=None, ac_mode="continuous", nonlin="tanh", max_members=16, count=TABLE):
    if kind == KIND_PENDULUM:
        e = PendulumGaHostEngine(hidden, 1 if n_out is None else n_out, ac_mode, nonlin, max_members)
    else:
        e = MjMazeGaHostEngine(hidden, 2 if n_out is None else n_out, ac_mode, nonlin, max_members)
        e.maze_set_walls(*MS.fixture_maze())
    if count:
        e.noise_upload(table(count))
    return e


def device_engine(kind, hidden=64, n_out=None, ac_mode="continuous", nonlin="tanh", max_members=16, count=TABLE, tab=None):
    from dne_hip import _lib
    n_out = (1 if kind == KIND_PENDULUM else 2) if n_out is None else n_out
    e = _lib.Engine(kind, n_out, max_members=max_members, hidden=hidden, ac_mode=ac_mode, nonlin=nonlin)
    if kind == KIND_MJMAZE:
        e.maze_set_walls(*MS.fixture_maze())
    e.noise_upload(table(count) if tab is None else tab)
    return e


def set_stat(e, kind):
    if kind == KIND_PENDULUM:
        e.pendulum_set_ob_stat(np.array([0.1, -0.2, 0.3], np.float32), np.array([0.8, 0.7, 2.5], np.float32))
    else:
        e.mjmaze_set_ob_stat(MS.MEAN, MS.STD)


def engine_calls(e, kind):
    """(set_rollout_options, ob_stats, final_state) of an engine of `kind`"""
    if kind == KIND_PENDULUM:
        return e.pendulum_set_rollout_options, e.pendulum_ob_stats, e.pendulum_final_state
    return e.mjmaze_set_rollout_options, e.mjmaze_ob_stats, e.maze_final_state


def ga_exp(kind, pop=8, population_size=4, num_elites=1, calc_obstat_prob=0.5, hidden=64, **kw):
    """configurations/humanoid.json under the GA: env_id, population_size, num_elites"""
    exp = (PS if kind == KIND_PENDULUM else MS).humanoid_exp(pop=pop, calc_obstat_prob=calc_obstat_prob, hidden=hidden, **kw)
    exp["population_size"], exp["num_elites"] = population_size, num_elites
    return exp


# ---- the drivers, shared by the CPU and the GPU tests --------------------------------------------------------------------------------------------------
def run_ga(exp, me, we, noise_table, log_dir, iters, worker_seed=1234, bank_reuse=True, timeout=120):
    """ga_mujoco.run_master on engine `me` and ga_mujoco.run_worker on engine `we` for `iters` iterations, in this process, with the wire spied on
    -> dict(policy, population, scores, pushed [(task id, Result)] of this worker, tasks)"""
    import es_driver_support as D
    from dne_hip import dist, ga_mujoco
    dist.reset_brokers()
    cfg = {"unix_socket_path": "/tmp/test_mujoco_ga.sock", "transport": "inprocess"}
    out, declared = {}, threading.Event()

    def master():
        try:
            out["r"] = ga_mujoco.run_master(cfg, str(log_dir), exp, engine=me, noise=noise_table, max_iters=iters)
        except BaseException as e:   # noqa: B902
            out["error"] = e
            declared.set()

    def worker():
        try:
            ga_mujoco.run_worker(cfg, cfg, noise_table, engine=we, max_tasks=iters, seed=worker_seed, reeval_after=1e9, bank_reuse=bank_reuse)
        except BaseException as e:   # noqa: B902
            out.setdefault("error", e)

    with D.wire_spies(None, declared) as (pushed, tasks, _):
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
    policy, population, scores = out["r"]
    wid = np.random.RandomState(worker_seed).randint(2 ** 31)     # (the spy sits on the class: keep this worker's Results)
    return dict(policy=policy, theta=policy.get_trainable_flat(), population=population, scores=np.asarray(scores),
                pushed=[(t, r) for t, r in pushed if r.worker_id == wid], tasks=list(tasks))


def assert_same_ga_runs(a, b, what):
    assert len(a["pushed"]) == len(b["pushed"]), what
    for (s, x), (t, y) in zip(a["pushed"], b["pushed"]):
        assert s == t and x.noise_inds_n == y.noise_inds_n and x.ob_count == y.ob_count, what
        assert x.eval_return == y.eval_return and x.eval_length == y.eval_length, what
        for f in ("returns_n2", "signreturns_n2", "lengths_n2", "ob_sum", "ob_sumsq"):
            u, v = getattr(x, f), getattr(y, f)
            assert (u is None and v is None) or (u.dtype == v.dtype and np.array_equal(u, v)), (what, f)
    assert [[list(c) for c in p] for p in (a["population"], )] == [[list(c) for c in p] for p in (b["population"], )], what
    assert np.array_equal(a["scores"].view(np.uint32), b["scores"].view(np.uint32)), what
    assert same(a["theta"], b["theta"]), what
    for s, t in zip(a["tasks"], b["tasks"]):
        assert same(s.params, t.params) and [list(c) for c in s.population] == [list(c) for c in t.population], what
