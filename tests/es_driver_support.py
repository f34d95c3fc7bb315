"""TEST-ONLY helpers shared by tests/test_gpu_es_drivers.py and the driver tests of tests/test_host_cpu.py: run one master/worker
scenario of dne_hip.es / dne_hip.es_modified on a given pair of engines with spies on everything that crosses the wire, and compare
two such runs value by value.  The engines may be the HIP engine or tests/oracle_engine.py:OracleEngine -- the drivers cannot tell."""
import contextlib
import threading
from collections import namedtuple

import numpy as np

NACT, NREF = 18, 16
RESULT_ARRAYS = ("noise_inds_n", "returns_n2", "signreturns_n2", "lengths_n2")
ADAM = {"type": "adam", "args": {"stepsize": 0.01}}

# theta: the returned policy's flat vector; pushed: every (task_id, Result) a worker pushed, in order; tasks: every declared Task, in
# order; ratios: the UpdateRatio the master logged per generation; evals / updates: the worker engine's eval_members and the master
# engine's es_update calls (positional arguments)
DriverRun = namedtuple("DriverRun", "theta policy pushed tasks ratios evals updates")


def es_exp(pop=8, cutoff=24, mode="centered_rank", optimizer=None, eval_prob=1.0, snapshot_freq=0):
    return {"config": {"calc_obstat_prob": 0.0, "episodes_per_batch": pop, "eval_prob": eval_prob, "l2coeff": 0.005,
                       "noise_stdev": 0.02, "snapshot_freq": snapshot_freq, "timesteps_per_batch": 10,
                       "return_proc_mode": mode, "episode_cutoff_mode": cutoff},
            "env_id": "FrostbiteNoFrameskip-v4", "optimizer": optimizer or ADAM, "policy": {"args": {}, "type": "ESAtariPolicy"}}


class _Stop(Exception):
    """ends a worker that loops without max_tasks once its master has returned"""


def record_calls(engine, name):
    """Wrap engine.<name> on this instance; -> the list its positional arguments are appended to, call by call."""
    calls, inner = [], getattr(engine, name)

    def spy(*a, **k):
        calls.append(tuple(np.array(x) if isinstance(x, np.ndarray) else x for x in a))
        return inner(*a, **k)
    setattr(engine, name, spy)
    return calls


@contextlib.contextmanager
def wire_spies(stop=None, declared=None):
    """Record WorkerClient.push_result, MasterClient.declare_task and the logged UpdateRatio for the duration of the block.
    stop (Event): once set, the next push ends its worker; declared (Event): set when the first task is on the wire."""
    from dne_hip import dist, tabular_logger
    pushed, tasks, ratios = [], [], []
    push, declare, record = dist.WorkerClient.push_result, dist.MasterClient.declare_task, tabular_logger.record_tabular

    def spy_push(self, task_id, result):
        if stop is not None and stop.is_set():
            raise _Stop()
        pushed.append((task_id, result))
        return push(self, task_id, result)

    def spy_declare(self, task_data):
        tasks.append(task_data)
        task_id = declare(self, task_data)
        if declared is not None:
            declared.set()
        return task_id

    def spy_record(key, val):
        if key == "UpdateRatio":
            ratios.append(val)
        return record(key, val)

    dist.WorkerClient.push_result, dist.MasterClient.declare_task, tabular_logger.record_tabular = spy_push, spy_declare, spy_record
    try:
        yield pushed, tasks, ratios
    finally:
        dist.WorkerClient.push_result, dist.MasterClient.declare_task, tabular_logger.record_tabular = push, declare, record


def run_driver(mod, exp, me, we, noise, log_dir, iters, *, master_cfg=None, relay_cfg=None, worker_master_cfg=None, master_seed=0,
               worker_seed=7, max_tasks="iters", reeval_after=1e9, master_kw=None, timeout=120):
    """mod.run_master on engine `me` and mod.run_worker on engine `we`, each on a daemon thread of this process, for `iters` generations.
    The worker starts once the first task is declared (over Redis a worker that finds no experiment or task yet sleeps for seconds
    between its looks, dist.py:46-64).  Both threads are joined with a timeout and must have ended; an exception in either is raised
    here.  max_tasks=None: the worker loops like a reference worker and is stopped (at its next push) once the master has returned."""
    from dne_hip import dist
    dist.reset_brokers()
    master_cfg = master_cfg or {"unix_socket_path": "/tmp/dne_es_drivers.sock", "transport": "inprocess"}
    worker_master_cfg = worker_master_cfg or master_cfg
    relay_cfg = relay_cfg or worker_master_cfg
    max_tasks = iters if max_tasks == "iters" else max_tasks
    out, stop, declared = {}, threading.Event(), threading.Event()
    evals, updates = record_calls(we, "eval_members"), record_calls(me, "es_update")

    def master():
        try:
            out["policy"] = mod.run_master(master_cfg, str(log_dir), exp, engine=me, noise=noise, max_iters=iters, seed=master_seed,
                                           **(master_kw or {}))
        except BaseException as e:       # noqa: B902  (reported by the joining thread)
            out["master_error"] = e
            declared.set()

    def worker():
        try:
            mod.run_worker(worker_master_cfg, relay_cfg, noise, engine=we, max_tasks=max_tasks, seed=worker_seed, reeval_after=reeval_after)
        except _Stop:
            pass
        except BaseException as e:       # noqa: B902
            out["worker_error"] = e

    with wire_spies(stop if max_tasks is None else None, declared) as (pushed, tasks, ratios):
        tm, tw = threading.Thread(target=master, daemon=True), threading.Thread(target=worker, daemon=True)
        tm.start()
        assert declared.wait(timeout), "the master declared no task"
        if "master_error" in out:
            raise out["master_error"]
        tw.start()
        tm.join(timeout=timeout)
        stop.set()
        tw.join(timeout=timeout if not tm.is_alive() else 1.0)
        for k in ("master_error", "worker_error"):
            if k in out:
                raise out[k]
        assert not tm.is_alive(), "the master did not return: %d Results pushed, %d tasks declared" % (len(pushed), len(tasks))
        assert not tw.is_alive(), "the worker did not return: %d Results pushed, %d tasks declared" % (len(pushed), len(tasks))
    policy = out["policy"]
    return DriverRun(policy.get_trainable_flat(), policy, list(pushed), list(tasks), list(ratios), evals, updates)


def _same_array(a, b, where):
    if a is None or b is None:
        assert a is None and b is None, where
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a, b), (where, a, b)


def assert_same_results(want, got, what):
    """Every pushed Result of two runs, in order, field by field (arrays: equal values, shapes and dtypes; scalars: ==)."""
    assert len(want) == len(got), (what, len(want), len(got))
    for k, ((wt, w), (gt, g)) in enumerate(zip(want, got)):
        where = "%s: pushed Result %d, iteration %d" % (what, k, wt)
        assert wt == gt and type(w) is type(g), where
        for f in RESULT_ARRAYS:
            _same_array(getattr(w, f), getattr(g, f), where + ", " + f)
        assert w.eval_return == g.eval_return and type(w.eval_return) is type(g.eval_return), (where, "eval_return", w.eval_return, g.eval_return)
        assert w.eval_length == g.eval_length and type(w.eval_length) is type(g.eval_length), (where, "eval_length", w.eval_length, g.eval_length)
        assert w.ob_count == g.ob_count, (where, "ob_count")
        if hasattr(w, "bc_vectors"):
            assert len(w.bc_vectors) == len(g.bc_vectors), (where, "bc_vectors")
            for j, (wv, gv) in enumerate(zip(w.bc_vectors, g.bc_vectors)):
                _same_array(wv[0], gv[0], where + ", bc_vectors[%d][0]" % j)
                for c, (x, y) in enumerate(zip(wv[1:], gv[1:]), 1):
                    assert x == y and type(x) is type(y), (where, "bc_vectors[%d][%d]" % (j, c), x, y)


def assert_same_run(want, got, what):
    """The whole comparison of a scenario: Results, the time limit of every declared Task, theta bit for bit, UpdateRatio to 1e-9
    relative (the bound tests/test_gpu_parity.py:test_reduce_and_update holds the ratio to)."""
    assert_same_results(want.pushed, got.pushed, what)
    assert [t.timestep_limit for t in want.tasks] == [t.timestep_limit for t in got.tasks], what
    for it, (w, g) in enumerate(zip(want.tasks, got.tasks)):
        _same_array(w.params, g.params, "%s: Task.params, iteration %d" % (what, it))
        _same_array(w.ref_batch, g.ref_batch, "%s: Task.ref_batch, iteration %d" % (what, it))
    assert len(want.ratios) == len(got.ratios) == len(want.tasks), what
    for it, (w, g) in enumerate(zip(want.ratios, got.ratios)):
        assert abs(g - w) <= 1e-9 * w, ("%s: UpdateRatio, iteration %d" % (what, it), w, g)
    _same_array(want.theta, got.theta, what + ": returned theta")


def eval_episodes(run):
    """[(task_id, Result, seed, tslimit)] of a run's evaluation episodes: the k-th evaluation Result goes with the worker engine's
    k-th eval_members call."""
    ev = [(t, r) for t, r in run.pushed if r.eval_length is not None]
    assert len(ev) == len(run.evals)
    return [(t, r, int(c[2][0]), int(c[1])) for (t, r), c in zip(ev, run.evals)]


def episodes_ended_by_game_over(oracle, run):
    """The evaluation episodes of `run` that ended by game over: shorter than their limit, and replayed by the oracle (same theta,
    reference batch and seed, one step more allowed) they end at the same length with the game-over byte of the final RAM set."""
    L, over = oracle.layout(oracle.KIND_ES, NACT), []
    for task_id, res, seed, tslimit in eval_episodes(run):
        if res.eval_length >= tslimit:
            continue
        task = run.tasks[task_id]
        r, _, l, traj = oracle.rollout(L, task.params, np.asarray(task.ref_batch), seed, res.eval_length + 1, want_bc=True)
        assert (r, l) == (res.eval_return, res.eval_length), (task_id, r, l, res)
        if traj[-1][9]:
            over.append((task_id, res.eval_length))
    return over
