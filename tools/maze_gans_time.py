#!/usr/bin/env python3
"""GA-NS on the hard maze, timed on the device: what scoring a generation against archive and population costs, on the device against on the host.

Population 5000, 20 parents, k = 25, 400 steps per episode, the fixture maze.  Every figure is a median over repetitions after --warmup, with
its min and max, from a host clock around calls that end in a device synchronise.  Per archive size (0 / 1000 / 10 000 points):

  (a) device_ms         maze_ga_eval + maze_novelty_pool(k) where k_maze_rollout left the final positions + maze_archive_append_members of the
                        members a 1 % mask picks (the archive is set back to its size before every repetition); pool_kernel_ms is
                        k_maze_novelty_pool alone between two device events, pool_call_ms and append_call_ms the two calls on the host clock
  (b) host_ms           the only form a tree without the kernel has: maze_ga_eval + maze_final_state + the dense numpy scoring on the host -- the
                        [population][archive + population] float64 matrix, the diagonal masked, a partition per row, the k smallest sorted
                        and averaged; host_scoring_ms is that scoring alone
  identical             the device's novelties equal dne_maze_novelty_pool_host's bit for bit (the timed work is the checked work)

  (c) iteration_ms      one whole iteration of ga_gpu.main with exp['novelty_search'] on this engine (10 validated individuals x 30 episodes, 200
                        test episodes), from one population evaluation to the next, the archive growing by archive_prob 0.01 from empty;
                        host_share = the part of an iteration not spent inside the engine's calls; sort_ms is the stable host sort of the
                        5000 doubles alone

Prints ONE JSON line (and writes it with --out).  A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/maze_gans_time.py [--population 5000] [--parents 20] [--k 25] [--archives 0,1000,10000] [--reps 50] [--host-reps 5] [--out FILE]
"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def host_scoring(xy, archive, k):
    """the pool novelty, dense: one [n][A + n] float64 matrix, the member's own column masked, the k smallest of every row, their mean"""
    p = xy.astype(np.float64)
    pool = np.concatenate([archive.astype(np.float64), p])
    d = np.sqrt((pool[None, :, 0] - p[:, None, 0]) ** 2 + (pool[None, :, 1] - p[:, None, 1]) ** 2)
    d[np.arange(len(p)), len(archive) + np.arange(len(p))] = np.inf
    kk = min(k, pool.shape[0] - 1)
    return np.sort(np.partition(d, kk - 1, axis=1)[:, :kk], axis=1).mean(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=5000)
    ap.add_argument("--parents", type=int, default=20)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--archives", default="0,1000,10000")
    ap.add_argument("--archive-prob", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--power", type=float, default=0.005)
    ap.add_argument("--maze", default=os.path.join(ROOT, "tests", "golden", "hard_maze.txt"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, es, ga_gpu, policies, tabular_logger
    n, T = a.population, a.parents
    header, lines = _lib.load_maze(a.maze)
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    last = noise.size - 498
    rs = np.random.RandomState(0)

    eng = _lib.Engine(_lib.KIND_MAZE, 2, max_members=n)
    eng.noise_upload(noise)
    eng.maze_set_walls(header, lines)
    eng.maze_ga_set_init_scale(policies.simple_scale_by())
    eng.maze_ga_build([(int(i), ) for i in rs.randint(0, last + 1, size=T)])
    parent = rs.randint(T, size=n).astype(np.int32)
    idx = rs.randint(0, last + 1, size=n).astype(np.int64)
    power = np.full(n, 0.02, np.float32)                         # (wide enough for the children to end at many different points)
    picked = np.flatnonzero(rs.random_sample(n) < a.archive_prob).astype(np.int32)
    gen = lambda: eng.maze_ga_eval(parent, idx, power, _lib.MAZE_STEPS)

    out = {"tool": "maze_gans_time", "population": n, "parents": T, "k": a.k, "walls": int(lines.shape[0]), "reps": a.reps, "host_reps": a.host_reps,
           "appended_per_generation": int(picked.size), "gen_ms": stats([0.0]), "archives": []}
    for _ in range(a.warmup):
        gen()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        gen()
        wall.append((time.perf_counter() - t0) * 1e3)
    out["gen_ms"] = stats(wall)
    ok = True
    for narch in (int(v) for v in a.archives.split(",")):
        archive = np.random.RandomState(narch).uniform(0, 300, (narch, 2)).astype(np.float32)

        def reset():
            eng.maze_archive_clear()
            if narch:
                eng.maze_archive_append(archive)

        def device():
            gen()
            t1 = time.perf_counter()
            nov = eng.maze_novelty_pool(a.k)
            t2 = time.perf_counter()
            eng.maze_archive_append_members(picked)
            return nov, t1, t2, time.perf_counter()

        for _ in range(a.warmup):
            reset(); device()
        both, call, kern, app = [], [], [], []
        for _ in range(a.reps):
            reset()
            t0 = time.perf_counter()
            nov, t1, t2, t3 = device()
            both.append((t3 - t0) * 1e3); call.append((t2 - t1) * 1e3); app.append((t3 - t2) * 1e3); kern.append(eng.maze_novelty_last_ms())
        assert eng.maze_archive_size() == narch + picked.size
        host_all, host_score = [], []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            gen()
            xy = eng.maze_final_state(n)
            t1 = time.perf_counter()
            host_nov = host_scoring(xy, archive, a.k)
            t2 = time.perf_counter()
            host_all.append((t2 - t0) * 1e3); host_score.append((t2 - t1) * 1e3)
        twin = _lib.maze_novelty_pool_host(xy, archive, a.k)
        same = bool(np.array_equal(nov.view(np.uint64), twin.view(np.uint64)))
        ok = ok and same
        out["archives"].append({"archive": narch, "device_ms": stats(both), "pool_call_ms": stats(call), "pool_kernel_ms": stats(kern),
                                "append_call_ms": stats(app), "host_ms": stats(host_all), "host_scoring_ms": stats(host_score), "identical": same,
                                "distinct_points": int(len(np.unique(xy, axis=0))),
                                "host_numpy_max_rel_diff": float(np.max(np.abs(host_nov - twin) / np.where(twin == 0, 1.0, twin)))})

    # (c) the driver: ONE run; an iteration spans from one whole-population evaluation to the next
    calls = []
    DEVICE = ("maze_ga_eval", "maze_ga_promote", "maze_ga_build", "ga_select", "maze_novelty_pool", "maze_archive_append_members", "maze_archive")

    class Clocked(object):
        """the engine with a host clock around the calls of the loop that go to the device"""

        def __init__(self, inner):
            self.inner = inner

        def __getattr__(self, name):
            attr = getattr(self.inner, name)
            if name not in DEVICE:
                return attr

            def call(*args, **kw):
                t0 = time.perf_counter()
                try:
                    return attr(*args, **kw)
                finally:
                    calls.append((name, t0, time.perf_counter()))
            return call

    table = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    table.noise, table._engines = noise, [eng]
    exp = {"game": "maze", "model": "SimpleClassifier", "population_size": n, "selection_threshold": T, "validation_threshold": 10,
           "num_validation_episodes": 30, "num_test_episodes": 200, "episode_cutoff_mode": "env_default", "mutation_power": a.power,
           "timesteps": 10 ** 12, "maze_file": a.maze, "novelty_search": {"k": a.k, "archive_prob": a.archive_prob}}
    skip = 1 + a.warmup
    with tempfile.TemporaryDirectory() as log_dir, open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
        _, _, state = ga_gpu.main(log_dir, engine=Clocked(eng), noise=table, seed=1, max_iters=skip + a.iterations + 1, **exp)
    starts = [i - 1 for i, c in enumerate(calls) if c[0] == "maze_novelty_pool"]      # the population's evaluation is the call in front of the scoring
    it_ms, dev_ms = [], []
    for lo, hi in zip(starts[skip:-1], starts[skip + 1:]):
        it_ms.append((calls[hi][1] - calls[lo][1]) * 1e3)
        dev_ms.append(sum(c[2] - c[1] for c in calls[lo:hi]) * 1e3)
    doubles = np.random.RandomState(9).uniform(0, 50, n)
    sort_ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        np.argsort(-doubles, kind="stable")
        sort_ms.append((time.perf_counter() - t0) * 1e3)
    eng.check_redzones()
    eng.close()
    out.update({"iteration_ms": stats(it_ms), "iteration_device_calls_ms": stats(dev_ms), "iterations": len(it_ms),
                "host_share": float(1.0 - np.median(dev_ms) / np.median(it_ms)), "sort_ms": stats(sort_ms),
                "archive_after_driver": int(state.archive.shape[0]), "identical": ok})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
