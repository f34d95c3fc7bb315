#!/usr/bin/env python3
"""Deep-GA on the hard maze, timed on the device: what a generation costs with device-resident parents.

Population 5000, 20 parents, 400 steps per episode, the fixture maze.  Every figure is a median over --reps repetitions after --warmup, with
its min and max, from a host clock around a call that ends in a device synchronise.  Prints ONE JSON line:

  eval_ms / eval_kernel_ms   (a) dne_maze_ga_eval of the population as children of the bank (one k_maze_rollout launch; kernel = dne_profile.eval_ms)
  roots_eval_ms              the same for a generation of roots (k_maze_ga_roots in front of the rollout)
  promote_ms                 (b) dne_maze_ga_promote of 20 children
  build_ms                   (c) dne_maze_ga_build of 20 parents at genome depth 1, 100 and 1000: what a generation would pay without promotion
  iteration_ms               (d) one whole iteration of ga_gpu.main on this engine (10 validated individuals x 30 episodes, 200 test episodes, as
                             configurations/ga_atari_config.json shapes them), from one population evaluation to the next; the driver's own
                             TimestepsPerSecondThisIter; host_share = the part of an iteration not spent inside the three dne_maze_ga_eval
                             calls, dne_ga_select and the promotion
  identical                  the device's returns of (a) equal dne_maze_rollout_host on dne_maze_ga_members_host's thetas bit for bit, on the
                             first --check members (the timed work is the checked work)

A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/maze_ga_time.py [--population 5000] [--parents 20] [--reps 200] [--warmup 3] [--iterations 12] [--out FILE]
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


def timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=5000)
    ap.add_argument("--parents", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--check", type=int, default=256)
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
    scale_by = policies.simple_scale_by()

    def genomes(depth):
        return [(int(rs.randint(0, last + 1)), ) + tuple((int(i), a.power) for i in rs.randint(0, last + 1, size=depth - 1)) for _ in range(T)]

    eng = _lib.Engine(_lib.KIND_MAZE, 2, max_members=n)
    eng.noise_upload(noise)
    eng.maze_set_walls(header, lines)
    eng.maze_ga_set_init_scale(scale_by)

    build = {}
    for depth in (1, 100, 1000):
        g = genomes(depth)
        build[str(depth)] = stats(timed(lambda: eng.maze_ga_build(g), max(a.reps // 4, 1), a.warmup))
    bank = np.stack([eng.maze_ga_get_parent(j) for j in range(T)])

    parent = rs.randint(T, size=n).astype(np.int32)
    idx = rs.randint(0, last + 1, size=n).astype(np.int64)
    power = np.full(n, a.power, np.float32)
    kern = []

    def evaluate():
        out = eng.maze_ga_eval(parent, idx, power, _lib.MAZE_STEPS)
        kern.append(eng.profile()["eval_ms"])
        return out

    wall = timed(evaluate, a.reps, a.warmup)
    ret, _, ln = evaluate()
    c = min(a.check, n)
    thetas = _lib.maze_ga_members_host(noise, scale_by, bank, parent[:c], idx[:c], power[:c])
    hret, hln, _ = _lib.maze_rollout_host(thetas, header, lines, _lib.MAZE_STEPS)
    identical = bool(np.array_equal(ret[:c].view(np.uint32), hret.view(np.uint32)) and np.array_equal(ln[:c], hln))

    roots = np.full(n, -1, np.int32)
    roots_wall = timed(lambda: eng.maze_ga_eval(roots, idx, power, _lib.MAZE_STEPS), max(a.reps // 4, 1), a.warmup)

    # promotion keeps T parents, so it repeats on its own result: children of whatever the bank holds
    promote = timed(lambda: eng.maze_ga_promote(parent[:T], idx[:T], power[:T]), a.reps, a.warmup)

    # (d) the driver: ONE run; an iteration spans from one whole-population evaluation to the next (selection, validation, the elite's test
    # episodes, the promotion, the tabular row and snapshot.pkl included).  Generation 0 (roots, the first bank) and --warmup more are left out.
    calls = []

    class Clocked(object):
        """the engine with a host clock around the calls of the loop that go to the device"""

        def __init__(self, inner):
            self.inner = inner

        def __getattr__(self, name):
            attr = getattr(self.inner, name)
            if name not in ("maze_ga_eval", "maze_ga_promote", "maze_ga_build", "ga_select"):
                return attr

            def call(*args, **kw):
                t0 = time.perf_counter()
                try:
                    return attr(*args, **kw)
                finally:
                    calls.append((name, len(args[0]), t0, time.perf_counter()))
            return call

    reported = []
    record = tabular_logger.record_tabular
    tabular_logger.record_tabular = lambda key, val: (reported.append(float(val)) if key == "TimestepsPerSecondThisIter" else None, record(key, val))[1]
    table = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    table.noise, table._engines = noise, [eng]
    exp = {"game": "maze", "model": "SimpleClassifier", "population_size": n, "selection_threshold": T, "validation_threshold": 10,
           "num_validation_episodes": 30, "num_test_episodes": 200, "episode_cutoff_mode": "env_default", "mutation_power": a.power,
           "timesteps": 10 ** 12, "maze_file": a.maze}
    skip = 1 + a.warmup
    with tempfile.TemporaryDirectory() as log_dir, open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
        ga_gpu.main(log_dir, engine=Clocked(eng), noise=table, seed=1, max_iters=skip + a.iterations + 1, **exp)
    tabular_logger.record_tabular = record
    starts = [i - 1 for i, c in enumerate(calls) if c[0] == "ga_select"]       # the population's evaluation is the call in front of the selection
    it_ms, dev_ms = [], []
    for lo, hi in zip(starts[skip:-1], starts[skip + 1:]):
        it_ms.append((calls[hi][2] - calls[lo][2]) * 1e3)
        dev_ms.append(sum(c[3] - c[2] for c in calls[lo:hi]) * 1e3)
    tps = reported[skip:skip + len(it_ms)]
    eng.check_redzones()
    eng.close()

    out = {"tool": "maze_ga_time", "population": n, "parents": T, "steps_per_episode": _lib.MAZE_STEPS, "walls": int(lines.shape[0]), "reps": a.reps,
           "eval_ms": stats(wall), "eval_kernel_ms": stats(kern), "env_steps_per_s": int(np.sum(ln)) / (float(np.median(wall)) * 1e-3),
           "roots_eval_ms": stats(roots_wall), "promote_ms": stats(promote), "build_ms": build,
           "iteration_ms": stats(it_ms), "iteration_device_calls_ms": stats(dev_ms), "iterations": len(it_ms),
           "timesteps_per_iteration": n * 400 + 10 * 30 * 400, "timesteps_per_s_this_iter": stats(tps),
           "host_share": float(1.0 - np.median(dev_ms) / np.median(it_ms)), "identical": identical}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
