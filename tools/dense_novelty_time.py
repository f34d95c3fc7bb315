#!/usr/bin/env python3
"""What k_dense_novelty costs (csrc/dense_novelty.h), beside k_maze_novelty, and what a whole NS-ES iteration on a dense policy costs.

  (a) per D in (2, 4) and archive size: n members' BCs handed in from the host, engine.dense_novelty(k) on a DNE_KIND_DENSE handle of that D.
      kernel_ms is the scoring kernel between two device events (dense_novelty_last_ms), call_ms the whole call on the host clock: medians of
      --reps repetitions after --warmup, with [min, max].  identical: the novelties equal dne_dense_novelty_host's bit for bit.
  (b) for D = 2, beside it: engine.maze_novelty(k) of a DNE_KIND_MAZE handle on the same points and archive, the two alternated repetition by
      repetition; ratio_kernel = dense median / maze median, as measured.
  (c) one whole nses_gpu.main iteration (the second of a resumed run) on a (16, 16) relu dense engine on the maze and on LinearClassifier on the
      cart-pole: wall time of the iteration and the share of it spent inside the engine's calls.

Prints ONE JSON line (and writes it with --out).  A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/dense_novelty_time.py [--members 5000] [--k 10] [--archives 1000,10000] [--reps 20] [--warmup 3] [--population 1000] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


class Timed(object):
    """an engine whose every call is timed on the host clock (the calls end in a device synchronise or are host work of the binding)"""

    def __init__(self, engine):
        object.__setattr__(self, "_e", engine)
        object.__setattr__(self, "spent", 0.0)

    def __getattr__(self, name):
        v = getattr(self._e, name)
        if not callable(v):
            return v

        def call(*a, **kw):
            t0 = time.perf_counter()
            try:
                return v(*a, **kw)
            finally:
                object.__setattr__(self, "spent", self.spent + time.perf_counter() - t0)
        return call


def iteration(game, hidden, population, k, maze):
    """the wall time of one resumed nses_gpu.main iteration and the time inside engine calls, milliseconds"""
    from dne_hip import _lib, es, nses_gpu
    exp = {"game": game, "model": None, "algo_type": "nsr", "population_size": population, "timesteps": 10 ** 12,
           "novelty_search": {"k": k, "population_size": 3, "num_rollouts": 1, "selection_method": "round_robin"},
           "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "maze_file": maze}
    table = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    table.noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    table._engines = []
    eng = _lib.Engine(_lib.KIND_DENSE, 2, max_members=population, env=_lib.KIND_MAZE if game == "maze" else _lib.KIND_CARTPOLE, hidden=hidden, nonlin="relu")
    timed = Timed(eng)
    with tempfile.TemporaryDirectory() as log_dir:
        with open(os.devnull, "w") as null:
            old = sys.stdout
            sys.stdout = null
            try:
                nses_gpu.main(log_dir, engine=eng, noise=table, seed=0, max_iters=2, **exp)       # the start and two iterations: warm
                walls, inside = [], []
                for _ in range(5):
                    object.__setattr__(timed, "spent", 0.0)
                    t0 = time.perf_counter()
                    nses_gpu.main(log_dir, engine=timed, noise=table, seed=0, max_iters=1, **exp)
                    walls.append((time.perf_counter() - t0) * 1e3); inside.append(timed.spent * 1e3)
            finally:
                sys.stdout = old
    eng.close()
    i = int(np.argsort(walls)[len(walls) // 2])
    return {"game": game, "hidden": list(hidden), "population": population, "iteration_ms": stats(walls), "engine_calls_ms": stats(inside),
            "engine_share": inside[i] / walls[i]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=5000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--archives", default="1000,10000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--population", type=int, default=1000)
    ap.add_argument("--maze", default=os.path.join(ROOT, "tests", "golden", "hard_maze.txt"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib
    n, ok = a.members, True
    out = {"tool": "dense_novelty_time", "members": n, "k": a.k, "reps": a.reps, "warmup": a.warmup, "kernels": []}
    maze = _lib.Engine(_lib.KIND_MAZE, 2, max_members=16)
    for dim, env in ((2, _lib.KIND_MAZE), (4, _lib.KIND_CARTPOLE)):
        eng = _lib.Engine(_lib.KIND_DENSE, 2, max_members=16, env=env, hidden=(), nonlin="relu")
        for narch in (int(v) for v in a.archives.split(",")):
            rs = np.random.RandomState(narch + dim)
            archive = rs.uniform(0, 300, (narch, dim)).astype(np.float32)
            bc = rs.uniform(0, 300, (n, dim)).astype(np.float32)
            eng.dense_archive_clear(); eng.dense_archive_append(archive)
            if dim == 2:
                maze.maze_archive_clear(); maze.maze_archive_append(archive)
            kern, call, mkern, mcall = [], [], [], []
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                nov = eng.dense_novelty(a.k, bc)
                t1 = time.perf_counter()
                if dim == 2:
                    mnov = maze.maze_novelty(a.k, bc)
                    t2 = time.perf_counter()
                if rep >= a.warmup:
                    kern.append(eng.dense_novelty_last_ms()); call.append((t1 - t0) * 1e3)
                    if dim == 2:
                        mkern.append(maze.maze_novelty_last_ms()); mcall.append((t2 - t1) * 1e3)
            twin = _lib.dense_novelty_host(bc, archive, a.k)
            same = bool(np.array_equal(nov.view(np.uint64), twin.view(np.uint64)))
            row = {"D": dim, "archive": narch, "kernel_ms": stats(kern), "call_ms": stats(call), "identical": same}
            if dim == 2:
                same = same and bool(np.array_equal(mnov.view(np.uint64), twin.view(np.uint64)))
                row.update(maze_kernel_ms=stats(mkern), maze_call_ms=stats(mcall), identical=same,
                           ratio_kernel=float(np.median(kern) / np.median(mkern)))
            ok = ok and same
            out["kernels"].append(row)
        eng.check_redzones()
        eng.close()
    maze.close()
    out["iterations"] = [iteration("maze", (16, 16), a.population, a.k, a.maze), iteration("gym.CartPole-v1", (), a.population, a.k, a.maze)]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
