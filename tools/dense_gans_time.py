#!/usr/bin/env python3
"""GA-NS on a dense policy, timed on the device: what scoring a generation against archive and population costs, on the device against on the host.

Population 5000, 20 parents, k = 25, the environment's own step limit; D = 2 is a dense policy without a hidden layer on the fixture maze, D = 4
a (5, 33) relu policy on the cart-pole.  Every figure is a median over repetitions after --warmup, with its min and max.  Per D and archive
size (0 / 1000 / 10 000 points):

  (a) device_ms         dense_ga_eval + dense_novelty_pool(k) on the BCs of that evaluation + dense_archive_append_members of the members a 1 %
                        mask picks (the archive is set back to its size before every repetition), on a host clock around calls that end in a
                        device synchronise; pool_kernel_ms is k_dense_novelty_pool<D> alone between two device events on the engine's stream
                        (dense_novelty_last_ms), pool_call_ms and append_call_ms the two calls on the host clock
  (b) host_ms           the only form a tree without the kernel has: dense_ga_eval + dense_final_state + the dense numpy scoring on the host --
                        the [population][archive + population] float64 matrix, the diagonal masked, a partition per row, the k smallest sorted
                        and averaged; host_scoring_ms is that scoring alone
  identical             the device's novelties equal dne_dense_novelty_pool_host's bit for bit (the timed work is the checked work)
  (c) D = 2 only        k_dense_novelty_pool<2> beside k_maze_novelty_pool of a DNE_KIND_MAZE handle on the same host-supplied points and archive,
                        the two alternated repetition by repetition: both kernels between device events; ratio_kernel = dense median / maze median

Prints ONE JSON line (and writes it with --out).  A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/dense_gans_time.py [--population 5000] [--parents 20] [--k 25] [--archives 0,1000,10000] [--reps 50] [--host-reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def host_scoring(bc, archive, k):
    """the pool novelty, dense: one [n][A + n] float64 matrix, the member's own column masked, the k smallest of every row, their mean"""
    p = bc.astype(np.float64)
    pool = np.concatenate([archive.astype(np.float64), p])
    d = (pool[None, :, 0] - p[:, None, 0]) ** 2
    for i in range(1, p.shape[1]):
        d += (pool[None, :, i] - p[:, None, i]) ** 2
    np.sqrt(d, out=d)
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
    ap.add_argument("--maze", default=os.path.join(ROOT, "tests", "golden", "hard_maze.txt"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, policies
    n, T = a.population, a.parents
    archives = [int(v) for v in a.archives.split(",")]
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    out = {"tool": "dense_gans_time", "population": n, "parents": T, "k": a.k, "reps": a.reps, "host_reps": a.host_reps, "warmup": a.warmup, "shapes": []}
    ok = True
    for dim, env, hidden, own in ((2, _lib.KIND_MAZE, (), _lib.MAZE_STEPS), (4, _lib.KIND_CARTPOLE, (5, 33), _lib.CARTPOLE_STEPS)):
        rs = np.random.RandomState(dim)
        eng = _lib.Engine(_lib.KIND_DENSE, 2, max_members=n, env=env, hidden=hidden, nonlin="relu")
        eng.noise_upload(noise)
        if env == _lib.KIND_MAZE:
            eng.maze_set_walls(*_lib.load_maze(a.maze))
        eng.dense_ga_set_init_scale(policies.dense_scale_by(env, hidden, 2))
        last = noise.size - eng.P
        eng.dense_ga_build([(int(i), ) for i in rs.randint(0, last + 1, size=T)])
        parent = rs.randint(T, size=n).astype(np.int32)
        idx = rs.randint(0, last + 1, size=n).astype(np.int64)
        power = np.full(n, 0.02, np.float32)                     # (wide enough for the children to end at many different points)
        seeds = None if env == _lib.KIND_MAZE else rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        picked = np.flatnonzero(rs.random_sample(n) < a.archive_prob).astype(np.int32)
        gen = lambda: eng.dense_ga_eval(parent, idx, power, own, seeds)
        for _ in range(a.warmup):
            gen()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            gen()
            wall.append((time.perf_counter() - t0) * 1e3)
        shape = {"D": dim, "env": int(env), "hidden": list(hidden), "P": int(eng.P), "appended_per_generation": int(picked.size), "gen_ms": stats(wall),
                 "archives": []}
        bc0 = _lib.dense_bc_host(env, eng.dense_final_state(n))
        lo, hi = bc0.min(axis=0), bc0.max(axis=0)
        for narch in archives:
            archive = np.random.RandomState(narch + dim).uniform(lo, np.maximum(hi, lo + 1e-3), (narch, dim)).astype(np.float32)   # where the BCs are

            def reset():
                eng.dense_archive_clear()
                if narch:
                    eng.dense_archive_append(archive)

            def device():
                gen()
                t1 = time.perf_counter()
                nov = eng.dense_novelty_pool(a.k)
                t2 = time.perf_counter()
                eng.dense_archive_append_members(picked)
                return nov, t1, t2, time.perf_counter()

            for _ in range(a.warmup):
                reset(); device()
            both, call, kern, app = [], [], [], []
            for _ in range(a.reps):
                reset()
                t0 = time.perf_counter()
                nov, t1, t2, t3 = device()
                both.append((t3 - t0) * 1e3); call.append((t2 - t1) * 1e3); app.append((t3 - t2) * 1e3); kern.append(eng.dense_novelty_last_ms())
            assert eng.dense_archive_size() == narch + picked.size
            host_all, host_score = [], []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                gen()
                bc = _lib.dense_bc_host(env, eng.dense_final_state(n))
                t1 = time.perf_counter()
                host_nov = host_scoring(bc, archive, a.k)
                t2 = time.perf_counter()
                host_all.append((t2 - t0) * 1e3); host_score.append((t2 - t1) * 1e3)
            twin = _lib.dense_novelty_pool_host(bc, archive, a.k)
            same = bool(np.array_equal(nov.view(np.uint64), twin.view(np.uint64)))
            ok = ok and same
            with np.errstate(all="ignore"):
                rel = np.abs(host_nov - twin) / np.where(twin == 0, 1.0, twin)
            shape["archives"].append({"archive": narch, "device_ms": stats(both), "pool_call_ms": stats(call), "pool_kernel_ms": stats(kern),
                                      "append_call_ms": stats(app), "host_ms": stats(host_all), "host_scoring_ms": stats(host_score), "identical": same,
                                      "distinct_points": int(len(np.unique(bc, axis=0))), "host_numpy_max_rel_diff": float(np.nanmax(rel))})
        if dim == 2:                                             # (c) beside k_maze_novelty_pool, on the last evaluation's points handed in from the host
            maze = _lib.Engine(_lib.KIND_MAZE, 2, max_members=16)
            shape["beside_maze"] = []
            for narch in archives:
                archive = np.random.RandomState(narch + dim).uniform(lo, np.maximum(hi, lo + 1e-3), (narch, dim)).astype(np.float32)
                eng.dense_archive_clear(); maze.maze_archive_clear()
                if narch:
                    eng.dense_archive_append(archive); maze.maze_archive_append(archive)
                kern, mkern = [], []
                for rep in range(a.warmup + a.reps):
                    nov = eng.dense_novelty_pool(a.k, bc)
                    mnov = maze.maze_novelty_pool(a.k, bc)
                    if rep >= a.warmup:
                        kern.append(eng.dense_novelty_last_ms()); mkern.append(maze.maze_novelty_last_ms())
                same = bool(np.array_equal(nov.view(np.uint64), mnov.view(np.uint64)))
                ok = ok and same
                shape["beside_maze"].append({"archive": narch, "dense_kernel_ms": stats(kern), "maze_kernel_ms": stats(mkern),
                                             "ratio_kernel": float(np.median(kern) / np.median(mkern)), "identical": same})
            maze.close()
        eng.check_redzones()
        eng.close()
        out["shapes"].append(shape)
    out["identical"] = ok
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
