#!/usr/bin/env python3
"""What scoring novelty costs a hard-maze generation: on the device against on the host.

A generation = dne_es_eval of population / 2 antithetic pairs of SimpleClassifier on the hard maze (tools/maze_gen_time.py).  Per archive size:

  (a) gen_ms            the generation alone, median wall time (host clock around a call that ends in a device synchronise)
  (b) gen_novelty_ms    the generation, then engine.maze_novelty(k) on the final positions where k_maze_rollout left them (k_maze_novelty,
                        csrc/maze_novelty.h; the archive is device-resident), median wall time of the two calls; novelty_kernel_ms is the
                        kernel alone between two device events, novelty_call_ms the maze_novelty call alone on the host clock
  (c) gen_host_ms       what a tree without the kernel has to do: the generation, maze_final_state, and nses.py:12-32 vectorised in numpy on the
                        host -- the [population][archive] float64 distance matrix, a partition per row, the k smallest sorted and averaged;
                        host_scoring_ms is that scoring alone
  identical             the device's novelties equal dne_maze_novelty_host's bit for bit (the timed work is the checked work)

Prints ONE JSON line (and writes it with --out).  --gen-json FILE embeds the line tools/maze_gen_time.py wrote in the same session.
A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/maze_novelty_time.py [--population 5000] [--k 10] [--archives 10,1000,10000] [--reps 50] [--host-reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))


def host_scoring(xy, archive, k):
    """nses.py:12-32 on (x, y) points, vectorised: one [n][A] float64 matrix, the k smallest of every row, their mean"""
    p, a = xy.astype(np.float64), archive.astype(np.float64)
    d = np.sqrt((a[None, :, 0] - p[:, None, 0]) ** 2 + (a[None, :, 1] - p[:, None, 1]) ** 2)
    kk = min(k, a.shape[0])
    near = np.partition(d, kk - 1, axis=1)[:, :kk] if kk < a.shape[0] else d
    return np.sort(near, axis=1).mean(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=5000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--archives", default="10,1000,10000")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--maze", default=os.path.join(ROOT, "tests", "golden", "hard_maze.txt"))
    ap.add_argument("--gen-json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, policies
    pairs = a.population // 2
    n = 2 * pairs
    header, lines = _lib.load_maze(a.maze)
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    rs = np.random.RandomState(0)
    theta = noise[rs.randint(0, noise.size - 498 + 1):][:498] * policies.simple_scale_by()
    idx = rs.randint(0, noise.size - 498 + 1, size=pairs).astype(np.int64)
    seeds = np.zeros(n, np.uint32)

    eng = _lib.Engine(_lib.KIND_MAZE, 2, max_members=n)
    eng.noise_upload(noise)
    eng.set_theta(theta)
    eng.maze_set_walls(header, lines)
    gen = lambda: eng.es_eval(idx, a.sigma, _lib.MAZE_STEPS, seeds)
    for _ in range(a.warmup):
        gen()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        gen()
        wall.append((time.perf_counter() - t0) * 1e3)
    out = {"tool": "maze_novelty_time", "population": n, "k": a.k, "walls": int(lines.shape[0]), "reps": a.reps, "host_reps": a.host_reps,
           "gen_ms": float(np.median(wall)), "gen_ms_min": float(np.min(wall)), "gen_ms_max": float(np.max(wall)), "archives": []}
    if a.gen_json:
        with open(a.gen_json) as f:
            out["maze_gen_time"] = json.loads(f.read())
    ok = True
    for narch in (int(v) for v in a.archives.split(",")):
        archive = np.random.RandomState(narch).uniform(0, 300, (narch, 2)).astype(np.float32)
        eng.maze_archive_clear()
        eng.maze_archive_append(archive)
        for _ in range(a.warmup):
            gen(); eng.maze_novelty(a.k)
        both, call, kern = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            gen()
            t1 = time.perf_counter()
            nov = eng.maze_novelty(a.k)
            t2 = time.perf_counter()
            both.append((t2 - t0) * 1e3); call.append((t2 - t1) * 1e3); kern.append(eng.maze_novelty_last_ms())
        host_all, host_score = [], []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            gen()
            xy = eng.maze_final_state(n)
            t1 = time.perf_counter()
            host_nov = host_scoring(xy, archive, a.k)
            t2 = time.perf_counter()
            host_all.append((t2 - t0) * 1e3); host_score.append((t2 - t1) * 1e3)
        twin = _lib.maze_novelty_host(xy, archive, a.k)
        same = bool(np.array_equal(nov.view(np.uint64), twin.view(np.uint64)))
        ok = ok and same
        out["archives"].append({"archive": narch, "gen_novelty_ms": float(np.median(both)), "gen_novelty_ms_min": float(np.min(both)),
                                "gen_novelty_ms_max": float(np.max(both)), "novelty_call_ms": float(np.median(call)),
                                "novelty_kernel_ms": float(np.median(kern)), "gen_host_ms": float(np.median(host_all)),
                                "host_scoring_ms": float(np.median(host_score)), "identical": same,
                                "host_numpy_max_rel_diff": float(np.max(np.abs(host_nov - twin) / np.where(twin == 0, 1.0, twin)))})
    eng.check_redzones()
    eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
