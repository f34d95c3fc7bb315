#!/usr/bin/env python3
"""One hard-maze generation on the device against the same population on one host core.

A generation = dne_es_eval of population / 2 antithetic pairs of SimpleClassifier on the hard maze (DNE_KIND_MAZE: one k_maze_rollout launch, 400
steps per member) including the copies of returns, sign-returns and lengths back to the host.  Prints ONE JSON line:

  gen_ms               median wall time of a generation over --reps repetitions after --warmup (host clock around a call that ends in a device
                       synchronise), with gen_ms_min / gen_ms_max for the spread
  kernel_ms            the same launch between two device events (dne_profile.eval_ms), median
  env_steps_per_s      population * 400 / gen_ms
  host_s               the same population through dne_maze_rollout_host (the same header compiled for the CPU) on one core, once
  host_env_steps_per_s population * 400 / host_s
  identical            the device's returns equal the host's bit for bit (the timed work is the checked work)

A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/maze_gen_time.py [--population 5000] [--reps 200] [--warmup 3] [--sigma 0.02] [--maze tests/golden/hard_maze.txt] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--maze", default=os.path.join(ROOT, "tests", "golden", "hard_maze.txt"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, policies
    pairs = a.population // 2
    header, lines = _lib.load_maze(a.maze)
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    rs = np.random.RandomState(0)
    theta = noise[rs.randint(0, noise.size - 498 + 1):][:498] * policies.simple_scale_by()
    idx = rs.randint(0, noise.size - 498 + 1, size=pairs).astype(np.int64)
    seeds = np.zeros(2 * pairs, np.uint32)

    eng = _lib.Engine(_lib.KIND_MAZE, 2, max_members=2 * pairs)
    eng.noise_upload(noise)
    eng.set_theta(theta)
    eng.maze_set_walls(header, lines)
    for _ in range(a.warmup):
        eng.es_eval(idx, a.sigma, _lib.MAZE_STEPS, seeds)
    wall, kern = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ret, sg, ln = eng.es_eval(idx, a.sigma, _lib.MAZE_STEPS, seeds)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(eng.profile()["eval_ms"])
    eng.check_redzones()
    eng.close()

    s = np.float32(a.sigma)
    th = np.empty((2 * pairs, 498), np.float32)
    for i, off in enumerate(idx):
        v = s * noise[off:off + 498]
        th[2 * i], th[2 * i + 1] = theta + v, theta - v
    t0 = time.perf_counter()
    hret, hln, _ = _lib.maze_rollout_host(th, header, lines, _lib.MAZE_STEPS)
    host_s = time.perf_counter() - t0

    steps = int(np.sum(ln))
    gen_ms = float(np.median(wall))
    out = {"tool": "maze_gen_time", "population": 2 * pairs, "steps_per_episode": _lib.MAZE_STEPS, "walls": int(lines.shape[0]), "reps": a.reps,
           "gen_ms": gen_ms, "gen_ms_min": float(np.min(wall)), "gen_ms_max": float(np.max(wall)), "kernel_ms": float(np.median(kern)),
           "env_steps_per_s": steps / (gen_ms * 1e-3), "host_s": host_s, "host_env_steps_per_s": int(np.sum(hln)) / host_s,
           "identical": bool(np.array_equal(ret.reshape(-1).view(np.uint32), hret.view(np.uint32)) and np.array_equal(ln.reshape(-1), hln))}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
