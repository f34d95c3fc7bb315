#!/usr/bin/env python3
"""The Deep GA with MujocoPolicy, timed on the device: one generation, the roots of generation 0, and promotion.

Hidden 256 on the hard maze (P = 69 378), 5000 children over 250 parents, whole episodes of 400 steps.  Every figure is a median over
repetitions after --warmup, with its min and max:

  gen_kernel_ms     k_mjmaze_rollout of one generation of children between the engine's two device events (dne_get_profile: eval_ms)
  gen_call_ms       the same dne_mujoco_ga_eval on a host clock (the call ends in a device synchronise): uploads, launch, copies back
  roots_call_minus_eval_ms   dne_mujoco_ga_eval of 5000 ROOTS at tslimit 1 on a host clock, minus that evaluation's own eval_ms.  NOT a kernel
                    time: beside k_mujoco_ga_colscale + k_mujoco_ga_roots it holds the four uploads, the copies back, the stream synchronise and the
                    call's own overhead -- an upper bound for the two kernels.  By bytes a root reads its P floats twice (the column sums, then the
                    scaling) and writes P
  promote_call_ms   dne_mujoco_ga_promote of 250 parents (125 kept, 125 children of the old bank), host clock: reads 2 P and writes P a parent
  identical         parent 0 after the promotion equals dne_mujoco_ga_members_host's bit for bit (the timed work is the checked work)

Prints ONE JSON line (and writes it with --out).  A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/mujoco_ga_time.py [--children 5000] [--parents 250] [--hidden 256] [--reps 20] [--out profiles/rNN_mujoco_ga_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--children", type=int, default=5000)
    ap.add_argument("--parents", type=int, default=250)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--maze", default=os.path.join(ROOT, "tests", "golden", "hard_maze.txt"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib
    n, T, H = a.children, a.parents, a.hidden
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    rs = np.random.RandomState(1)
    eng = _lib.Engine(_lib.KIND_MJMAZE, 2, max_members=n, hidden=H, ac_mode="continuous", nonlin="tanh")
    eng.noise_upload(noise)
    eng.maze_set_walls(*_lib.load_maze(a.maze))
    eng.mjmaze_set_ob_stat(np.zeros(_lib.MJMAZE_OBS, np.float32), np.ones(_lib.MJMAZE_OBS, np.float32))
    eng.mujoco_ga_reserve(T)
    last = noise.size - eng.P
    eng.mujoco_ga_build([(int(i), ) for i in rs.randint(0, last + 1, size=T)])
    parent = rs.randint(T, size=n).astype(np.int32)
    idx = rs.randint(0, last + 1, size=n).astype(np.int64)
    power = np.full(n, 0.02, np.float32)

    def timed(f):
        wall, kern = [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            f()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= a.warmup:
                wall.append(dt); kern.append(eng.profile()["eval_ms"])
        return np.array(wall), np.array(kern)

    gen_wall, gen_kern = timed(lambda: eng.mujoco_ga_eval(parent, idx, power, _lib.MJMAZE_STEPS))
    steps = int(eng.profile()["env_steps"])
    root_wall, root_kern = timed(lambda: eng.mujoco_ga_eval(np.full(n, -1, np.int32), idx, power, 1))
    pp = np.where(np.arange(T) % 2 == 0, np.arange(T), (np.arange(T) * 7) % T).astype(np.int32)
    pi = np.where(np.arange(T) % 2 == 0, -1, idx[:T]).astype(np.int64)
    before = np.stack([eng.mujoco_ga_get_parent(j) for j in (int(pp[0]), int(pp[1]))])
    prom = []
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        eng.mujoco_ga_promote(pp, pi, power[:T])
        if rep >= a.warmup:
            prom.append((time.perf_counter() - t0) * 1e3)
        if rep == 0:
            want = _lib.mujoco_ga_members_host(noise, _lib.KIND_MJMAZE, H, 2, before, [0, 1], pi[:2], power[:2])
            same = bool(np.array_equal(np.stack([eng.mujoco_ga_get_parent(0), eng.mujoco_ga_get_parent(1)]).view(np.uint32), want.view(np.uint32)))
    eng.check_redzones()
    out = {"tool": "mujoco_ga_time", "kind": "mjmaze", "hidden": H, "P": int(eng.P), "children": n, "parents": T, "reps": a.reps, "warmup": a.warmup,
           "env_steps_per_generation": steps, "gen_kernel_ms": stats(gen_kern), "gen_call_ms": stats(gen_wall), "roots_call_minus_eval_ms": stats(root_wall - root_kern),
           "roots_eval_ms": stats(root_kern), "promote_call_ms": stats(prom), "bytes_per_root": 12 * int(eng.P), "bytes_per_promotion": 12 * int(eng.P),
           "identical": same}
    eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
