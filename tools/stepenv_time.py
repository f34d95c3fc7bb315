#!/usr/bin/env python3
"""One step of a batch of environments through dne_stepenv_step_* (csrc/step_env.h), for the maze, the cart-pole and the pendulum, beside the
whole-episode kernel's time per step for the same batch.

Prints ONE JSON line; per kind:

  step_ms              median wall time over --reps repetitions after --warmup of ONE Engine.stepenv_step call on --batch environments: indices and
                       actions copied up, the step kernel, reward and done copied back (host clock around a call that ends in a device
                       synchronise); step_ms_range: (min, max).  The batch is reset before every repetition (not timed), so every repetition
                       steps live environments from the same states.
  kernel_ms            the step kernel alone between two device events (dne_stepenv_last_ms) over the same repetitions, median and range
  episode_kernel_ms    the whole-episode kernel (k_maze_rollout / k_cartpole_rollout / k_pendulum_rollout<64, tanh>) for --batch members of
                       theta_0 between two device events (dne_profile.eval_ms), median of --reps; episode_steps: the steps of that evaluation;
                       episode_ms_per_step = episode_kernel_ms / (episode_steps / batch): what one step of the batch costs inside that kernel,
                       the policy's forward pass included
  identical            state, steps, done, observation and reward after the last timed step equal the host twin's, bit for bit

A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/stepenv_time.py [--batch 1000] [--reps 30] [--warmup 3] [--out FILE]
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
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, maze_run, policies
    n = a.batch
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    rs = np.random.RandomState(0)
    seeds = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    maze = _lib.load_maze(maze_run.maze_file({}))
    rng = lambda v: (float(np.min(v)), float(np.max(v)))
    same = lambda x, y: x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    out = {"tool": "stepenv_time", "batch": n, "reps": a.reps, "warmup": a.warmup}
    ok = True
    for name, kind in (("maze", _lib.KIND_MAZE), ("cartpole", _lib.KIND_CARTPOLE), ("pendulum", _lib.KIND_PENDULUM)):
        if kind == _lib.KIND_PENDULUM:
            e = _lib.Engine(kind, 1, max_members=n, hidden=64, ac_mode="continuous", nonlin="tanh")
            e.pendulum_set_ob_stat(np.zeros(3, np.float32), np.ones(3, np.float32))
            theta0, limit = policies.normc_flat(64, 1, 0), _lib.PENDULUM_STEPS
        else:
            e = _lib.Engine(kind, 2, max_members=n)
            theta0 = noise[1234:1234 + e.P] * policies.simple_scale_by(kind)
            limit = _lib.MAZE_STEPS if kind == _lib.KIND_MAZE else _lib.CARTPOLE_STEPS
        if kind == _lib.KIND_MAZE:
            e.maze_set_walls(*maze)
        e.noise_upload(noise)
        e.set_theta(theta0)
        obs_w, act_w, S, is_int = _lib.stepenv_dims(kind)
        if kind == _lib.KIND_MAZE:
            act = rs.uniform(-0.7, 0.7, (n, 2)).astype(np.float32)
        elif is_int:
            act = rs.randint(0, 2, n).astype(np.int32)
        else:
            act = rs.uniform(-3, 3, n).astype(np.float32)
        wall, kern = [], []
        for rep in range(a.warmup + a.reps):
            e.stepenv_reset(n=n, seeds=seeds)
            t0 = time.perf_counter()
            rew, done = e.stepenv_step(act)
            t1 = time.perf_counter()
            if rep >= a.warmup:
                wall.append((t1 - t0) * 1e3); kern.append(e.stepenv_last_ms())
        state, steps, dn = e.stepenv_state(n=n)
        obs = e.stepenv_observation(n=n)
        hw = dict(header=maze[0], lines=maze[1]) if kind == _lib.KIND_MAZE else {}
        hst, hsteps, hlim, hdone, hobs = _lib.stepenv_reset_host(kind, n, seeds, 0, **hw)
        hrew = _lib.stepenv_step_host(kind, act, hst, hsteps, hlim, hdone, hobs, **hw)
        identical = bool(same(state, hst) and same(steps, hsteps) and same(dn, hdone.astype(bool)) and same(obs, hobs) and same(rew, hrew))
        ok = ok and identical
        e.set_members(np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.float32))
        ep, ep_steps = [], 0
        for rep in range(a.warmup + a.reps):
            ln = e.eval_members(n, limit, seeds)[2]
            if rep >= a.warmup:
                ep.append(e.profile()["eval_ms"])
            ep_steps = int(np.sum(ln))
        e.check_redzones()
        e.close()
        ep_ms = float(np.median(ep))
        out[name] = {"step_ms": float(np.median(wall)), "step_ms_range": rng(wall), "kernel_ms": float(np.median(kern)), "kernel_ms_range": rng(kern),
                     "episode_kernel_ms": ep_ms, "episode_kernel_ms_range": rng(ep), "episode_steps": ep_steps,
                     "episode_ms_per_step": ep_ms / (ep_steps / n), "identical": identical}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
