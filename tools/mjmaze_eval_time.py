#!/usr/bin/env python3
"""The time of one evaluation of MujocoPolicy on the hard maze (k_mjmaze_rollout) beside k_pendulum_rollout at the same
hidden width and member count, and two iterations of the shipped NS-ES / NSR-ES configurations on the device.

Prints ONE JSON line (the last line of its output):

  kernel_ms        {hidden width: median over --reps evaluations after --warmup} of the rollout kernel for --members members between two device
                   events (dne_profile.eval_ms), tanh, continuous action, action noise on every episode, statistics on a hundredth of them;
                   kernel_ms_range: (min, max) of each
  steps            the steps of one episode (the maze: 400, the pendulum: 200); us_per_step: kernel_ms / steps in microseconds -- the time of one
                   step of the whole population
  drivers          (--kind mjmaze with --drivers) for humanoid_nses.json and humanoid_nsres.json with "env_id": "HardMaze-v0", restated here (the
                   files hold only settings): the wall time of two iterations through nses.run_master / run_worker, the archive's size, the mean
                   novelty and mean return of the last iteration's Results

--kind pendulum measures k_pendulum_rollout alone; with DNE_LIB_PATH naming another build of the library (the parent commit's) it measures that one.
A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/mjmaze_eval_time.py [--kind mjmaze|pendulum] [--members 2000] [--reps 30] [--warmup 3] [--drivers] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))

SHIPPED_NS = {"config": {"calc_obstat_prob": 0.01, "episodes_per_batch": 1000, "eval_prob": 0.03, "l2coeff": 0.005, "noise_stdev": 0.02, "snapshot_freq": 10,
                         "timesteps_per_batch": 100000, "return_proc_mode": "centered_sign_rank", "episode_cutoff_mode": "env_default"},
              "env_id": "HardMaze-v0", "algo_type": "ns", "exp_prefix": "humanoid",
              "novelty_search": {"k": 10, "population_size": 5, "num_rollouts": 5, "selection_method": "novelty_prob"},
              "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"},
              "policy": {"args": {"ac_bins": "continuous:", "ac_noise_std": 0.01, "connection_type": "ff", "hidden_dims": [256, 256], "nonlin_type": "tanh"},
                         "type": "MujocoPolicy"}}


def run_drivers(algo, noise):
    from dne_hip import dist, es, nses
    exp = json.loads(json.dumps(SHIPPED_NS))
    exp["algo_type"] = algo
    exp["config"]["snapshot_freq"] = 0
    table = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    table.noise, table._engines = noise, []
    dist.reset_brokers()
    cfg = {"unix_socket_path": "/tmp/dne_mjmaze_eval_time.sock", "transport": "inprocess"}
    out, pushed = {}, []
    push = dist.WorkerClient.push_result

    def spy(self, task_id, result):
        pushed.append(result)
        return push(self, task_id, result)

    def master():
        with tempfile.TemporaryDirectory() as log_dir:
            out["r"] = nses.run_master(cfg, log_dir, exp, noise=table, max_iters=2, seed=0)
    dist.WorkerClient.push_result = spy
    try:
        t0 = time.perf_counter()
        tm = threading.Thread(target=master, daemon=True)
        tw = threading.Thread(target=lambda: nses.run_worker(cfg, cfg, table, max_tasks=2, seed=7, reeval_after=1e9), daemon=True)
        tm.start(); tw.start()
        tm.join(timeout=300); tw.join(timeout=60)
        wall = time.perf_counter() - t0
    finally:
        dist.WorkerClient.push_result = push
    assert not tm.is_alive() and not tw.is_alive() and "r" in out, "the drivers did not finish"
    last = pushed[-1]
    return {"iterations": 2, "wall_s": wall, "archive": len(out["r"][1]), "novelty_mean": float(last.signreturns_n2.mean()),
            "return_mean": float(last.returns_n2.mean()), "episodes": int(last.lengths_n2.size), "ob_count": int(last.ob_count)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("mjmaze", "pendulum"), default="mjmaze")
    ap.add_argument("--members", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--drivers", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, maze_run, policies
    maze = a.kind == "mjmaze"
    n = a.members - a.members % 2
    steps, per_ep = (400, 800) if maze else (200, 200)
    n_obs, n_out = (11, 2) if maze else (3, 1)
    noise = np.random.RandomState(123).randn(20_000_000 if a.drivers else 2_000_000).astype(np.float32)
    rs = np.random.RandomState(0)
    seeds = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    ac_off = rs.randint(0, noise.size - per_ep + 1, size=n).astype(np.int64)
    flag = (rs.rand(n) < 0.01).astype(np.uint8)
    kernel, kernel_range = {}, {}
    for H in (64, 256):
        e = _lib.Engine(_lib.KIND_MJMAZE if maze else _lib.KIND_PENDULUM, n_out, max_members=n, hidden=H, ac_mode="continuous", nonlin="tanh")
        e.noise_upload(noise)
        e.set_theta(policies.normc_flat(H, n_out, 0, n_obs))
        if maze:
            e.maze_set_walls(*_lib.load_maze(maze_run.maze_file({})))
        set_stat, set_options = (e.mjmaze_set_ob_stat, e.mjmaze_set_rollout_options) if maze else (e.pendulum_set_ob_stat, e.pendulum_set_rollout_options)
        set_stat(np.zeros(n_obs, np.float32), np.ones(n_obs, np.float32))
        idx = np.sort(np.random.RandomState(H).randint(0, noise.size - e.P + 1, size=n // 2)).astype(np.int64)
        k = []
        for rep in range(a.warmup + a.reps):
            set_options(n, 0.01, ac_off, flag)
            _, _, ln = e.es_eval(idx, 0.02, steps, seeds)
            if rep >= a.warmup:
                k.append(e.profile()["eval_ms"])
        assert (ln == steps).all()
        e.check_redzones()
        e.close()
        kernel[str(H)], kernel_range[str(H)] = float(np.median(k)), (float(np.min(k)), float(np.max(k)))
    out = {"tool": "mjmaze_eval_time", "kind": a.kind, "lib": os.environ.get("DNE_LIB_PATH", "in-tree"), "members": n, "reps": a.reps, "steps": steps,
           "kernel_ms": kernel, "kernel_ms_range": kernel_range, "us_per_step": {h: 1e3 * v / steps for h, v in kernel.items()}}
    if a.drivers and maze:
        out["drivers"] = {algo: run_drivers(algo, noise) for algo in ("ns", "nsr")}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
