#!/usr/bin/env python3
"""One generation of the GPU tree's gym configuration (configurations/es_gym_config.json: gym.CartPole-v1, SimpleClassifier, population 5000, Adam)
on the device, the evaluation kernel alone, what 20 iterations of that configuration do to theta, and the CPU twin's rate beside them.

Prints ONE JSON line (the last line of its output: the driver's tabular log comes before it):

  gen_ms               median wall time over --reps repetitions after --warmup of one generation FROM theta_0: dne_es_eval of population / 2
                       antithetic pairs (one k_cartpole_rollout launch, every episode under its own seed, results copied back) + dne_es_update
                       (centered ranks, weighted noise sum, Adam); theta and the optimizer are put back before every repetition, so each
                       repetition does the same work.  Host clock around calls that end in a device synchronise; gen_ms_min / gen_ms_max: the spread
  eval_ms, update_ms   the two calls of that generation apart, medians
  kernel_ms            k_cartpole_rollout of that evaluation between two device events (dne_profile.eval_ms), median
  env_steps            the steps of one such evaluation; env_steps_per_s = env_steps / gen_ms
  test_return_before   the mean return of --test-episodes episodes of the run's theta_0, each under its own seed
  test_return_after    the same, under the same seeds, for theta after --iters iterations of es_gpu.main on the shipped configuration
  train_s              the wall time of those iterations, test episodes and snapshots included
  host_threads, host_episodes_per_s, host_env_steps_per_s
                       the generation's 5000 episodes through dne_cartpole_rollout_host (the same header compiled for the CPU), split over
                       --threads Python threads (ctypes releases the GIL around the call); the only available stand-in for GymEnv
  identical            the device's returns, lengths and final states of the timed evaluation equal the host's bit for bit

A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/cartpole_gen_time.py [--population 5000] [--reps 30] [--warmup 3] [--iters 20] [--test-episodes 200] [--threads 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))

# configurations/es_gym_config.json of the reference's GPU tree, restated (the file holds only settings)
SHIPPED = {"game": "gym.CartPole-v1", "model": "SimpleClassifier", "num_validation_episodes": 30, "num_test_episodes": 200, "population_size": 5000,
           "timesteps": 250e6, "episode_cutoff_mode": 5000, "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=SHIPPED["population_size"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--test-episodes", type=int, default=SHIPPED["num_test_episodes"])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, es, es_gpu, policies
    P = _lib.CARTPOLE_P
    pairs = a.population // 2
    exp = dict(SHIPPED, population_size=2 * pairs, num_test_episodes=a.test_episodes)
    sigma, l2, step = exp["mutation_power"], exp["l2coeff"], exp["optimizer"]["args"]["stepsize"]
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    rs = np.random.RandomState(0)
    theta0 = noise[rs.randint(0, noise.size - P + 1):][:P] * policies.simple_scale_by(_lib.KIND_CARTPOLE)
    idx = rs.randint(0, noise.size - P + 1, size=pairs).astype(np.int64)
    seeds = rs.randint(0, 2 ** 32, size=2 * pairs, dtype=np.uint64).astype(np.uint32)

    eng = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=2 * pairs)
    eng.noise_upload(noise)
    wall, ev, up, kern = [], [], [], []
    for rep in range(a.warmup + a.reps):
        eng.set_theta(theta0)
        eng.optimizer_reset()
        t0 = time.perf_counter()
        ret, sg, ln = eng.es_eval(idx, sigma, _lib.CARTPOLE_STEPS, seeds)
        t1 = time.perf_counter()
        eng.es_update(idx, ret, sg, "centered_rank", "adam", l2, step)
        eng.get_theta()                                           # (ends in a device synchronise)
        t2 = time.perf_counter()
        if rep >= a.warmup:
            wall.append((t2 - t0) * 1e3); ev.append((t1 - t0) * 1e3); up.append((t2 - t1) * 1e3)
    eng.set_theta(theta0)
    for _ in range(a.reps):                                       # the same evaluation again, its kernel read from the profile right behind it
        ret, sg, ln = eng.es_eval(idx, sigma, _lib.CARTPOLE_STEPS, seeds)
        kern.append(eng.profile()["eval_ms"])
    state = eng.cartpole_final_state(2 * pairs)
    eng.check_redzones()

    def test_return(theta, stream):
        eng.set_theta(theta)
        r, _ = es_gpu._episodes_of_theta(eng, a.test_episodes, None, stream)
        return float(np.mean(r))

    table = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    table.noise, table._engines = noise, []
    with tempfile.TemporaryDirectory() as log_dir:                # the run's own theta_0 (its stream's first draw): no iteration, no snapshot
        first = np.array(es_gpu.main(log_dir, engine=eng, noise=table, seed=0, max_iters=0, **exp).theta, np.float32)
    with tempfile.TemporaryDirectory() as log_dir:
        t0 = time.perf_counter()
        st = es_gpu.main(log_dir, engine=eng, noise=table, seed=0, max_iters=a.iters, **exp)
        train_s = time.perf_counter() - t0
    before = test_return(first, np.random.RandomState(1))         # the same test seeds for both
    after = test_return(np.array(st.theta, np.float32), np.random.RandomState(1))
    eng.close()

    s = np.float32(sigma)
    th = np.empty((2 * pairs, P), np.float32)
    for i, off in enumerate(idx):
        v = s * noise[off:off + P]
        th[2 * i], th[2 * i + 1] = theta0 + v, theta0 - v
    cuts = np.linspace(0, 2 * pairs, a.threads + 1).astype(int)
    parts = [(cuts[k], cuts[k + 1]) for k in range(a.threads) if cuts[k + 1] > cuts[k]]
    _lib.cartpole_rollout_host(th[:8], seeds[:8], _lib.CARTPOLE_STEPS)   # (the library is loaded and warm)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=len(parts)) as pool:
        res = list(pool.map(lambda lohi: _lib.cartpole_rollout_host(th[lohi[0]:lohi[1]], seeds[lohi[0]:lohi[1]], _lib.CARTPOLE_STEPS), parts))
    host_s = time.perf_counter() - t0
    hret = np.concatenate([r[0] for r in res]); hln = np.concatenate([r[1] for r in res]); hstate = np.concatenate([r[2] for r in res])

    steps = int(np.sum(ln))
    gen_ms = float(np.median(wall))
    out = {"tool": "cartpole_gen_time", "population": 2 * pairs, "reps": a.reps, "gen_ms": gen_ms, "gen_ms_min": float(np.min(wall)),
           "gen_ms_max": float(np.max(wall)), "eval_ms": float(np.median(ev)), "update_ms": float(np.median(up)), "kernel_ms": float(np.median(kern)),
           "env_steps": steps, "mean_episode_length": steps / (2.0 * pairs), "env_steps_per_s": steps / (gen_ms * 1e-3),
           "iters": a.iters, "test_episodes": a.test_episodes, "test_return_before": before, "test_return_after": after, "train_s": train_s,
           "train_timesteps": int(st.timesteps_so_far),
           "host_threads": len(parts), "host_s": host_s, "host_episodes_per_s": 2 * pairs / host_s, "host_env_steps_per_s": int(np.sum(hln)) / host_s,
           "identical": bool(np.array_equal(ret.reshape(-1).view(np.uint32), hret.view(np.uint32)) and np.array_equal(ln.reshape(-1), hln)
                             and np.array_equal(state.view(np.uint64), hstate.view(np.uint64)))}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
