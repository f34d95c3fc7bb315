#!/usr/bin/env python3
"""What a dense policy of the caller's own shape costs on the device (DNE_KIND_DENSE, k_dense_run of csrc/dense.h), beside
the kernels of the baked shape and beside the route a policy outside the kernels had before: a host `act` callback around the step-at-a-time batch.

Prints ONE JSON line.  Per environment of --games ('maze', 'cartpole' and, when asked for, 'acrobot') and --members members (antithetic pairs around theta_0 = noise * scale_by at sigma 0.02,
every episode under its own seed, run to the environment's own limit):

  dense["<shape>"]     k_dense_run whole episodes for the shapes linear (LinearClassifier), 16x16 and 64x64x64 (relu):
                         kernel_ms      the launch between two device events (dne_profile.eval_ms), median of --reps after --warmup, with its range
                         wall_ms        dne_es_eval as the caller sees it (members uploaded, the launch, results copied back), host clock around a
                                        call that ends in a device synchronise, median and range
                         env_steps      the steps of one such evaluation
  baked                the same members on 16x16 through DNE_KIND_MAZE / DNE_KIND_CARTPOLE (k_maze_rollout / k_cartpole_rollout) in this process:
                       kernel_ms, wall_ms as above; identical: returns, sign-returns and lengths equal k_dense_run's bit for bit.  The price of
                       the generic kernel against the specialised ones: recorded, not gated.
  host_act             LinearClassifier as a host callback: envs.rollout on a DNE_KIND_MAZE / DNE_KIND_CARTPOLE engine with a numpy act (one
                       einsum over the members' thetas): per step one observation copy to the host, one action copy back and one step kernel.
                       wall_ms median and range over --host-reps, steps_per_episode.  This route exists on the commit before the kind; run the
                       tool with --route host under DNE_LIB_PATH=<that commit's library> to time it there.
  device_beats_host    wall_ms of dense["linear"] at its slowest repetition is below host_act's wall_ms at its fastest

'acrobot' (gym.Acrobot-v1, csrc/acrobot.h) has no baked kernel and no engine kind of its own: its entry holds dense[...] alone (three outputs, own
limit 500).  --shapes picks among linear, 16x16 and 64x64x64 for the games that have no baked kernel to be compared with.

A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/dense_timing.py [--members 1000] [--reps 10] [--warmup 3] [--host-reps 3] [--route all|host] [--games maze,cartpole]
                                    [--shapes linear,16x16,64x64x64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))

SHAPES = {"linear": (), "16x16": (16, 16), "64x64x64": (64, 64, 64)}
GAMES = {"maze": "maze", "cartpole": "gym.CartPole-v1", "acrobot": "gym.Acrobot-v1"}
N_IN = {"maze": 11, "cartpole": 4, "acrobot": 6}
SIGMA = 0.02


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "range": [float(v.min()), float(v.max())]}


def linear_scale_by(env):
    """policies.dense_scale_by for no hidden layer, written out (the route before the kind has no such function): 1 / sqrt(inputs), biases 0"""
    return np.concatenate([np.full(N_IN[env] * 2, np.float32(1.0 / np.sqrt(N_IN[env])), np.float32), np.zeros(2, np.float32)])


def timed_evals(eng, idx, seeds, limit, reps, warmup):
    kern, wall, out = [], [], None
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        out = eng.es_eval(idx, SIGMA, limit, seeds)
        t1 = time.perf_counter()
        if rep >= warmup:
            kern.append(eng.profile()["eval_ms"]); wall.append((t1 - t0) * 1e3)
    return {"kernel_ms": stats(kern), "wall_ms": stats(wall), "env_steps": int(np.sum(out[2]))}, out


def host_act_route(_lib, envs, env, noise, theta0, idx, seeds, reps):
    """envs.rollout under a numpy LinearClassifier, member i = pair i // 2 at +-sigma, on the engine kind the environments always had"""
    n = 2 * idx.size
    P = theta0.size
    th = np.stack([(theta0 + np.float32(s) * noise[i:i + P]).astype(np.float32) for i in idx for s in (SIGMA, -SIGMA)])
    W, b = th[:, :P - 2].reshape(n, N_IN[env], 2), th[:, P - 2:]

    def act(obs):
        out = np.einsum("nk,nkj->nj", obs, W) + b
        return out.astype(np.float32) if env == "maze" else (out[:, 1] > out[:, 0]).astype(np.int32)

    e = envs.make(GAMES[env], n)
    wall, lens = [], None
    try:
        for rep in range(1 + reps):                                      # (one warm-up episode)
            t0 = time.perf_counter()
            _, lens = envs.rollout(e, act, seeds=seeds)
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
    finally:
        e.close()
    return {"wall_ms": stats(wall), "steps_per_episode": int(lens.max()), "env_steps": int(lens.sum())}


def acrobot_entry(_lib, noise, pairs, shapes, reps, warmup):
    """dense[<shape>] on gym.Acrobot-v1: the members, seeds and indices drawn as for the other games, whole episodes to the own limit of 500"""
    from dne_hip import policies
    rs = np.random.RandomState(0)
    seeds = rs.randint(0, 2 ** 32, size=2 * pairs, dtype=np.uint64).astype(np.uint32)
    idx = rs.randint(0, noise.size - 9218 + 1, size=pairs).astype(np.int64)
    r = {"dense": {}}
    for name in shapes:
        eng = _lib.Engine(_lib.KIND_DENSE, _lib.ACROBOT_ACTIONS, max_members=2 * pairs, env=_lib.ENV_ACROBOT, hidden=SHAPES[name], nonlin="relu")
        try:
            eng.noise_upload(noise)
            eng.set_theta(noise[4321:4321 + eng.P] * policies.dense_scale_by(_lib.ENV_ACROBOT, SHAPES[name], _lib.ACROBOT_ACTIONS))
            r["dense"][name], out = timed_evals(eng, idx, seeds, _lib.ACROBOT_STEPS, reps, warmup)
            r["dense"][name]["episodes_ended_early"] = int(np.sum(out[2] < _lib.ACROBOT_STEPS))
            assert eng.check_redzones() == 0
        finally:
            eng.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--route", choices=("all", "host"), default="all")
    ap.add_argument("--games", default="maze,cartpole", help="comma-separated: maze, cartpole, acrobot")
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated shapes of the acrobot's entry: " + ", ".join(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 3 or a.host_reps < 3:
        ap.error("at least three repetitions")
    games, shapes = a.games.split(","), a.shapes.split(",")
    if not games or any(g not in GAMES for g in games) or not shapes or any(s not in SHAPES for s in shapes):
        ap.error("--games takes %s, --shapes %s" % (", ".join(GAMES), ", ".join(SHAPES)))
    from dne_hip import _lib, envs
    pairs = a.members // 2
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    res = {"tool": "dense_timing", "members": 2 * pairs, "reps": a.reps, "warmup": a.warmup, "host_reps": a.host_reps, "route": a.route, "games": games, "lib": "DNE_LIB_PATH" if os.environ.get("DNE_LIB_PATH") else "in-tree"}
    for env in games:
        if env == "acrobot":
            res[env] = acrobot_entry(_lib, noise, pairs, [s for s in SHAPES if s in shapes], a.reps, a.warmup)
            continue
        kind = _lib.KIND_MAZE if env == "maze" else _lib.KIND_CARTPOLE
        limit = _lib.MAZE_STEPS if env == "maze" else _lib.CARTPOLE_STEPS
        rs = np.random.RandomState(0)
        seeds = rs.randint(0, 2 ** 32, size=2 * pairs, dtype=np.uint64).astype(np.uint32)
        r = {}
        P = (N_IN[env] + 1) * 2
        idx = rs.randint(0, noise.size - 9218 + 1, size=pairs).astype(np.int64)
        theta_lin = noise[4321:4321 + P] * linear_scale_by(env)
        r["host_act"] = host_act_route(_lib, envs, env, noise, theta_lin, idx, seeds, a.host_reps)
        if a.route == "all":
            from dne_hip import policies
            r["dense"] = {}
            kept = None
            for name, hidden in SHAPES.items():
                eng = _lib.Engine(_lib.KIND_DENSE, 2, max_members=2 * pairs, env=kind, hidden=hidden, nonlin="relu")
                try:
                    if env == "maze":
                        eng.maze_set_walls(*_lib.load_maze(os.path.join(ROOT, "tests", "golden", "hard_maze.txt")))
                    eng.noise_upload(noise)
                    eng.set_theta(noise[4321:4321 + eng.P] * policies.dense_scale_by(kind, hidden, 2))
                    r["dense"][name], out = timed_evals(eng, idx, seeds, limit, a.reps, a.warmup)
                    assert eng.check_redzones() == 0
                    if name == "16x16":
                        kept = out
                finally:
                    eng.close()
            eng = _lib.Engine(kind, 2, max_members=2 * pairs)
            try:
                if env == "maze":
                    eng.maze_set_walls(*_lib.load_maze(os.path.join(ROOT, "tests", "golden", "hard_maze.txt")))
                eng.noise_upload(noise)
                eng.set_theta(noise[4321:4321 + eng.P] * policies.simple_scale_by(kind))
                r["baked"], out = timed_evals(eng, idx, seeds, limit, a.reps, a.warmup)
                r["baked"]["identical"] = bool(all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                                                   for x, y in zip(out, kept)))
            finally:
                eng.close()
            r["generic_over_baked_kernel"] = r["dense"]["16x16"]["kernel_ms"]["median"] / r["baked"]["kernel_ms"]["median"]
            r["device_beats_host"] = bool(r["dense"]["linear"]["wall_ms"]["range"][1] < r["host_act"]["wall_ms"]["range"][0])
            r["host_over_device_wall"] = r["host_act"]["wall_ms"]["median"] / r["dense"]["linear"]["wall_ms"]["median"]
        res[env] = r
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
