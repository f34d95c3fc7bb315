#!/usr/bin/env python3
"""Deep-GA on a dense policy (DNE_KIND_DENSE, csrc/dense_ga.h), timed on the device: what a generation costs with
device-resident parents of a shape the caller chose.

Population --population (5000), --parents (20), every episode to the environment's own limit (maze 400 on the fixture maze, cart-pole 500 under
its own seeds).  Per environment ('maze', 'cartpole') and shape (linear, 16x16, 64x64x64, relu) it prints, in ONE JSON line:

  eval            (a) dne_dense_ga_eval of the population as children of the bank: kernel_ms = the k_dense_run launch between two device events
                  (dne_profile.eval_ms), wall_ms = the call as the caller sees it (host clock around a call that ends in a device
                  synchronise); medians of --reps after --warmup with min and max; env_steps of one evaluation
  es_eval         dne_es_eval of population / 2 antithetic pairs on the SAME handle, the same figures.  The pairs are the GA's members: the
                  bank holds --parents copies of theta_0 (each built from the one-seed genome of theta_0's index), child i is (i mod parents,
                  idx[i / 2], +-sigma), so both calls run bit-identical thetas under the same seeds -- `same_episodes` says the returns and
                  lengths agree bit for bit -- and what is left between the two kernel_ms is the operands alone: base rows from 20 bank slots
                  instead of one, descriptors from the GA's own arrays.  It was not taken apart further.
  roots_eval      the same population as roots (k_dense_ga_roots in front of k_dense_run): wall_ms
  promote_ms      (b) dne_dense_ga_promote of --parents children (wall, a call that synchronises)
  build_ms        (c) dne_dense_ga_build of --parents parents at genome depth 1, 100 and 1000 (wall)
  iteration       (d) 16x16 only: one whole iteration of ga_gpu.main on this engine (10 validated individuals x 30 episodes, 200 test
                  episodes), from one population evaluation to the next: ms, the part spent inside the engine's calls, host_share
  identical       the device's returns and lengths of (a) equal dne_dense_rollout_host on dne_dense_ga_members_host's thetas bit for bit on
                  the first --check members

A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/dense_ga_time.py [--population 5000] [--parents 20] [--reps 20] [--warmup 3] [--iterations 8] [--out FILE]
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

SHAPES = {"linear": (), "16x16": (16, 16), "64x64x64": (64, 64, 64)}
GAMES = {"maze": "maze", "cartpole": "gym.CartPole-v1"}
SIGMA = 0.02


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


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=5000)
    ap.add_argument("--parents", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--power", type=float, default=0.005)
    ap.add_argument("--maze", default=os.path.join(ROOT, "tests", "golden", "hard_maze.txt"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, es, ga_gpu, policies, tabular_logger
    n, T = a.population // 2 * 2, a.parents
    header, lines = _lib.load_maze(a.maze)
    noise = np.random.RandomState(123).randn(2_000_000).astype(np.float32)
    kinds = {"maze": _lib.KIND_MAZE, "cartpole": _lib.KIND_CARTPOLE}
    own = {"maze": _lib.MAZE_STEPS, "cartpole": _lib.CARTPOLE_STEPS}
    ok, result = True, {}
    for env in ("maze", "cartpole"):
        result[env] = {}
        for name, hidden in SHAPES.items():
            rs = np.random.RandomState(0)
            eng = _lib.Engine(_lib.KIND_DENSE, 2, max_members=n, env=kinds[env], hidden=hidden, nonlin="relu")
            P, last = eng.P, noise.size - eng.P
            eng.noise_upload(noise)
            if env == "maze":
                eng.maze_set_walls(header, lines)
            scale_by = policies.dense_scale_by(kinds[env], hidden, 2)
            eng.dense_ga_set_init_scale(scale_by)
            seeds = None if env == "maze" else rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
            limit = own[env]
            maze_kw = dict(header=header, lines=lines) if env == "maze" else {}
            row = {"P": P}

            def genomes(depth):
                return [(int(rs.randint(0, last + 1)), ) + tuple((int(i), a.power) for i in rs.randint(0, last + 1, size=depth - 1)) for _ in range(T)]

            # (c) build
            row["build_ms"] = {}
            for depth in (1, 100, 1000):
                g = genomes(depth)
                row["build_ms"][str(depth)] = stats(timed(lambda: eng.dense_ga_build(g), max(a.reps // 2, 1), a.warmup))
            # (a) children of a bank of T different parents (depth 1), checked against the twins
            eng.dense_ga_build(genomes(1))
            bank = np.stack([eng.dense_ga_get_parent(j) for j in range(T)])
            parent = rs.randint(T, size=n).astype(np.int32)
            idx = rs.randint(0, last + 1, size=n).astype(np.int64)
            power = np.full(n, a.power, np.float32)
            kern = []

            def evaluate(parent=parent, idx=idx, power=power, kern=kern):
                out = eng.dense_ga_eval(parent, idx, power, limit, seeds)
                kern.append(eng.profile()["eval_ms"])
                return out

            wall = timed(evaluate, a.reps, a.warmup)
            ret, _, ln = evaluate()
            c = min(a.check, n)
            thetas = _lib.dense_ga_members_host(noise, scale_by, bank, parent[:c], idx[:c], power[:c])
            h = _lib.dense_rollout_host(thetas, kinds[env], hidden, "relu", 2, seeds=None if seeds is None else seeds[:c], tslimit=limit, **maze_kw)
            row["identical"] = bool(same((ret[:c], ln[:c]), (h["returns"], h["lengths"])))
            ok = ok and row["identical"]
            row["eval"] = {"kernel_ms": stats(kern[a.warmup:a.warmup + a.reps]), "wall_ms": stats(wall), "env_steps": int(ln.sum())}
            roots = np.full(n, -1, np.int32)
            row["roots_eval"] = {"wall_ms": stats(timed(lambda: eng.dense_ga_eval(roots, idx, power, limit, seeds), max(a.reps // 2, 1), a.warmup))}
            # (b) promotion keeps T parents, so it repeats on its own result
            row["promote_ms"] = stats(timed(lambda: eng.dense_ga_promote(parent[:T], idx[:T], power[:T]), a.reps, a.warmup))
            # (a) again, as the twin of an ES evaluation: the same thetas under the same seeds through both entry points
            idx0 = int(rs.randint(0, last + 1))
            eng.set_theta((noise[idx0:idx0 + P] * scale_by).astype(np.float32), 0)
            eng.dense_ga_build([(idx0, )] * T)
            pair_idx = rs.randint(0, last + 1, size=n // 2).astype(np.int64)
            tw_parent = (np.arange(n) % T).astype(np.int32)
            tw_idx = np.repeat(pair_idx, 2)
            tw_power = np.tile(np.array([SIGMA, -SIGMA], np.float32), n // 2)
            es_seeds = np.zeros(n, np.uint32) if seeds is None else seeds
            k_ga, k_es = [], []

            def ga_twin():
                out = eng.dense_ga_eval(tw_parent, tw_idx, tw_power, limit, seeds)
                k_ga.append(eng.profile()["eval_ms"])
                return out

            def es_twin():
                out = eng.es_eval(pair_idx, SIGMA, limit, es_seeds)
                k_es.append(eng.profile()["eval_ms"])
                return out

            w_ga, w_es = [], []
            for rep in range(a.warmup + a.reps):                                 # interleaved, so that both see the same clocks
                t0 = time.perf_counter(); g_out = ga_twin(); t1 = time.perf_counter(); e_out = es_twin(); t2 = time.perf_counter()
                if rep >= a.warmup:
                    w_ga.append((t1 - t0) * 1e3); w_es.append((t2 - t1) * 1e3)
            same_eps = bool(same((g_out[0], g_out[2]), (e_out[0].reshape(-1), e_out[2].reshape(-1))))
            ok = ok and same_eps
            row["twin"] = {"same_episodes": same_eps, "env_steps": int(g_out[2].sum()),
                           "ga_eval": {"kernel_ms": stats(k_ga[a.warmup:]), "wall_ms": stats(w_ga)},
                           "es_eval": {"kernel_ms": stats(k_es[a.warmup:]), "wall_ms": stats(w_es)}}
            # (d) the driver, at 16x16
            if name == "16x16":
                calls = []

                class Clocked(object):
                    """the engine with a host clock around the calls of the loop that go to the device"""

                    def __init__(self, inner):
                        self.inner = inner

                    def __getattr__(self, attr_name):
                        attr = getattr(self.inner, attr_name)
                        if attr_name not in ("dense_ga_eval", "dense_ga_promote", "dense_ga_build", "ga_select"):
                            return attr

                        def call(*args, **kw):
                            t0 = time.perf_counter()
                            try:
                                return attr(*args, **kw)
                            finally:
                                calls.append((attr_name, t0, time.perf_counter()))
                        return call

                table = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
                table.noise, table._engines = noise, [eng]
                exp = {"game": GAMES[env], "population_size": n, "selection_threshold": T, "validation_threshold": 10,
                       "num_validation_episodes": 30, "num_test_episodes": 200, "episode_cutoff_mode": "env_default", "mutation_power": a.power,
                       "timesteps": 10 ** 12, "maze_file": a.maze}
                skip = 1 + a.warmup
                with tempfile.TemporaryDirectory() as log_dir, open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
                    ga_gpu.main(log_dir, engine=Clocked(eng), noise=table, seed=1, max_iters=skip + a.iterations + 1, **exp)
                starts = [i - 1 for i, cl in enumerate(calls) if cl[0] == "ga_select"]   # the population's evaluation is the call in front of the selection
                it_ms, dev_ms = [], []
                for lo, hi in zip(starts[skip:-1], starts[skip + 1:]):
                    it_ms.append((calls[hi][1] - calls[lo][1]) * 1e3)
                    dev_ms.append(sum(cl[2] - cl[1] for cl in calls[lo:hi]) * 1e3)
                row["iteration"] = {"ms": stats(it_ms), "engine_calls_ms": stats(dev_ms), "iterations": len(it_ms),
                                    "host_share": float(1.0 - np.median(dev_ms) / np.median(it_ms))}
            eng.check_redzones()
            eng.close()
            result[env][name] = row
    out = {"tool": "dense_ga_time", "population": n, "parents": T, "reps": a.reps, "warmup": a.warmup, "sigma": SIGMA, "power": a.power,
           "steps_limit": own, "results": result, "ok": ok}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
