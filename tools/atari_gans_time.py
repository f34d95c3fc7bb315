#!/usr/bin/env python3
"""GA-NS on Atari, timed on the device: what scoring a generation's final RAM states against archive and population costs, on the device
against on the host.

Population 5000 (`Model`, DNE_KIND_GA with record_bc), 20 parents, k = 25, --tslimit steps an episode.  Every figure is a median over
repetitions after --warmup, with its min and max.  Per archive size (0 / 1000 / 10 000 points):

  (a) device_ms         ga_eval_powers + ram_novelty_pool(k) on the final RAM states where the evaluation left them + archive_append_members of
                        the members a 1 % mask picks (the archive is set back to its size before every repetition), on a host clock around
                        calls that end in a device synchronise; pool_kernel_ms is k_ram_novelty_pool alone between two device events on the
                        engine's stream (ram_novelty_last_ms), pool_call_ms and append_call_ms the two calls on the host clock, eval_ms the
                        evaluation alone
  (b) host_ms           the only form a tree without the kernel has: ga_eval_powers with the bc download + the dense numpy scoring on the host --
                        the [population][archive + population] float64 matrix (squared norms and one matrix product: exact integers), its
                        square root, the diagonal masked, a partition per row, the k smallest averaged; host_scoring_ms is that scoring alone
  ratio                 host_ms median / device_ms median
  identical             the device's novelties AND neighbours equal dne_ram_novelty_pool_host's bit for bit (the timed work is the checked work)
  pool_bytes            (archive + population) * 128 B, what each member tile's pass reads out of L2, and tiles = ceil(population / 4)

Prints ONE JSON line (and writes it with --out).  A machine without a GPU fails at Engine(): there is no fall-back.

Usage: python tools/atari_gans_time.py [--population 5000] [--parents 20] [--k 25] [--archives 0,1000,10000] [--tslimit 100] [--reps 10] [--host-reps 3] [--out FILE]
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
    d = (p * p).sum(axis=1)[:, None] + (pool * pool).sum(axis=1)[None, :] - 2.0 * (p @ pool.T)     # exact: integers below 2^53
    np.sqrt(d, out=d)
    d[np.arange(len(p)), len(archive) + np.arange(len(p))] = np.inf
    kk = min(k, pool.shape[0] - 1)
    return np.partition(d, kk - 1, axis=1)[:, :kk].mean(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=5000)
    ap.add_argument("--parents", type=int, default=20)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--archives", default="0,1000,10000")
    ap.add_argument("--archive-prob", type=float, default=0.01)
    ap.add_argument("--tslimit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dne_hip import _lib, ga_gpu
    n, T = a.population, a.parents
    archives = [int(v) for v in a.archives.split(",")]
    noise = np.random.RandomState(123).randn(25_000_000).astype(np.float32)
    rs = np.random.RandomState(21)
    eng = _lib.Engine(_lib.KIND_GA, 18, max_members=n, record_bc=True)
    eng.noise_upload(noise)
    eng.ga_set_init_scale(ga_gpu.model_scale_by(18, _lib.KIND_GA))
    last = noise.size - eng.P
    parents = [(int(i), ) for i in rs.randint(0, last + 1, size=T)]
    genomes = [parents[int(p)] + ((int(i), 0.005), ) for p, i in zip(rs.randint(T, size=n), rs.randint(0, last + 1, size=n))]
    seeds = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    picked = np.flatnonzero(rs.random_sample(n) < a.archive_prob).astype(np.int32)
    gen = lambda want_bc=False: eng.ga_eval_powers(genomes, a.tslimit, seeds, want_bc=want_bc)
    for _ in range(a.warmup):
        gen()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        gen()
        wall.append((time.perf_counter() - t0) * 1e3)
    bc0 = gen(True)[3]
    out = {"tool": "atari_gans_time", "population": n, "parents": T, "k": a.k, "tslimit": a.tslimit, "reps": a.reps, "host_reps": a.host_reps,
           "warmup": a.warmup, "P": int(eng.P), "appended_per_generation": int(picked.size), "distinct_points": int(len(np.unique(bc0, axis=0))),
           "tiles": (n + _lib.RAM_NOVELTY_MEMBERS - 1) // _lib.RAM_NOVELTY_MEMBERS, "eval_ms": stats(wall), "archives": []}
    ok = True
    for narch in archives:
        ars = np.random.RandomState(narch + 1)
        archive = bc0[ars.randint(n, size=narch)].copy()                                               # where the final states are, a few bytes moved
        if narch:
            archive[np.arange(narch)[:, None], ars.randint(0, 128, (narch, 8))] = ars.randint(0, 256, (narch, 8)).astype(np.uint8)

        def reset():
            eng.archive_clear()
            if narch:
                eng.archive_append_points(archive)

        def device():
            gen()
            t1 = time.perf_counter()
            res = eng.ram_novelty_pool(a.k, neighbours=True)
            t2 = time.perf_counter()
            eng.archive_append_members(picked)
            return res, t1, t2, time.perf_counter()

        for _ in range(a.warmup):
            reset(); device()
        both, call, kern, app = [], [], [], []
        for _ in range(a.reps):
            reset()
            t0 = time.perf_counter()
            (nov, nb), t1, t2, t3 = device()
            both.append((t3 - t0) * 1e3); call.append((t2 - t1) * 1e3); app.append((t3 - t2) * 1e3); kern.append(eng.ram_novelty_last_ms())
        assert eng.archive_size() == narch + picked.size
        host_all, host_score = [], []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            bc = gen(True)[3]
            t1 = time.perf_counter()
            host_nov = host_scoring(bc, archive, a.k)
            t2 = time.perf_counter()
            host_all.append((t2 - t0) * 1e3); host_score.append((t2 - t1) * 1e3)
        twin, twin_nb = _lib.ram_novelty_pool_host(bc, archive, a.k, neighbours=True)
        same = bool(np.array_equal(nov.view(np.uint64), twin.view(np.uint64)) and np.array_equal(nb, twin_nb))
        ok = ok and same
        out["archives"].append({"archive": narch, "device_ms": stats(both), "pool_call_ms": stats(call), "pool_kernel_ms": stats(kern),
                                "append_call_ms": stats(app), "host_ms": stats(host_all), "host_scoring_ms": stats(host_score),
                                "ratio": float(np.median(host_all) / np.median(both)), "identical": same,
                                "pool_bytes": (narch + n) * 128, "host_numpy_max_abs_diff": float(np.abs(host_nov - twin).max())})
    eng.check_redzones()
    eng.close()
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
