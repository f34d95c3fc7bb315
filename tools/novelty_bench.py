#!/usr/bin/env python3
"""Novelty scoring at NS-ES scale: the 5 000 RAM trajectories recorded by one pop-5000 es_eval
(2500 antithetic pairs; tools/workloads.py's engine, iteration 0 inputs) scored against device-resident archives of 32 .. 4096 entries.

Section "batch" needs only novelty_batch + dne_archive_append, so the parent commit's library runs it too (DNE_LIB_PATH):
  fixture  entries with the recorded trajectories' own lengths (the NS-ES leg's profile, mean ~140 rows)
  long     synthetic entries of 1000-5000 rows (every pair walks the entry's rows)
Section "single" (both builds): dne_novelty, the one-trajectory call the drivers make per parent (nses.py:24), with a
trajectory of the fixture's median length ("fixture") or of 3000 rows ("long") against the same archives.
Section "knn" (this build only): Engine.novelty_knn on host-supplied member sets of 1000-5000 rows.
Each case: one warm-up, then --repeats timed calls (host clock around a call that ends in a stream synchronise), the
median; the sha256 of the outputs lets two builds be compared.  One JSON line per case (stdout, and --out if given)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workloads as W  # noqa: E402
from dne_hip import _lib, es  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="32,256,1024,4096")
ap.add_argument("--kinds", default="fixture,long")
ap.add_argument("--sections", default="batch,single,knn")
ap.add_argument("--knn-members", default="256,1024")
ap.add_argument("--knn-sizes", default="32,1024")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()

POOL = np.random.RandomState(2024).randint(0, 256, (12000, 128)).astype(np.uint8)   # entries are row windows of one pool


def entries(lengths, seed):
    rs = np.random.RandomState(seed)
    return [POOL[o:o + n] for n, o in zip(lengths, rs.randint(0, POOL.shape[0] - 5000, len(lengths)))]


def timed(fn):
    out = fn()                                   # warm-up (uploads any new archive entries)
    ts = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


noise = es.SharedNoiseTable()
e = W._es_engine(noise, 18, 2500, 0, 1, 0, 0, 0, 0, None, None, record_bc=True, bc_max_steps=5000)
with open(_lib.LIB_PATH, "rb") as f:   # which build: DNE_LIB_PATH (another build of the same ABI) or the in-tree library
    lib = {"lib": "DNE_LIB_PATH" if os.environ.get("DNE_LIB_PATH") else "in-tree", "lib_sha16": hashlib.sha256(f.read()).hexdigest()[:16]}
try:
    _, idx, seeds = es.generation_inputs(noise.noise.size, e.P, 2500, 0, 0, 1)
    _, _, ln = e.es_eval(idx, 0.02, 5000, seeds)
    ln = ln.reshape(-1).astype(np.int32)
    base = dict(lib, members=int(ln.size), member_len_mean=float(ln.mean()), member_len_max=int(ln.max()), k=a.k)
    rs = np.random.RandomState(5)
    if "batch" in a.sections:
        for kind in a.kinds.split(","):
            for narch in [int(s) for s in a.sizes.split(",")]:
                lens = rs.choice(ln, narch) if kind == "fixture" else rs.randint(1000, 5001, narch)
                arch = entries(lens, narch)
                out, ts = timed(lambda: e.novelty_batch(arch, ln, a.k))
                emit(dict(base, section="batch", kind=kind, archive=narch, archive_len_mean=float(np.mean(lens)),
                          median_ms=1e3 * float(np.median(ts)), times_ms=[round(1e3 * t, 3) for t in ts],
                          checksum=hashlib.sha256(out.tobytes()).hexdigest()[:16], novelty_mean=float(out.mean())))
    if "single" in a.sections:
        for kind in a.kinds.split(","):
            bc = entries([int(np.median(ln)) if kind == "fixture" else 3000], 55)[0]
            for narch in [int(s) for s in a.sizes.split(",")]:
                lens = rs.choice(ln, narch) if kind == "fixture" else rs.randint(1000, 5001, narch)
                arch = entries(lens, narch)
                out, ts = timed(lambda: np.array([e.novelty(arch, bc, a.k)]))
                emit(dict(lib, section="single", kind=kind, bc_len=int(bc.shape[0]), archive=narch, archive_len_mean=float(np.mean(lens)),
                          k=a.k, median_ms=1e3 * float(np.median(ts)), times_ms=[round(1e3 * t, 3) for t in ts],
                          checksum=hashlib.sha256(out.tobytes()).hexdigest()[:16]))
    if "knn" in a.sections and hasattr(e.lib, "dne_novelty_knn"):
        for nm in [int(s) for s in a.knn_members.split(",")]:
            mlen = rs.randint(1000, 5001, nm).astype(np.int32)
            members = entries(mlen, 77 + nm)
            for narch in [int(s) for s in a.knn_sizes.split(",")]:
                lens = rs.randint(1000, 5001, narch)
                arch = entries(lens, 99 + narch)
                out, ts = timed(lambda: e.novelty_knn(arch, a.k, bcs=members))
                emit(dict(base, section="knn", members=nm, member_len_mean=float(mlen.mean()), member_len_max=int(mlen.max()), archive=narch,
                          archive_len_mean=float(np.mean(lens)), median_ms=1e3 * float(np.median(ts)),
                          times_ms=[round(1e3 * t, 3) for t in ts], checksum=hashlib.sha256(out.tobytes()).hexdigest()[:16]))
finally:
    e.close()
