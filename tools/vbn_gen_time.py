#!/usr/bin/env python3
"""Same-process timing of one full-width ES generation on the two flat layouts of the GPU tree's ES model: DNE_KIND_ES (es_distributed
parameterisation) and DNE_KIND_ES_VBN (ModelVirtualBN's own).  Both engines share one noise table and one theta -- the native kind runs
theta_0 = noise slice * scale_by, the ES kind its expansion onto the ES layout (+0 biases, unit gammas: the same network) -- and the same
indices and environment seeds; the kinds alternate `--rounds` times after one warm-up generation each.  The members are not the same
networks (the perturbation lands on other offsets), so the env-steps of each generation are printed next to its time.
    python tools/vbn_gen_time.py --rounds 4
"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))
from dne_hip import _lib, es, policies

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2500)
ap.add_argument("--sigma", type=float, default=0.02)
ap.add_argument("--tslimit", type=int, default=5000)
ap.add_argument("--rounds", type=int, default=4)
a = ap.parse_args()

noise = es.SharedNoiseTable()
nact = 18
P = _lib.num_params(_lib.KIND_ES_VBN, nact)
th = noise.get(noise.sample_index(np.random.RandomState(0), P), P) * policies.vbn_scale_by(nact)
vspec, _ = policies.flat_layout(_lib.KIND_ES_VBN, nact)
espec, Pes = policies.flat_layout(_lib.KIND_ES, nact)
th_es = np.zeros(Pes, np.float32)
for vname, ename in (("layer1/conv1/w", "conv1/weights"), ("layer1/BatchNorm/b", "BatchNorm/beta"), ("layer2/conv2/w", "conv2/weights"),
                     ("layer2/BatchNorm/b", "BatchNorm_1/beta"), ("layer3/fc/w", "fc/weights"), ("layer3/BatchNorm/b", "BatchNorm_2/beta"),
                     ("layer4/out/w", "out/weights"), ("layer4/out/b", "out/biases")):
    (vo, vs), (eo, _) = vspec[vname], espec[ename]
    th_es[eo:eo + int(np.prod(vs))] = th[vo:vo + int(np.prod(vs))]
for g in ("BatchNorm/gamma", "BatchNorm_1/gamma", "BatchNorm_2/gamma"):
    o, s = espec[g]
    th_es[o:o + int(np.prod(s))] = 1.0

engines = {}
for name, kind, theta in (("es", _lib.KIND_ES, th_es), ("es_vbn", _lib.KIND_ES_VBN, th)):
    e = _lib.Engine(kind, nact, max_members=2 * a.pairs, ref_count=128)
    noise.attach(e)
    e.set_theta(theta)
    engines[name] = e
env = policies.HipAtariEnv(engines["es"], seed=0)
ref = np.rint(np.stack(es.get_ref_batch(env, batch_size=128, random_stream=np.random.RandomState(0))) * 255.0).astype(np.uint8)
for e in engines.values():
    e.set_ref_batch(ref)
_, idx, seeds = es.generation_inputs(noise.noise.size, Pes, a.pairs, 0, 0, 1)   # legal offsets for both P

rows = []
for r in range(a.rounds + 1):
    for name, e in engines.items():
        e.barrier()
        t0 = time.perf_counter()
        ret, sg, ln = e.es_eval(idx, a.sigma, a.tslimit, seeds)
        ms = (time.perf_counter() - t0) * 1e3
        row = {"round": r, "kind": name, "gen_ms": round(ms, 2), "env_steps": int(ln.sum()), "max_len": int(ln.max()),
               "ms_per_M_steps": round(ms / (ln.sum() / 1e6), 2), "warmup": r == 0}
        rows.append(row)
        print(json.dumps(row), flush=True)
summary = {}
for name in engines:
    t = [x["gen_ms"] for x in rows if x["kind"] == name and not x["warmup"]]
    s = [x["ms_per_M_steps"] for x in rows if x["kind"] == name and not x["warmup"]]
    summary[name] = {"gen_ms_median": float(np.median(t)), "gen_ms_min": min(t), "ms_per_M_steps_median": float(np.median(s))}
print(json.dumps({"summary": summary}))
for e in engines.values():
    e.close()
