#!/usr/bin/env python3
"""Same-box A/B of ES over the LargeModel: antithetic pairs through dne_es_eval (k_lfc_pair: a pair's theta and noise rows fetched once) against the
same members as groups of one through dne_set_members + dne_eval_members (k_lfc<true, 4>: every row fetched per member) on ANOTHER build of the
library -- the parent commit's, which has no dne_es_eval for this kind; the baseline leg uses only calls that build has.

    python tools/es_large_ab.py --baseline-lib /path/to/parent/libdne_hip.so

Workload: 1000 pairs, sigma 0.02, tslimit 100, the reference's 250 M-entry table (1 GB, past the 256 MiB Infinity Cache), fixed indices and seeds.  A library is chosen when the process loads it, so
every run is a child process (one engine each): a warm-up evaluation, a timed one (host clock around the call, which ends in a device
synchronise) -> env-steps/s, then a second engine with profile_events -> the fc kernel's own time (dne_profile.fc_full_*).  The legs alternate,
--reps times each; one JSON line per run goes to --out, then one summary line: the pair route's median must beat the parent's median by more than
the parent's own spread (max - min over its repetitions) -- the two are claimed to differ only in bytes fetched, anything inside the parent's noise is
no result.  Read against the HBM arithmetic: 7744 x 512 x 4 B = 15.9 MB of eps (and as much theta) per PAIR-step instead of per member-step.
The third leg (the per-member route on THIS build) shows what the group -> member expansion costs the kernels the parent already had."""
import argparse, hashlib, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "deep-neuroevolution_amd"))
    import numpy as np
    from dne_hip import _lib, ga_gpu
    n, P = a.pairs, _lib.num_params(_lib.KIND_GA_LARGE, 18)
    noise = np.random.RandomState(123).randn(a.table).astype(np.float32)
    theta = noise[1234:1234 + P] * ga_gpu.model_scale_by(18, _lib.KIND_GA_LARGE)
    rs = np.random.RandomState(7)
    idx = rs.randint(0, a.table - P + 1, n).astype(np.int64)
    seeds = rs.randint(0, 2 ** 32, size=2 * n, dtype=np.uint64).astype(np.uint32)
    out = {"leg": a.leg, "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "rep": a.rep, "pairs": n, "tslimit": a.tslimit, "table": a.table}

    def evaluate(e):
        if a.leg == "pairs":
            ret, sg, ln = e.es_eval(idx, a.sigma, a.tslimit, seeds)
        else:                                    # calls the parent build has: the same 2n members as groups of one
            e.set_members(np.zeros(2 * n, np.int32), np.repeat(idx, 2), np.tile(np.array([a.sigma, -a.sigma], np.float32), n))
            ret, sg, ln = e.eval_members(2 * n, a.tslimit, seeds)
        return np.asarray(ret).reshape(-1), np.asarray(ln).reshape(-1)

    for prof in (False, True):
        e = _lib.Engine(_lib.KIND_GA_LARGE, 18, max_members=2 * n, profile_events=prof)
        try:
            e.noise_upload(noise)
            e.set_theta(theta)
            evaluate(e)                          # warm-up: code objects, every window shape of the evaluation
            t0 = time.perf_counter()
            ret, ln = evaluate(e)
            dt = time.perf_counter() - t0
            p = e.profile()
            if not prof:
                out.update(env_steps=int(ln.sum()), eval_s=round(dt, 4), env_steps_per_s=round(float(ln.sum()) / dt, 1), eval_ms_events=round(p["eval_ms"], 2),
                           results_sha=hashlib.sha256(ret.tobytes() + ln.tobytes()).hexdigest()[:16])
            else:
                out.update(fc_kind=int(p["fc_full_kind"]), fc_ms=round(p["fc_full_ms"], 2), fc_union_ms=round(p["fc_full_union_ms"], 2),
                           fc_launches=int(p["fc_full_launches"]), fc_member_steps=int(p["fc_full_units"]), profiled_eval_s=round(dt, 4))
                if p["fc_full_units"] > 0:       # achieved bytes/s of the stream each route HAS to fetch: per member-step 2 x 15.9 MB, per pair-step (two member-steps) 2 x 15.9 MB
                    need = 2 * 7744 * 512 * 4 * p["fc_full_units"] / (2 if a.leg == "pairs" else 1)
                    out["fc_needed_TBps_over_union"] = round(need / (p["fc_full_union_ms"] * 1e-3) / 1e12, 3)
        finally:
            e.close()
    print("AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", help="libdne_hip.so built from the parent commit")
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--tslimit", type=int, default=100)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--table", type=int, default=250_000_000, help="noise-table entries (the reference's 250 M = 1 GB: four times the Infinity Cache)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "es_large_pair_ab.jsonl"))
    ap.add_argument("--leg", choices=["parent_members", "members", "pairs"])
    ap.add_argument("--rep", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child run")
    a = ap.parse_args()
    if a.leg:
        return child(a)
    if not a.baseline_lib or not os.path.exists(a.baseline_lib):
        sys.exit("--baseline-lib: the parent commit's libdne_hip.so (build the parent in another checkout)")
    rows = []
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rep in range(a.reps):
            for leg in ("parent_members", "pairs", "members"):
                env = dict(os.environ)
                env.pop("DNE_LIB_PATH", None)
                env["DNE_NSUB"] = "4"   # plan_step cuts windows by GROUPS (1000 pairs / 2000 single members): four windows is what both get at full width; pinned so that they keep it as episodes end
                if leg == "parent_members":
                    env["DNE_LIB_PATH"] = os.path.abspath(a.baseline_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rep", str(rep), "--pairs", str(a.pairs), "--tslimit", str(a.tslimit),
                       "--sigma", str(a.sigma), "--table", str(a.table)]
                r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
                line = [l for l in r.stdout.splitlines() if l.startswith("AB ")]
                if r.returncode != 0 or not line:   # a run that failed ends the A/B: nothing more is started on the device
                    sys.exit("leg %s rep %d failed (exit %d):\n%s" % (leg, rep, r.returncode, r.stdout[-2000:]))
                row = json.loads(line[0][3:])
                rows.append(row)
                f.write(json.dumps(row) + "\n"); f.flush()
                print(json.dumps(row), flush=True)
        rate = {leg: [r["env_steps_per_s"] for r in rows if r["leg"] == leg] for leg in ("parent_members", "pairs", "members")}
        fc = {leg: [r["fc_union_ms"] for r in rows if r["leg"] == leg] for leg in rate}
        spread = max(rate["parent_members"]) - min(rate["parent_members"])
        med = {leg: sorted(v)[len(v) // 2] for leg, v in rate.items()}
        summary = {"summary": "es_large_pair_ab", "pairs": a.pairs, "tslimit": a.tslimit, "table": a.table, "env_steps_per_s": rate, "fc_union_ms": fc,
                   "parent_spread": round(spread, 1), "ratio_pairs_over_parent_median": round(med["pairs"] / med["parent_members"], 4),
                   "ratio_members_over_parent_median": round(med["members"] / med["parent_members"], 4),
                   "same_results": len({r["results_sha"] for r in rows}) == 1,
                   "pairs_clear_parent_noise": med["pairs"] - med["parent_members"] > spread,
                   "every_pairs_run_above_every_parent_run": min(rate["pairs"]) > max(rate["parent_members"])}
        f.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
