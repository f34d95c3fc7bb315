#!/usr/bin/env python3
"""Two builds of the maze code compared on one box in one session: the lines tools/maze_novelty_time.py, tools/maze_gans_time.py and
tools/maze_ga_time.py wrote for a parent tree and a new one, run alternately R times each, into one .jsonl with a verdict per figure.

DIR holds <tool>_<side>_<r>.json for side in (parent, new), r = 1 .. R.  Per figure -- novelty_kernel_ms / novelty_call_ms and pool_kernel_ms /
pool_call_ms per archive size, the whole GA and GA-NS iteration -- the parent's R medians give the noise of that box and hour: spread = their
largest minus their smallest.  A figure holds if the median of the new tree's R medians is at most the parent's largest plus that spread.
Every `identical` field of every line has to be true.

Writes every input line (tagged with side and run), then one summary line; exits 1 if a figure or an `identical` fails.

Usage: python tools/maze_ab_summary.py DIR --out profiles/FILE.jsonl
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

TOOLS = ("maze_novelty_time", "maze_gans_time", "maze_ga_time")


def figures(tool, d):
    """name -> milliseconds, the figures of one tool's line that the comparison is about"""
    med = lambda v: v["median"] if isinstance(v, dict) else v
    out = {}
    if tool == "maze_novelty_time":
        for a in d["archives"]:
            out["novelty_kernel_ms[%d]" % a["archive"]] = med(a["novelty_kernel_ms"])
            out["novelty_call_ms[%d]" % a["archive"]] = med(a["novelty_call_ms"])
    elif tool == "maze_gans_time":
        for a in d["archives"]:
            out["pool_kernel_ms[%d]" % a["archive"]] = med(a["pool_kernel_ms"])
            out["pool_call_ms[%d]" % a["archive"]] = med(a["pool_call_ms"])
        out["ga_ns_iteration_ms"] = med(d["iteration_ms"])
    else:
        out["ga_iteration_ms"] = med(d["iteration_ms"])
    return out


def identical(d):
    return bool(d.get("identical", True)) and all(a["identical"] for a in d.get("archives", []))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    lines, vals, same = [], {"parent": {}, "new": {}}, True
    for tool in TOOLS:
        for side in ("parent", "new"):
            for path in sorted(glob.glob(os.path.join(a.dir, "%s_%s_*.json" % (tool, side)))):
                d = json.loads(open(path).read())
                run = int(os.path.splitext(path)[0].rsplit("_", 1)[1])
                lines.append(dict(d, side=side, run=run))
                same = same and identical(d)
                for name, ms in figures(tool, d).items():
                    vals[side].setdefault(name, []).append(ms)
    summary, ok = {}, same
    for name, parent in vals["parent"].items():
        new = vals["new"][name]
        spread = max(parent) - min(parent)
        holds = bool(np.median(new) <= max(parent) + spread)
        ok = ok and holds
        summary[name] = {"parent_medians": parent, "new_medians": new, "parent_median": float(np.median(parent)), "new_median": float(np.median(new)),
                         "spread": spread, "bound": max(parent) + spread, "holds": holds}
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")
        f.write(json.dumps({"tool": "maze_ab_summary", "runs_per_side": len(lines) // (2 * len(TOOLS)), "all_identical": same, "all_hold": ok,
                            "figures": summary}) + "\n")
    for name, s in summary.items():
        print("%-24s parent %.4f (spread %.4f)  new %.4f  bound %.4f  %s" % (name, s["parent_median"], s["spread"], s["new_median"], s["bound"],
                                                                           "holds" if s["holds"] else "FAILS"))
    print("identical on every line:", same)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
