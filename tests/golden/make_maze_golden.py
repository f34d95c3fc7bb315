#!/usr/bin/env python3
"""Record the reference's hard maze (gpu_implementation/gym_tensorflow/maze/maze.h, unmodified) under open-loop action sequences.

Like make_golden.py this runs only where the reference tree is present; its outputs tests/golden/maze_reference_rollouts.npz and
tests/golden/hard_maze.txt (the reference's data file, copied byte for byte) are committed.  Nothing compiled and no reference text is:
the driver below is this project's own, it is compiled against the reference's header into a temporary directory (g++ -O2, x86-64
baseline: no FMA, glibc's float trig) and deleted with it.

The driver does what tf_maze.cpp:78-98 does around the header -- reset(), then per step interpret_outputs(a0 + 0.5, 0.5 + a1), Update(),
steps++, reward = -distance_to_target() once steps >= 400 -- and writes per step: obs[11], x, y, heading, speed, ang_vel, collisions, reward.

32 sequences of 400 steps, piecewise-constant actions in [-0.7, 0.7], segments of 5..40 steps, in five families (checked below on the
recording itself): random; gentle (off the walls for >= 100 steps); pinned (driven into a wall, colliding for hundreds of steps);
spin (the heading wraps through 0 / 360 again and again); saturate (alternating +-0.7: the +-3 clamps and the +-0.2 rate limit).

A second recording, tests/golden/maze_reference_edges.npz, takes the same driver over the edge mazes below (maze_edge_*.txt, this project's own
files in the reference's format, written here) under constant and piecewise-constant sequences that include NaN, infinite, 1e30 and denormal
actions: the branches and comparisons at equality that the fixture maze never reaches.  Each intended consequence is checked on the recording.

Usage: python tests/golden/make_maze_golden.py --reference DIR     (DIR: the reference tree's root; or DNE_REFERENCE=DIR)
"""
import argparse
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
T = 400
FAMILIES = ("random", "gentle", "pinned", "spin", "saturate")
COUNTS = (12, 6, 6, 4, 4)

DRIVER = r"""
// usage: driver MAZE_FILE ACTIONS_IN ROWS_OUT N T      actions: float32 [N][T][2]; rows: float32 [N][11 + T * 18]
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "maze.h"
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int n = atoi(argv[4]), T = atoi(argv[5]);
    std::vector<float> act((size_t)n * T * 2), rows((size_t)n * (11 + T * 18));
    FILE *f = fopen(argv[2], "rb");
    if (!f || fread(act.data(), sizeof(float), act.size(), f) != act.size()) return 3;
    fclose(f);
    for (int i = 0; i < n; i++) {
        maze::Environment env(argv[1]);
        env.reset();
        int steps = 0;
        float *out = rows.data() + (size_t)i * (11 + T * 18);
        env.generate_neural_inputs(out);
        out += 11;
        for (int t = 0; t < T; t++, out += 18) {
            const float *a = act.data() + ((size_t)i * T + t) * 2;
            env.interpret_outputs(float(a[0]) + 0.5, 0.5 + float(a[1]));
            env.Update();
            steps += 1;
            env.generate_neural_inputs(out);
            out[11] = env.hero.location.x; out[12] = env.hero.location.y; out[13] = env.hero.heading;
            out[14] = env.hero.speed; out[15] = env.hero.ang_vel; out[16] = (float)env.hero.collisions;
            out[17] = steps >= 400 ? -env.distance_to_target() : 0.0f;
        }
    }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(rows.data(), sizeof(float), rows.size(), f) != rows.size()) return 4;
    fclose(f);
    return 0;
}
"""


def piecewise(rs, draw):
    """[T][2] float32: segments of 5..40 steps, draw(segment number) -> (a0, a1)"""
    out = np.zeros((T, 2), np.float32)
    t = k = 0
    while t < T:
        n = int(rs.randint(5, 41))
        out[t:t + n] = np.clip(np.asarray(draw(k), np.float32), -0.7, 0.7)
        t += n
        k += 1
    return out


def sequences(seed=2018):
    rs = np.random.RandomState(seed)
    seqs, fam = [], []
    for f, count in zip(FAMILIES, COUNTS):
        for i in range(count):
            sign = 1.0 if i % 2 == 0 else -1.0
            if f == "random":
                draw = lambda k: rs.uniform(-0.7, 0.7, size=2)
            elif f == "gentle":      # a slow small circle away from the start corner's walls
                draw = lambda k: (-rs.uniform(0.12, 0.3), rs.uniform(0.0, 0.02))
            elif f == "pinned":      # straight ahead at speed until a wall stops it
                draw = lambda k: (rs.uniform(-0.004, 0.004), rs.uniform(0.4, 0.7))
            elif f == "spin":
                draw = lambda k: (sign * rs.uniform(0.45, 0.7), rs.uniform(-0.05, 0.05))
            else:
                draw = lambda k: (0.7 if (k + i) % 2 == 0 else -0.7, -0.7 if (k + i // 2) % 2 == 0 else 0.7)
            seqs.append(piecewise(rs, draw))
            fam.append(FAMILIES.index(f))
    return np.stack(seqs), np.array(fam, np.int32)


# ---- the edge mazes and their sequences ---------------------------------------------------------------------------------------------------
BOX = [(0, 0, 200, 0), (200, 0, 200, 200), (200, 200, 0, 200), (0, 200, 0, 0)]
ON_Y_LINE = (120, 100, 160, 100)          # on the start's y line, 60 away: parallel to the heading-0 and heading-180 rays (rBot == 0)
EDGE_SEQS = ("still", "straight", "spin", "mixed", "wait_then_straight", "nan_turn_from_10", "nan_speed_from_50", "inf_inf", "ninf_1e30",
             "n1e30_ninf", "denormal")


def edge_mazes(fixture_path):
    """name -> (disable, start, goal, walls): hard_maze's geometry is read from the fixture, as numbers"""
    v = [float(t) for t in open(fixture_path).read().split()]
    n = int(v[2])
    hard = [tuple(v[10 + 4 * i:14 + 4 * i]) for i in range(n)]
    start, goal = (v[3], v[4]), (v[6], v[7])
    return {
        "disable": (1, start, goal, hard),
        "zero_wall": (0, start, goal, hard + [(150, 100, 150, 100)]),                       # a zero-length wall far from the start
        "dist_8": (0, (60, 100), (60, 30), BOX + [(68, 60, 68, 140), ON_Y_LINE]),           # a wall at distance exactly 8.0; goal straight above
        "dist_7_99": (0, (60, 100), (60, 170), BOX + [(67.99, 60, 67.99, 140), ON_Y_LINE]), # ... at 7.99; goal straight below
        "goal_on_start": (1, (60, 100), (60, 100), BOX + [ON_Y_LINE]),
        # the heading-0 ray from (60, 100) to (160, 100) meets the first wall at its end A (r == 0), the second at its end B (r == 1) and the
        # third with its own tip (s == 1): none of them is a hit, the rangefinder stays at 100
        "ray_endpoint": (0, (60, 100), (170, 30), BOX + [(90, 100, 90, 140), (110, 60, 110, 100), (160, 50, 160, 150)]),
    }


def write_maze(path, disable, start, goal, walls):
    fmt = lambda x: repr(float(x)).rstrip("0").rstrip(".") if float(x) != int(x) else str(int(x))
    with open(path, "w") as f:
        f.write("%d\n400\n%d\n%s %s\n0\n%s %s\n%s %s\n" % (disable, len(walls), fmt(start[0]), fmt(start[1]), fmt(goal[0]), fmt(goal[1]),
                                                                fmt(goal[0]), fmt(goal[1])))
        for w in walls:
            f.write(" ".join(fmt(c) for c in w) + "\n")


def edge_sequences():
    """[len(EDGE_SEQS)][T][2] float32"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    out = np.zeros((len(EDGE_SEQS), T, 2), np.float32)
    const = {"still": (0, 0), "straight": (0, 0.7), "spin": (0.7, 0), "mixed": (-0.3, 0.5), "inf_inf": (inf, inf), "ninf_1e30": (-inf, 1e30),
             "n1e30_ninf": (-1e30, -inf), "denormal": (1e-40, -1e-40)}
    for k, name in enumerate(EDGE_SEQS):
        if name in const:
            out[k] = np.asarray(const[name], np.float32)
        elif name == "wait_then_straight":
            out[k, 20:] = (0, 0.7)
        elif name == "nan_turn_from_10":
            out[k] = (0, 0.7); out[k, 10:, 0] = nan
        else:
            out[k] = (-0.3, 0.5); out[k, 50:, 1] = nan
    assert out[EDGE_SEQS.index("denormal"), 0, 0] != 0 and abs(out[EDGE_SEQS.index("denormal"), 0, 0]) < np.finfo(np.float32).tiny
    return out


def record(cxx, maze_dir, tmp, maze_file, actions):
    """the driver (compiled once per run) on one maze file: (obs0 [n][11], rows [n][T][18])"""
    exe = os.path.join(tmp, "driver")
    if not os.path.exists(exe):
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        subprocess.check_call([cxx, "-O2", "-I", maze_dir, "-o", exe, os.path.join(tmp, "driver.cpp")])
    n = actions.shape[0]
    actions.tofile(os.path.join(tmp, "actions.bin"))
    subprocess.check_call([exe, maze_file, os.path.join(tmp, "actions.bin"), os.path.join(tmp, "rows.bin"), str(n), str(T)],
                          stdout=subprocess.DEVNULL)        # (the reference prints a line per NaN it meets)
    raw = np.fromfile(os.path.join(tmp, "rows.bin"), np.float32).reshape(n, 11 + T * 18)
    return raw[:, :11].copy(), raw[:, 11:].reshape(n, T, 18).copy()


def check_edges(name, disable, obs0, rows):
    """the consequences each edge maze is there for, on the recording itself"""
    q = {s: k for k, s in enumerate(EDGE_SEQS)}
    x, y, speed, coll, reward = rows[..., 11], rows[..., 12], rows[..., 14], rows[..., 16], rows[..., 17]
    steps = np.arange(1, T + 1)
    finite = [k for k, s in enumerate(EDGE_SEQS) if not s.startswith("nan")]
    assert np.all(np.isfinite(rows[finite])) and np.all(rows[finite, -1, 17] <= 0), name
    for s in ("nan_turn_from_10", "nan_speed_from_50"):
        assert np.any(np.isnan(rows[q[s]])), (name, s)
        assert (reward[q[s], -1] == -500) == bool(np.isnan(x[q[s], -1])), (name, s)            # a NaN position ends at -500, no other does
    if disable:
        for k in finite:
            if coll[k, -1] > 0:
                t0 = int(np.flatnonzero(coll[k] > 0)[0])
                assert np.all(x[k, t0:] == x[k, t0]) and np.all(y[k, t0:] == y[k, t0]), (name, k)  # frozen from the first collision on
                assert np.array_equal(coll[k, t0:], np.arange(1, T - t0 + 1)), (name, k)            # one more collision per step
        k = q["straight"]
        assert 0 < coll[k, -1] < T and speed[k, -1] != 0, name                                       # ... while the speed is not 0
    if name == "disable":
        assert coll[q["still"], -1] == 0
    if name == "zero_wall":
        assert np.all(coll == steps) and np.all(x == x[0, 0]) and np.all(y == y[0, 0])               # every step collides, nobody moves
    if name == "dist_8":
        assert np.all(coll[q["still"]] == 0) and np.all(coll[q["spin"]] == 0)                        # d == 8.0 is no collision
        assert obs0[q["still"], 7:].tolist() == [0, 0, 0, 1] and np.all(rows[q["still"], :, 7:11] == [0, 0, 0, 1])
        assert reward[q["nan_turn_from_10"], -1] == -500 and reward[q["nan_speed_from_50"], -1] == -500
    if name == "dist_7_99":
        for s in ("still", "spin", "straight"):
            assert np.all(coll[q[s]] == steps), s                                                    # d == 7.99 is one, on every step
        assert obs0[q["still"], 7:].tolist() == [0, 1, 0, 0] and np.all(rows[q["still"], :, 7:11] == [0, 1, 0, 0])
    if name == "goal_on_start":
        assert obs0[q["still"], 7:].tolist() == [0, 0, 0, 1] and np.all(rows[q["still"], :, 7:11] == [0, 0, 0, 1])
        assert rows[q["still"], -1, 17] == 0 and np.signbit(rows[q["still"], -1, 17])                # -distance = -0.0
    if name == "ray_endpoint":
        assert obs0[q["still"], 3] == 1.0 and np.all(rows[q["still"], :, 3] == 1.0)                  # the heading-0 ray hits nothing
        assert obs0[q["still"], 4] < 1.0                                                             # (the +45 degree ray meets the first wall)
        assert reward[q["nan_turn_from_10"], -1] == -500 and reward[q["nan_speed_from_50"], -1] == -500


def main_edges(cxx, maze_dir, tmp, version):
    mazes = edge_mazes(os.path.join(HERE, "hard_maze.txt"))
    actions = edge_sequences()
    obs0, rows = [], []
    for name, (disable, start, goal, walls) in mazes.items():
        path = os.path.join(HERE, "maze_edge_%s.txt" % name)
        write_maze(path, disable, start, goal, walls)
        o, r = record(cxx, maze_dir, tmp, path, actions)
        check_edges(name, disable, o, r)
        obs0.append(o); rows.append(r)
    obs0, rows = np.stack(obs0), np.stack(rows)
    np.savez_compressed(os.path.join(HERE, "maze_reference_edges.npz"), actions=actions, mazes=np.array(list(mazes)), sequences=np.array(EDGE_SEQS),
                        obs0=obs0, rows=rows, compiler=np.array(version))
    print("wrote", rows.shape[0], "edge mazes x", rows.shape[1], "sequences; collisions at the end:")
    for k, name in enumerate(mazes):
        print("  %-14s" % name, rows[k, :, -1, 16].astype(int).tolist(), "NaN rows:", int(np.isnan(rows[k]).any(axis=-1).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DNE_REFERENCE"), help="root of the reference tree (or DNE_REFERENCE)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or DNE_REFERENCE) must name the reference tree's root")
    maze_dir = os.path.join(args.reference, "gpu_implementation", "gym_tensorflow", "maze")
    shutil.copyfile(os.path.join(maze_dir, "hard_maze.txt"), os.path.join(HERE, "hard_maze.txt"))
    actions, fam = sequences()
    n = actions.shape[0]
    cxx = os.environ.get("CXX", "g++")
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        subprocess.check_call([cxx, "-O2", "-I", maze_dir, "-o", os.path.join(tmp, "driver"), os.path.join(tmp, "driver.cpp")])
        actions.tofile(os.path.join(tmp, "actions.bin"))
        subprocess.check_call([os.path.join(tmp, "driver"), os.path.join(HERE, "hard_maze.txt"), os.path.join(tmp, "actions.bin"),
                               os.path.join(tmp, "rows.bin"), str(n), str(T)])
        raw = np.fromfile(os.path.join(tmp, "rows.bin"), np.float32).reshape(n, 11 + T * 18)
        version = subprocess.check_output([cxx, "--version"]).decode().splitlines()[0]
        os.remove(os.path.join(tmp, "driver"))
        main_edges(cxx, maze_dir, tmp, version)
    obs0, rows = raw[:, :11].copy(), raw[:, 11:].reshape(n, T, 18).copy()
    coll, heading, speed, angv = rows[:, :, 16], rows[:, :, 13], rows[:, :, 14], rows[:, :, 15]
    # the families are what they claim to be, on the recording itself
    for i in range(n):
        f = FAMILIES[fam[i]]
        if f == "gentle":
            assert coll[i, 99] == 0, (i, "gentle sequence collided within 100 steps")
        if f == "pinned":
            assert coll[i, -1] >= 200, (i, coll[i, -1])
        if f == "spin":
            assert np.sum(np.abs(np.diff(heading[i])) > 300) >= 2, i
        if f == "saturate":
            assert np.any(np.abs(speed[i]) == 3.0) and np.any(np.abs(angv[i]) == 3.0), i
            assert np.any(np.isclose(np.abs(np.diff(speed[i])), 0.2, atol=1e-6)), i
    assert np.all(rows[:, :-1, 17] == 0) and np.all(rows[:, -1, 17] < 0)
    np.savez_compressed(os.path.join(HERE, "maze_reference_rollouts.npz"), actions=actions, family=fam, families=np.array(FAMILIES),
                        obs0=obs0, rows=rows, compiler=np.array(version))
    print("wrote", n, "sequences;", {f: int(np.sum(fam == k)) for k, f in enumerate(FAMILIES)}, "collisions at the end:", coll[:, -1].astype(int).tolist())


if __name__ == "__main__":
    main()
