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
