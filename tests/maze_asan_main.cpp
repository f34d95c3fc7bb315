// Stand-alone host program over csrc/maze.h for tests/test_maze_cpu.py, which builds it with -fsanitize=address,undefined and runs it:
// the host rollout (with and without a trace) and the open-loop stepper on the maze file given as argv[1], on thetas from a small
// generator, with exactly sized heap buffers so that any access past a wall array, a theta or a trace row is reported.
// Then thetas outside every contract -- output biases NaN, +-inf, +-1e30, weights near FLT_MAX -- and the math probe on NaN, infinities and
// huge arguments: built with -fsanitize=float-cast-overflow as well, so a NaN or an infinity reaching a cast to int is reported.
// Prints one line "ok <episodes> <checksum> nan <episodes outside the contract> <how many of them returned -500>"; a sanitizer finding aborts it.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "maze.h"

using namespace dne::maze;

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s MAZE_FILE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    float disable, steps, poi[2];
    int nlines = 0;
    Header m{};
    in >> disable >> steps >> nlines >> m.sx >> m.sy >> m.heading >> m.gx >> m.gy >> poi[0] >> poi[1];
    if (!in || nlines < 1 || nlines > MAX_WALLS) { fprintf(stderr, "bad maze file\n"); return 2; }
    m.disable = disable; m.steps = steps;
    std::vector<float> walls((size_t)nlines * 4);
    for (float &v : walls) in >> v;
    if (!in) { fprintf(stderr, "short maze file\n"); return 2; }

    uint32_t lcg = 12345u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) * (1.0f / 8388608.0f) - 1.0f); };   // [-1, 1)
    double sum = 0.0;
    int episodes = 0;
    const int limits[4] = {1, 7, 399, 400};
    for (int e = 0; e < 12; e++) {
        std::vector<float> theta(NPARAMS);
        const float scale = e < 6 ? 0.3f : 3.0f;
        for (float &v : theta) v = scale * next();
        for (int nw = 1; nw <= nlines; nw += (nlines > 1 ? nlines - 1 : 1)) {      // the first wall alone, then all of them
            std::vector<float> w(walls.begin(), walls.begin() + (size_t)nw * 4);
            const int tslimit = limits[e % 4];
            std::vector<float> trace((size_t)tslimit * TRACE_W);
            float ret, xy[2];
            int32_t len;
            rollout_host(theta.data(), m, w.data(), nw, tslimit, &ret, &len, xy, e % 2 ? trace.data() : nullptr);
            sum += ret + len + xy[0] + xy[1];
            episodes++;
        }
    }
    {   // the open-loop stepper: saturating actions, with the collision freeze of `disable` switched on
        Header md = m;
        md.disable = 1.0f;
        const int T = 400;
        std::vector<float> act((size_t)T * 2), rows((size_t)T * 18), obs0(OBS);
        for (int t = 0; t < T; t++) { act[2 * t] = 0.7f * next(); act[2 * t + 1] = 0.7f; }
        actions_host(act.data(), T, md, walls.data(), nlines, rows.data(), obs0.data());
        sum += rows[(size_t)(T - 1) * 18 + 17];
        episodes++;
    }
    int wild = 0, lost = 0;
    {   // outside the contract: the actions are NaN, infinite or huge on every step, or become so when the fmaf chains overflow
        const float bias[6][2] = {{NAN, NAN}, {NAN, 0.7f}, {0.0f, NAN}, {INFINITY, -INFINITY}, {-1e30f, 1e30f}, {0.0f, 0.0f}};
        for (int e = 0; e < 6; e++) {
            std::vector<float> theta(NPARAMS, e == 5 ? 3e38f : 0.0f);
            theta[B3] = bias[e][0]; theta[B3 + 1] = bias[e][1];
            for (int tslimit : {7, 400}) {
                std::vector<float> trace((size_t)tslimit * TRACE_W);
                float ret, xy[2];
                int32_t len;
                rollout_host(theta.data(), m, walls.data(), nlines, tslimit, &ret, &len, xy, trace.data());
                wild++;
                lost += ret == -500.0f;
            }
        }
        const double xs[10] = {NAN, -NAN, INFINITY, -INFINITY, 1e300, -1e300, 1e10, -4.4e9, 3e38, -0.0};
        std::vector<double> out(2);
        for (int fn = 0; fn < MATH_FNS; fn++)
            for (double x : xs) math_probe(fn, x, out.data());
    }
    printf("ok %d %.6f nan %d %d\n", episodes, sum, wild, lost);
    return 0;
}
