// Stand-alone host program over csrc/maze.h for tests/test_maze_cpu.py, which builds it with -fsanitize=address,undefined and runs it:
// the host rollout (with and without a trace) and the open-loop stepper on the maze file given as argv[1], on thetas from a small
// generator, with exactly sized heap buffers so that any access past a wall array, a theta or a trace row is reported.
// Prints one line "ok <episodes> <checksum>"; a sanitizer finding aborts it.
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
    printf("ok %d %.6f\n", episodes, sum);
    return 0;
}
