// TEST-ONLY: csrc/mjmaze.h alone in a stand-alone program, built by tests/test_mjmaze_cpu.py with -fsanitize=address,undefined,float-cast-overflow
// and run on the CPU (in the manner of tests/pendulum_asan_main.cpp).  Inside the contract: episodes of every width, output count and
// nonlinearity the header builds, with action noise and statistics, in a maze of 1 wall and in one of 64, every buffer of exactly its size.
// Outside it: thetas of NaN, +-inf and +-1e30, a deviation of 0 and of NaN -- nothing in the header may cast such a float to an integer,
// index out of an array or overflow a signed integer.
// Prints "ok <episodes> <steps> facts <n> wild <episodes> <steps>"; any sanitizer report aborts with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "mjmaze.h"

using namespace dne::mjmaze;

static int facts = 0;
#define FACT(c) do { if (!(c)) { std::fprintf(stderr, "fact failed, line %d: %s\n", __LINE__, #c); return 1; } facts++; } while (0)

static uint64_t lcg = 0x7654321;
static float frand() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (float)((lcg >> 40) & 0xffff) / 65536.0f - 0.5f; }

// n walls of exactly 4 n floats: the first across the navigator's path, the others short and scattered
static std::vector<float> walls_of(int n) {
    std::vector<float> w((size_t)n * 4);
    for (int k = 0; k < n; k++) {
        const float cx = k == 0 ? 95.0f : 100.0f + 180.0f * frand(), cy = k == 0 ? 100.0f : 100.0f + 180.0f * frand();
        w[4 * k] = cx; w[4 * k + 1] = cy - (k == 0 ? 80.0f : 6.0f); w[4 * k + 2] = cx + 3.0f; w[4 * k + 3] = cy + (k == 0 ? 80.0f : 6.0f);
    }
    return w;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    long episodes = 0, steps = 0, wild = 0, wild_steps = 0;
    std::vector<float> table(4096);
    for (float &v : table) v = 4.0f * frand();
    Header m{};
    m.disable = 0.0f; m.steps = 400.0f; m.sx = 60.0f; m.sy = 100.0f; m.heading = 0.0f; m.gx = 170.0f; m.gy = 30.0f;
    const int wall_counts[2] = {1, dne::maze::MAX_WALLS};

    // ---- inside the contract
    const int Hs[3] = {64, 128, 256};
    const int outs[4] = {2, 4, 10, 16};
    for (int hi = 0; hi < 3; hi++)
        for (int oi = 0; oi < 4; oi++)
            for (int nl = 0; nl < 2; nl++) {
                const int H = Hs[hi], O = outs[oi], mode = O == 2 ? AC_CONTINUOUS : AC_UNIFORM;
                FACT(shape_ok(H, O, mode, nl));
                Options o{};
                o.n_out = O; o.ac_mode = mode; o.ac_noise_std = 0.01f;
                for (int i = 0; i < OBS; i++) { o.mean[i] = 0.05f * i; o.std[i] = 0.5f + 0.1f * i; }
                const int P = offsets(H, O).P;
                std::vector<float> theta(P);                       // exactly P: a read past the last parameter is a report
                for (float &v : theta) v = 0.3f * frand();
                const int nw = wall_counts[(hi + oi + nl) & 1];
                const std::vector<float> walls = walls_of(nw);
                const int limit = hi == 0 && oi == 0 ? 400 : 23;
                std::vector<float> trace((size_t)limit * TRACE_W);   // exactly [steps][20]
                const Episode e = rollout_host(H, nl, theta.data(), o, m, walls.data(), nw, limit, table.data() + 4096 - AC_NOISE, true, trace.data());
                FACT(e.len == limit);
                FACT(limit == 400 ? e.ret < 0.0f && e.sign == -1.0f : e.ret == 0.0f && e.sign == 0.0f);
                FACT(e.ob_sum[0] == (double)limit);                // the bias input is 1 at every step
                episodes++; steps += e.len;
                std::vector<float> x(OBS), h1(H), h2(H), out(O), act(ADIM);   // exactly their sizes
                const float ob[OBS] = {1.0f, 0.2f, 0.3f, 1.0f, 0.5f, 0.1f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f};
                forward_host(H, nl, theta.data(), o, ob, x.data(), h1.data(), h2.data(), out.data(), act.data());
                FACT(mode == AC_CONTINUOUS || (act[0] >= -0.5f && act[0] <= 0.5f && act[1] >= -0.5f && act[1] <= 0.5f));
            }
    {
        const float tie[4] = {2.0f, 2.0f, nan, nan};
        FACT(pick_dim(tie, 0, 4, AC_UNIFORM) == -0.5f && pick_dim(tie, 1, 4, AC_UNIFORM) == -0.5f);   // a tie picks the lower bin; all NaN gives bin 0
        const float up[4] = {1.0f, 3.0f, nan, 0.0f};
        FACT(pick_dim(up, 0, 4, AC_UNIFORM) == 0.5f && pick_dim(up, 1, 4, AC_UNIFORM) == 0.5f);       // a NaN never wins
        FACT(!shape_ok(96, 2, AC_CONTINUOUS, NL_TANH) && !shape_ok(64, 18, AC_UNIFORM, NL_TANH) && !shape_ok(64, 3, AC_UNIFORM, NL_TANH) &&
             !shape_ok(64, 2, AC_UNIFORM, NL_TANH) && !shape_ok(64, 4, AC_CONTINUOUS, NL_RELU));
        FACT(offsets(256, 2).P == 69378 && offsets(64, 2).P == 5058);
    }

    // ---- outside the contract: no value checked, only that nothing faults
    const float fills[6] = {nan, inf, -inf, 1e30f, -1e30f, 0.0f};
    const float stds[3] = {0.0f, nan, 1.0f};
    for (int f = 0; f < 6; f++)
        for (int sd = 0; sd < 3; sd++)
            for (int nl = 0; nl < 2; nl++) {
                const int H = 64, O = nl ? 10 : 2;
                Options o{};
                o.n_out = O; o.ac_mode = O == 2 ? AC_CONTINUOUS : AC_UNIFORM; o.ac_noise_std = f == 1 ? inf : 1e30f;
                for (int i = 0; i < OBS; i++) { o.mean[i] = f == 0 ? nan : 0.0f; o.std[i] = stds[sd]; }
                std::vector<float> theta(offsets(H, O).P, fills[f]);
                const int nw = wall_counts[(f + sd) & 1];
                const std::vector<float> walls = walls_of(nw);
                const Episode e = rollout_host(H, nl, theta.data(), o, m, walls.data(), nw, 25, table.data(), true, nullptr);
                wild++; wild_steps += e.len;
            }
    std::printf("ok %ld %ld facts %d wild %ld %ld\n", episodes, steps, facts, wild, wild_steps);
    return 0;
}
