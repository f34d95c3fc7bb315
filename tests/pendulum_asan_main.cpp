// TEST-ONLY: csrc/pendulum.h alone in a stand-alone program, built by tests/test_pendulum_cpu.py with -fsanitize=address,undefined,float-cast-overflow
// and run on the CPU (in the manner of tests/cartpole_asan_main.cpp).  Inside the contract: episodes of every shape the header builds, with
// action noise and statistics, traces written to buffers of exactly their size.  Outside it: thetas of NaN, +-inf and +-1e30, a deviation
// of 0 and of NaN, states no reset gives -- nothing in the header may cast such a float to an integer (tanh_f's range reduction is guarded
// by its two early returns, sincos_d's by its own), index out of an array or overflow a signed integer.
// Prints "ok <episodes> <steps> facts <n> wild <episodes> <steps>"; any sanitizer report aborts with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pendulum.h"

using namespace dne::pendulum;

static int facts = 0;
#define FACT(c) do { if (!(c)) { std::fprintf(stderr, "fact failed, line %d: %s\n", __LINE__, #c); return 1; } facts++; } while (0)

static uint64_t lcg = 0x1234567;
static float frand() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (float)((lcg >> 40) & 0xffff) / 65536.0f - 0.5f; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    long episodes = 0, steps = 0, wild = 0, wild_steps = 0;
    std::vector<float> table(4096);
    for (float &v : table) v = 4.0f * frand();

    // ---- inside the contract
    const int Hs[3] = {64, 128, 256};
    const int outs[4] = {1, 2, 5, 16};
    for (int hi = 0; hi < 3; hi++)
        for (int oi = 0; oi < 4; oi++)
            for (int nl = 0; nl < 2; nl++) {
                const int H = Hs[hi], O = outs[oi];
                Options o{};
                o.n_out = O; o.ac_mode = O == 1 ? AC_CONTINUOUS : AC_UNIFORM; o.ac_noise_std = 0.01f;
                for (int i = 0; i < OBS; i++) { o.mean[i] = 0.1f * i; o.std[i] = 0.5f + i; }
                const int P = offsets(H, O).P;
                std::vector<float> theta(P);                       // exactly P: a read past the last parameter is a report
                for (float &v : theta) v = 0.3f * frand();
                const int limit = hi == 0 ? 200 : 37;
                std::vector<double> trace((size_t)limit * TRACE_W);   // exactly [steps][8]
                const Episode e = rollout_host(H, nl, theta.data(), o, 1000u + hi, nullptr, limit, table.data() + 4096 - EPISODE_STEPS, true, trace.data());
                FACT(e.len == limit);
                FACT(e.ret <= 0.0f && e.sign >= -(float)limit);
                episodes++; steps += e.len;
                std::vector<float> x(OBS), h1(H), h2(H), out(O);   // exactly their sizes
                const float ob[OBS] = {1.0f, 0.0f, 8.0f};
                const float a = forward_host(H, nl, theta.data(), o, ob, x.data(), h1.data(), h2.data(), out.data());
                FACT(a >= -2.0f - 1e-6f || o.ac_mode == AC_CONTINUOUS);
            }
    {
        FACT(tanh_f(0.0f) == 0.0f && tanh_f(-0.0f) == -0.0f && tanh_f(inf) == 1.0f && tanh_f(-inf) == -1.0f && tanh_f(nan) != tanh_f(nan));
        FACT(tanh_f(1e-30f) == 1e-30f && tanh_f(3.4e38f) == 1.0f && tanh_f(-1e-45f) == -1e-45f);
        const State r0 = reset_state(0u), r1 = reset_state(0xffffffffu);
        FACT(r0.theta >= -PI && r0.theta < PI && r1.theta_dot >= -1.0 && r1.theta_dot < 1.0);
        const float first[3] = {nan, 2.0f, 2.0f};
        FACT(pick_action(first, 3, AC_UNIFORM) == 0.0f);     // a NaN never wins, the first of two equal maxima does: bin 1 of 3 = 0
    }

    // ---- outside the contract: no value checked, only that nothing faults
    const float fills[6] = {nan, inf, -inf, 1e30f, -1e30f, 0.0f};
    const float stds[3] = {0.0f, nan, 1.0f};
    const double inits[6][2] = {{1e300, 0.0}, {-1e300, 1e300}, {(double)inf, 0.0}, {0.0, (double)nan}, {1e17, -1e17}, {(double)nan, (double)inf}};
    for (int f = 0; f < 6; f++)
        for (int sd = 0; sd < 3; sd++)
            for (int nl = 0; nl < 2; nl++) {
                const int H = 64, O = nl ? 5 : 1;
                Options o{};
                o.n_out = O; o.ac_mode = O == 1 ? AC_CONTINUOUS : AC_UNIFORM; o.ac_noise_std = f == 1 ? inf : 1e30f;
                for (int i = 0; i < OBS; i++) { o.mean[i] = f == 0 ? nan : 0.0f; o.std[i] = stds[sd]; }
                std::vector<float> theta(offsets(H, O).P, fills[f]);
                const Episode e = rollout_host(H, nl, theta.data(), o, 7u, inits[(f + sd) % 6], 25, table.data(), true, nullptr);
                wild++; wild_steps += e.len;
            }
    std::printf("ok %ld %ld facts %d wild %ld %ld\n", episodes, steps, facts, wild, wild_steps);
    return 0;
}
