// Stand-alone host program over csrc/cartpole.h for tests/test_cartpole_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: the reset, the open-loop stepper, the forward pass and whole episodes (with
// and without a trace, from seeds and from explicit states) on exactly sized heap buffers, so that any access past a theta, a row or a trace
// is reported; the facts of the contract (seed 0, the zero state under constant and alternating actions, the threshold states, theta = 0 and
// the balancing theta); then thetas outside the contract -- NaN, +-inf and 1e30 weights, weights near FLT_MAX -- and states outside it.
// Prints one line "ok <episodes> <checksum> facts <facts that held> wild <episodes outside the contract> <steps they took>"; a sanitizer
// finding aborts it, a fact that does not hold ends it with status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cartpole.h"

using namespace dne::cartpole;

static int g_facts = 0;
#define FACT(cond)                                                         \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "fact failed: %s\n", #cond); return 1; } \
        g_facts++;                                                         \
    } while (0)

static int first_done(const std::vector<double> &rows, int T) {
    for (int t = 0; t < T; t++)
        if (rows[(size_t)t * 5 + 4] != 0.0) return t + 1;
    return T;
}

int main() {
    uint32_t lcg = 12345u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) * (1.0f / 8388608.0f) - 1.0f); };   // [-1, 1)
    double sum = 0.0;
    int episodes = 0;

    {   // the reset: seed 0 as the contract states it, the extreme seeds inside [-0.05, 0.05)
        const State s = reset_state(0u);
        FACT(s.x == 0.03833108082136426 && s.x_dot == -0.006847200295149 && s.theta == -0.04735662284074023 && s.theta_dot == 0.04708819781538286);
        for (uint32_t seed : {1u, 0x80000000u, 0xFFFFFFFFu}) {
            const State r = reset_state(seed);
            for (double v : {r.x, r.x_dot, r.theta, r.theta_dot}) FACT(v >= -0.05 && v < 0.05);
        }
    }
    {   // open loop from the zero state: constant 1 ends at step 9 with theta -0.21518604988500967, constant 0 mirrors it, alternating ends at 33
        const int T = 40;
        const double zero[4] = {0.0, 0.0, 0.0, 0.0};
        std::vector<int32_t> act(T);
        std::vector<double> rows((size_t)T * 5);
        for (int t = 0; t < T; t++) act[t] = 1;
        actions_host(act.data(), T, zero, rows.data());
        FACT(first_done(rows, T) == 9 && rows[8 * 5 + 2] == -0.21518604988500967);
        const double x9 = rows[8 * 5];
        for (int t = 0; t < T; t++) act[t] = 0;
        actions_host(act.data(), T, zero, rows.data());
        FACT(first_done(rows, T) == 9 && rows[8 * 5 + 2] == 0.21518604988500967 && rows[8 * 5] == -x9);
        for (int t = 0; t < T; t++) act[t] = t & 1;
        actions_host(act.data(), T, zero, rows.data());
        FACT(first_done(rows, T) == 33);
        sum += rows[(size_t)(T - 1) * 5];
    }
    {   // the thresholds: ON one goes on, the next double beyond ends (x_dot = theta_dot = 0: the first step leaves x and theta alone)
        for (double sign : {1.0, -1.0})
            for (int a = 0; a < 2; a++) {
                State s{0.0, 0.0, sign * THETA_THRESHOLD, 0.0};
                FACT(!step(s, a));
                s = State{0.0, 0.0, sign * nextafter(THETA_THRESHOLD, 1.0), 0.0};
                FACT(step(s, a));
                s = State{sign * X_THRESHOLD, 0.0, 0.0, 0.0};
                FACT(!step(s, a));
                s = State{sign * nextafter(X_THRESHOLD, 3.0), 0.0, 0.0, 0.0};
                FACT(step(s, a));
            }
    }
    {   // closed loop: theta = 0 (equal logits, action 0) from the zero state, the balancing theta from (0.03, -0.02, 0.04, 0.01)
        std::vector<float> theta(NPARAMS, 0.0f);
        const double zero[4] = {0.0, 0.0, 0.0, 0.0}, init[4] = {0.03, -0.02, 0.04, 0.01};
        std::vector<double> st(4), trace((size_t)EPISODE_STEPS * TRACE_W);
        FACT(rollout_host(theta.data(), 0u, zero, 5000, st.data(), trace.data()) == 9);
        const float w[4] = {0.02f, 0.1f, 1.0f, 0.5f};
        for (int k = 0; k < 4; k++) { theta[W1 + k * HID] = w[k]; theta[W1 + k * HID + 1] = -w[k]; }
        theta[W2] = theta[W2 + HID + 1] = 1.0f;
        theta[W3 + 1] = theta[W3 + ACT] = 1.0f;
        FACT(rollout_host(theta.data(), 0u, init, 5000, st.data(), trace.data()) == 500 && st[0] == 1.2402981400520736);
        FACT(trace[(size_t)499 * TRACE_W + 4] == st[0] && trace[(size_t)499 * TRACE_W] == (double)(float)st[0]);
        std::vector<double> short_trace((size_t)7 * TRACE_W);
        FACT(rollout_host(theta.data(), 0u, init, 7, st.data(), short_trace.data()) == 7);
        episodes += 3;
    }
    {   // ties and NaN in the action rule
        FACT(pick_action(1.0f, 1.0f) == 0 && pick_action(1.0f, nextafterf(1.0f, 2.0f)) == 1 && pick_action(nextafterf(1.0f, 2.0f), 1.0f) == 0);
        FACT(pick_action(NAN, 1.0f) == 0 && pick_action(1.0f, NAN) == 0 && pick_action(NAN, NAN) == 0 && pick_action(-0.0f, 0.0f) == 0);
    }
    const int limits[4] = {1, 7, 499, 500};
    for (int e = 0; e < 12; e++) {   // thetas from a small generator, from seeds, every limit, with and without a trace
        std::vector<float> theta(NPARAMS);
        const float scale = e < 6 ? 0.3f : 3.0f;
        for (float &v : theta) v = scale * next();
        const int tslimit = limits[e % 4];
        std::vector<double> st(4), trace((size_t)tslimit * TRACE_W);
        const int len = rollout_host(theta.data(), 1000u + (uint32_t)e, nullptr, tslimit, st.data(), e % 2 ? trace.data() : nullptr);
        FACT(len >= 1 && len <= tslimit);
        sum += len + st[0] + st[2];
        episodes++;
        std::vector<float> obs(OBS), h1(HID), h2(HID), out(ACT);
        for (float &v : obs) v = next();
        forward_host(theta.data(), obs.data(), h1.data(), h2.data(), out.data());
        sum += out[0] + out[1];
    }
    int wild = 0;
    long wild_steps = 0;
    {   // outside the contract: NaN, infinite and huge weights (the logits are NaN, infinite or overflow), and states no reset gives
        const float fill[6] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 3e38f};
        for (int e = 0; e < 6; e++)
            for (int part = 0; part < 2; part++) {
                std::vector<float> theta(NPARAMS, 0.0f);
                for (int p = part ? B3 : 0; p < NPARAMS; p++) theta[p] = fill[e];   // everything, or the output biases alone
                for (int tslimit : {7, 500}) {
                    std::vector<double> st(4), trace((size_t)tslimit * TRACE_W);
                    wild_steps += rollout_host(theta.data(), 77u + (uint32_t)e, nullptr, tslimit, st.data(), trace.data());
                    wild++;
                }
            }
        const double bad[6][4] = {{NAN, 0, 0, 0}, {0, 0, NAN, 0}, {0, INFINITY, 0, 0}, {0, 0, 0, -INFINITY}, {0, 0, 1e300, 0}, {0, 1e308, 0, 1e308}};
        std::vector<float> theta(NPARAMS, 0.25f);
        for (int e = 0; e < 6; e++) {
            std::vector<double> st(4), trace((size_t)500 * TRACE_W);
            wild_steps += rollout_host(theta.data(), 0u, bad[e], 500, st.data(), trace.data());
            wild++;
        }
    }
    printf("ok %d %.6f facts %d wild %d %ld\n", episodes, sum, g_facts, wild, wild_steps);
    return 0;
}
