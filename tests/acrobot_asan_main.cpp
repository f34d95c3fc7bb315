// Stand-alone host program over csrc/acrobot.h (through csrc/dense.h and csrc/step_env.h) for tests/test_acrobot_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: the reset, the open-loop stepper, the step-at-a-time twins and whole episodes of
// dense policies on exactly sized heap buffers, so that any access past a theta, a state record or an observation is reported.  The facts of the
// contract (seed 0, the three anchors to 1e-12, the solving and the all-zero member on seeds 0..19, ties and NaN in the action rule, the clamps,
// a refused action); members perturbed from a noise table of exactly the size its last admissible offset needs, on the four shapes; then thetas
// and states outside the contract -- NaN, +-inf, 1e30, near FLT_MAX; NaN, infinite and 1e300 states.
// Prints one line "ok episodes <n> <checksum> facts <facts that held> wild <episodes outside the contract>"; a sanitizer finding aborts it, a
// fact that does not hold ends it with status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dense.h"

using namespace dne;

static int g_facts = 0;
#define FACT(cond)                                                         \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "fact failed: %s\n", #cond); return 1; } \
        g_facts++;                                                         \
    } while (0)

static bool near(double a, double b) { return fabs(a - b) <= 1e-12; }

int main() {
    uint32_t lcg = 12345u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) * (1.0f / 8388608.0f) - 1.0f); };   // [-1, 1)
    double sum = 0.0;
    int episodes = 0, wild = 0;
    const stepenv::MazeCtx none{};

    {   // the reset: seed 0 as the contract states it, the extreme seeds inside [-0.1, 0.1)
        const acrobot::State s = acrobot::reset_state(0u);
        FACT(s.th1 == 0.07666216164272852 && s.th2 == -0.013694400590298 && s.w1 == -0.09471324568148046 && s.w2 == 0.09417639563076571);
        for (uint32_t seed : {1u, 0x80000000u, 0xFFFFFFFFu}) {
            const acrobot::State r = acrobot::reset_state(seed);
            for (double v : {r.th1, r.th2, r.w1, r.w2}) FACT(v >= -0.1 && v < 0.1);
        }
    }
    {   // the anchors: (0, 0, 0, 0) under actions 2, 2, 0 (libm's values in gym's spelling, to 1e-12), on a buffer of exactly three rows
        const int32_t act[3] = {2, 2, 0};
        const double zero[4] = {0.0, 0.0, 0.0, 0.0};
        std::vector<double> rows(3 * 5);
        acrobot::actions_host(act, 3, zero, rows.data());
        FACT(near(rows[0], -0.013262967177227795) && near(rows[1], 0.03428722934738544) && near(rows[2], -0.12866185280996106) && near(rows[3], 0.33450108998660194));
        FACT(near(rows[5], -0.0484896538093726) && near(rows[6], 0.12748779480535294) && near(rows[7], -0.2132848732767469) && near(rows[8], 0.5754630640496233));
        FACT(near(rows[10], -0.06723706338620503) && near(rows[11], 0.18553771278886602) && near(rows[12], 0.030714304370452555) && near(rows[13], -0.0064477093097422555));
        FACT(rows[4] == 0.0 && rows[9] == 0.0 && rows[14] == 0.0);
    }
    {   // the action rule: the first maximum, a NaN never wins, all NaN gives 0
        const float up = nextafterf(1.0f, 2.0f);
        const float t0[3] = {1.0f, 1.0f, 1.0f}, t1[3] = {1.0f, up, up}, t2[3] = {1.0f, 1.0f, up}, t3[3] = {NAN, NAN, NAN}, t4[3] = {NAN, 0.0f, 1.0f},
                    t5[3] = {0.0f, NAN, 1.0f}, t6[3] = {0.0f, 1.0f, NAN}, t7[3] = {-0.0f, 0.0f, 0.0f}, t8[3] = {up, 1.0f, up};
        FACT(acrobot::pick_action(t0) == 0 && acrobot::pick_action(t1) == 1 && acrobot::pick_action(t2) == 2 && acrobot::pick_action(t3) == 0);
        FACT(acrobot::pick_action(t4) == 0 && acrobot::pick_action(t5) == 2 && acrobot::pick_action(t6) == 1 && acrobot::pick_action(t7) == 0 && acrobot::pick_action(t8) == 0);
    }
    {   // the clamps: a state beyond both stays ON them; the step twins refuse action 3 for the whole batch before anything moves
        acrobot::State s{-2.0, 2.5, -acrobot::MAX_VEL_1, acrobot::MAX_VEL_2};
        acrobot::step(s, 1);
        FACT(s.w1 == -acrobot::MAX_VEL_1 && s.w2 == acrobot::MAX_VEL_2 && s.th1 >= -pendulum::PI && s.th1 <= pendulum::PI);
        const int n = 3;
        const uint32_t seeds[n] = {1u, 2u, 3u};
        std::vector<double> st((size_t)n * 4), before;
        std::vector<int32_t> steps(n), limit(n);
        std::vector<uint8_t> done(n);
        std::vector<float> obs((size_t)n * acrobot::OBS), rew(n);
        FACT(stepenv::reset_host(stepenv::ENV_ACROBOT, n, seeds, &none, 0, st.data(), steps.data(), limit.data(), done.data(), obs.data()) == 0);
        FACT(limit[0] == 500 && steps[2] == 0 && done[1] == 0);
        before = st;
        const int32_t bad[n] = {0, 1, 3}, good[n] = {0, 1, 2};
        FACT(stepenv::step_host(stepenv::ENV_ACROBOT, n, bad, &none, st.data(), steps.data(), limit.data(), done.data(), rew.data(), obs.data()) == -2);
        FACT(st == before && steps[0] == 0);
        FACT(stepenv::step_host(stepenv::ENV_ACROBOT, n, good, &none, st.data(), steps.data(), limit.data(), done.data(), rew.data(), obs.data()) == 0);
        FACT(steps[0] == 1 && steps[2] == 1 && rew[0] == -1.0f && st != before);
        stepenv::Dims d;
        FACT(stepenv::dims(stepenv::ENV_ACROBOT, &d) && d.obs == 6 && d.act == 1 && d.state == 4 && d.act_is_int == 1 && d.own_limit == 500);
    }
    dense::Shape lin;
    FACT(dense::make_shape(stepenv::ENV_ACROBOT, 0, nullptr, 0, dense::NL_RELU, 3, &lin) == dense::SHAPE_OK && lin.P == 21);
    FACT(dense::make_shape(stepenv::ENV_ACROBOT, 0, nullptr, 0, dense::NL_RELU, 2, &lin) == dense::SHAPE_OUT);
    FACT(dense::make_shape(stepenv::ENV_ACROBOT, 0, nullptr, 0, dense::NL_RELU, 3, &lin) == dense::SHAPE_OK && dense::MAX_P == 9218);
    {   // the two named members on seeds 0..19: "torque follows omega2" ends early with return -(length - 1), the all-zero member runs 500 steps
        const int n = 20;
        std::vector<float> solver((size_t)n * 21, 0.0f), zero((size_t)n * 21, 0.0f), ret(n), sg(n);
        std::vector<uint32_t> seeds(n);
        std::vector<int32_t> len(n);
        std::vector<double> st((size_t)n * 4);
        for (int i = 0; i < n; i++) { seeds[i] = (uint32_t)i; solver[(size_t)i * 21 + 15] = -1.0f; solver[(size_t)i * 21 + 17] = 1.0f; solver[(size_t)i * 21 + 19] = -1e-3f; }
        dense::rollout_host(lin, solver.data(), n, seeds.data(), nullptr, none, 500, ret.data(), sg.data(), len.data(), st.data());
        for (int i = 0; i < n; i++) { FACT(len[i] >= 60 && len[i] < 500 && ret[i] == -(float)(len[i] - 1) && sg[i] == ret[i]); sum += len[i]; }
        dense::rollout_host(lin, zero.data(), n, seeds.data(), nullptr, none, 5000, ret.data(), sg.data(), len.data(), st.data());
        for (int i = 0; i < n; i++) FACT(len[i] == 500 && ret[i] == -500.0f);
        episodes += 2 * n;
    }
    const int32_t widths[4][3] = {{0, 0, 0}, {16, 16, 0}, {5, 33, 0}, {64, 64, 64}};
    const int n_hidden[4] = {0, 2, 2, 3}, nonlin[4] = {dense::NL_RELU, dense::NL_RELU, dense::NL_TANH, dense::NL_RELU}, want_p[4] = {21, 435, 335, 8963};
    for (int c = 0; c < 4; c++) {   // the four shapes: members base + scale * table[off + p] with off at 0 and at the table's last admissible position
        dense::Shape sh;
        FACT(dense::make_shape(stepenv::ENV_ACROBOT, n_hidden[c], widths[c], n_hidden[c], nonlin[c], 3, &sh) == dense::SHAPE_OK && sh.P == want_p[c]);
        const size_t P = (size_t)sh.P, count = P + 777;
        std::vector<float> table(count), base(P);
        for (float &v : table) v = next();
        for (float &v : base) v = 0.5f * next();
        const size_t offs[3] = {0, 31, count - P};
        const int limits[3] = {1, 7, 500};
        for (int e = 0; e < 3; e++) {
            std::vector<float> theta(P), ret(1), sg(1), obs(acrobot::OBS), out(3);
            for (size_t p = 0; p < P; p++) theta[p] = maze::perturbed(base[p], e == 1 ? -0.05f : 0.05f, table[offs[e] + p]);
            const uint32_t seed = 1000u + (uint32_t)(3 * c + e);
            std::vector<int32_t> len(1);
            std::vector<double> st(4);
            for (int l = 0; l < 3; l++) {
                dense::rollout_host(sh, theta.data(), 1, &seed, nullptr, none, limits[l], ret.data(), sg.data(), len.data(), st.data());
                FACT(len[0] >= 1 && len[0] <= limits[l] && (ret[0] == -(float)len[0] || ret[0] == -(float)(len[0] - 1)));
                sum += len[0] + st[0] + st[3];
                episodes++;
            }
            for (float &v : obs) v = next();
            int hid = 0;
            for (int l = 1; l <= sh.n_hidden; l++) hid += sh.dim[l];
            std::vector<float> layers((size_t)hid);
            dense::forward_host(sh, theta.data(), obs.data(), hid ? layers.data() : nullptr, out.data());
            int32_t a = -1;
            dense::write_action(stepenv::ENV_ACROBOT, out.data(), &a);
            FACT(a >= 0 && a <= 2);
            sum += out[0] + out[1] + out[2];
        }
        // outside the contract: non-finite and huge parameters, then states no reset gives
        const float fill[6] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 3e38f};
        for (int e = 0; e < 6; e++) {
            std::vector<float> theta(P, fill[e]), ret(1), sg(1);
            const uint32_t seed = 77u + (uint32_t)e;
            std::vector<int32_t> len(1);
            std::vector<double> st(4);
            dense::rollout_host(sh, theta.data(), 1, &seed, nullptr, none, 500, ret.data(), sg.data(), len.data(), st.data());
            FACT(len[0] >= 1 && len[0] <= 500);
            wild++;
        }
        const double bad[6][4] = {{NAN, 0, 0, 0}, {0, 0, NAN, 0}, {0, INFINITY, 0, 0}, {0, 0, 0, -INFINITY}, {1e300, 0, 0, 0}, {0, 1e308, 1e308, 0}};
        std::vector<float> theta(P, 0.25f), ret(1), sg(1);
        for (int e = 0; e < 6; e++) {
            const uint32_t seed = 0u;
            std::vector<int32_t> len(1);
            std::vector<double> st(4);
            dense::rollout_host(sh, theta.data(), 1, &seed, bad[e], none, 40, ret.data(), sg.data(), len.data(), st.data());
            FACT(len[0] >= 1 && len[0] <= 40);
            wild++;
        }
    }
    printf("ok episodes %d %.6f facts %d wild %d\n", episodes, sum, g_facts, wild);
    return 0;
}
