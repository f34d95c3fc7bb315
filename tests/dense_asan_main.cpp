// Stand-alone host program over csrc/dense.h for tests/test_dense_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: make_shape, forward_host and rollout_host of every shape of the test list on
// heap buffers of exactly P floats a theta, OBS floats an observation, sum(hidden) floats of layers, OUT floats of outputs, n returns,
// lengths and n * S doubles of state, so that any access past a member's record is reported; the facts of the semantics (P, the offsets, the
// limits, the maze's reward on step 400 alone, reward 1 per cart-pole step, the sign-returns); then outside the contract: thetas filled with
// NaN, +-inf, 1e30, -0.0 and a mixture.
// Prints one line "ok shapes <n> episodes <n> wild <n> facts <n> <checksum>"; a sanitizer finding aborts it, a fact that does not hold ends
// it with status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dense.h"

using namespace dne;
using namespace dne::dense;

static int g_facts = 0;
#define FACT(cond)                                                         \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "fact failed: %s (line %d)\n", #cond, __LINE__); return 1; } \
        g_facts++;                                                         \
    } while (0)

struct Case { int env, n_hidden; int32_t w[3]; int nonlin; };

int main() {
    uint32_t lcg = 2024u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) * (1.0f / 8388608.0f) - 1.0f); };   // [-1, 1)
    // a small maze of its own: a box and one wall inside it, start (30, 30), goal (170, 170)
    const std::vector<float> walls = {0, 0, 200, 0, 200, 0, 200, 200, 200, 200, 0, 200, 0, 200, 0, 0, 100, 20, 100, 150};
    stepenv::MazeCtx mz{};
    mz.hdr = maze::Header{0.0f, 400.0f, 30.0f, 30.0f, 0.0f, 170.0f, 170.0f, 0.0f};
    mz.walls = walls.data(); mz.nw = (int)walls.size() / 4;

    std::vector<Case> cases;
    for (int env : {KIND_MAZE, KIND_CARTPOLE}) {
        cases.push_back({env, 0, {0, 0, 0}, NL_RELU});
        cases.push_back({env, 1, {1, 0, 0}, NL_RELU});
        cases.push_back({env, 2, {16, 16, 0}, NL_RELU});
        cases.push_back({env, 2, {5, 33, 0}, NL_RELU});
        cases.push_back({env, 3, {64, 64, 64}, NL_RELU});
        cases.push_back({env, 1, {64, 0, 0}, NL_TANH});
    }
    cases.push_back({KIND_PENDULUM, 0, {0, 0, 0}, NL_RELU});
    cases.push_back({KIND_PENDULUM, 2, {5, 33, 0}, NL_RELU});
    cases.push_back({KIND_PENDULUM, 1, {64, 0, 0}, NL_TANH});

    {   // what make_shape refuses, and the layouts the baked kernels share
        Shape sh;
        const int32_t w16[3] = {16, 16, 0}, bad_w[3] = {16, 65, 0}, tail[3] = {16, 0, 4}, zero[3] = {0, 0, 0};
        FACT(make_shape(KIND_MAZE, 2, w16, 3, NL_RELU, 2, &sh) == SHAPE_OK && sh.P == maze::NPARAMS);
        FACT(sh.off[0] == maze::W1 && sh.off[1] == maze::W2 && sh.off[2] == maze::W3 && sh.off[1] - 16 == maze::B1 && sh.off[2] - 16 == maze::B2 && sh.P - 2 == maze::B3);
        FACT(make_shape(KIND_CARTPOLE, 2, w16, 3, NL_RELU, 2, &sh) == SHAPE_OK && sh.P == cartpole::NPARAMS && sh.off[1] == cartpole::W2 && sh.off[2] == cartpole::W3);
        const int32_t w64[3] = {64, 64, 64};
        FACT(make_shape(KIND_MAZE, 3, w64, 3, NL_TANH, 2, &sh) == SHAPE_OK && sh.P == MAX_P && MAX_P == 9218);
        FACT(make_shape(7, 0, zero, 3, NL_RELU, 2, &sh) == SHAPE_ENV && make_shape(0, 0, zero, 3, NL_RELU, 2, &sh) == SHAPE_ENV);
        FACT(make_shape(KIND_MAZE, 4, w64, 3, NL_RELU, 2, &sh) == SHAPE_LAYERS && make_shape(KIND_MAZE, -1, w64, 3, NL_RELU, 2, &sh) == SHAPE_LAYERS);
        FACT(make_shape(KIND_MAZE, 2, bad_w, 3, NL_RELU, 2, &sh) == SHAPE_WIDTH && make_shape(KIND_MAZE, 1, zero, 3, NL_RELU, 2, &sh) == SHAPE_WIDTH);
        FACT(make_shape(KIND_MAZE, 1, tail, 3, NL_RELU, 2, &sh) == SHAPE_TAIL);
        FACT(make_shape(KIND_MAZE, 0, zero, 3, NL_RELU, 1, &sh) == SHAPE_OUT && make_shape(KIND_PENDULUM, 0, zero, 3, NL_RELU, 2, &sh) == SHAPE_OUT);
        FACT(make_shape(KIND_MAZE, 0, zero, 3, 2, 2, &sh) == SHAPE_NONLIN && make_shape(KIND_MAZE, 0, zero, 3, -1, 2, &sh) == SHAPE_NONLIN);
    }

    double sum = 0.0;
    long episodes = 0, wild = 0;
    for (const Case &c : cases) {
        Shape sh;
        const int n_out = env_outputs(c.env);
        FACT(make_shape(c.env, c.n_hidden, c.w, 3, c.nonlin, n_out, &sh) == SHAPE_OK);
        stepenv::Dims d;
        FACT(stepenv::dims(c.env, &d) && sh.dim[0] == d.obs && sh.dim[c.n_hidden + 1] == n_out);
        int hid = 0, P = 0;
        for (int l = 0; l <= c.n_hidden; l++) { FACT(sh.off[l] == P); P += (sh.dim[l] + 1) * sh.dim[l + 1]; if (l) hid += sh.dim[l]; }
        FACT(P == sh.P);
        const int n = 3;
        std::vector<float> theta((size_t)n * P);
        for (float &v : theta) v = 0.6f * next();
        {   // the forward pass: every buffer exactly its size; theta = 0 gives the biases (here 0) on every layer
            std::vector<float> obs(d.obs), layers(hid), out(n_out), zeros(P, 0.0f);
            for (float &v : obs) v = next();
            std::vector<float> actf(c.env == KIND_MAZE ? 2 : 1);
            std::vector<int32_t> act(1, 0);
            void *actp = c.env == KIND_CARTPOLE ? (void *)act.data() : (void *)actf.data();
            for (int i = 0; i < n; i++) {
                forward_host(sh, theta.data() + (size_t)i * P, obs.data(), hid ? layers.data() : nullptr, out.data());
                write_action(c.env, out.data(), actp);
                for (float v : out) { FACT(std::isfinite(v)); sum += v; }
                if (c.nonlin == NL_RELU) for (float v : layers) FACT(v >= 0.0f);
                else for (float v : layers) FACT(v >= -1.0f && v <= 1.0f);
                if (c.env == KIND_CARTPOLE) FACT(act[0] == (out[1] > out[0] ? 1 : 0));
            }
            forward_host(sh, zeros.data(), obs.data(), nullptr, out.data());
            for (float v : out) FACT(v == 0.0f);
            write_action(c.env, out.data(), actp);
            if (c.env == KIND_CARTPOLE) FACT(act[0] == 0);                   // two equal logits: the first maximum
        }
        const std::vector<uint32_t> seeds = {0u, 0x80000000u, 0xFFFFFFFFu};
        for (int tslimit : {1, 7, 100000}) {
            std::vector<float> ret(n), sg(n);
            std::vector<int32_t> len(n);
            std::vector<double> state((size_t)n * d.state);
            rollout_host(sh, theta.data(), n, seeds.data(), nullptr, mz, tslimit, ret.data(), sg.data(), len.data(), state.data());
            const int limit = stepenv::step_limit(tslimit, d.own_limit);
            for (int i = 0; i < n; i++) {
                FACT(len[i] >= 1 && len[i] <= limit);
                if (c.env != KIND_CARTPOLE) FACT(len[i] == limit);
                if (c.env == KIND_CARTPOLE) FACT(ret[i] == (float)len[i] && sg[i] == ret[i]);
                if (c.env == KIND_MAZE) FACT(limit == 400 ? (ret[i] < 0.0f && sg[i] == -1.0f) : (ret[i] == 0.0f && sg[i] == 0.0f));
                if (c.env == KIND_PENDULUM) FACT(ret[i] < 0.0f && sg[i] == -(float)limit);
                sum += ret[i] + state[(size_t)i * d.state];
                episodes++;
            }
        }
        // outside the contract: thetas no run gives
        const float fills[5] = {NAN, INFINITY, -INFINITY, 1e30f, -0.0f};
        for (int e = 0; e < 6; e++) {
            std::vector<float> th((size_t)n * P);
            for (size_t k = 0; k < th.size(); k++) th[k] = e < 5 ? fills[e] : (k % 5 == 4 ? 0.3f * next() : fills[k % 5]);
            std::vector<float> ret(n), sg(n);
            std::vector<int32_t> len(n);
            std::vector<double> state((size_t)n * d.state);
            rollout_host(sh, th.data(), n, seeds.data(), nullptr, mz, 12, ret.data(), sg.data(), len.data(), state.data());
            for (int i = 0; i < n; i++) FACT(len[i] >= 1 && len[i] <= 12);
            wild++;
        }
    }
    printf("ok shapes %zu episodes %ld wild %ld facts %d %.6f\n", cases.size(), episodes, wild, g_facts, sum);
    return 0;
}
