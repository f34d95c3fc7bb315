// Stand-alone host program over csrc/step_env.h for tests/test_stepenv_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: reset_host, step_host and observe_host of every kind on heap buffers of exactly
// n * S doubles, n * OBS floats, n steps, limits, flags, rewards and actions, so that any access past an environment's record is reported;
// the facts of the semantics (limits, the maze's reward on step 400 alone, reward 1 per cart-pole step, frozen done environments, a refused
// cart-pole action leaves the batch alone); then outside the contract: NaN and +-inf actions, and NaN, infinite and huge states written into
// the records as dne_stepenv_set_state would (a NaN where the maze keeps an int included).
// Prints one line "ok <environments stepped> <checksum> facts <facts that held> wild <batches outside the contract>"; a sanitizer finding
// aborts it, a fact that does not hold ends it with status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "step_env.h"

using namespace dne;
using namespace dne::stepenv;

static int g_facts = 0;
#define FACT(cond)                                                         \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "fact failed: %s (line %d)\n", #cond, __LINE__); return 1; } \
        g_facts++;                                                         \
    } while (0)

// a batch of n environments, every array exactly its size
struct HostBatch {
    int kind, n;
    Dims d;
    std::vector<double> state;
    std::vector<int32_t> steps, limit;
    std::vector<uint8_t> done;
    std::vector<float> obs, reward;
    HostBatch(int kind_, int n_) : kind(kind_), n(n_) {
        dims(kind, &d);
        state.resize((size_t)n * d.state); steps.resize(n); limit.resize(n); done.resize(n); obs.resize((size_t)n * d.obs); reward.resize(n);
    }
    int reset(const uint32_t *seeds, const MazeCtx *mz, int max_steps) {
        return reset_host(kind, n, seeds, mz, max_steps, state.data(), steps.data(), limit.data(), done.data(), obs.data());
    }
    int step(const void *act, const MazeCtx *mz) {
        return step_host(kind, n, act, mz, state.data(), steps.data(), limit.data(), done.data(), reward.data(), obs.data());
    }
};

int main() {
    uint32_t lcg = 12345u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) * (1.0f / 8388608.0f) - 1.0f); };   // [-1, 1)
    double sum = 0.0;
    long stepped = 0;

    // a small maze of its own: a box and one wall inside it, start (30, 30), goal (170, 170)
    const std::vector<float> walls = {0, 0, 200, 0, 200, 0, 200, 200, 200, 200, 0, 200, 0, 200, 0, 0, 100, 20, 100, 150};
    MazeCtx mz{};
    mz.hdr = maze::Header{0.0f, 400.0f, 30.0f, 30.0f, 0.0f, 170.0f, 170.0f, 0.0f};
    mz.walls = walls.data(); mz.nw = (int)walls.size() / 4;

    {   // the widths
        Dims d;
        FACT(dims(KIND_MAZE, &d) && d.obs == 11 && d.act == 2 && d.state == 7 && !d.act_is_int && d.own_limit == 400);
        FACT(dims(KIND_CARTPOLE, &d) && d.obs == 4 && d.act == 1 && d.state == 4 && d.act_is_int && d.own_limit == 500);
        FACT(dims(KIND_PENDULUM, &d) && d.obs == 3 && d.act == 1 && d.state == 2 && !d.act_is_int && d.own_limit == 200);
        for (int k = 0; k < 4; k++) FACT(!dims(k, &d));
        FACT(step_limit(0, 400) == 400 && step_limit(-3, 400) == 400 && step_limit(399, 400) == 399 && step_limit(5000, 400) == 400 && step_limit(1, 200) == 1);
        FACT(to_int(NAN) == 0 && to_int(INFINITY) == 0 && to_int(-1e300) == 0 && to_int(3.0) == 3 && to_int(-2147483648.0) == -2147483647 - 1);
    }
    for (int max_steps : {0, 1, 7}) {   // every kind: its limit's steps and three more
        for (int kind : {KIND_MAZE, KIND_CARTPOLE, KIND_PENDULUM}) {
            const int n = 3;
            HostBatch b(kind, n);
            const std::vector<uint32_t> seeds = {0u, 0x80000000u, 0xFFFFFFFFu};
            FACT(b.reset(seeds.data(), &mz, max_steps) == 0);
            const int limit = step_limit(max_steps, b.d.own_limit);
            for (int i = 0; i < n; i++) FACT(b.steps[i] == 0 && b.done[i] == 0 && b.limit[i] == limit);
            std::vector<float> fa((size_t)n * b.d.act);
            std::vector<int32_t> ia(n);
            std::vector<double> ret(n, 0.0), frozen;
            std::vector<float> frozen_obs;
            for (int t = 0; t < limit + 3; t++) {
                for (float &v : fa) v = (kind == KIND_PENDULUM ? 3.0f : 0.7f) * next();
                for (int32_t &v : ia) v = next() > 0.0f ? 1 : 0;
                const bool all_done = b.done[0] && b.done[1] && b.done[2];
                if (all_done && frozen.empty()) { frozen = b.state; frozen_obs = b.obs; }
                FACT(b.step(kind == KIND_CARTPOLE ? (const void *)ia.data() : (const void *)fa.data(), &mz) == 0);
                for (int i = 0; i < n; i++) ret[i] += (double)b.reward[i];
                if (all_done) {
                    for (int i = 0; i < n; i++) FACT(b.reward[i] == 0.0f && b.done[i] == 1);
                    FACT(memcmp(frozen.data(), b.state.data(), frozen.size() * sizeof(double)) == 0);
                    FACT(memcmp(frozen_obs.data(), b.obs.data(), frozen_obs.size() * sizeof(float)) == 0);
                }
            }
            for (int i = 0; i < n; i++) {
                FACT(b.done[i] == 1 && b.steps[i] >= 1 && b.steps[i] <= limit);
                if (kind != KIND_CARTPOLE) FACT(b.steps[i] == limit);
                if (kind == KIND_CARTPOLE) FACT(ret[i] == (double)b.steps[i]);
                if (kind == KIND_MAZE) FACT(limit == 400 ? ret[i] < 0.0 : ret[i] == 0.0);
                sum += ret[i] + b.state[(size_t)i * b.d.state];
                stepped++;
            }
        }
    }
    {   // a cart-pole action outside {0, 1} moves nothing
        HostBatch b(KIND_CARTPOLE, 2);
        const uint32_t seeds[2] = {5u, 6u};
        FACT(b.reset(seeds, nullptr, 0) == 0);
        const std::vector<double> before = b.state;
        const int32_t bad[2] = {1, 2};
        FACT(b.step(bad, nullptr) == -2 && b.state == before && b.steps[0] == 0 && b.steps[1] == 0);
        FACT(reset_host(2, 1, seeds, nullptr, 0, b.state.data(), b.steps.data(), b.limit.data(), b.done.data(), b.obs.data()) == -1);
    }
    int wild = 0;
    {   // outside the contract: NaN and +-inf actions
        const float bad[5] = {NAN, INFINITY, -INFINITY, 1e30f, -3e38f};
        for (int kind : {KIND_MAZE, KIND_PENDULUM})
            for (int e = 0; e < 5; e++) {
                HostBatch b(kind, 2);
                const uint32_t seeds[2] = {7u, 8u};
                FACT(b.reset(seeds, &mz, 12) == 0);
                std::vector<float> fa((size_t)2 * b.d.act);
                for (int t = 0; t < 14; t++) {
                    for (size_t k = 0; k < fa.size(); k++) fa[k] = (t + k) % 3 == 0 ? bad[e] : 0.3f;
                    FACT(b.step(fa.data(), &mz) == 0);
                }
                FACT(b.done[0] == 1 && b.done[1] == 1 && b.steps[0] == 12);
                wild++;
            }
        // ... and states no reset gives, written into the records: observed, then stepped
        const double vals[6] = {NAN, INFINITY, -INFINITY, 1e300, -1e308, 4e9};
        for (int kind : {KIND_MAZE, KIND_CARTPOLE, KIND_PENDULUM})
            for (int e = 0; e < 6; e++) {
                HostBatch b(kind, 7);
                std::vector<uint32_t> seeds(b.n, 3u);
                FACT(b.reset(seeds.data(), &mz, 0) == 0);
                for (int i = 0; i < b.n; i++) b.state[(size_t)i * b.d.state + i % b.d.state] = vals[e];   // one field each, the maze's ints included
                FACT(observe_host(kind, b.n, b.state.data(), &mz, b.obs.data()) == 0);
                std::vector<float> fa((size_t)b.n * b.d.act, 0.4f);
                std::vector<int32_t> ia(b.n, 1);
                for (int t = 0; t < 5; t++) FACT(b.step(kind == KIND_CARTPOLE ? (const void *)ia.data() : (const void *)fa.data(), &mz) == 0);
                for (int i = 0; i < b.n; i++) FACT(b.steps[i] >= 1 && b.steps[i] <= 5);
                wild++;
            }
    }
    printf("ok %ld %.6f facts %d wild %d\n", stepped, sum, g_facts, wild);
    return 0;
}
