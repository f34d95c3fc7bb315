// cartpole.h -- the GPU tree's gym configuration (configurations/es_gym_config.json: gym.CartPole-v1 under SimpleClassifier, models/simple.py:29-35
// over dqn.Model: dense 4 -> 16, relu, dense 16 -> 16, relu, dense 16 -> 2, argmax) as ONE __host__ __device__ text, in the manner of maze.h: the
// reset, the step and the forward pass below compile for the CPU (dne_cartpole_rollout_host, the feature's oracle) and for gfx950
// (k_cartpole_rollout: whole episodes in one launch), and the two agree bit for bit.  DESIGN.md section 13 holds the contract.
//   * The environment is the classic cart-pole restated from its published equations (Barto, Sutton & Anderson 1983 as gym's
//     classic_control/cartpole.py writes them, Euler integration, the CartPole-v1 registration's 500 steps) -- not recorded from gym.
//   * Every operation of the step is an IEEE double operation in the association written here; sine and cosine are maze.h's sincos_d (fma
//     chains, no libm), used, not copied; -ffp-contract=off on both passes.
//   * The reset stream is ours (the reference's reset is unseeded): four splitmix64 draws from the member's uint32 environment seed.
// A plain C++ compiler can include this file (the kernel is behind __HIPCC__): tests/cartpole_asan_main.cpp does.
#pragma once
#include "maze.h"

namespace dne {
namespace cartpole {

using maze::SinCosD;
using maze::dense_unit;
using maze::perturbed;
using maze::relu;
using maze::sincos_d;

constexpr int OBS = 4, HID = 16, ACT = 2, NPARAMS = 386, EPISODE_STEPS = 500 /* CartPole-v1: max_episode_steps */, TRACE_W = 8, ROW = 16;
// flat order = creation order (models/base.py:35-44): fc1/w [4][16], fc1/b, fc2/w [16][16], fc2/b, out/w [16][2], out/b
constexpr int W1 = 0, B1 = 64, W2 = 80, B2 = 336, W3 = 352, B3 = 384;
constexpr double GRAVITY = 9.8, MASSCART = 1.0, MASSPOLE = 0.1, TOTAL_MASS = MASSPOLE + MASSCART, LENGTH = 0.5 /* half the pole */,
                 POLEMASS_LENGTH = MASSPOLE * LENGTH, FORCE_MAG = 10.0, TAU = 0.02, X_THRESHOLD = 2.4,
                 THETA_THRESHOLD = 0x1.acee9f37bebd5p-3;   // 12 * 2 * pi / 360 = 0.20943951023931953

struct State { double x, x_dot, theta, theta_dot; };

// ---- the reset ---------------------------------------------------------------------------------------------------------------------------
// splitmix64 from z = seed: four draws, each u = (r >> 11) * 2^-53 in [0, 1) (the conversion is exact), state[i] = -0.05 + 0.1 * u
MZ_HD State reset_state(uint32_t seed) {
    uint64_t z = seed;
    double v[4];
    for (int i = 0; i < 4; i++) {
        z += 0x9E3779B97F4A7C15ull;
        uint64_t r = z;
        r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull;
        r = (r ^ (r >> 27)) * 0x94D049BB133111EBull;
        r ^= r >> 31;
        const double u = (double)(r >> 11) * 0x1p-53;
        v[i] = -0.05 + 0.1 * u;
    }
    State s;
    s.x = v[0]; s.x_dot = v[1]; s.theta = v[2]; s.theta_dot = v[3];
    return s;
}

// ---- the step ----------------------------------------------------------------------------------------------------------------------------
// one Euler step under action a in {0, 1}; returns done.  The comparisons are strict: a state ON a threshold goes on, and a NaN state
// (outside the contract) is never done.
MZ_HD bool step(State &s, int a) {
    const double force = a == 1 ? FORCE_MAG : -FORCE_MAG;
    const SinCosD t = sincos_d(s.theta);
    const double temp = (force + ((POLEMASS_LENGTH * s.theta_dot) * s.theta_dot) * t.s) / TOTAL_MASS;
    const double thetaacc = (GRAVITY * t.s - t.c * temp) / (LENGTH * (4.0 / 3.0 - ((MASSPOLE * t.c) * t.c) / TOTAL_MASS));
    const double xacc = temp - ((POLEMASS_LENGTH * thetaacc) * t.c) / TOTAL_MASS;
    s.x = s.x + TAU * s.x_dot;
    s.x_dot = s.x_dot + TAU * xacc;
    s.theta = s.theta + TAU * s.theta_dot;
    s.theta_dot = s.theta_dot + TAU * thetaacc;
    return s.x < -X_THRESHOLD || s.x > X_THRESHOLD || s.theta < -THETA_THRESHOLD || s.theta > THETA_THRESHOLD;
}

// the observation: the four state values each cast to float32 (tf_env.py:113,119)
MZ_HD void make_obs(const State &s, float *obs) {
    obs[0] = (float)s.x; obs[1] = (float)s.x_dot; obs[2] = (float)s.theta; obs[3] = (float)s.theta_dot;
}

// tf.argmax over two logits (concurrent_worker.py:64-65): the first maximum on a tie; action 0 when either logit is NaN is ours
MZ_HD int pick_action(float out0, float out1) { return out1 > out0 ? 1 : 0; }

// trace row: the observation after the step as 4 doubles (what the policy sees next), then the state
MZ_HD void write_trace(double *row, const State &s) {
    float obs[OBS];
    make_obs(s, obs);
    for (int i = 0; i < OBS; i++) row[i] = (double)obs[i];
    row[4] = s.x; row[5] = s.x_dot; row[6] = s.theta; row[7] = s.theta_dot;
}

// ---- the CPU side ------------------------------------------------------------------------------------------------------------------------
// the forward pass alone (tests): out[2] and the two hidden layers after their relus
inline void forward_host(const float *theta, const float *obs, float *h1, float *h2, float *out) {
    for (int j = 0; j < HID; j++) h1[j] = relu(dense_unit<OBS>(obs, theta + W1 + j, HID, theta[B1 + j]));
    for (int j = 0; j < HID; j++) h2[j] = relu(dense_unit<HID>(h1, theta + W2 + j, HID, theta[B2 + j]));
    for (int j = 0; j < ACT; j++) out[j] = dense_unit<HID>(h2, theta + W3 + j, ACT, theta[B3 + j]);
}

// one episode of one theta from reset_state(seed), or from init4 when given: until done or min(tslimit, 500) steps.  state4: the final
// state; trace (may be null): [steps][8], rows past the episode's length are not written.  Returns the steps taken (= the return).
inline int rollout_host(const float *theta, uint32_t seed, const double *init4, int tslimit, double *state4, double *trace) {
    State s = reset_state(seed);
    if (init4) { s.x = init4[0]; s.x_dot = init4[1]; s.theta = init4[2]; s.theta_dot = init4[3]; }
    const int steps = tslimit < EPISODE_STEPS ? tslimit : EPISODE_STEPS;
    float obs[OBS], h1[HID], h2[HID], out[ACT];
    int t = 0;
    while (t < steps) {
        make_obs(s, obs);
        forward_host(theta, obs, h1, h2, out);
        const bool done = step(s, pick_action(out[0], out[1]));
        if (trace) write_trace(trace + (size_t)t * TRACE_W, s);
        t++;
        if (done) break;
    }
    state4[0] = s.x; state4[1] = s.x_dot; state4[2] = s.theta; state4[3] = s.theta_dot;
    return t;
}

// open-loop: the environment alone under T given actions from init4.  rows [T][5]: the state after the step, then done (1.0 / 0.0); the
// stepping goes on past done (the caller reads where it first shows).
inline void actions_host(const int32_t *actions, int T, const double *init4, double *rows) {
    State s;
    s.x = init4[0]; s.x_dot = init4[1]; s.theta = init4[2]; s.theta_dot = init4[3];
    for (int t = 0; t < T; t++) {
        const bool done = step(s, actions[t]);
        double *row = rows + (size_t)t * 5;
        row[0] = s.x; row[1] = s.x_dot; row[2] = s.theta; row[3] = s.theta_dot; row[4] = done ? 1.0 : 0.0;
    }
}

#if defined(__HIPCC__)
// ---- the device side: whole episodes in one launch ------------------------------------------------------------------------------------------
// 16 lanes (one DPP row) per member, four members per wave, one wave per workgroup, as k_maze_rollout.  Lane j owns hidden unit j of fc1 and
// of fc2 -- its weight columns are built once from base slot and noise table and stay in registers -- and output unit j & 1; activations
// travel inside the row.  The cart's state is kept redundantly by all 16 lanes (the same operations on the same values), so a row's lanes
// decide `done` alike and leave the loop together: a row is the unit of divergence.  Every __shfl has width ROW and so reads a lane of the
// reader's own row, which is in the loop whenever the reader is; no operation reaches across rows, there is no LDS and no barrier, so rows
// of one wave that end at different steps cannot disturb each other.  Between steps nothing touches global memory unless a trace is asked for.
struct RolloutArgs {
    const float *noise, *bases; size_t base_stride;
    const int32_t *m_slot; const int64_t *m_off; const float *m_scale;
    int first, count;              // members [first, first + count)
    const uint32_t *seed;          // per member: the environment seed
    int has_init; double init4[4]; // the trace's explicit initial state (has_init != 0), else reset_state(seed)
    int tslimit;
    float *ret, *sign; int32_t *len; double *state;   // per member (null when tracing); state [member][4]
    double *trace; int32_t *trace_steps;              // [steps][8] of member `first` (count == 1) and its length, or null
};

__global__ __launch_bounds__(64) void k_cartpole_rollout(const RolloutArgs A) {
    const int lane = threadIdx.x & (ROW - 1), row = threadIdx.x / ROW;
    int mi = blockIdx.x * 4 + row;
    const bool live = mi < A.count;
    if (!live) mi = A.count - 1;           // a partial last wave: the spare rows shadow the last member and write nothing
    const int m = A.first + mi;
    const float *base = A.bases + (size_t)A.m_slot[m] * A.base_stride;
    const float *eps = A.noise + A.m_off[m];
    const float scale = A.m_scale[m];
    const int o = lane & 1;
    float w1[OBS], w2[HID], w3[HID];
#pragma unroll
    for (int k = 0; k < OBS; k++) w1[k] = perturbed(base[W1 + k * HID + lane], scale, eps[W1 + k * HID + lane]);
#pragma unroll
    for (int k = 0; k < HID; k++) w2[k] = perturbed(base[W2 + k * HID + lane], scale, eps[W2 + k * HID + lane]);
#pragma unroll
    for (int k = 0; k < HID; k++) w3[k] = perturbed(base[W3 + k * ACT + o], scale, eps[W3 + k * ACT + o]);
    const float b1 = perturbed(base[B1 + lane], scale, eps[B1 + lane]), b2 = perturbed(base[B2 + lane], scale, eps[B2 + lane]);
    const float b3 = perturbed(base[B3 + o], scale, eps[B3 + o]);

    State s = reset_state(A.seed[m]);
    if (A.has_init) { s.x = A.init4[0]; s.x_dot = A.init4[1]; s.theta = A.init4[2]; s.theta_dot = A.init4[3]; }
    const int steps = A.tslimit < EPISODE_STEPS ? A.tslimit : EPISODE_STEPS;
    float obs[OBS], in[HID];
    int t = 0;
    while (t < steps) {
        make_obs(s, obs);
        const float h1 = relu(dense_unit<OBS>(obs, w1, 1, b1));
#pragma unroll
        for (int k = 0; k < HID; k++) in[k] = __shfl(h1, k, ROW);
        const float h2 = relu(dense_unit<HID>(in, w2, 1, b2));
#pragma unroll
        for (int k = 0; k < HID; k++) in[k] = __shfl(h2, k, ROW);
        const float out = dense_unit<HID>(in, w3, 1, b3);
        const float out0 = __shfl(out, 0, ROW), out1 = __shfl(out, 1, ROW);
        const bool done = step(s, pick_action(out0, out1));
        if (A.trace && lane == 0 && live) write_trace(A.trace + (size_t)t * TRACE_W, s);
        t++;
        if (done) break;                   // the whole row at once: its 16 lanes hold the same state
    }
    if (lane == 0 && live) {
        if (A.ret) {
            A.ret[m] = (float)t;           // reward 1.0 per step taken, the terminating one included
            A.sign[m] = (float)t;          // sign(1.0) per step: the same sum
            A.len[m] = t;
            double *st = A.state + 4 * (size_t)m;
            st[0] = s.x; st[1] = s.x_dot; st[2] = s.theta; st[3] = s.theta_dot;
        }
        if (A.trace_steps) *A.trace_steps = t;
    }
}
#endif

}  // namespace cartpole
}  // namespace dne
