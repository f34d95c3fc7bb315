// dense.h -- a dense policy of any small shape on the four step environments (the model half of concurrent_worker.py:56-67: env.observation,
// model.make_net over IndexedBatchMatMul, env.step), as ONE __host__ __device__ text in the manner of its siblings.  The environment is
// step_env.h's (advance, observe, the reset_state of each kind), the arithmetic is maze.h's and pendulum.h's (perturbed, relu, tanh_f,
// pick_action): used, not copied, so a value this header produces is bit for bit the one the whole-episode kernels of the baked shapes and the
// step-at-a-time batch produce.  A plain C++ compiler can include this file (the kernel is behind __HIPCC__): tests/dense_asan_main.cpp does.
// DESIGN.md section 17.
//
// The shape: `n_hidden` (0..3) hidden layers of width 1..64 between the environment's inputs (maze 11, cart-pole 4, pendulum 3, acrobot 6) and its
// outputs (2, 2, 1, 3); one nonlinearity (tanh_f or relu) behind every hidden layer, none behind the last.  n_hidden = 0 is models/simple.py:23-27
// LinearClassifier.  The flat vector is in creation order (models/base.py:166-178): per layer w [in][out] row-major, then b [out] -- so (16, 16)
// on the maze is maze.h's own layout and on the cart-pole cartpole.h's.
// The numerics: one output unit is one fmaf chain over k ascending from +0.0f, then + b, then the nonlinearity (maze.h's dense_unit with the
// widths at run time); -ffp-contract=off on both passes; theta_p = perturbed(base[slot][p], scale, noise[off + p]).
// The action: the maze takes the two raw outputs, the cart-pole cartpole::pick_action of them, the pendulum the raw output as its torque (the
// step clips it; observations are raw, nothing is normalised here), the acrobot acrobot::pick_action of its three.
// An episode's return is the float64 sum of its rewards in step order, cast once; its sign-return the sum of np.sign of each reward, likewise.
#pragma once
#include "step_env.h"

namespace dne {
namespace dense {

using stepenv::KIND_MAZE;
using stepenv::KIND_CARTPOLE;
using stepenv::KIND_PENDULUM;
using stepenv::ENV_ACROBOT;
using stepenv::MazeCtx;

constexpr int MAX_HIDDEN = 3, MAX_WIDTH = 64, MAX_LAYERS = MAX_HIDDEN + 1, MAX_OUT = 3;
// the widest shape an environment takes: obs -> 64 -> 64 -> 64 -> out
constexpr int widest_p(int obs, int out) { return (obs + 1) * MAX_WIDTH + 2 * (MAX_WIDTH + 1) * MAX_WIDTH + (MAX_WIDTH + 1) * out; }
constexpr int max_i(int a, int b) { return a > b ? a : b; }
constexpr int MAX_P = max_i(max_i(widest_p(maze::OBS, 2), widest_p(cartpole::OBS, 2)),
                            max_i(widest_p(pendulum::OBS, 1), widest_p(acrobot::OBS, acrobot::ACT)));   // the maze's: 9218 (the acrobot's: 8963)
static_assert(MAX_P == 9218, "the maze's 11 -> 64 -> 64 -> 64 -> 2");
enum { NL_TANH = 0, NL_RELU = 1 };
enum { SHAPE_OK = 0, SHAPE_ENV, SHAPE_LAYERS, SHAPE_WIDTH, SHAPE_TAIL, SHAPE_OUT, SHAPE_NONLIN };

// dim: inputs, the hidden widths, outputs; off[l]: where layer l's w starts (its b follows at off[l] + dim[l] * dim[l + 1])
struct Shape { int env, n_hidden, nonlin, dim[MAX_LAYERS + 1], off[MAX_LAYERS], P; };

MZ_HD int env_outputs(int env) { return env == KIND_PENDULUM ? 1 : env == ENV_ACROBOT ? acrobot::ACT : 2; }

// the shape from its parts, or which part is refused (SHAPE_*).  widths holds n_widths entries: the n_hidden widths, then zeros
MZ_HD int make_shape(int env, int n_hidden, const int32_t *widths, int n_widths, int nonlin, int n_out, Shape *sh) {
    stepenv::Dims d;
    if (!stepenv::dims(env, &d)) return SHAPE_ENV;
    if (n_hidden < 0 || n_hidden > MAX_HIDDEN || n_hidden > n_widths) return SHAPE_LAYERS;
    for (int i = 0; i < n_hidden; i++) if (widths[i] < 1 || widths[i] > MAX_WIDTH) return SHAPE_WIDTH;
    for (int i = n_hidden; i < n_widths; i++) if (widths[i] != 0) return SHAPE_TAIL;
    if (n_out != env_outputs(env)) return SHAPE_OUT;
    if (nonlin != NL_TANH && nonlin != NL_RELU) return SHAPE_NONLIN;
    sh->env = env; sh->n_hidden = n_hidden; sh->nonlin = nonlin;
    for (int i = 0; i <= MAX_LAYERS; i++) sh->dim[i] = 0;
    for (int i = 0; i < MAX_LAYERS; i++) sh->off[i] = 0;
    sh->dim[0] = d.obs;
    for (int i = 0; i < n_hidden; i++) sh->dim[1 + i] = widths[i];
    sh->dim[1 + n_hidden] = n_out;
    int o = 0;
    for (int l = 0; l <= n_hidden; l++) { sh->off[l] = o; o += (sh->dim[l] + 1) * sh->dim[l + 1]; }
    sh->P = o;
    return SHAPE_OK;
}

// ---- the forward pass ------------------------------------------------------------------------------------------------------------------------
// one output unit: w points at the unit's column (w[k * n_out] is input k's weight)
MZ_HD float unit(const float *in, const float *w, int n_in, int n_out, float b) {
    float acc = 0.0f;
#if defined(__HIPCC__)
#pragma unroll 8                       // (the device reads in[] and w[] from LDS: eight reads in flight ahead of the chain, whose order stays k ascending)
#endif
    for (int k = 0; k < n_in; k++) acc = fmaf(in[k], w[k * n_out], acc);
    return acc + b;
}
MZ_HD float activate(int nonlin, float v) { return nonlin == NL_TANH ? pendulum::tanh_f(v) : maze::relu(v); }

// unit j of layer l from the layer's inputs (theta: the member's flat vector, wherever it lives)
MZ_HD float layer_unit(const Shape &sh, const float *theta, int l, const float *in, int j) {
    const int n_in = sh.dim[l], n_out = sh.dim[l + 1];
    const float *w = theta + sh.off[l];
    const float v = unit(in, w + j, n_in, n_out, w[n_in * n_out + j]);
    return l < sh.n_hidden ? activate(sh.nonlin, v) : v;
}

// the action as the environment's step takes it: maze float [2], cart-pole int32 [1], pendulum float [1], acrobot int32 [1]
MZ_HD void write_action(int env, const float *out, void *action) {
    if (env == KIND_MAZE) { ((float *)action)[0] = out[0]; ((float *)action)[1] = out[1]; }
    else if (env == KIND_CARTPOLE) ((int32_t *)action)[0] = cartpole::pick_action(out[0], out[1]);
    else if (env == ENV_ACROBOT) ((int32_t *)action)[0] = acrobot::pick_action(out);
    else ((float *)action)[0] = out[0];
}

// ---- the four environments under one spelling - ------------------------------------------------------------------------------------------------
template <int ENV> struct EnvOf;
template <> struct EnvOf<KIND_MAZE> { typedef maze::State State; static constexpr int OBS = maze::OBS, S = 7, OUT = 2, OWN = maze::EPISODE_STEPS; };
template <> struct EnvOf<KIND_CARTPOLE> { typedef cartpole::State State; static constexpr int OBS = cartpole::OBS, S = 4, OUT = 2, OWN = cartpole::EPISODE_STEPS; };
template <> struct EnvOf<KIND_PENDULUM> { typedef pendulum::State State; static constexpr int OBS = pendulum::OBS, S = 2, OUT = 1, OWN = pendulum::EPISODE_STEPS; };
template <> struct EnvOf<ENV_ACROBOT> { typedef acrobot::State State; static constexpr int OBS = acrobot::OBS, S = 4, OUT = acrobot::ACT, OWN = acrobot::EPISODE_STEPS; };

MZ_HD void reset(maze::State &s, uint32_t, const MazeCtx &c) { s = maze::reset_state(c.hdr); }
MZ_HD void reset(cartpole::State &s, uint32_t seed, const MazeCtx &) { s = cartpole::reset_state(seed); }
MZ_HD void reset(pendulum::State &s, uint32_t seed, const MazeCtx &) { s = pendulum::reset_state(seed); }
MZ_HD void reset(acrobot::State &s, uint32_t seed, const MazeCtx &) { s = acrobot::reset_state(seed); }

template <class R> MZ_HD void look(const maze::State &s, const MazeCtx &c, const maze::SinCosF *dir, const R &r, float *obs) { stepenv::observe(s, c, dir, r, obs); }
template <class R> MZ_HD void look(const cartpole::State &s, const MazeCtx &, const maze::SinCosF *, const R &, float *obs) { stepenv::observe(s, obs); }
template <class R> MZ_HD void look(const pendulum::State &s, const MazeCtx &, const maze::SinCosF *, const R &, float *obs) { stepenv::observe(s, obs); }
template <class R> MZ_HD void look(const acrobot::State &s, const MazeCtx &, const maze::SinCosF *, const R &, float *obs) { stepenv::observe(s, obs); }

// outputs -> action -> stepenv::advance
template <class R>
MZ_HD bool act_advance(maze::State &s, int &steps, int limit, int &done, const float *out, const MazeCtx &c, const maze::SinCosF *dir, const R &r,
                       float &reward, float *obs) {
    return stepenv::advance(s, steps, limit, done, out, c, dir, r, reward, obs);
}
template <class R>
MZ_HD bool act_advance(cartpole::State &s, int &steps, int limit, int &done, const float *out, const MazeCtx &, const maze::SinCosF *, const R &,
                       float &reward, float *obs) {
    return stepenv::advance(s, steps, limit, done, cartpole::pick_action(out[0], out[1]), reward, obs);
}
template <class R>
MZ_HD bool act_advance(pendulum::State &s, int &steps, int limit, int &done, const float *out, const MazeCtx &, const maze::SinCosF *, const R &,
                       float &reward, float *obs) {
    return stepenv::advance(s, steps, limit, done, out[0], reward, obs);
}
template <class R>
MZ_HD bool act_advance(acrobot::State &s, int &steps, int limit, int &done, const float *out, const MazeCtx &, const maze::SinCosF *, const R &,
                       float &reward, float *obs) {
    return stepenv::advance(s, steps, limit, done, acrobot::pick_action(out), reward, obs);
}

// ---- the CPU twins ----------------------------------------------------------------------------------------------------------------------------
// layers (may be null): the hidden layers' activations behind their nonlinearity, concatenated (dim[1] + .. + dim[n_hidden] floats); out [dim[last]]
inline void forward_host(const Shape &sh, const float *theta, const float *obs, float *layers, float *out) {
    float a[2][MAX_WIDTH];
    const float *in = obs;
    for (int l = 0; l <= sh.n_hidden; l++) {
        float *o = l < sh.n_hidden ? a[l & 1] : out;
        for (int j = 0; j < sh.dim[l + 1]; j++) o[j] = layer_unit(sh, theta, l, in, j);
        if (l < sh.n_hidden && layers) { for (int j = 0; j < sh.dim[l + 1]; j++) layers[j] = o[j]; layers += sh.dim[l + 1]; }
        in = o;
    }
}

// one episode of one theta from the reset (init: the state record instead), to the environment's own limit or tslimit
template <int ENV>
inline void rollout_one(const Shape &sh, const float *theta, uint32_t seed, const double *init, const MazeCtx &c, int tslimit, float *ret, float *sign,
                        int32_t *len, double *state) {
    typedef EnvOf<ENV> E;
    typename E::State s;
    reset(s, seed, c);
    if (init) stepenv::unpack(init, s);
    maze::SinCosF dir[6] = {};
    if (ENV == KIND_MAZE) maze::rangefinder_dirs(dir);
    float obs[E::OBS], out[MAX_OUT] = {};
    look(s, c, dir, stepenv::Solo(), obs);
    int steps = 0, done = 0;
    const int limit = stepenv::step_limit(tslimit, E::OWN);
    double r = 0.0, sg = 0.0;
    while (!done) {
        forward_host(sh, theta, obs, nullptr, out);
        float rew;
        act_advance(s, steps, limit, done, out, c, dir, stepenv::Solo(), rew, obs);
        r += (double)rew;
        sg += pendulum::sign_d(rew);
    }
    *ret = (float)r;
    if (sign) *sign = (float)sg;
    *len = steps;
    stepenv::pack(s, state);
}

inline void rollout_host(const Shape &sh, const float *theta, int n, const uint32_t *seeds, const double *init, const MazeCtx &c, int tslimit, float *ret,
                         float *sign, int32_t *len, double *state) {
    for (int i = 0; i < n; i++) {
        const float *th = theta + (size_t)i * sh.P;
        const uint32_t seed = seeds ? seeds[i] : 0;
        float *sg = sign ? sign + i : nullptr;
        if (sh.env == KIND_MAZE) rollout_one<KIND_MAZE>(sh, th, seed, init ? init + (size_t)i * 7 : nullptr, c, tslimit, ret + i, sg, len + i, state + (size_t)i * 7);
        else if (sh.env == KIND_CARTPOLE) rollout_one<KIND_CARTPOLE>(sh, th, seed, init ? init + (size_t)i * 4 : nullptr, c, tslimit, ret + i, sg, len + i, state + (size_t)i * 4);
        else if (sh.env == KIND_PENDULUM) rollout_one<KIND_PENDULUM>(sh, th, seed, init ? init + (size_t)i * 2 : nullptr, c, tslimit, ret + i, sg, len + i, state + (size_t)i * 2);
        else rollout_one<ENV_ACROBOT>(sh, th, seed, init ? init + (size_t)i * 4 : nullptr, c, tslimit, ret + i, sg, len + i, state + (size_t)i * 4);
    }
}

#if defined(__HIPCC__)
// ---- the device side: one kernel, three uses -----------------------------------------------------------------------------------------------------
// One 64-lane workgroup (one wave) per item = (environment, member).  The member's perturbed theta is staged ONCE into LDS in its flat layout,
// read from base and noise table coalesced (lane p, p + 64, ...).  A layer is one lane per unit: lane j reads w[k * out + j] -- consecutive
// floats over the lanes, so whatever the width (5, 33, 64) the 64 reads of one k fall into distinct banks -- and in[k] as a broadcast; the
// activations alternate between two 64-float rows of LDS.  The environment's state is kept redundantly by every lane (the same operations on
// the same values), so `done` is the workgroup's own and every barrier below is met by all 64 lanes or by none.  The maze's walls are dealt
// over rows of 16 lanes (Row16), the four rows computing the same environment: a minimum and an "any" are exact over any partition.
// Between rounds nothing touches global memory; lane 0 writes at the end, and writes the batch back only if a step was taken (an environment
// that was done keeps every bit).
//   episode != 0: item i is member i; the environment is reset from seed[i] (the maze: its header) under limit = step_limit(max_steps, own),
//                 runs until done and leaves ret / sign / steps_out (the length) / state_out; the batch B is not touched
//   episode == 0: item i is environment idx[i] of the batch under member mem[i]; max_steps >= 1 rounds of forward -> action -> advance from the
//                 batch's current state, which is written back; ret (the float64 sum of this call's rewards, cast once), steps_out (the steps
//                 this call took) and done_out per item, each unless null.  max_steps == 0: the forward pass alone on the batch's current
//                 observation: out [n][OUT] and act (the action as write_action forms it), each unless null; nothing else is written
struct RunArgs {
    const float *noise, *bases; size_t base_stride;
    const int32_t *m_slot; const int64_t *m_off; const float *m_scale;
    Shape shape;
    const int32_t *idx, *mem;
    stepenv::Batch B; MazeCtx C;
    const uint32_t *seed;
    int episode, max_steps;
    float *ret, *sign; int32_t *steps_out; uint8_t *done_out; double *state_out;
    float *out; void *act;
};

template <int ENV>
__global__ __launch_bounds__(64) void k_dense_run(const RunArgs A) {
    typedef EnvOf<ENV> E;
    extern __shared__ float s_theta[];
    __shared__ float s_act[2][MAX_WIDTH];
    __shared__ float s_walls[ENV == KIND_MAZE ? maze::MAX_WALLS * 4 : 1];
    const int lane = threadIdx.x, item = blockIdx.x;
    const Shape &sh = A.shape;
    const int m = A.episode ? item : A.mem[item];
    const float *base = A.bases + (size_t)A.m_slot[m] * A.base_stride;
    const float *eps = A.noise + A.m_off[m];
    const float scale = A.m_scale[m];
    for (int p = lane; p < sh.P; p += 64) s_theta[p] = maze::perturbed(base[p], scale, eps[p]);
    MazeCtx c = A.C;
    if (ENV == KIND_MAZE) {
        for (int i = lane; i < c.nw * 4; i += 64) s_walls[i] = A.C.walls[i];
        c.walls = s_walls;
    }
    __syncthreads();
    const stepenv::Row16 row{lane & (maze::ROW - 1)};
    maze::SinCosF dir[6];
    if (ENV == KIND_MAZE) maze::rangefinder_dirs(dir);

    typename E::State s;
    int steps = 0, done = 0, limit;
    float obs[E::OBS];
    const int e = A.episode ? 0 : A.idx[item];
    if (A.episode) {
        reset(s, ENV == KIND_MAZE ? 0u : A.seed[item], c);
        limit = stepenv::step_limit(A.max_steps, E::OWN);
        look(s, c, dir, row, obs);
    } else {
        stepenv::unpack(A.B.state + (size_t)e * E::S, s);
        steps = A.B.steps[e]; done = A.B.done[e]; limit = A.B.limit[e];
#pragma unroll
        for (int i = 0; i < E::OBS; i++) obs[i] = A.B.obs[(size_t)e * E::OBS + i];
    }

    // the forward pass on obs: the outputs end in s_act[(n_hidden + 1) & 1][0 .. OUT); every lane leaves with them in o[]
    float o[MAX_OUT] = {};
    auto forward = [&]() {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < E::OBS; i++) s_act[0][i] = obs[i];
        }
        __syncthreads();
        for (int l = 0; l <= sh.n_hidden; l++) {
            if (lane < sh.dim[l + 1]) s_act[(l + 1) & 1][lane] = layer_unit(sh, s_theta, l, s_act[l & 1], lane);
            __syncthreads();
        }
        const float *last = s_act[(sh.n_hidden + 1) & 1];
#pragma unroll
        for (int i = 0; i < E::OUT; i++) o[i] = last[i];
        __syncthreads();               // read by every lane before the next pass writes the rows again
    };

    if (!A.episode && A.max_steps == 0) {
        forward();
        if (A.out && lane < E::OUT) A.out[(size_t)item * E::OUT + lane] = o[lane < MAX_OUT ? lane : 0];
        if (A.act && lane == 0) write_action(ENV, o, (char *)A.act + (size_t)item * (ENV == KIND_MAZE ? 2 : 1) * sizeof(float));
        return;
    }

    const int steps0 = steps, rounds = A.episode ? limit : A.max_steps;
    double ret = 0.0, sg = 0.0;
    for (int t = 0; t < rounds && !done; t++) {
        forward();
        float rew;
        act_advance(s, steps, limit, done, o, c, dir, row, rew, obs);
        ret += (double)rew;
        sg += pendulum::sign_d(rew);
    }
    if (lane != 0) return;
    if (A.episode) stepenv::pack(s, A.state_out + (size_t)item * E::S);
    else if (steps != steps0) {
        stepenv::pack(s, A.B.state + (size_t)e * E::S);
        A.B.steps[e] = steps; A.B.done[e] = (uint8_t)done;
#pragma unroll
        for (int i = 0; i < E::OBS; i++) A.B.obs[(size_t)e * E::OBS + i] = obs[i];
    }
    if (A.ret) A.ret[item] = (float)ret;
    if (A.sign) A.sign[item] = (float)sg;
    if (A.steps_out) A.steps_out[item] = A.episode ? steps : steps - steps0;
    if (A.done_out) A.done_out[item] = (uint8_t)done;
}
#endif

}  // namespace dense
}  // namespace dne
