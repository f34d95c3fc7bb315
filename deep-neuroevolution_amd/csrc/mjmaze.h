// mjmaze.h -- es_distributed's MujocoPolicy (pendulum.h: observations normalised by a running mean and deviation and clipped to +-5, two dense
// layers of one width under tanh or relu, a continuous or binned action, Gaussian action noise) on the deceptive hard maze of maze.h, whose
// behaviour characterisation is the navigator's final (x, y): the pair the reference's humanoid_nses / humanoid_nsres experiments need (their
// novelty vector is the final (x_pos, y_pos), policies.py:292-299).  ONE __host__ __device__ text in the manner of pendulum.h: the step, the
// action and the forward pass below compile for the CPU (dne_mjmaze_rollout_host, the feature's oracle) and for gfx950 (k_mjmaze_rollout: whole
// episodes in one launch), and the two agree bit for bit.  DESIGN.md section 16 holds the contract.
//   * The environment is maze.h's, function by function, strung together as maze::rollout_host does: reset_state, then per step
//     interpret_outputs, propose_move, collide_partial, commit_move, sense_partial, radar_bits, make_obs; 400 steps, never done early; the
//     reward is 0 until step 400 and final_reward there.  No seed: every member starts from the header's start point.
//   * The policy is pendulum.h's, function by function: normalise over all 11 observations (the constant bias input included), dense4 in four
//     fmaf chains, nonlin, and per action dimension pick_action's strict > scan from -inf.  The action space is Box(-0.5, 0.5, (2,)): the
//     values the maze clamps its two raw outputs to.
//   * Every reduction over walls is a minimum or an "any" (maze.h): dealing the walls over the lanes of a wave cannot change a bit.
// A plain C++ compiler can include this file (the kernel is behind __HIPCC__): tests/mjmaze_asan_main.cpp does.
#pragma once
#include "maze.h"
#include "pendulum.h"

namespace dne {
namespace mjmaze {

using maze::Header;
using maze::SinCosF;
using maze::State;
using maze::perturbed;
using pendulum::AC_CONTINUOUS;
using pendulum::AC_UNIFORM;
using pendulum::NL_RELU;
using pendulum::NL_TANH;
using pendulum::dense4;
using pendulum::hidden_ok;
using pendulum::nonlin;
using pendulum::normalise;

constexpr int OBS = maze::OBS, ADIM = maze::ACT, MAX_OUT = pendulum::MAX_OUT, MAX_BINS = MAX_OUT / ADIM, EPISODE_STEPS = maze::EPISODE_STEPS;
constexpr int AC_NOISE = ADIM * EPISODE_STEPS;   // action-noise values one episode reads: table[ac_off + 2 t + i]
constexpr int TRACE_W = 20;                      // the 11 observations acted on, the net's 2 actions, the 2 applied, then x, y, heading, speed, ang_vel after the step
constexpr float AC_LOW = -0.5f, AC_RANGE = 1.0f; // the action space: Box(-0.5, 0.5)

// flat order = TF's creation order (policies.py:155-200 over tf_util.dense): l0/w [11][H], l0/b, l1/w [H][H], l1/b, out/w [H][O], out/b
struct Offsets { int w1, b1, w2, b2, w3, b3, P; };
MZ_HD Offsets offsets(int H, int O) {
    Offsets o;
    o.w1 = 0; o.b1 = OBS * H; o.w2 = o.b1 + H; o.b2 = o.w2 + H * H; o.w3 = o.b2 + H; o.b3 = o.w3 + H * O; o.P = o.b3 + O;
    return o;
}
// continuous: 2 outputs; uniform over B bins a dimension, 2 <= B <= 8: 2 B outputs, output i B + b is bin b of dimension i (policies.py:116-119)
inline bool shape_ok(int H, int O, int mode, int nl) {
    return hidden_ok(H) && (nl == NL_TANH || nl == NL_RELU) &&
           (mode == AC_CONTINUOUS ? O == ADIM : (mode == AC_UNIFORM && O % ADIM == 0 && O / ADIM >= 2 && O / ADIM <= MAX_BINS));
}

// what one episode reads beside theta (the same values on both sides)
struct Options {
    int n_out, ac_mode;
    float mean[OBS], std[OBS];
    float ac_noise_std;
};

// ---- the environment ---------------------------------------------------------------------------------------------------------------------
// how a caller that deals the walls over lanes brings its lanes' partial results together; alone, there is nothing to do
struct Alone {
    MZ_HD float min(float v) const { return v; }
    MZ_HD bool any(bool b) const { return b; }
};

// maze::observe_host over walls w0, w0 + stride, ...: the six range minima reduced by R, then the radar and the observation
template <typename R>
MZ_HD void observe(const State &s, const Header &m, const SinCosF *dir, const float *walls, int w0, int stride, int nw, const R &red, float *obs) {
    float range[6], radar[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; i++) range[i] = maze::RF_RANGE;
    maze::sense_partial(s, maze::sincos_f(maze::to_rad_f(s.heading)), dir, walls, w0, stride, nw, range);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; i++) range[i] = red.min(range[i]);
    maze::radar_bits(s, m, radar);
    maze::make_obs(range, radar, obs);
}

// maze::step_host likewise: the two sensor passes of a step, collision then rangefinders
template <typename R>
MZ_HD void env_step(State &s, const Header &m, const SinCosF *dir, const float *walls, int w0, int stride, int nw, const R &red, float a0, float a1,
                    float *obs) {
    float nx, ny;
    maze::interpret_outputs(s, a0, a1);
    maze::propose_move(s, &nx, &ny);
    maze::commit_move(s, m, nx, ny, red.any(maze::collide_partial(nx, ny, walls, w0, stride, nw)));
    observe(s, m, dir, walls, w0, stride, nw, red, obs);
}

MZ_HD float episode_return(const State &s, const Header &m, int steps) { return 0.0f + (steps == EPISODE_STEPS ? maze::final_reward(s, m) : 0.0f); }
MZ_HD float sign_of(float r) { return (float)((r > 0.0f) - (r < 0.0f)); }   // as k_maze_rollout forms it

// ---- the action --------------------------------------------------------------------------------------------------------------------------
// dimension i of the action from the n_out output values.  continuous: out[i].  uniform over B = n_out / 2 bins: the first maximum of
// out[i B .. i B + B) under pendulum::pick_action's strict > scan from -inf (a NaN never wins; all NaN gives bin 0), then
// 1 / (B - 1) * aidx * (high - low) + low with high - low = 1 and low = -0.5
MZ_HD float pick_dim(const float *out, int i, int n_out, int mode) {
    if (mode == AC_CONTINUOUS) return out[i];
    const int B = n_out / ADIM;
    int aidx = 0;
    float best = -INFINITY;
    for (int b = 0; b < B; b++)
        if (out[i * B + b] > best) { best = out[i * B + b]; aidx = b; }
    return ((1.0f / ((float)B - 1.0f)) * (float)aidx) * AC_RANGE + AC_LOW;
}

MZ_HD void trace_head(float *row, const float *obs, const float *a_net, const float *a) {
    for (int i = 0; i < OBS; i++) row[i] = obs[i];
    row[11] = a_net[0]; row[12] = a_net[1]; row[13] = a[0]; row[14] = a[1];
}
MZ_HD void trace_tail(float *row, const State &s) { row[15] = s.x; row[16] = s.y; row[17] = s.heading; row[18] = s.speed; row[19] = s.ang_vel; }

// ---- the CPU side ------------------------------------------------------------------------------------------------------------------------
// the forward pass alone on one raw observation: x [11] the normalised input, h1 [H], h2 [H], out [n_out], act [2] the net's action
template <int H, bool TANH>
inline void forward_host_t(const float *theta, const Options &o, const float *ob, float *x, float *h1, float *h2, float *out, float *act) {
    const Offsets L = offsets(H, o.n_out);
    for (int i = 0; i < OBS; i++) x[i] = normalise(ob[i], o.mean[i], o.std[i]);
    for (int j = 0; j < H; j++) h1[j] = nonlin<TANH>(dense4<OBS>(x, theta + L.w1 + j, H, theta[L.b1 + j]));
    for (int j = 0; j < H; j++) h2[j] = nonlin<TANH>(dense4<H>(h1, theta + L.w2 + j, H, theta[L.b2 + j]));
    for (int j = 0; j < o.n_out; j++) out[j] = dense4<H>(h2, theta + L.w3 + j, o.n_out, theta[L.b3 + j]);
    for (int i = 0; i < ADIM; i++) act[i] = pick_dim(out, i, o.n_out, o.ac_mode);
}

// what one episode leaves
struct Episode { float ret, sign; int len; State s; double ob_sum[OBS], ob_sumsq[OBS]; };

// one episode of one theta from the header's start point: min(tslimit, 400) steps, never done early.  ac_eps (may be null): the 800 values of
// the noise table the action noise reads; stat: accumulate the observations acted on.  trace (may be null): [steps][20].
template <int H, bool TANH>
inline Episode rollout_host_t(const float *theta, const Options &o, const Header &m, const float *walls, int nw, int tslimit, const float *ac_eps,
                              bool stat, float *trace) {
    Episode e{};
    SinCosF dir[6];
    maze::rangefinder_dirs(dir);
    State s = maze::reset_state(m);
    const int steps = tslimit < EPISODE_STEPS ? tslimit : EPISODE_STEPS;
    float obs[OBS], x[OBS], h1[H], h2[H], out[MAX_OUT], a_net[ADIM], a[ADIM];
    const Alone alone;
    observe(s, m, dir, walls, 0, 1, nw, alone, obs);
    for (int t = 0; t < steps; t++) {
        forward_host_t<H, TANH>(theta, o, obs, x, h1, h2, out, a_net);
        for (int i = 0; i < ADIM; i++) a[i] = ac_eps ? perturbed(a_net[i], o.ac_noise_std, ac_eps[ADIM * t + i]) : a_net[i];
        if (stat)
            for (int i = 0; i < OBS; i++) { const double d = (double)obs[i]; e.ob_sum[i] += d; e.ob_sumsq[i] += d * d; }
        if (trace) trace_head(trace + (size_t)t * TRACE_W, obs, a_net, a);
        env_step(s, m, dir, walls, 0, 1, nw, alone, a[0], a[1], obs);
        if (trace) trace_tail(trace + (size_t)t * TRACE_W, s);
    }
    e.ret = episode_return(s, m, steps); e.sign = sign_of(e.ret); e.len = steps; e.s = s;
    return e;
}

// the two above for a run-time (H, nonlinearity); the shape must pass shape_ok
inline void forward_host(int H, int nl, const float *theta, const Options &o, const float *ob, float *x, float *h1, float *h2, float *out, float *act) {
    const bool th = nl == NL_TANH;
    switch (H) {
    case 64: th ? forward_host_t<64, true>(theta, o, ob, x, h1, h2, out, act) : forward_host_t<64, false>(theta, o, ob, x, h1, h2, out, act); break;
    case 128: th ? forward_host_t<128, true>(theta, o, ob, x, h1, h2, out, act) : forward_host_t<128, false>(theta, o, ob, x, h1, h2, out, act); break;
    default: th ? forward_host_t<256, true>(theta, o, ob, x, h1, h2, out, act) : forward_host_t<256, false>(theta, o, ob, x, h1, h2, out, act);
    }
}
inline Episode rollout_host(int H, int nl, const float *theta, const Options &o, const Header &m, const float *walls, int nw, int tslimit,
                            const float *ac_eps, bool stat, float *trace) {
    const bool th = nl == NL_TANH;
    switch (H) {
    case 64: return th ? rollout_host_t<64, true>(theta, o, m, walls, nw, tslimit, ac_eps, stat, trace)
                       : rollout_host_t<64, false>(theta, o, m, walls, nw, tslimit, ac_eps, stat, trace);
    case 128: return th ? rollout_host_t<128, true>(theta, o, m, walls, nw, tslimit, ac_eps, stat, trace)
                        : rollout_host_t<128, false>(theta, o, m, walls, nw, tslimit, ac_eps, stat, trace);
    default: return th ? rollout_host_t<256, true>(theta, o, m, walls, nw, tslimit, ac_eps, stat, trace)
                       : rollout_host_t<256, false>(theta, o, m, walls, nw, tslimit, ac_eps, stat, trace);
    }
}

#if defined(__HIPCC__)
// ---- the device side: whole episodes in one launch ------------------------------------------------------------------------------------------
// One workgroup of H threads (1, 2 or 4 waves) per member.  The policy is k_pendulum_rollout's scheme: thread j owns hidden unit j of both
// layers; its l1/w column (H values) stays in registers, at H = 256 the upper half in accumulator registers (pendulum::park / fetch); out/w
// is transposed in LDS; h1 and h2 are LDS broadcasts; a dense layer goes in pieces of 16 inputs (pendulum::dense4_lds).  New here:
//   * l0/w is ELEVEN values a thread, not three.  They live in LDS, s_w1[k][j]: thread j reads only its own column, at consecutive addresses
//     across the wave (no bank conflict), so the register file holds what it held on the pendulum.
//   * the maze step.  The walls are staged in LDS once.  EVERY wave keeps the navigator's state redundantly (the same operations on the same
//     values, as k_pendulum_rollout keeps its state in every thread) and deals the walls over its own 64 lanes: sense_partial and
//     collide_partial at lane stride 64, the six range minima and the collision "any" reduced across that wave (exact in any order, maze.h).
//     Nothing is published between waves, so the step adds no barrier: three a step, as on the pendulum.
// Invariants:
//   * every barrier is reached by the whole workgroup: the step loop runs min(tslimit, 400) times for every thread, no thread leaves it, and no
//     barrier or cross-lane operation stands under a condition that differs inside a wave;
//   * every LDS buffer's next write is separated by a barrier from its last read: s_h1 is written before barrier 1 and last read before
//     barrier 2; s_h2 is written before barrier 2 and last read before barrier 3; s_out is written before barrier 3 and read behind it, its
//     next write lies behind barriers 1 and 2 of the next step; s_w1, s_ow, s_ob and s_walls are written once, ahead of the first barrier;
//   * every loop has a compile-time bound or one the host checked: steps <= 400, walls <= MAX_WALLS (dne_maze_set_walls), bins <= 8 (dne_create);
//   * between steps nothing touches global memory but the two action-noise values (ac_off + 800 lies inside the table: checked when the
//     options are set and again at the launch) and the trace when asked for.
struct RolloutArgs {
    const float *noise, *bases; size_t base_stride;
    const int32_t *m_slot; const int64_t *m_off; const float *m_scale;
    int first, count;              // members [first, first + count): one workgroup each
    Header hdr; const float *walls; int nw; int tslimit;
    Options opt;
    const int64_t *ac_off;         // per member: where its 800 action-noise values start in the noise table, < 0 for none; null: nobody has any
    const uint8_t *stat_flag;      // per member: accumulate the observations acted on; null: nobody does
    float *ret, *sign; int32_t *len; float *xy;       // per member (null when tracing); xy [member][2]
    double *ob_sum, *ob_sumsq; int32_t *ob_count;     // per member [11], [11], 1 (zero for an unflagged member)
    float *trace; int32_t *trace_steps;               // [steps][20] of member `first` (count == 1) and its length, or null
};

// a wave's 64 lanes brought together: butterfly minima (every lane ends with the minimum), and the wave-wide vote
struct WaveReduce {
    __device__ __forceinline__ float min(float v) const {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const float o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
        return v;
    }
    __device__ __forceinline__ bool any(bool b) const { return __any(b ? 1 : 0) != 0; }
};

template <int H, bool TANH>
__global__ __launch_bounds__(H) void k_mjmaze_rollout(const RolloutArgs A) {
    using pendulum::CH;
    using pendulum::OW_ROW_PAD;
    using pendulum::dense4_lds;
    using pendulum::fetch;
    using pendulum::park;
    __shared__ __attribute__((aligned(16))) float s_h1[H], s_h2[H];
    __shared__ __attribute__((aligned(16))) float s_ow[MAX_OUT * (H + OW_ROW_PAD)];   // out/w transposed: row o holds column o, 16 bytes of padding
    __shared__ float s_w1[OBS * H];                                                   // l0/w as it lies in theta: [k][j]
    __shared__ float s_ob[MAX_OUT], s_out[MAX_OUT];
    __shared__ float s_walls[maze::MAX_WALLS * 4];
    const int j = threadIdx.x, lane = j & 63;
    const int m = A.first + blockIdx.x;    // the grid is `count` workgroups
    const int O = A.opt.n_out;
    const Offsets L = offsets(H, O);
    const float *base = A.bases + (size_t)A.m_slot[m] * A.base_stride;
    const float *eps = A.noise + A.m_off[m];
    const float scale = A.m_scale[m];
    constexpr int NV = H > 128 ? 128 : H, NA = H - NV;   // l1/w values in vector / in accumulator registers
    float w2[NV], wa[NA > 0 ? NA : 1];
    for (int i = j; i < A.nw * 4; i += H) s_walls[i] = A.walls[i];
#pragma unroll
    for (int k = 0; k < OBS; k++) s_w1[k * H + j] = perturbed(base[L.w1 + k * H + j], scale, eps[L.w1 + k * H + j]);
#pragma unroll
    for (int k = 0; k < H; k++) {
        float wk = perturbed(base[L.w2 + k * H + j], scale, eps[L.w2 + k * H + j]);
        if (k < NV) { asm volatile("" : "+v"(wk)); w2[k] = wk; } else park(wa[k - NV], wk);   // formed here, not where it is first used
        if (k % CH == CH - 1) __builtin_amdgcn_sched_barrier(0);   // CH columns' loads in flight, not H
    }
    const float b1 = perturbed(base[L.b1 + j], scale, eps[L.b1 + j]), b2 = perturbed(base[L.b2 + j], scale, eps[L.b2 + j]);
    for (int i = j; i < H * O; i += H) s_ow[(i % O) * (H + OW_ROW_PAD) + i / O] = perturbed(base[L.w3 + i], scale, eps[L.w3 + i]);   // out/w [H][O]
    if (j < O) s_ob[j] = perturbed(base[L.b3 + j], scale, eps[L.b3 + j]);

    const int steps = A.tslimit < EPISODE_STEPS ? A.tslimit : EPISODE_STEPS;
    const int64_t ac_off = A.ac_off ? A.ac_off[m] : -1;
    const bool stat = A.stat_flag && A.stat_flag[m];
    double ob_sum = 0.0, ob_sumsq = 0.0;   // thread j < 11 accumulates observation j
    const WaveReduce wave;
    SinCosF dir[6];
    maze::rangefinder_dirs(dir);
    State s = maze::reset_state(A.hdr);
    float obs[OBS], x[OBS], a_net[ADIM], a[ADIM];
    __syncthreads();                       // s_walls, s_w1, s_ow and s_ob are complete
    observe(s, A.hdr, dir, s_walls, lane, 64, A.nw, wave, obs);
    for (int t = 0; t < steps; t++) {
#pragma unroll
        for (int i = 0; i < OBS; i++) x[i] = normalise(obs[i], A.opt.mean[i], A.opt.std[i]);
        s_h1[j] = nonlin<TANH>(dense4<OBS>(x, s_w1 + j, H, b1));
        __syncthreads();
        s_h2[j] = nonlin<TANH>(dense4_lds<H>(s_h1, [&](int q) {
            return 4 * q < NV ? make_float4(w2[(4 * q) % NV], w2[(4 * q + 1) % NV], w2[(4 * q + 2) % NV], w2[(4 * q + 3) % NV])
                              : make_float4(fetch(wa[(4 * q - NV) % (NA + 1)]), fetch(wa[(4 * q + 1 - NV) % (NA + 1)]), fetch(wa[(4 * q + 2 - NV) % (NA + 1)]),
                                            fetch(wa[(4 * q + 3 - NV) % (NA + 1)]));
        }, b2));
        __syncthreads();
        if (j < O) s_out[j] = dense4_lds<H>(s_h2, [&](int q) { return reinterpret_cast<const float4 *>(s_ow + j * (H + OW_ROW_PAD))[q]; }, s_ob[j]);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ADIM; i++) {   // every thread, from LDS: the same scan on the same values
            a_net[i] = pick_dim(s_out, i, O, A.opt.ac_mode);
            a[i] = ac_off >= 0 ? perturbed(a_net[i], A.opt.ac_noise_std, A.noise[ac_off + ADIM * t + i]) : a_net[i];
        }
        if (stat) {
            float mine = obs[0];
#pragma unroll
            for (int i = 1; i < OBS; i++) mine = j == i ? obs[i] : mine;
            const double d = (double)mine;
            ob_sum += d; ob_sumsq += d * d;
        }
        if (A.trace && j == 0) trace_head(A.trace + (size_t)t * TRACE_W, obs, a_net, a);
        env_step(s, A.hdr, dir, s_walls, lane, 64, A.nw, wave, a[0], a[1], obs);
        if (A.trace && j == 0) trace_tail(A.trace + (size_t)t * TRACE_W, s);
    }
    if (A.ret) {
        if (j == 0) {
            const float r = episode_return(s, A.hdr, steps);
            A.ret[m] = r; A.sign[m] = sign_of(r); A.len[m] = steps;
            A.xy[2 * (size_t)m] = s.x; A.xy[2 * (size_t)m + 1] = s.y;
            A.ob_count[m] = stat ? steps : 0;
        }
        if (j < OBS) { A.ob_sum[OBS * (size_t)m + j] = ob_sum; A.ob_sumsq[OBS * (size_t)m + j] = ob_sumsq; }
    }
    if (j == 0 && A.trace_steps) *A.trace_steps = steps;
}
#endif

}  // namespace mjmaze
}  // namespace dne
