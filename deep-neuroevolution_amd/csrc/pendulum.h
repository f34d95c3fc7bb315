// pendulum.h -- es_distributed's MujocoPolicy (policies.py:122-217: observations normalised by a running mean and deviation and clipped to +-5,
// `hidden_dims` dense layers under tanh or relu, a continuous or binned action, Gaussian action noise) on the classic torque-limited pendulum
// swing-up, as ONE __host__ __device__ text in the manner of cartpole.h: the reset, the step, tanh_f and the forward pass below compile for the
// CPU (dne_pendulum_rollout_host, the feature's oracle) and for gfx950 (k_pendulum_rollout: whole episodes in one launch), and the two agree
// bit for bit.  DESIGN.md section 14 holds the contract.
//   * The environment is the pendulum restated from its published equations in the form and with the constants of gym's
//     classic_control/pendulum.py (g 10, m 1, l 1, dt 0.05, speed 8, torque 2, the Pendulum-v0 registration's 200 steps) -- not recorded from gym.
//   * Every operation of the step is an IEEE double operation in the association written here; sine and cosine are maze.h's sincos_d on the
//     angle normalised by norm_angle(); tanh_f evaluates in double (fma chains, no libm) and rounds once; -ffp-contract=off on both passes.
//   * The reset stream is ours: two splitmix64 draws from the member's uint32 environment seed (cartpole.h's generator, restated here so that
//     cartpole.h stays as it is).
//   * A dense unit is FOUR fmaf chains (k = r mod 4, ascending, from +0) added as ((c0 + c1) + (c2 + c3)) + b: part of the contract.
// A plain C++ compiler can include this file (the kernel is behind __HIPCC__): tests/pendulum_asan_main.cpp does.
#pragma once
#include <string.h>
#include "maze.h"

namespace dne {
namespace pendulum {

using maze::SinCosD;
using maze::perturbed;
using maze::relu;
using maze::sincos_d;

constexpr int OBS = 3, MAX_OUT = 16, EPISODE_STEPS = 200 /* Pendulum-v0: max_episode_steps */, TRACE_W = 8;
constexpr double PI = 3.141592653589793, TWO_PI = 6.283185307179586;   // the doubles nearest pi and 2 pi
constexpr double DT = 0.05, MAX_SPEED = 8.0, MAX_TORQUE = 2.0;
constexpr float AC_LOW = -2.0f, AC_RANGE = 4.0f;                      // the action space: Box(-2, 2)
enum { AC_CONTINUOUS = 0, AC_UNIFORM = 1 };
enum { NL_TANH = 0, NL_RELU = 1 };

// flat order = TF's creation order (policies.py:155-200 over tf_util.dense): l0/w [3][H], l0/b, l1/w [H][H], l1/b, out/w [H][O], out/b
struct Offsets { int w1, b1, w2, b2, w3, b3, P; };
MZ_HD Offsets offsets(int H, int O) {
    Offsets o;
    o.w1 = 0; o.b1 = OBS * H; o.w2 = o.b1 + H; o.b2 = o.w2 + H * H; o.w3 = o.b2 + H; o.b3 = o.w3 + H * O; o.P = o.b3 + O;
    return o;
}
inline bool hidden_ok(int H) { return H == 64 || H == 128 || H == 256; }

struct State { double theta, theta_dot; };
struct Seen { double n, s; float ob[OBS]; };   // what one look at the state gives: the normalised angle, its sine, the observation

// ---- math --------------------------------------------------------------------------------------------------------------------------------
// the angle brought to [-pi, pi] (to rounding): x - 2 pi * floor((x + pi) / (2 pi)); floor is exact, a NaN or an infinity goes through as NaN
MZ_HD double norm_angle(double x) { return x - TWO_PI * floor((x + PI) / TWO_PI); }

// tanh of a float: |x| < 2^-12 -> x (the cubic term is below a quarter ulp), |x| >= 10 -> +-1, NaN -> NaN; between, t = exp(-2|x|) in double
// -- n = round(y / ln 2) for y = -2|x| in (-20, 0), so |n| <= 29 and the cast is guarded by the two branches above; r = y - n ln 2 with ln 2
// split in two (n LN2_HI is exact: LN2_HI keeps 32 bits); the Taylor series of exp to r^13 on |r| <= 0.347 (truncation below 5e-18) as one fma
// chain; 2^n built in the exponent field -- then (1 - t) / (1 + t), the sign restored, rounded to float once.  The cancellation in 1 - t costs at
// most 12 bits of the double's 53, so the float is within 1 ulp of the correctly rounded value.
MZ_HD float tanh_f(float x) {
    if (x != x) return x;
    const float ax = x < 0.0f ? -x : x;
    if (ax < 0x1p-12f) return x;
    if (ax >= 10.0f) return x < 0.0f ? -1.0f : 1.0f;
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double y = -2.0 * (double)ax;
    const int n = (int)(y * 1.44269504088896338700e+00 - 0.5);   // y < 0: round half away from zero
    const double nd = (double)n;
    double r = fma(-nd, LN2_HI, y);
    r = fma(-nd, LN2_LO, r);
    double p = 1.0 / 6227020800.0;               // 1/13!
    p = fma(p, r, 1.0 / 479001600.0);            // 1/12!
    p = fma(p, r, 1.0 / 39916800.0);             // 1/11!
    p = fma(p, r, 1.0 / 3628800.0);              // 1/10!
    p = fma(p, r, 1.0 / 362880.0);               // 1/9!
    p = fma(p, r, 1.0 / 40320.0);                // 1/8!
    p = fma(p, r, 1.0 / 5040.0);                 // 1/7!
    p = fma(p, r, 1.0 / 720.0);                  // 1/6!
    p = fma(p, r, 1.0 / 120.0);                  // 1/5!
    p = fma(p, r, 1.0 / 24.0);                   // 1/4!
    p = fma(p, r, 1.0 / 6.0);                    // 1/3!
    p = fma(p, r, 0.5);                          // 1/2!
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const uint64_t bits = (uint64_t)(1023 + n) << 52;   // 2^n, n in [-29, 0]
    double scale;
    memcpy(&scale, &bits, sizeof(scale));
    const double t = p * scale;                  // exact scaling: no underflow this far up
    const double v = (1.0 - t) / (1.0 + t);
    return (float)(x < 0.0f ? -v : v);
}

// ---- the reset ---------------------------------------------------------------------------------------------------------------------------
// splitmix64 from z = seed: two draws, each u = (r >> 11) * 2^-53 in [0, 1) (the conversion is exact); theta = -pi + 2 pi u0, theta_dot = -1 + 2 u1
MZ_HD State reset_state(uint32_t seed) {
    uint64_t z = seed;
    double u[2];
    for (int i = 0; i < 2; i++) {
        z += 0x9E3779B97F4A7C15ull;
        uint64_t r = z;
        r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull;
        r = (r ^ (r >> 27)) * 0x94D049BB133111EBull;
        r ^= r >> 31;
        u[i] = (double)(r >> 11) * 0x1p-53;
    }
    State s;
    s.theta = -PI + TWO_PI * u[0];
    s.theta_dot = -1.0 + 2.0 * u[1];
    return s;
}

// ---- the step ----------------------------------------------------------------------------------------------------------------------------
// one look at the state: the observation (cos, sin, theta_dot) as floats, and the two doubles the step shares with it
MZ_HD Seen look(const State &s) {
    Seen v;
    v.n = norm_angle(s.theta);
    const SinCosD t = sincos_d(v.n);
    v.s = t.s;
    v.ob[0] = (float)t.c; v.ob[1] = (float)t.s; v.ob[2] = (float)s.theta_dot;
    return v;
}

// one Euler step under the float action a from the state `v` was taken of; returns the reward.  The comparisons let a NaN through.
MZ_HD float step(State &s, const Seen &v, float a) {
    const double u = a < -2.0f ? -MAX_TORQUE : (a > 2.0f ? MAX_TORQUE : (double)a);
    const double cost = (v.n * v.n + 0.1 * (s.theta_dot * s.theta_dot)) + 0.001 * (u * u);
    const double nd = s.theta_dot + (15.0 * v.s + 3.0 * u) * DT;   // -3 g / (2 l) sin(theta + pi) = 15 sin(theta); 3 / (m l^2) = 3
    s.theta = s.theta + nd * DT;
    s.theta_dot = nd < -MAX_SPEED ? -MAX_SPEED : (nd > MAX_SPEED ? MAX_SPEED : nd);
    return (float)(-cost);
}

MZ_HD double sign_d(float r) { return r > 0.0f ? 1.0 : (r < 0.0f ? -1.0 : (double)r); }   // np.sign: 0 and NaN stay

// ---- the policy --------------------------------------------------------------------------------------------------------------------------
// tf.clip_by_value((o - ob_mean) / ob_std, -5, 5) on one component: one subtraction, one correctly rounded division; a NaN goes through
MZ_HD float normalise(float ob, float mean, float std) {
    const float x = (ob - mean) / std;
    return x < -5.0f ? -5.0f : (x > 5.0f ? 5.0f : x);
}

// one output unit of a dense layer: four fmaf chains over k = r (mod 4), ascending, each from +0.0f, then ((c0 + c1) + (c2 + c3)) + b.
// dense4_acc takes the chains over N more inputs (a caller that goes in pieces starts each piece at a multiple of 4)
template <int N>
MZ_HD void dense4_acc(float *c, const float *in, const float *w, int wstride) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < N; k++) c[k & 3] = fmaf(in[k], w[k * wstride], c[k & 3]);
}
MZ_HD float dense4_sum(const float *c, float b) { return ((c[0] + c[1]) + (c[2] + c[3])) + b; }
template <int N>
MZ_HD float dense4(const float *in, const float *w, int wstride, float b) {
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    dense4_acc<N>(c, in, w, wstride);
    return dense4_sum(c, b);
}

template <bool TANH>
MZ_HD float nonlin(float v) { return TANH ? tanh_f(v) : relu(v); }

// the action of n_out output values.  continuous: out[0].  uniform over B = n_out bins (policies.py:116-119, 169-174): the first maximum
// under a strict > scan from -inf (a NaN never wins; all NaN, or all -inf, gives bin 0), then 1 / (B - 1) * aidx * (high - low) + low
MZ_HD float pick_action(const float *out, int n_out, int mode) {
    if (mode == AC_CONTINUOUS) return out[0];
    int aidx = 0;
    float best = -INFINITY;
    for (int i = 0; i < n_out; i++)
        if (out[i] > best) { best = out[i]; aidx = i; }
    return ((1.0f / ((float)n_out - 1.0f)) * (float)aidx) * AC_RANGE + AC_LOW;
}

// what one episode reads beside theta (the same values on both sides)
struct Options {
    int n_out, ac_mode;
    float mean[OBS], std[OBS];
    float ac_noise_std;
};

MZ_HD void write_trace(double *row, const Seen &v, float a_net, float a, float rew, const State &s) {
    row[0] = (double)v.ob[0]; row[1] = (double)v.ob[1]; row[2] = (double)v.ob[2];
    row[3] = (double)a_net; row[4] = (double)a; row[5] = (double)rew; row[6] = s.theta; row[7] = s.theta_dot;
}

// ---- the CPU side ------------------------------------------------------------------------------------------------------------------------
// the forward pass alone on one raw observation: x [3] the normalised input, h1 [H], h2 [H], out [n_out]; returns the action
template <int H, bool TANH>
inline float forward_host_t(const float *theta, const Options &o, const float *ob, float *x, float *h1, float *h2, float *out) {
    const Offsets L = offsets(H, o.n_out);
    for (int i = 0; i < OBS; i++) x[i] = normalise(ob[i], o.mean[i], o.std[i]);
    for (int j = 0; j < H; j++) h1[j] = nonlin<TANH>(dense4<OBS>(x, theta + L.w1 + j, H, theta[L.b1 + j]));
    for (int j = 0; j < H; j++) h2[j] = nonlin<TANH>(dense4<H>(h1, theta + L.w2 + j, H, theta[L.b2 + j]));
    for (int j = 0; j < o.n_out; j++) out[j] = dense4<H>(h2, theta + L.w3 + j, o.n_out, theta[L.b3 + j]);
    return pick_action(out, o.n_out, o.ac_mode);
}

// what one episode leaves
struct Episode { float ret, sign; int len; State s; double ob_sum[OBS], ob_sumsq[OBS]; };

// one episode of one theta from reset_state(seed), or from init2 when given: min(tslimit, 200) steps, never done early.  ac_eps (may be null):
// the 200 values of the noise table the action noise reads; stat: accumulate the observations acted on.  trace (may be null): [steps][8].
template <int H, bool TANH>
inline Episode rollout_host_t(const float *theta, const Options &o, uint32_t seed, const double *init2, int tslimit, const float *ac_eps,
                              bool stat, double *trace) {
    Episode e{};
    State s = reset_state(seed);
    if (init2) { s.theta = init2[0]; s.theta_dot = init2[1]; }
    const int steps = tslimit < EPISODE_STEPS ? tslimit : EPISODE_STEPS;
    float x[OBS], h1[H], h2[H], out[MAX_OUT];
    double ret = 0.0, sg = 0.0;
    for (int t = 0; t < steps; t++) {
        const Seen v = look(s);
        const float a_net = forward_host_t<H, TANH>(theta, o, v.ob, x, h1, h2, out);
        const float a = ac_eps ? perturbed(a_net, o.ac_noise_std, ac_eps[t]) : a_net;
        if (stat)
            for (int i = 0; i < OBS; i++) { const double d = (double)v.ob[i]; e.ob_sum[i] += d; e.ob_sumsq[i] += d * d; }
        const float rew = step(s, v, a);
        ret += (double)rew;
        sg += sign_d(rew);
        if (trace) write_trace(trace + (size_t)t * TRACE_W, v, a_net, a, rew, s);
    }
    e.ret = (float)ret; e.sign = (float)sg; e.len = steps; e.s = s;
    return e;
}

// the two above for a run-time (H, nonlinearity); H must pass hidden_ok
inline float forward_host(int H, int nl, const float *theta, const Options &o, const float *ob, float *x, float *h1, float *h2, float *out) {
    const bool th = nl == NL_TANH;
    switch (H) {
    case 64: return th ? forward_host_t<64, true>(theta, o, ob, x, h1, h2, out) : forward_host_t<64, false>(theta, o, ob, x, h1, h2, out);
    case 128: return th ? forward_host_t<128, true>(theta, o, ob, x, h1, h2, out) : forward_host_t<128, false>(theta, o, ob, x, h1, h2, out);
    default: return th ? forward_host_t<256, true>(theta, o, ob, x, h1, h2, out) : forward_host_t<256, false>(theta, o, ob, x, h1, h2, out);
    }
}
inline Episode rollout_host(int H, int nl, const float *theta, const Options &o, uint32_t seed, const double *init2, int tslimit,
                            const float *ac_eps, bool stat, double *trace) {
    const bool th = nl == NL_TANH;
    switch (H) {
    case 64: return th ? rollout_host_t<64, true>(theta, o, seed, init2, tslimit, ac_eps, stat, trace)
                       : rollout_host_t<64, false>(theta, o, seed, init2, tslimit, ac_eps, stat, trace);
    case 128: return th ? rollout_host_t<128, true>(theta, o, seed, init2, tslimit, ac_eps, stat, trace)
                        : rollout_host_t<128, false>(theta, o, seed, init2, tslimit, ac_eps, stat, trace);
    default: return th ? rollout_host_t<256, true>(theta, o, seed, init2, tslimit, ac_eps, stat, trace)
                       : rollout_host_t<256, false>(theta, o, seed, init2, tslimit, ac_eps, stat, trace);
    }
}

// open-loop: the environment alone under T given float actions from init2.  rows [T][3]: theta and theta_dot after the step, then the reward
inline void actions_host(const float *actions, int T, const double *init2, double *rows) {
    State s;
    s.theta = init2[0]; s.theta_dot = init2[1];
    for (int t = 0; t < T; t++) {
        const Seen v = look(s);
        const float rew = step(s, v, actions[t]);
        double *row = rows + (size_t)t * 3;
        row[0] = s.theta; row[1] = s.theta_dot; row[2] = (double)rew;
    }
}

// value by value (dne_pendulum_math_host / dne_pendulum_debug_math): fn 0 tanh_f(x), 1 norm_angle(x), 2 normalise(x, a, b)
enum { MATH_TANH = 0, MATH_NORM = 1, MATH_NORMALISE = 2, MATH_FNS = 3 };
MZ_HD double math_fn(int fn, double x, float a, float b) {
    if (fn == MATH_TANH) return (double)tanh_f((float)x);
    if (fn == MATH_NORM) return norm_angle(x);
    return (double)normalise((float)x, a, b);
}

#if defined(__HIPCC__)
// ---- the device side: whole episodes in one launch ------------------------------------------------------------------------------------------
// One workgroup of H threads (1, 2 or 4 waves) per member.  Thread j owns hidden unit j of both layers: its l0/w column (3 values), its l1/w
// column (H values) and its two biases are built once from base slot and noise table and stay in registers -- w2 is indexed by compile-time
// constants only (every loop over it is fully unrolled), so it never goes to scratch.  out/w (transposed) and out/b are perturbed once into LDS.  h1 and h2 are H floats
// of LDS each, written by their owners and read by everyone at the same address (a broadcast: no bank conflict at any width).  The state is
// kept redundantly by every thread -- the same operations on the same values -- and every thread picks the action from the outputs in LDS, so
// nothing is broadcast after it.  Three barriers a step (after h1, after h2, after the outputs); each buffer's next write lies at least two
// barriers behind its last read.  Every member runs min(tslimit, 200) steps: no thread leaves the loop early, every barrier is reached by the
// whole workgroup.  Between steps nothing touches global memory but the one action-noise value, and the trace when asked for.
struct RolloutArgs {
    const float *noise, *bases; size_t base_stride;
    const int32_t *m_slot; const int64_t *m_off; const float *m_scale;
    int first, count;              // members [first, first + count): one workgroup each
    const uint32_t *seed;          // per member: the environment seed
    int has_init; double init2[2]; // the trace's explicit initial state (has_init != 0), else reset_state(seed)
    int tslimit;
    Options opt;
    const int64_t *ac_off;         // per member: where its 200 action-noise values start in the noise table, < 0 for none; null: nobody has any
    const uint8_t *stat_flag;      // per member: accumulate the observations acted on; null: nobody does
    float *ret, *sign; int32_t *len; double *state;   // per member (null when tracing); state [member][2]
    double *ob_sum, *ob_sumsq; int32_t *ob_count;     // per member [3], [3], 1 (zero for an unflagged member)
    double *trace; int32_t *trace_steps;              // [steps][8] of member `first` (count == 1) and its length, or null
};

constexpr int CH = 16, OW_ROW_PAD = 4;   // inputs per piece of a dense layer; floats of padding behind each row of out/w in LDS
// A VALU instruction cannot read an accumulator register, so of a thread's H = 256 l1/w values only 128 stay in vector registers; the other
// 128 are parked in accumulator registers (allocated by the compiler through the "a" constraint, never named) and copied out, one
// v_accvgpr_read each, as their piece comes up.  Left to choose for itself the compiler spilled some 300 registers to scratch at H = 256.
__device__ __forceinline__ void park(float &a, float v) { asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(v)); }
__device__ __forceinline__ float fetch(const float &a) { float v; asm("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a)); return v; }
// dense4 over H inputs in LDS, in pieces of CH: piece i + 1 is read into registers (16-byte reads) before piece i's chains run, and the
// scheduler may not move anything across a piece's end -- left to itself it reads all H inputs ahead of the first fmaf, which at H = 256
// beside the 256 weights does not fit the register file.  W: w(q) gives weights 4 q .. 4 q + 3 (from a register array, or from LDS).
template <int H, typename W>
__device__ __forceinline__ float dense4_lds(const float *s_in, W w, float b) {
    const float4 *in4 = reinterpret_cast<const float4 *>(s_in);
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 buf[2][CH / 4];
#pragma unroll
    for (int q = 0; q < CH / 4; q++) buf[0][q] = in4[q];
#pragma unroll
    for (int p = 0; p < H / CH; p++) {
        if (p + 1 < H / CH) {
#pragma unroll
            for (int q = 0; q < CH / 4; q++) buf[(p + 1) & 1][q] = in4[(p + 1) * (CH / 4) + q];
        }
#pragma unroll
        for (int q = 0; q < CH / 4; q++) {
            const float4 x = buf[p & 1][q], wq = w(p * (CH / 4) + q);
            const float xv[4] = {x.x, x.y, x.z, x.w}, wv[4] = {wq.x, wq.y, wq.z, wq.w};
            dense4_acc<4>(c, xv, wv, 1);
        }
        asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));   // the piece's fmafs are done HERE: a pure operation has no place otherwise
        __builtin_amdgcn_sched_barrier(0);
    }
    return dense4_sum(c, b);
}

template <int H, bool TANH>
__global__ __launch_bounds__(H) void k_pendulum_rollout(const RolloutArgs A) {
    __shared__ __attribute__((aligned(16))) float s_h1[H], s_h2[H];
    __shared__ __attribute__((aligned(16))) float s_ow[MAX_OUT * (H + OW_ROW_PAD)];   // out/w transposed: row o holds column o, 16 bytes of padding
    __shared__ float s_ob[MAX_OUT], s_out[MAX_OUT];
    const int j = threadIdx.x;
    const int m = A.first + blockIdx.x;    // the grid is `count` workgroups
    const int O = A.opt.n_out;
    const Offsets L = offsets(H, O);
    const float *base = A.bases + (size_t)A.m_slot[m] * A.base_stride;
    const float *eps = A.noise + A.m_off[m];
    const float scale = A.m_scale[m];
    constexpr int NV = H > 128 ? 128 : H, NA = H - NV;   // l1/w values in vector / in accumulator registers
    float w1[OBS], w2[NV], wa[NA > 0 ? NA : 1];
#pragma unroll
    for (int k = 0; k < OBS; k++) w1[k] = perturbed(base[L.w1 + k * H + j], scale, eps[L.w1 + k * H + j]);
#pragma unroll
    for (int k = 0; k < H; k++) {
        float wk = perturbed(base[L.w2 + k * H + j], scale, eps[L.w2 + k * H + j]);
        if (k < NV) { asm volatile("" : "+v"(wk)); w2[k] = wk; } else park(wa[k - NV], wk);   // formed here, not where it is first used
        if (k % CH == CH - 1) __builtin_amdgcn_sched_barrier(0);   // CH columns' loads in flight, not H
    }
    const float b1 = perturbed(base[L.b1 + j], scale, eps[L.b1 + j]), b2 = perturbed(base[L.b2 + j], scale, eps[L.b2 + j]);
    for (int i = j; i < H * O; i += H) s_ow[(i % O) * (H + OW_ROW_PAD) + i / O] = perturbed(base[L.w3 + i], scale, eps[L.w3 + i]);   // out/w [H][O]
    if (j < O) s_ob[j] = perturbed(base[L.b3 + j], scale, eps[L.b3 + j]);

    State s = reset_state(A.seed[m]);
    if (A.has_init) { s.theta = A.init2[0]; s.theta_dot = A.init2[1]; }
    const int steps = A.tslimit < EPISODE_STEPS ? A.tslimit : EPISODE_STEPS;
    const int64_t ac_off = A.ac_off ? A.ac_off[m] : -1;
    const bool stat = A.stat_flag && A.stat_flag[m];
    double ret = 0.0, sg = 0.0, ob_sum[OBS] = {0.0, 0.0, 0.0}, ob_sumsq[OBS] = {0.0, 0.0, 0.0};
    float x[OBS];
    __syncthreads();                       // s_ow and s_ob are complete
    for (int t = 0; t < steps; t++) {
        const Seen v = look(s);
#pragma unroll
        for (int i = 0; i < OBS; i++) x[i] = normalise(v.ob[i], A.opt.mean[i], A.opt.std[i]);
        s_h1[j] = nonlin<TANH>(dense4<OBS>(x, w1, 1, b1));
        __syncthreads();
        s_h2[j] = nonlin<TANH>(dense4_lds<H>(s_h1, [&](int q) {
            return 4 * q < NV ? make_float4(w2[(4 * q) % NV], w2[(4 * q + 1) % NV], w2[(4 * q + 2) % NV], w2[(4 * q + 3) % NV])
                              : make_float4(fetch(wa[(4 * q - NV) % (NA + 1)]), fetch(wa[(4 * q + 1 - NV) % (NA + 1)]), fetch(wa[(4 * q + 2 - NV) % (NA + 1)]),
                                            fetch(wa[(4 * q + 3 - NV) % (NA + 1)]));
        }, b2));
        __syncthreads();
        if (j < O) s_out[j] = dense4_lds<H>(s_h2, [&](int q) { return reinterpret_cast<const float4 *>(s_ow + j * (H + OW_ROW_PAD))[q]; }, s_ob[j]);
        __syncthreads();
        const float a_net = pick_action(s_out, O, A.opt.ac_mode);   // every thread, from LDS: the same scan on the same values
        const float a = ac_off >= 0 ? perturbed(a_net, A.opt.ac_noise_std, A.noise[ac_off + t]) : a_net;
        if (stat) {
#pragma unroll
            for (int i = 0; i < OBS; i++) { const double d = (double)v.ob[i]; ob_sum[i] += d; ob_sumsq[i] += d * d; }
        }
        const float rew = step(s, v, a);
        ret += (double)rew;
        sg += sign_d(rew);
        if (A.trace && j == 0) write_trace(A.trace + (size_t)t * TRACE_W, v, a_net, a, rew, s);
    }
    if (j == 0) {
        if (A.ret) {
            A.ret[m] = (float)ret; A.sign[m] = (float)sg; A.len[m] = steps;
            A.state[2 * (size_t)m] = s.theta; A.state[2 * (size_t)m + 1] = s.theta_dot;
#pragma unroll
            for (int i = 0; i < OBS; i++) { A.ob_sum[OBS * (size_t)m + i] = ob_sum[i]; A.ob_sumsq[OBS * (size_t)m + i] = ob_sumsq[i]; }
            A.ob_count[m] = stat ? steps : 0;
        }
        if (A.trace_steps) *A.trace_steps = steps;
    }
}

// value by value, one thread per element
__global__ void k_pendulum_math(int fn, const double *x, int n, float a, float b, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = math_fn(fn, x[i], a, b);
}
#endif

}  // namespace pendulum
}  // namespace dne
