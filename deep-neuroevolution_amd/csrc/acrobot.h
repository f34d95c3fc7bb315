// acrobot.h -- gym.Acrobot-v1, the fourth step environment, as ONE __host__ __device__ text in the manner of cartpole.h: the reset, the step, the
// observation and the action below compile for the CPU (the host twins of step_env.h and dense.h) and for gfx950 (k_stepenv_*_acrobot,
// k_dense_run<DNE_ENV_ACROBOT>), and the two agree bit for bit.  DESIGN.md section 19 holds the contract.
//   * The environment is Sutton & Barto's acrobot restated from its published equations, in the "book" form that gym's
//     classic_control/acrobot.py integrates with one classical RK4 step of 0.2 s -- not recorded from gym.  There is no policy here: the policy
//     is dense.h's, the environment has no engine kind of its own (DNE_ENV_ACROBOT is an environment id).
//   * Every operation is an IEEE double operation in the association written here; -ffp-contract=off on both passes.  Every sine and cosine is
//     maze.h's sincos_d (fma chains, no libm) on pendulum.h's norm_angle of the argument: sincos_d is good for |x| <= 3 pi, and an argument in
//     the middle of a step (theta1 + theta2 near 2 pi plus half a step at 13 pi rad/s) exceeds that.  gym writes cos(x - pi/2) where this says
//     sin(x): the same function, one rounding apart.
//   * OURS, not gym's: the angles are wrapped by norm_angle's floor form, which sends pi to -pi where gym's wrap() loop keeps pi -- no loop over
//     data appears here; the reset stream (gym's is unseeded): cart-pole's four splitmix64 draws from the uint32 seed, here over [-0.1, 0.1); the
//     first maximum of the three outputs with a NaN never winning.
// A plain C++ compiler can include this file: tests/acrobot_asan_main.cpp does.
#pragma once
#include "maze.h"
#include "pendulum.h"

namespace dne {
namespace acrobot {

using maze::SinCosD;

constexpr int OBS = 6, ACT = 3, EPISODE_STEPS = 500 /* Acrobot-v1: max_episode_steps */;
constexpr double M1 = 1.0, M2 = 1.0, L1 = 1.0, LC1 = 0.5, LC2 = 0.5, I1 = 1.0, I2 = 1.0, G = 9.8, DT = 0.2;
constexpr double MAX_VEL_1 = 4.0 * pendulum::PI, MAX_VEL_2 = 9.0 * pendulum::PI;   // products of the double nearest pi
// the constant factors of the derivative, each in the association of the formula it comes from
constexpr double K_D1 = M1 * (LC1 * LC1), K_LL = L1 * L1 + LC2 * LC2, K_2LL = (2.0 * L1) * LC2, K_D2 = LC2 * LC2, K_LLC = L1 * LC2,
                 K_PHI2 = (M2 * LC2) * G, K_T1 = (M2 * L1) * LC2, K_T2 = ((2.0 * M2) * L1) * LC2, K_T3 = (M1 * LC1 + M2 * L1) * G,
                 K_DEN = M2 * (LC2 * LC2) + I2, HALF_DT = DT / 2.0, SIXTH_DT = DT / 6.0;

struct State { double th1, th2, w1, w2; };

MZ_HD SinCosD sc(double x) { return maze::sincos_d(pendulum::norm_angle(x)); }

// ---- the reset ---------------------------------------------------------------------------------------------------------------------------
// cartpole::reset_state's stream: splitmix64 from z = seed, four draws, each u = (r >> 11) * 2^-53 in [0, 1); state[i] = -0.1 + 0.2 * u
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
        v[i] = -0.1 + 0.2 * u;
    }
    State s;
    s.th1 = v[0]; s.th2 = v[1]; s.w1 = v[2]; s.w2 = v[3];
    return s;
}

// ---- the derivative ------------------------------------------------------------------------------------------------------------------------
// f(th1, th2, w1, w2; tau) = (w1, w2, dw1, dw2), the book form
MZ_HD State deriv(const State &s, double tau) {
    const SinCosD t2 = sc(s.th2);
    const double d1 = ((K_D1 + M2 * (K_LL + K_2LL * t2.c)) + I1) + I2;
    const double d2 = M2 * (K_D2 + K_LLC * t2.c) + I2;
    const double phi2 = K_PHI2 * sc(s.th1 + s.th2).s;
    const double phi1 = (((-K_T1 * (s.w2 * s.w2)) * t2.s - ((K_T2 * s.w2) * s.w1) * t2.s) + K_T3 * sc(s.th1).s) + phi2;
    const double dw2 = (((tau + (d2 / d1) * phi1) - (K_T1 * (s.w1 * s.w1)) * t2.s) - phi2) / (K_DEN - (d2 * d2) / d1);
    const double dw1 = -(d2 * dw2 + phi1) / d1;
    State f;
    f.th1 = s.w1; f.th2 = s.w2; f.w1 = dw1; f.w2 = dw2;
    return f;
}

MZ_HD State nudged(const State &s, double h, const State &k) {
    State o;
    o.th1 = s.th1 + h * k.th1; o.th2 = s.th2 + h * k.th2; o.w1 = s.w1 + h * k.w1; o.w2 = s.w2 + h * k.w2;
    return o;
}
MZ_HD double rk4_sum(double a, double b, double c, double d) { return ((a + 2.0 * b) + 2.0 * c) + d; }

// -cos(th1) - cos(th2 + th1) > 1.0: the free end above the line one link over the pivot.  Strict, so a NaN is never terminal
MZ_HD bool terminal(const State &s) { return -sc(s.th1).c - sc(s.th2 + s.th1).c > 1.0; }

// ---- the step ----------------------------------------------------------------------------------------------------------------------------
// one RK4 step of DT under action a in {0, 1, 2} (torque a - 1), the angles wrapped, the velocities clamped by comparisons that let a NaN
// through; returns terminal
MZ_HD bool step(State &s, int a) {
    const double tau = (double)(a - 1);
    const State k1 = deriv(s, tau);
    const State k2 = deriv(nudged(s, HALF_DT, k1), tau);
    const State k3 = deriv(nudged(s, HALF_DT, k2), tau);
    const State k4 = deriv(nudged(s, DT, k3), tau);
    State n;
    n.th1 = s.th1 + SIXTH_DT * rk4_sum(k1.th1, k2.th1, k3.th1, k4.th1);
    n.th2 = s.th2 + SIXTH_DT * rk4_sum(k1.th2, k2.th2, k3.th2, k4.th2);
    n.w1 = s.w1 + SIXTH_DT * rk4_sum(k1.w1, k2.w1, k3.w1, k4.w1);
    n.w2 = s.w2 + SIXTH_DT * rk4_sum(k1.w2, k2.w2, k3.w2, k4.w2);
    n.th1 = pendulum::norm_angle(n.th1);
    n.th2 = pendulum::norm_angle(n.th2);
    if (n.w1 < -MAX_VEL_1) n.w1 = -MAX_VEL_1;
    if (n.w1 > MAX_VEL_1) n.w1 = MAX_VEL_1;
    if (n.w2 < -MAX_VEL_2) n.w2 = -MAX_VEL_2;
    if (n.w2 > MAX_VEL_2) n.w2 = MAX_VEL_2;
    s = n;
    return terminal(s);
}

// the observation: (cos th1, sin th1, cos th2, sin th2, w1, w2), each double cast to float
MZ_HD void make_obs(const State &s, float *obs) {
    const SinCosD a = sc(s.th1), b = sc(s.th2);
    obs[0] = (float)a.c; obs[1] = (float)a.s; obs[2] = (float)b.c; obs[3] = (float)b.s; obs[4] = (float)s.w1; obs[5] = (float)s.w2;
}

// the first maximum of three outputs; a NaN never wins, all NaN gives 0
MZ_HD int pick_action(const float *out) {
    int a = 0;
    if (out[1] > out[a]) a = 1;
    if (out[2] > out[a]) a = 2;
    return a;
}

// ---- the CPU side ------------------------------------------------------------------------------------------------------------------------
// open-loop: the environment alone under T given actions from init4.  rows [T][5]: the state after the step, then terminal (1.0 / 0.0); the
// stepping goes on past it (the caller reads where it first shows)
inline void actions_host(const int32_t *actions, int T, const double *init4, double *rows) {
    State s;
    s.th1 = init4[0]; s.th2 = init4[1]; s.w1 = init4[2]; s.w2 = init4[3];
    for (int t = 0; t < T; t++) {
        const bool over = step(s, actions[t]);
        double *row = rows + (size_t)t * 5;
        row[0] = s.th1; row[1] = s.th2; row[2] = s.w1; row[3] = s.w2; row[4] = over ? 1.0 : 0.0;
    }
}

}  // namespace acrobot
}  // namespace dne
