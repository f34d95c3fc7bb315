// step_env.h -- the hard maze, the cart-pole, the pendulum and the acrobot as environments of their own: a batch that persists between calls and moves ONE
// step per call under actions the caller supplies (the seam of gym_tensorflow/tf_env.py:27-124: reset, step, observation, final_state apart
// from the model).  Nothing is derived here: every operation is a function of maze.h, cartpole.h or pendulum.h, used, not copied, so a value
// this header produces is bit for bit the one the whole-episode kernels and their host twins produce.  As those headers it is ONE
// __host__ __device__ text: `advance` below is called by the CPU twin (step_host) and by the kernels, -ffp-contract=off on both passes.  A plain
// C++ compiler can include this file (the kernels are behind __HIPCC__): tests/stepenv_asan_main.cpp does.  DESIGN.md section 15.
//
// One environment is (state double[S], steps, limit, done, observation float[OBS]):
//   maze       S 7: x, y, heading, speed, ang_vel, collide, collisions -- the floats and ints of maze::State, which widen to double exactly (a
//              state given from outside is rounded to those types, a value no int holds becomes 0); OBS 11; action float[2]; own limit 400
//   cart-pole  S 4: x, x_dot, theta, theta_dot; OBS 4; action int32 in {0, 1}; own limit 500
//   pendulum   S 2: theta, theta_dot; OBS 3; action float[1]; own limit 200
//   acrobot    S 4: theta1, theta2, omega1, omega2; OBS 6; action int32 in {0, 1, 2}; own limit 500.  An environment id (ENV_ACROBOT,
//              DNE_ENV_ACROBOT), not an engine kind: a DNE_KIND_DENSE engine created on it steps it, and every host twin takes the id
// reset    maze: reset_state(header), the seed is not read; cart-pole and pendulum: reset_state(seed).  steps = 0, done = 0,
//          limit = min(max_steps, own limit), max_steps <= 0 meaning the own limit (max_frames=None).
// observe  what the whole-episode kernel's policy would see next: the maze's 11 floats of observe_host; the cart-pole's four state values cast
//          to float; the pendulum's three raw floats of look(s).ob (normalising them is the policy's business).
// step     maze: interpret_outputs -> propose_move -> collide_partial -> commit_move; reward final_reward on the step that makes steps == 400
//          and 0 on every other one (a smaller limit ends the episode at reward 0, as maze::rollout_host); done when steps == limit.
//          cart-pole: reward 1 on every step taken, the terminating one included; done when cartpole::step's strict thresholds fire or
//          steps == limit.  pendulum: pendulum::step (the torque clip is inside it), its float reward; done when steps == limit, never earlier.
//          acrobot: acrobot::step; reward -1 on every step but the terminal one, which earns 0; done when terminal or steps == limit.
// a done environment stepped again: reward 0, done stays 1, state, steps and observation keep every bit (advance returns false and its
//          caller writes nothing back), so a caller may go on stepping a whole batch until its last member ends.
#pragma once
#include "maze.h"
#include "cartpole.h"
#include "pendulum.h"
#include "acrobot.h"

namespace dne {
namespace stepenv {

enum { KIND_MAZE = 4, KIND_CARTPOLE = 5, KIND_PENDULUM = 6 };   // DNE_KIND_* of include/dne_hip.h (engine.hip asserts the three)
enum { ENV_ACROBOT = 9 };                                        // DNE_ENV_ACROBOT: an environment without an engine kind of its own
constexpr int MAX_S = 7, MAX_OBS = 11, MAX_ACT = 2;

struct Dims { int obs, act, state, act_is_int, own_limit; };
MZ_HD bool dims(int kind, Dims *d) {
    if (kind == KIND_MAZE) { d->obs = maze::OBS; d->act = 2; d->state = 7; d->act_is_int = 0; d->own_limit = maze::EPISODE_STEPS; return true; }
    if (kind == KIND_CARTPOLE) { d->obs = cartpole::OBS; d->act = 1; d->state = 4; d->act_is_int = 1; d->own_limit = cartpole::EPISODE_STEPS; return true; }
    if (kind == KIND_PENDULUM) { d->obs = pendulum::OBS; d->act = 1; d->state = 2; d->act_is_int = 0; d->own_limit = pendulum::EPISODE_STEPS; return true; }
    if (kind == ENV_ACROBOT) { d->obs = acrobot::OBS; d->act = 1; d->state = 4; d->act_is_int = 1; d->own_limit = acrobot::EPISODE_STEPS; return true; }
    return false;
}
MZ_HD int step_limit(int max_steps, int own) { return max_steps <= 0 || max_steps > own ? own : max_steps; }

// ---- the state record ----------------------------------------------------------------------------------------------------------------------
// a double that no int holds (a NaN, an infinity, anything beyond 2^31) is never cast: C++ leaves that undefined, and x86 and gfx950 answer differently
MZ_HD int to_int(double v) { return v > -2147483649.0 && v < 2147483648.0 ? (int)v : 0; }
MZ_HD void unpack(const double *p, maze::State &s) {
    s.x = (float)p[0]; s.y = (float)p[1]; s.heading = (float)p[2]; s.speed = (float)p[3]; s.ang_vel = (float)p[4];
    s.collide = to_int(p[5]); s.collisions = to_int(p[6]);
}
MZ_HD void pack(const maze::State &s, double *p) {
    p[0] = (double)s.x; p[1] = (double)s.y; p[2] = (double)s.heading; p[3] = (double)s.speed; p[4] = (double)s.ang_vel;
    p[5] = (double)s.collide; p[6] = (double)s.collisions;
}
MZ_HD void unpack(const double *p, cartpole::State &s) { s.x = p[0]; s.x_dot = p[1]; s.theta = p[2]; s.theta_dot = p[3]; }
MZ_HD void pack(const cartpole::State &s, double *p) { p[0] = s.x; p[1] = s.x_dot; p[2] = s.theta; p[3] = s.theta_dot; }
MZ_HD void unpack(const double *p, pendulum::State &s) { s.theta = p[0]; s.theta_dot = p[1]; }
MZ_HD void pack(const pendulum::State &s, double *p) { p[0] = s.theta; p[1] = s.theta_dot; }
MZ_HD void unpack(const double *p, acrobot::State &s) { s.th1 = p[0]; s.th2 = p[1]; s.w1 = p[2]; s.w2 = p[3]; }
MZ_HD void pack(const acrobot::State &s, double *p) { p[0] = s.th1; p[1] = s.th2; p[2] = s.w1; p[3] = s.w2; }

// ---- the maze: who looks at which walls -------------------------------------------------------------------------------------------------------
// sense_partial and collide_partial take (w0, stride).  Solo is one caller over every wall (the CPU twin: observe_host's own call); Row16 is
// lane `lane` of a row of 16 over walls lane, lane + 16, ..., combined by maze.h's row_min and row_any.  A minimum and an "any" are exact in
// any order and over any partition of the walls, so the two give the same bits.
struct MazeCtx { maze::Header hdr; const float *walls; int nw; };
struct Solo {
    MZ_HD int w0() const { return 0; }
    MZ_HD int stride() const { return 1; }
    MZ_HD float min(float v) const { return v; }
    MZ_HD bool any(bool b) const { return b; }
};
#if defined(__HIPCC__)
struct Row16 {
    int lane;
    __device__ __forceinline__ int w0() const { return lane; }
    __device__ __forceinline__ int stride() const { return maze::ROW; }
    __device__ __forceinline__ float min(float v) const { return maze::row_min(v); }
    __device__ __forceinline__ bool any(bool b) const { return maze::row_any(b); }
};
#endif

// ---- observe ------------------------------------------------------------------------------------------------------------------------------
template <class R>
MZ_HD void observe(const maze::State &s, const MazeCtx &c, const maze::SinCosF *dir, const R &r, float *obs) {
    float range[6], radar[4];
    for (int i = 0; i < 6; i++) range[i] = maze::RF_RANGE;
    maze::sense_partial(s, maze::sincos_f(maze::to_rad_f(s.heading)), dir, c.walls, r.w0(), r.stride(), c.nw, range);
    for (int i = 0; i < 6; i++) range[i] = r.min(range[i]);
    maze::radar_bits(s, c.hdr, radar);
    maze::make_obs(range, radar, obs);
}
MZ_HD void observe(const cartpole::State &s, float *obs) { cartpole::make_obs(s, obs); }
MZ_HD void observe(const pendulum::State &s, float *obs) {
    const pendulum::Seen v = pendulum::look(s);
    for (int i = 0; i < pendulum::OBS; i++) obs[i] = v.ob[i];
}
MZ_HD void observe(const acrobot::State &s, float *obs) { acrobot::make_obs(s, obs); }

// ---- advance: one step of one environment -----------------------------------------------------------------------------------------------------
// (state, steps, limit, done, action) -> (state, steps, done, reward, observation).  Returns false for an environment that was done already:
// the reward is 0 and nothing else was touched (obs included), so the caller writes nothing back.
template <class R>
MZ_HD bool advance(maze::State &s, int &steps, int limit, int &done, const float *a, const MazeCtx &c, const maze::SinCosF *dir, const R &r,
                   float &reward, float *obs) {
    reward = 0.0f;
    if (done) return false;
    float nx, ny;
    maze::interpret_outputs(s, a[0], a[1]);
    maze::propose_move(s, &nx, &ny);
    maze::commit_move(s, c.hdr, nx, ny, r.any(maze::collide_partial(nx, ny, c.walls, r.w0(), r.stride(), c.nw)));
    observe(s, c, dir, r, obs);
    steps++;
    if (steps == maze::EPISODE_STEPS) reward = maze::final_reward(s, c.hdr);
    done = steps >= limit;
    return true;
}
MZ_HD bool advance(cartpole::State &s, int &steps, int limit, int &done, int a, float &reward, float *obs) {
    reward = 0.0f;
    if (done) return false;
    const bool over = cartpole::step(s, a);
    steps++;
    reward = 1.0f;
    done = over || steps >= limit;
    observe(s, obs);
    return true;
}
MZ_HD bool advance(pendulum::State &s, int &steps, int limit, int &done, float a, float &reward, float *obs) {
    reward = 0.0f;
    if (done) return false;
    reward = pendulum::step(s, pendulum::look(s), a);
    steps++;
    done = steps >= limit;
    observe(s, obs);
    return true;
}
MZ_HD bool advance(acrobot::State &s, int &steps, int limit, int &done, int a, float &reward, float *obs) {
    reward = 0.0f;
    if (done) return false;
    const bool over = acrobot::step(s, a);
    steps++;
    reward = over ? 0.0f : -1.0f;
    done = over || steps >= limit;
    observe(s, obs);
    return true;
}

// ---- the CPU twins: n environments in arrays of exactly their size -------------------------------------------------------------------------------
// state [n][S], steps [n], limit [n], done [n], obs [n][OBS]; mz for the maze only.  Return 0, -1 for a kind that has no environment here,
// -2 for a cart-pole action outside {0, 1} or an acrobot action outside {0, 1, 2} (checked for all n before anything moves).
inline int observe_host(int kind, int n, const double *state, const MazeCtx *mz, float *obs) {
    if (kind == KIND_MAZE) {
        maze::SinCosF dir[6];
        maze::rangefinder_dirs(dir);
        for (int i = 0; i < n; i++) { maze::State s; unpack(state + (size_t)i * 7, s); observe(s, *mz, dir, Solo(), obs + (size_t)i * maze::OBS); }
    } else if (kind == KIND_CARTPOLE) {
        for (int i = 0; i < n; i++) { cartpole::State s; unpack(state + (size_t)i * 4, s); observe(s, obs + (size_t)i * cartpole::OBS); }
    } else if (kind == KIND_PENDULUM) {
        for (int i = 0; i < n; i++) { pendulum::State s; unpack(state + (size_t)i * 2, s); observe(s, obs + (size_t)i * pendulum::OBS); }
    } else if (kind == ENV_ACROBOT) {
        for (int i = 0; i < n; i++) { acrobot::State s; unpack(state + (size_t)i * 4, s); observe(s, obs + (size_t)i * acrobot::OBS); }
    } else return -1;
    return 0;
}

inline int reset_host(int kind, int n, const uint32_t *seeds, const MazeCtx *mz, int max_steps, double *state, int32_t *steps, int32_t *limit,
                      uint8_t *done, float *obs) {
    Dims d;
    if (!dims(kind, &d)) return -1;
    for (int i = 0; i < n; i++) {
        if (kind == KIND_MAZE) pack(maze::reset_state(mz->hdr), state + (size_t)i * 7);
        else if (kind == KIND_CARTPOLE) pack(cartpole::reset_state(seeds[i]), state + (size_t)i * 4);
        else if (kind == KIND_PENDULUM) pack(pendulum::reset_state(seeds[i]), state + (size_t)i * 2);
        else pack(acrobot::reset_state(seeds[i]), state + (size_t)i * 4);
        steps[i] = 0; done[i] = 0; limit[i] = step_limit(max_steps, d.own_limit);
    }
    return observe_host(kind, n, state, mz, obs);
}

inline int step_host(int kind, int n, const void *actions, const MazeCtx *mz, double *state, int32_t *steps, const int32_t *limit, uint8_t *done,
                     float *reward, float *obs) {
    if (kind == KIND_MAZE) {
        const float *a = (const float *)actions;
        maze::SinCosF dir[6];
        maze::rangefinder_dirs(dir);
        for (int i = 0; i < n; i++) {
            maze::State s; unpack(state + (size_t)i * 7, s);
            int t = steps[i], dn = done[i];
            float o[maze::OBS];
            if (advance(s, t, limit[i], dn, a + 2 * (size_t)i, *mz, dir, Solo(), reward[i], o)) {
                pack(s, state + (size_t)i * 7); steps[i] = t; done[i] = (uint8_t)dn;
                for (int k = 0; k < maze::OBS; k++) obs[(size_t)i * maze::OBS + k] = o[k];
            }
        }
    } else if (kind == KIND_CARTPOLE) {
        const int32_t *a = (const int32_t *)actions;
        for (int i = 0; i < n; i++) if (a[i] != 0 && a[i] != 1) return -2;
        for (int i = 0; i < n; i++) {
            cartpole::State s; unpack(state + (size_t)i * 4, s);
            int t = steps[i], dn = done[i];
            float o[cartpole::OBS];
            if (advance(s, t, limit[i], dn, (int)a[i], reward[i], o)) {
                pack(s, state + (size_t)i * 4); steps[i] = t; done[i] = (uint8_t)dn;
                for (int k = 0; k < cartpole::OBS; k++) obs[(size_t)i * cartpole::OBS + k] = o[k];
            }
        }
    } else if (kind == KIND_PENDULUM) {
        const float *a = (const float *)actions;
        for (int i = 0; i < n; i++) {
            pendulum::State s; unpack(state + (size_t)i * 2, s);
            int t = steps[i], dn = done[i];
            float o[pendulum::OBS];
            if (advance(s, t, limit[i], dn, a[i], reward[i], o)) {
                pack(s, state + (size_t)i * 2); steps[i] = t; done[i] = (uint8_t)dn;
                for (int k = 0; k < pendulum::OBS; k++) obs[(size_t)i * pendulum::OBS + k] = o[k];
            }
        }
    } else if (kind == ENV_ACROBOT) {
        const int32_t *a = (const int32_t *)actions;
        for (int i = 0; i < n; i++) if (a[i] < 0 || a[i] > 2) return -2;
        for (int i = 0; i < n; i++) {
            acrobot::State s; unpack(state + (size_t)i * 4, s);
            int t = steps[i], dn = done[i];
            float o[acrobot::OBS];
            if (advance(s, t, limit[i], dn, (int)a[i], reward[i], o)) {
                pack(s, state + (size_t)i * 4); steps[i] = t; done[i] = (uint8_t)dn;
                for (int k = 0; k < acrobot::OBS; k++) obs[(size_t)i * acrobot::OBS + k] = o[k];
            }
        }
    } else return -1;
    return 0;
}

#if defined(__HIPCC__)
// ---- the device side: one launch per call ------------------------------------------------------------------------------------------------------
// The batch lives in five arrays over the engine's max_members environments.  Every kernel takes the index list idx [n] (distinct, each in
// range: the engine checks both before it launches) and touches the environments it names, nothing else; its per-call inputs and outputs are
// arrays [n] in the order of the list.
struct Batch { double *state; int32_t *steps, *limit; uint8_t *done; float *obs; };

// The maze: a row of 16 lanes per environment, four environments per wave, one wave per workgroup, the walls staged in LDS and dealt over the
// row's lanes as k_maze_rollout deals them; the rangefinder minima and the collision test are row-wide combines (Row16: exact whatever the
// partition).  The navigator's state is kept redundantly by the 16 lanes, lane 0 writes.  A partial last wave: the spare rows shadow the
// list's last environment -- they load what its own row loads (the same wave, before any store) -- and write nothing.
// init != null: the states [n][7] and steps [n] of dne_stepenv_set_state instead of the reset.
__global__ __launch_bounds__(64) void k_stepenv_reset_maze(const Batch B, const MazeCtx C, const int32_t *idx, int n, const double *init,
                                                           const int32_t *init_steps, int limit) {
    __shared__ float s_walls[maze::MAX_WALLS * 4];
    for (int i = threadIdx.x; i < C.nw * 4; i += 64) s_walls[i] = C.walls[i];
    __syncthreads();
    const int lane = threadIdx.x & (maze::ROW - 1), row = threadIdx.x / maze::ROW;
    int k = blockIdx.x * 4 + row;
    const bool live = k < n;
    if (!live) k = n - 1;
    const int e = idx[k];
    MazeCtx c = C;
    c.walls = s_walls;
    maze::SinCosF dir[6];
    maze::rangefinder_dirs(dir);
    maze::State s = maze::reset_state(c.hdr);
    if (init) unpack(init + (size_t)k * 7, s);
    float obs[maze::OBS];
    observe(s, c, dir, Row16{lane}, obs);
    if (lane == 0 && live) {
        pack(s, B.state + (size_t)e * 7);
        B.steps[e] = init ? init_steps[k] : 0; B.limit[e] = limit; B.done[e] = 0;
#pragma unroll
        for (int i = 0; i < maze::OBS; i++) B.obs[(size_t)e * maze::OBS + i] = obs[i];
    }
}

__global__ __launch_bounds__(64) void k_stepenv_step_maze(const Batch B, const MazeCtx C, const int32_t *idx, int n, const float *act, float *reward,
                                                          uint8_t *done_out) {
    __shared__ float s_walls[maze::MAX_WALLS * 4];
    for (int i = threadIdx.x; i < C.nw * 4; i += 64) s_walls[i] = C.walls[i];
    __syncthreads();
    const int lane = threadIdx.x & (maze::ROW - 1), row = threadIdx.x / maze::ROW;
    int k = blockIdx.x * 4 + row;
    const bool live = k < n;
    if (!live) k = n - 1;
    const int e = idx[k];
    MazeCtx c = C;
    c.walls = s_walls;
    maze::SinCosF dir[6];
    maze::rangefinder_dirs(dir);
    maze::State s;
    unpack(B.state + (size_t)e * 7, s);
    int steps = B.steps[e], done = B.done[e];
    const int limit = B.limit[e];
    const float a[2] = {act[2 * (size_t)k], act[2 * (size_t)k + 1]};
    float obs[maze::OBS], r;
    // done is the row's own (its 16 lanes hold the same values), so a row skips the step as a whole: the shuffles inside have width ROW
    const bool moved = advance(s, steps, limit, done, a, c, dir, Row16{lane}, r, obs);
    if (lane == 0 && live) {
        if (moved) {
            pack(s, B.state + (size_t)e * 7);
            B.steps[e] = steps; B.done[e] = (uint8_t)done;
#pragma unroll
            for (int i = 0; i < maze::OBS; i++) B.obs[(size_t)e * maze::OBS + i] = obs[i];
        }
        reward[k] = r; done_out[k] = (uint8_t)done;
    }
}

// The cart-pole, the pendulum and the acrobot: one lane per environment, 64-thread workgroups.
__global__ __launch_bounds__(64) void k_stepenv_reset_cartpole(const Batch B, const int32_t *idx, int n, const uint32_t *seeds, const double *init,
                                                               const int32_t *init_steps, int limit) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int e = idx[k];
    cartpole::State s;
    if (init) unpack(init + (size_t)k * 4, s); else s = cartpole::reset_state(seeds[k]);
    pack(s, B.state + (size_t)e * 4);
    B.steps[e] = init ? init_steps[k] : 0; B.limit[e] = limit; B.done[e] = 0;
    observe(s, B.obs + (size_t)e * cartpole::OBS);
}

__global__ __launch_bounds__(64) void k_stepenv_step_cartpole(const Batch B, const int32_t *idx, int n, const int32_t *act, float *reward,
                                                              uint8_t *done_out) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int e = idx[k];
    cartpole::State s;
    unpack(B.state + (size_t)e * 4, s);
    int steps = B.steps[e], done = B.done[e];
    float obs[cartpole::OBS], r;
    if (advance(s, steps, B.limit[e], done, (int)act[k], r, obs)) {
        pack(s, B.state + (size_t)e * 4);
        B.steps[e] = steps; B.done[e] = (uint8_t)done;
#pragma unroll
        for (int i = 0; i < cartpole::OBS; i++) B.obs[(size_t)e * cartpole::OBS + i] = obs[i];
    }
    reward[k] = r; done_out[k] = (uint8_t)done;
}

__global__ __launch_bounds__(64) void k_stepenv_reset_pendulum(const Batch B, const int32_t *idx, int n, const uint32_t *seeds, const double *init,
                                                               const int32_t *init_steps, int limit) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int e = idx[k];
    pendulum::State s;
    if (init) unpack(init + (size_t)k * 2, s); else s = pendulum::reset_state(seeds[k]);
    pack(s, B.state + (size_t)e * 2);
    B.steps[e] = init ? init_steps[k] : 0; B.limit[e] = limit; B.done[e] = 0;
    observe(s, B.obs + (size_t)e * pendulum::OBS);
}

__global__ __launch_bounds__(64) void k_stepenv_step_pendulum(const Batch B, const int32_t *idx, int n, const float *act, float *reward,
                                                              uint8_t *done_out) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int e = idx[k];
    pendulum::State s;
    unpack(B.state + (size_t)e * 2, s);
    int steps = B.steps[e], done = B.done[e];
    float obs[pendulum::OBS], r;
    if (advance(s, steps, B.limit[e], done, act[k], r, obs)) {
        pack(s, B.state + (size_t)e * 2);
        B.steps[e] = steps; B.done[e] = (uint8_t)done;
#pragma unroll
        for (int i = 0; i < pendulum::OBS; i++) B.obs[(size_t)e * pendulum::OBS + i] = obs[i];
    }
    reward[k] = r; done_out[k] = (uint8_t)done;
}

__global__ __launch_bounds__(64) void k_stepenv_reset_acrobot(const Batch B, const int32_t *idx, int n, const uint32_t *seeds, const double *init,
                                                              const int32_t *init_steps, int limit) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int e = idx[k];
    acrobot::State s;
    if (init) unpack(init + (size_t)k * 4, s); else s = acrobot::reset_state(seeds[k]);
    pack(s, B.state + (size_t)e * 4);
    B.steps[e] = init ? init_steps[k] : 0; B.limit[e] = limit; B.done[e] = 0;
    observe(s, B.obs + (size_t)e * acrobot::OBS);
}

__global__ __launch_bounds__(64) void k_stepenv_step_acrobot(const Batch B, const int32_t *idx, int n, const int32_t *act, float *reward,
                                                             uint8_t *done_out) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int e = idx[k];
    acrobot::State s;
    unpack(B.state + (size_t)e * 4, s);
    int steps = B.steps[e], done = B.done[e];
    float obs[acrobot::OBS], r;
    if (advance(s, steps, B.limit[e], done, (int)act[k], r, obs)) {
        pack(s, B.state + (size_t)e * 4);
        B.steps[e] = steps; B.done[e] = (uint8_t)done;
#pragma unroll
        for (int i = 0; i < acrobot::OBS; i++) B.obs[(size_t)e * acrobot::OBS + i] = obs[i];
    }
    reward[k] = r; done_out[k] = (uint8_t)done;
}

// observations and state of the listed environments, packed in the order of the list; an output that is null is not written
__global__ __launch_bounds__(64) void k_stepenv_gather(const Batch B, int S, int OBS, const int32_t *idx, int n, float *obs, double *state,
                                                       int32_t *steps, uint8_t *done) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int e = idx[k];
    if (obs) for (int i = 0; i < OBS; i++) obs[(size_t)k * OBS + i] = B.obs[(size_t)e * OBS + i];
    if (state) for (int i = 0; i < S; i++) state[(size_t)k * S + i] = B.state[(size_t)e * S + i];
    if (steps) steps[k] = B.steps[e];
    if (done) done[k] = B.done[e];
}
#endif

}  // namespace stepenv
}  // namespace dne
