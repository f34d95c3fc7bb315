// maze.h -- the GPU tree's hard maze (gym_tensorflow/maze/maze.h, tf_maze.cpp, tf_maze.py) and its policy (models/simple.py:29-35 over
// dqn.Model: dense 11 -> 16, relu, dense 16 -> 16, relu, dense 16 -> 2) restated as ONE __host__ __device__ text: the step, the sensors and the
// forward pass below compile for the CPU (dne_maze_rollout_host, the feature's oracle) and for gfx950 (k_maze_rollout: whole episodes in one
// launch), and the two agree bit for bit.  DESIGN.md section 12 holds the contract; what makes the agreement possible:
//   * no libm transcendental: sincos_d / atan_d are explicit fma() chains over IEEE double operations, the float versions evaluate in
//     double and round once; sqrtf and every division are the IEEE operations (correctly rounded on both sides);
//   * -ffp-contract=off on both passes (csrc/Makefile): a fused operation exists only where fma() / fmaf() is written;
//   * every reduction over walls is a minimum or an "any": exact in any order, so dealing walls over lanes cannot change a bit.
// The reference's promotions are part of the contract (its maze.h mixes float state with double literals); each is spelled out where it
// happens, by a cast.  A plain C++ compiler can include this file (the kernel is behind __HIPCC__): tests/maze_asan_main.cpp does.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MZ_HD __host__ __device__ __forceinline__
#else
#define MZ_HD inline
#endif

namespace dne {
namespace maze {

constexpr int OBS = 11, HID = 16, ACT = 2, NPARAMS = 498, MAX_WALLS = 64, EPISODE_STEPS = 400 /* tf_maze.cpp:90-93 */, TRACE_W = 16, ROW = 16;
// flat order = creation order (models/base.py:35-44): fc1/w [11][16], fc1/b, fc2/w [16][16], fc2/b, out/w [16][2], out/b
constexpr int W1 = 0, B1 = 176, W2 = 192, B2 = 448, W3 = 464, B3 = 496;
constexpr double PI_REF = 3.1415926;   // the reference's pi (maze.h:151,166,661,714)
constexpr float RF_RANGE = 100.0f, RADIUS = 8.0f;   // Character(): rangefinder_range, radius

struct SinCosD { double s, c; };
struct SinCosF { float s, c; };
struct Header { float disable, steps, sx, sy, heading, gx, gy, reserved; };   // header8 of the C ABI
struct State { float x, y, heading, speed, ang_vel; int collide, collisions; };

// ---- trigonometry ---------------------------------------------------------------------------------------------------------------------
// sin and cos of |x| <= 3 pi: k = round(x * 2 / pi), r = x - k * pi/2 in two fma steps (the first product is exact: PIO2_HI keeps 33 bits and
// |k| <= 6), then the Taylor series of sin and cos on |r| <= pi/4 (truncation below 1e-19 and 3e-18), Horner in fma.
// Outside the contract (a NaN heading after a NaN action, an infinity) k is 0 and the result is NaN through r: a NaN or an infinity is never
// cast to int, which C++ leaves undefined and on which x86 (INT_MIN) and gfx950 (0, saturation) answer differently.
MZ_HD SinCosD sincos_d(double x) {
    const double PIO2_HI = 1.57079632673412561417e+00, PIO2_LO = 6.07710050650619224932e-11;
    const double t = x * 6.36619772367581382433e-01;
    const int k = fabs(t) < 7.0 ? (int)(t + (t < 0.0 ? -0.5 : 0.5)) : 0;
    const double kd = (double)k;
    double r = fma(-kd, PIO2_HI, x);
    r = fma(-kd, PIO2_LO, r);
    const double z = r * r;
    double ps = -1.0 / 1307674368000.0;          // -1/15!
    ps = fma(ps, z, 1.0 / 6227020800.0);         // +1/13!
    ps = fma(ps, z, -1.0 / 39916800.0);          // -1/11!
    ps = fma(ps, z, 1.0 / 362880.0);             // +1/9!
    ps = fma(ps, z, -1.0 / 5040.0);              // -1/7!
    ps = fma(ps, z, 1.0 / 120.0);                // +1/5!
    ps = fma(ps, z, -1.0 / 6.0);                 // -1/3!
    const double sr = fma(r * z, ps, r);
    double pc = 1.0 / 20922789888000.0;          // +1/16!
    pc = fma(pc, z, -1.0 / 87178291200.0);       // -1/14!
    pc = fma(pc, z, 1.0 / 479001600.0);          // +1/12!
    pc = fma(pc, z, -1.0 / 3628800.0);           // -1/10!
    pc = fma(pc, z, 1.0 / 40320.0);              // +1/8!
    pc = fma(pc, z, -1.0 / 720.0);               // -1/6!
    pc = fma(pc, z, 1.0 / 24.0);                 // +1/4!
    pc = fma(pc, z, -0.5);                       // -1/2!
    const double cr = fma(pc, z, 1.0);
    SinCosD o;
    switch (k & 3) {
    case 0: o.s = sr; o.c = cr; break;
    case 1: o.s = cr; o.c = -sr; break;
    case 2: o.s = -sr; o.c = -cr; break;
    default: o.s = -cr; o.c = sr; break;
    }
    return o;
}

// the float functions: evaluated in double, rounded once
MZ_HD SinCosF sincos_f(float x) {
    const SinCosD d = sincos_d((double)x);
    SinCosF o;
    o.s = (float)d.s; o.c = (float)d.c;
    return o;
}

// atan over the whole line: the classic reduction to |x| < 7/16 around atan(1/2), atan(1), atan(3/2), atan(inf) (each constant as a
// high and a low part) and an odd minimax polynomial in two interleaved fma chains
MZ_HD double atan_d(double t) {
    const double ax = t < 0.0 ? -t : t;
    double x, hi = 0.0, lo = 0.0;
    bool reduced = true;
    if (ax < 0.4375) { x = ax; reduced = false; }
    else if (ax < 0.6875) { x = (2.0 * ax - 1.0) / (2.0 + ax); hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17; }
    else if (ax < 1.1875) { x = (ax - 1.0) / (ax + 1.0); hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17; }
    else if (ax < 2.4375) { x = (ax - 1.5) / (1.0 + 1.5 * ax); hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17; }
    else { x = -1.0 / ax; hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17; }
    const double z = x * x, w = z * z;
    double s1 = 1.62858201153657823623e-02;
    s1 = fma(s1, w, 4.97687799461593236017e-02);
    s1 = fma(s1, w, 6.66107313738753120669e-02);
    s1 = fma(s1, w, 9.09088713343650656196e-02);
    s1 = fma(s1, w, 1.42857142725034663711e-01);
    s1 = fma(s1, w, 3.33333333333329318027e-01);
    s1 = z * s1;
    double s2 = -3.65315727442169155270e-02;
    s2 = fma(s2, w, -5.83357013379057348645e-02);
    s2 = fma(s2, w, -7.69187620504482999495e-02);
    s2 = fma(s2, w, -1.11111104054623557880e-01);
    s2 = fma(s2, w, -1.99999999998764832476e-01);
    s2 = w * s2;
    const double corr = x * (s1 + s2);
    const double r = reduced ? hi - ((corr - lo) - x) : x - corr;
    return t < 0.0 ? -r : r;
}
MZ_HD float atan_f(float t) { return (float)atan_d((double)t); }
// `float ang=atan(y/x)/3.1415926*180.0` (maze.h:151) from the quotient: float atan, double quotient and product, rounded on assignment
MZ_HD float quotient_angle_f(float q) { return (float)((double)atan_f(q) / PI_REF * 180.0); }

// `float rad = angle/180.0*3.1415926` (maze.h:166, 714): the quotient and the product are double, the assignment rounds
MZ_HD float to_rad_f(float angle) { return (float)((double)angle / 180.0 * PI_REF); }

// ---- sensors --------------------------------------------------------------------------------------------------------------------------
// Point::distance (maze.h:179-184): float throughout, sqrt on a float is the float function
MZ_HD float dist_f(float ax, float ay, float bx, float by) {
    const float dx = bx - ax, dy = by - ay;
    return sqrtf(dx * dx + dy * dy);
}

// cos / sin of the six rangefinder angles (Character(): -90, -45, 0, 45, 90, -180), constant over an episode
MZ_HD void rangefinder_dirs(SinCosF *dir) {
    const float ang[6] = {-90.0f, -45.0f, 0.0f, 45.0f, 90.0f, -180.0f};
    for (int i = 0; i < 6; i++) dir[i] = sincos_f(to_rad_f(ang[i]));
}

// update_rangefinders (maze.h:709-747) over walls w0, w0 + stride, ...: range[i] comes in as the best so far (100 at the start) and leaves as
// the minimum over these walls too.  hd = sincos_f(to_rad_f(heading)): Point::rotate's rad, the same for the six sensors.  The walls are the
// outer loop and the six sensors the inner one (a minimum does not care), so that six independent chains are in flight per wall.
MZ_HD void sense_partial(const State &s, SinCosF hd, const SinCosF *dir, const float *walls, int w0, int stride, int n, float *range) {
    float px[6], py[6];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; i++) {
        // proj_point(location.x + cos(rad) * range, location.y + sin(rad) * range): float products and sums, unfused
        float x = s.x + dir[i].c * RF_RANGE, y = s.y + dir[i].s * RF_RANGE;
        // proj_point.rotate(heading, location) (maze.h:164-177)
        x -= s.x; y -= s.y;
        const float ox = x, oy = y;
        x = hd.c * ox - hd.s * oy;
        y = hd.s * ox + hd.c * oy;
        px[i] = x + s.x; py[i] = y + s.y;
    }
    const float cx = s.x, cy = s.y;
    for (int w = w0; w < n; w += stride) {
        // lines[j]->intersection(projected_line) (maze.h:218-261): A, B the wall, C the navigator, D the projected point
        const float ax = walls[4 * w], ay = walls[4 * w + 1], bx = walls[4 * w + 2], by = walls[4 * w + 3];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 6; i++) {
            const float rtop = (ay - cy) * (px[i] - cx) - (ax - cx) * (py[i] - cy);
            const float rbot = (bx - ax) * (py[i] - cy) - (by - ay) * (px[i] - cx);
            const float stop = (ay - cy) * (bx - ax) - (ax - cx) * (by - ay);
            if (rbot == 0.0f) continue;                     // (sBot is the same expression)
            const float r = rtop / rbot, q = stop / rbot;
            if (r > 0.0f && r < 1.0f && q > 0.0f && q < 1.0f) {
                const float ix = ax + r * (bx - ax), iy = ay + r * (by - ay);
                const float found = dist_f(ix, iy, s.x, s.y);       // intersection.distance(h.location)
                if (found < range[i]) range[i] = found;
            }
        }
    }
}

// collide_lines (maze.h:694-702) over walls w0, w0 + stride, ...: Line::distance (maze.h:264-287) < radius for any of them
MZ_HD bool collide_partial(float nx, float ny, const float *walls, int w0, int stride, int n) {
    bool hit = false;
    for (int w = w0; w < n; w += stride) {
        const float ax = walls[4 * w], ay = walls[4 * w + 1], bx = walls[4 * w + 2], by = walls[4 * w + 3];
        const float utop = (nx - ax) * (bx - ax) + (ny - ay) * (by - ay);
        float ubot = dist_f(ax, ay, bx, by);
        ubot *= ubot;
        float d;
        if (ubot == 0.0f) d = 0.0f;
        else {
            const float u = utop / ubot;
            if (u < 0.0f || u > 1.0f) {
                const float d1 = dist_f(ax, ay, nx, ny), d2 = dist_f(bx, by, nx, ny);
                d = d1 < d2 ? d1 : d2;
            } else {
                const float qx = ax + u * (bx - ax), qy = ay + u * (by - ay);
                d = dist_f(qx, qy, nx, ny);
            }
        }
        hit = hit || d < RADIUS;
    }
    return hit;
}

// update_radar_gen for the goal (maze.h:761-795) + Point::angle (maze.h:144-161); the poi radar is computed by the reference and never observed
MZ_HD void radar_bits(const State &s, const Header &m, float *radar) {
    const SinCosF t = sincos_f(to_rad_f(-s.heading));       // target.rotate(-h.heading, h.location)
    float tx = m.gx - s.x, ty = m.gy - s.y;
    const float ox = tx, oy = ty;
    tx = t.c * ox - t.s * oy;
    ty = t.s * ox + t.c * oy;
    tx += s.x; ty += s.y;
    tx -= s.x; ty -= s.y;                                   // (maze.h:778-779: the sum and the difference each round)
    float angle;
    if (tx == 0.0f) angle = ty > 0.0f ? 90.0f : 270.0f;
    else {
        const float ang = quotient_angle_f(ty / tx);
        angle = tx > 0.0f ? ang : (float)((double)ang + 180.0);
    }
    const float a1[4] = {315.0f, 45.0f, 135.0f, 225.0f}, a2[4] = {405.0f, 135.0f, 225.0f, 315.0f};
    for (int i = 0; i < 4; i++) {
        float v = 0.0f;
        if (angle >= a1[i] && angle < a2[i]) v = 1.0f;
        const double wrapped = (double)angle + 360.0;       // `angle+360.0` is a double
        if (wrapped >= (double)a1[i] && wrapped < (double)a2[i]) v = 1.0f;
        radar[i] = v;
    }
}

// generate_neural_inputs (maze.h:553-601): bias, six rangefinders / 100, four goal-radar bits
MZ_HD void make_obs(const float *range, const float *radar, float *obs) {
    obs[0] = 1.0f;
    for (int i = 0; i < 6; i++) obs[1 + i] = range[i] / RF_RANGE;
    for (int i = 0; i < 4; i++) obs[7 + i] = radar[i];
}

// ---- the step --------------------------------------------------------------------------------------------------------------------------
// Character::reset + Environment::reset (maze.h:321-331, 460-466): the heading restarts at 0 whatever the file said
MZ_HD State reset_state(const Header &m) {
    State s;
    s.x = m.sx; s.y = m.sy; s.heading = 0.0f; s.speed = 0.0f; s.ang_vel = 0.0f; s.collide = 0; s.collisions = 0;
    return s;
}

MZ_HD float clamp_rate(float d) {   // `if(d>=0.2) d=0.2; if(d<=-0.2) d=-0.2;`: a float compared with the double 0.2, then 0.2 rounded to float
    if ((double)d >= 0.2) d = (float)0.2;
    if ((double)d <= -0.2) d = (float)-0.2;
    return d;
}

// tf_maze.cpp:80 `interpret_outputs(float(action[0]) + 0.5, 0.5 + float(action[1]))`: double sums rounded into the float parameters, then maze.h:604-654
MZ_HD void interpret_outputs(State &s, float a0, float a1) {
    float o1 = (float)((double)a0 + 0.5), o2 = (float)(0.5 + (double)a1);
    if (o1 > 1.0f) o1 = 1.0f;
    if (o1 < 0.0f) o1 = 0.0f;
    if (o2 > 1.0f) o2 = 1.0f;
    if (o2 < 0.0f) o2 = 0.0f;
    const float new_ang_vel = (float)(((double)o1 - 0.5) * 6.0), new_speed = (float)(((double)o2 - 0.5) * 6.0);
    s.ang_vel += clamp_rate(new_ang_vel - s.ang_vel);
    s.speed += clamp_rate(new_speed - s.speed);
    if (s.speed > 3.0f) s.speed = 3.0f;
    if (s.speed < -3.0f) s.speed = -3.0f;
    if (s.ang_vel > 3.0f) s.ang_vel = 3.0f;
    if (s.ang_vel < -3.0f) s.ang_vel = -3.0f;
}

// Update() up to the collision test (maze.h:657-675): `cos(hero.heading/180.0*3.1415926)*hero.speed` is double trig on a double argument whose
// product with the (promoted) speed rounds to float; the heading turns and wraps in float
MZ_HD void propose_move(State &s, float *nx, float *ny) {
    const SinCosD h = sincos_d((double)s.heading / 180.0 * PI_REF);
    const float vx = (float)(h.c * (double)s.speed), vy = (float)(h.s * (double)s.speed);
    s.heading += s.ang_vel;
    if (s.heading > 360.0f) s.heading -= 360.0f;
    if (s.heading < 0.0f) s.heading += 360.0f;
    *nx = vx + s.x; *ny = vy + s.y;
}

// the rest of Update() (maze.h:677-688); `disable` freezes the navigator after its first collision
MZ_HD void commit_move(State &s, const Header &m, float nx, float ny, bool hit) {
    if (!s.collide && !hit) { s.x = nx; s.y = ny; }
    else {
        s.collisions++;
        if (m.disable != 0.0f) s.collide = 1;
    }
}

// tf_maze.cpp:83-87: 0 until the episode's last step, then -distance_to_target() (maze.h:514-531)
MZ_HD float final_reward(const State &s, const Header &m) {
    float d = dist_f(s.x, s.y, m.gx, m.gy);
    if (d != d) d = 500.0f;
    return -d;
}

// ---- the policy ------------------------------------------------------------------------------------------------------------------------
// theta_p = base_p + fl(scale * noise_p): two roundings (the oracle's orc_perturb)
MZ_HD float perturbed(float base, float scale, float eps) {
    const float v = scale * eps;
    return base + v;
}

// one output unit of a dense layer: a fmaf chain over k ascending from +0.0f, then + b (the tree's convention for every small dense layer)
template <int N>
MZ_HD float dense_unit(const float *in, const float *w, int wstride, float b) {
    float acc = 0.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < N; k++) acc = fmaf(in[k], w[k * wstride], acc);
    return acc + b;
}
MZ_HD float relu(float v) { return v > 0.0f ? v : 0.0f; }

MZ_HD void write_trace(float *row, const float *obs, const State &s) {
    for (int i = 0; i < OBS; i++) row[i] = obs[i];
    row[11] = s.x; row[12] = s.y; row[13] = s.heading; row[14] = s.speed; row[15] = s.ang_vel;
}

// ---- the CPU side: one episode of one theta ------------------------------------------------------------------------------------------------
// trace (may be null): [steps][16] = the observation AFTER each step (what the policy sees next), then x, y, heading, speed, ang_vel
inline void observe_host(const State &s, const Header &m, const SinCosF *dir, const float *walls, int nw, float *obs) {
    float range[6], radar[4];
    for (int i = 0; i < 6; i++) range[i] = RF_RANGE;
    sense_partial(s, sincos_f(to_rad_f(s.heading)), dir, walls, 0, 1, nw, range);
    radar_bits(s, m, radar);
    make_obs(range, radar, obs);
}

inline void step_host(State &s, const Header &m, const SinCosF *dir, const float *walls, int nw, float a0, float a1, float *obs) {
    float nx, ny;
    interpret_outputs(s, a0, a1);
    propose_move(s, &nx, &ny);
    commit_move(s, m, nx, ny, collide_partial(nx, ny, walls, 0, 1, nw));
    observe_host(s, m, dir, walls, nw, obs);
}

inline void rollout_host(const float *theta, const Header &m, const float *walls, int nw, int tslimit, float *ret, int32_t *len, float *xy,
                         float *trace) {
    SinCosF dir[6];
    rangefinder_dirs(dir);
    State s = reset_state(m);
    float obs[OBS], h1[HID], h2[HID], out[ACT];
    observe_host(s, m, dir, walls, nw, obs);
    const int steps = tslimit < EPISODE_STEPS ? tslimit : EPISODE_STEPS;
    for (int t = 0; t < steps; t++) {
        for (int j = 0; j < HID; j++) h1[j] = relu(dense_unit<OBS>(obs, theta + W1 + j, HID, theta[B1 + j]));
        for (int j = 0; j < HID; j++) h2[j] = relu(dense_unit<HID>(h1, theta + W2 + j, HID, theta[B2 + j]));
        for (int j = 0; j < ACT; j++) out[j] = dense_unit<HID>(h2, theta + W3 + j, ACT, theta[B3 + j]);
        step_host(s, m, dir, walls, nw, out[0], out[1], obs);
        if (trace) write_trace(trace + (size_t)t * TRACE_W, obs, s);
    }
    *ret = 0.0f + (steps == EPISODE_STEPS ? final_reward(s, m) : 0.0f);
    *len = steps;
    xy[0] = s.x; xy[1] = s.y;
}

// the forward pass alone (tests): out[2] and the two hidden layers after their relus
inline void forward_host(const float *theta, const float *obs, float *h1, float *h2, float *out) {
    for (int j = 0; j < HID; j++) h1[j] = relu(dense_unit<OBS>(obs, theta + W1 + j, HID, theta[B1 + j]));
    for (int j = 0; j < HID; j++) h2[j] = relu(dense_unit<HID>(h1, theta + W2 + j, HID, theta[B2 + j]));
    for (int j = 0; j < ACT; j++) out[j] = dense_unit<HID>(h2, theta + W3 + j, ACT, theta[B3 + j]);
}

// open-loop: the environment alone under given actions (the recording of the reference's own maze.h is compared against this).
// rows [T][18]: obs[11], x, y, heading, speed, ang_vel, collisions, reward -- all after the step; obs0 [11]: the observation after reset
inline void actions_host(const float *actions, int T, const Header &m, const float *walls, int nw, float *rows, float *obs0) {
    SinCosF dir[6];
    rangefinder_dirs(dir);
    State s = reset_state(m);
    float obs[OBS];
    observe_host(s, m, dir, walls, nw, obs);
    if (obs0) for (int i = 0; i < OBS; i++) obs0[i] = obs[i];
    for (int t = 0; t < T; t++) {
        step_host(s, m, dir, walls, nw, actions[2 * t], actions[2 * t + 1], obs);
        float *row = rows + (size_t)t * 18;
        write_trace(row, obs, s);
        row[16] = (float)s.collisions;
        row[17] = t + 1 >= EPISODE_STEPS ? final_reward(s, m) : 0.0f;
    }
}

// ---- the math probe (tests): the trigonometry outside an episode, on both sides ------------------------------------------------------------
// fn: 0 sincos_d(x) -> (sin, cos); 1 atan_d(x) -> (atan, 0); 2 (float)x degrees -> to_rad_f -> sincos_f -> (sin, cos);
// 3 (float)x = ty / tx -> the goal's angle in degrees as radar_bits forms it -> (tx > 0, tx < 0).  Values travel as doubles, out [2] per input.
constexpr int MATH_FNS = 4;
MZ_HD void math_probe(int fn, double x, double *out) {
    if (fn == 0) { const SinCosD r = sincos_d(x); out[0] = r.s; out[1] = r.c; }
    else if (fn == 1) { out[0] = atan_d(x); out[1] = 0.0; }
    else if (fn == 2) { const SinCosF r = sincos_f(to_rad_f((float)x)); out[0] = (double)r.s; out[1] = (double)r.c; }
    else { const float ang = quotient_angle_f((float)x); out[0] = (double)ang; out[1] = (double)(float)((double)ang + 180.0); }
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void k_maze_math(int fn, const double *x, int n, double *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) math_probe(fn, x[i], out + 2 * (size_t)i);
}

// ---- the device side: whole episodes in one launch ------------------------------------------------------------------------------------------
// 16 lanes (one DPP row) per member, four members per wave, one wave per workgroup.  Lane j owns hidden unit j of fc1 and of fc2 -- its
// weight columns are built once from base slot and noise table and stay in registers -- and output unit j & 1; activations travel inside
// the row.  Walls are staged in LDS once and dealt over the row's lanes; every rangefinder minimum and the collision test are row-wide
// reductions.  The navigator's state is kept redundantly by all 16 lanes (the same operations on the same values).  Between steps nothing
// touches global memory unless behaviour (bc) or a trace is recorded.
__device__ __forceinline__ float row_min(float v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) { const float o = __shfl_xor(v, d, ROW); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ bool row_any(bool b) {
    int v = b ? 1 : 0;
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v |= __shfl_xor(v, d, ROW);
    return v != 0;
}

struct RolloutArgs {
    const float *noise, *bases; size_t base_stride;
    const int32_t *m_slot; const int64_t *m_off; const float *m_scale;
    int first, count;              // members [first, first + count)
    Header hdr; const float *walls; int nw; int tslimit;
    float *ret, *sign; int32_t *len; float *xy;   // per member (null when tracing)
    float *bc; int bc_max_steps;   // [member][bc_max_steps][2]: (x, y) after every step, or null
    float *trace;                  // [steps][16] of member `first` (count == 1), or null
};

__global__ __launch_bounds__(64) void k_maze_rollout(const RolloutArgs A) {
    __shared__ float s_walls[MAX_WALLS * 4];
    for (int i = threadIdx.x; i < A.nw * 4; i += 64) s_walls[i] = A.walls[i];
    __syncthreads();
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

    SinCosF dir[6];
    rangefinder_dirs(dir);
    State s = reset_state(A.hdr);
    float obs[OBS], range[6], radar[4], in[HID];
    auto observe = [&]() {
#pragma unroll
        for (int i = 0; i < 6; i++) range[i] = RF_RANGE;
        sense_partial(s, sincos_f(to_rad_f(s.heading)), dir, s_walls, lane, ROW, A.nw, range);
#pragma unroll
        for (int i = 0; i < 6; i++) range[i] = row_min(range[i]);
        radar_bits(s, A.hdr, radar);
        make_obs(range, radar, obs);
    };
    observe();
    const int steps = A.tslimit < EPISODE_STEPS ? A.tslimit : EPISODE_STEPS;
    for (int t = 0; t < steps; t++) {
        const float h1 = relu(dense_unit<OBS>(obs, w1, 1, b1));
#pragma unroll
        for (int k = 0; k < HID; k++) in[k] = __shfl(h1, k, ROW);
        const float h2 = relu(dense_unit<HID>(in, w2, 1, b2));
#pragma unroll
        for (int k = 0; k < HID; k++) in[k] = __shfl(h2, k, ROW);
        const float out = dense_unit<HID>(in, w3, 1, b3);
        const float a0 = __shfl(out, 0, ROW), a1 = __shfl(out, 1, ROW);
        float nx, ny;
        interpret_outputs(s, a0, a1);
        propose_move(s, &nx, &ny);
        commit_move(s, A.hdr, nx, ny, row_any(collide_partial(nx, ny, s_walls, lane, ROW, A.nw)));
        observe();
        if (lane == 0 && live) {
            if (A.bc && t < A.bc_max_steps) { float *p = A.bc + ((size_t)m * A.bc_max_steps + t) * 2; p[0] = s.x; p[1] = s.y; }
            if (A.trace) write_trace(A.trace + (size_t)t * TRACE_W, obs, s);
        }
    }
    if (lane == 0 && live && A.ret) {
        const float r = 0.0f + (steps == EPISODE_STEPS ? final_reward(s, A.hdr) : 0.0f);
        A.ret[m] = r;
        A.sign[m] = (float)((r > 0.0f) - (r < 0.0f));
        A.len[m] = steps;
        A.xy[2 * m] = s.x; A.xy[2 * m + 1] = s.y;
    }
}
#endif

}  // namespace maze
}  // namespace dne
