// dense_novelty.h -- nses.py:12-32 for a dense policy of any small shape (DNE_KIND_DENSE): maze_novelty.h's archive form with the width of a
// behaviour characterisation (BC), D, a run-time value on the host and a template argument on the device.  ONE __host__ __device__ text for the
// arithmetic, a CPU twin (behind dne_dense_novelty_host / dne_dense_bc_host) and kernels for gfx950, which agree bit for bit.  The key, its
// order and the constants are maze_novelty.h's (sort_key, key_value, KMAX, TILE, KEY_NAN, KEY_NONE): used, not copied.  DESIGN.md section 17b:
//   * the BC of a member is D float32 values of its final state record (stepenv::pack's doubles), one IEEE round-to-nearest cast each, NaN and
//     +-inf passing through.  The reference has no BC for these environments; the choice is this project's:
//       maze       D = 2: (float)rec[0], (float)rec[1] -- the record holds widened floats, so this is MazeFinalState, the (x, y) k_maze_rollout leaves
//       cart-pole  D = 4: (float) of x, x_dot, theta, theta_dot
//       pendulum   D = 2: (float) of theta, theta_dot
//       acrobot    D = 4: (float) of theta1, theta2, omega1, omega2
//   * d(p, a) = sqrt(s): per coordinate d_i = (double)a_i - (double)p_i; s = d_0 * d_0, then s = s + d_i * d_i for i ascending, never fused
//     (-ffp-contract=off on both passes); sqrt the correctly rounded one.  For D = 2 this is maze_novelty::distance bit for bit;
//   * the order is (isnan, value, archive slot) through sort_key;
//   * novelty = (the kk = min(k, narch) first distances of that order, added one by one in that order into a double that starts at 0.0) / kk.
// Two forms, as in maze_novelty.h.  The archive form (NS-ES / NSR-ES, section 17b) is the one above.  The pool form (GA-NS, section 17c,
// ga_gpu.dense_ns_main) scores member p of n members against the archive AND the population it belongs to: the slots are the combined ones, the
// archive's points at 0 .. narch - 1, then the population's at narch .. narch + n - 1 (on equal distances an archive point comes first); p's own
// combined slot narch + p is left out by index, not by value; kk = min(k, narch + n - 1); a NaN member gets a NaN novelty; narch may be 0, and a
// pool with nothing in it (n = 1, narch = 0) has no novelty: the callers refuse it.  No [n][narch] or [n][narch + n] matrix exists on either side.
// A plain C++ compiler can include this file (the kernels are behind __HIPCC__): tests/dense_novelty_asan_main.cpp does.
#pragma once
#include "dense.h"
#include "maze_novelty.h"

namespace dne {
namespace dense_novelty {

using maze_novelty::KEY_NAN;
using maze_novelty::KEY_NONE;
using maze_novelty::KMAX;
using maze_novelty::TILE;
using maze_novelty::key_value;
using maze_novelty::sort_key;

constexpr int MAX_D = 4;

// ---- the behaviour characterisation ---------------------------------------------------------------------------------------------------------
MZ_HD int bc_dim(int env) { return env == dense::KIND_CARTPOLE || env == dense::ENV_ACROBOT ? 4 : 2; }

MZ_HD void bc_of_record(int env, const double *rec, float *bc) {
    const int D = bc_dim(env);
    for (int i = 0; i < D; i++) bc[i] = (float)rec[i];
}

MZN_HD double distance(const float *p, const float *a, int D) {
    double d = (double)a[0] - (double)p[0];
    double s = d * d;
    for (int i = 1; i < D; i++) {
        d = (double)a[i] - (double)p[i];
        s = s + d * d;
    }
    return sqrt(s);
}

// ---- the CPU side: a plain partial sort on (key, slot), then the sum in that order, as maze_novelty::novelty_host_body ------------------------
inline void bc_host(int env, const double *rec, int n, float *bc) {
    const int S = env == dense::KIND_MAZE ? 7 : env == dense::KIND_CARTPOLE || env == dense::ENV_ACROBOT ? 4 : 2, D = bc_dim(env);
    for (int i = 0; i < n; i++) bc_of_record(env, rec + (size_t)i * S, bc + (size_t)i * D);
}

inline void novelty_host(const float *bc, int n, const float *archive, int narch, int D, int k, double *out) {
    const int kk = k < narch ? k : narch;
    std::vector<std::pair<uint64_t, int32_t>> e((size_t)narch);
    for (int p = 0; p < n; p++) {
        for (int c = 0; c < narch; c++) e[c] = std::make_pair(sort_key(distance(bc + (size_t)D * p, archive + (size_t)D * c, D)), (int32_t)c);
        std::partial_sort(e.begin(), e.begin() + kk, e.end());
        double s = 0.0;
        for (int t = 0; t < kk; t++) s += key_value(e[t].first);
        out[p] = s / (double)kk;
    }
}

// the pool form: the entries are the combined slots 0 .. narch + n - 1 without narch + p (narch may be 0, archive is not read then; narch + n - 1 >= 1)
inline void novelty_pool_host(const float *bc, int n, const float *archive, int narch, int D, int k, double *out) {
    const int total = narch + n, pool = total - 1, kk = k < pool ? k : pool;
    std::vector<std::pair<uint64_t, int32_t>> e((size_t)pool);
    for (int p = 0; p < n; p++) {
        size_t at = 0;
        for (int c = 0; c < total; c++) {
            if (c == narch + p) continue;
            const float *q = c < narch ? archive + (size_t)D * c : bc + (size_t)D * (c - narch);
            e[at++] = std::make_pair(sort_key(distance(bc + (size_t)D * p, q, D)), (int32_t)c);
        }
        std::partial_sort(e.begin(), e.begin() + kk, e.end());
        double s = 0.0;
        for (int t = 0; t < kk; t++) s += key_value(e[t].first);
        out[p] = s / (double)kk;
    }
}

#if defined(__HIPCC__)
// ---- the device side --------------------------------------------------------------------------------------------------------------------------
// one thread per member: the last evaluation's records [n][S] -> float [n][D]
template <int ENV>
__global__ __launch_bounds__(256) void k_dense_bc(const double *__restrict__ rec, int n, float *__restrict__ bc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[MAX_D];
    bc_of_record(ENV, rec + (size_t)i * dense::EnvOf<ENV>::S, v);
#pragma unroll
    for (int d = 0; d < bc_dim(ENV); d++) bc[(size_t)i * bc_dim(ENV) + d] = v[d];
}

template <int D> struct PointOf;
template <> struct PointOf<2> { typedef float2 T; };
template <> struct PointOf<4> { typedef float4 T; };
__device__ __forceinline__ void spread(const float2 &q, float *a) { a[0] = q.x; a[1] = q.y; }
__device__ __forceinline__ void spread(const float4 &q, float *a) { a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w; }

// k_maze_novelty's scheme with D floats a point.  grid ceil(n / 4), 256 threads: wave w of block b scores member 4b + w against the whole
// archive.  The archive goes through LDS in tiles of TILE points that the four waves share (D = 2: 8 KiB, D = 4: 16 KiB, a point is ONE LDS
// read of 8 or 16 bytes); a lane walks points lane, lane + 64, ... of each tile, so what it sees comes in ascending slot order, and keeps its
// KMAX best (key, slot) pairs sorted in registers: every index below is a compile-time constant after unrolling.  `worst` is the list's place
// kk - 1: a point that does not come before it can be none of this lane's kk best, so none of the wave's, and skips the insert.  After the last
// tile, kk rounds of a wave-wide minimum over (key, slot).  Spare waves of a partial last workgroup shadow the last member and write nothing; no
// wave leaves ahead of a barrier.  bc and archive are 4 D bytes aligned (the engine's allocations are).
template <int D>
__global__ __launch_bounds__(256) void k_dense_novelty(const float *__restrict__ bc, int n, const float *__restrict__ archive, int narch, int kk,
                                                       double *__restrict__ out) {
    typedef typename PointOf<D>::T Pt;
    __shared__ Pt s_pts[TILE];
    const int lane = threadIdx.x & 63;
    int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = m < n;
    if (!live) m = n - 1;
    float p[D], a[D];
    spread(((const Pt *)bc)[(size_t)m], p);
    uint64_t key[KMAX];
    int slot[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++) { key[i] = KEY_NONE; slot[i] = INT_MAX; }
    uint64_t worst = KEY_NONE;
    for (int t0 = 0; t0 < narch; t0 += TILE) {
        const int cnt = narch - t0 < TILE ? narch - t0 : TILE;
        __syncthreads();                            // the tile before this one has been read by every wave
        for (int i = threadIdx.x; i < cnt; i += 256) s_pts[i] = ((const Pt *)archive)[(size_t)t0 + i];
        __syncthreads();
        for (int j = lane; j < cnt; j += 64) {
            spread(s_pts[j], a);
            const uint64_t ck = sort_key(distance(p, a, D));
            if (ck < worst) {                       // (the candidate's slot is above every slot of the list: on equal keys it comes after)
                const int cs = t0 + j;
#pragma unroll
                for (int i = KMAX - 1; i >= 1; i--) {
                    const bool shift = key[i - 1] > ck, here = key[i] > ck;
                    key[i] = shift ? key[i - 1] : here ? ck : key[i];
                    slot[i] = shift ? slot[i - 1] : here ? cs : slot[i];
                }
                if (key[0] > ck) { key[0] = ck; slot[0] = cs; }
#pragma unroll
                for (int i = 0; i < KMAX; i++) worst = i == kk - 1 ? key[i] : worst;
            }
        }
    }
    double sum = 0.0;
    for (int t = 0; t < kk; t++) {
        uint64_t bk = key[0];
        int bs = slot[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ok = (uint64_t)__shfl_xor((long long)bk, o);
            const int os = __shfl_xor(bs, o);
            if (ok < bk || (ok == bk && os < bs)) { bk = ok; bs = os; }
        }
        if (slot[0] == bs) {                        // an archive slot lives in one lane
#pragma unroll
            for (int i = 0; i < KMAX - 1; i++) { key[i] = key[i + 1]; slot[i] = slot[i + 1]; }
            key[KMAX - 1] = KEY_NONE; slot[KMAX - 1] = INT_MAX;
        }
        sum += key_value(bk);
    }
    if (lane == 0 && live) out[m] = sum / (double)kk;
}

// k_dense_novelty's scheme over the pool, as k_maze_novelty_pool is to k_maze_novelty: the tiles run over the COMBINED slots 0 .. narch + n - 1,
// the archive first and the population behind it (the staging loop picks the source per point, so a tile may hold the end of one and the start
// of the other); a lane still sees its points in ascending combined slot and a candidate still comes after everything already in its list.  The
// member's own combined slot narch + m is passed over, by index.  kk <= narch + n - 1, so the kk rounds never reach an empty place.  archive is
// not read when narch == 0 (it may be null).  Same list, same compile-time indices.
template <int D>
__global__ __launch_bounds__(256) void k_dense_novelty_pool(const float *__restrict__ bc, int n, const float *__restrict__ archive, int narch, int kk,
                                                            double *__restrict__ out) {
    typedef typename PointOf<D>::T Pt;
    __shared__ Pt s_pts[TILE];
    const int lane = threadIdx.x & 63;
    int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = m < n;
    if (!live) m = n - 1;
    float p[D], a[D];
    spread(((const Pt *)bc)[(size_t)m], p);
    const int total = narch + n, self = narch + m;
    uint64_t key[KMAX];
    int slot[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++) { key[i] = KEY_NONE; slot[i] = INT_MAX; }
    uint64_t worst = KEY_NONE;
    for (int t0 = 0; t0 < total; t0 += TILE) {
        const int cnt = total - t0 < TILE ? total - t0 : TILE;
        __syncthreads();                            // the tile before this one has been read by every wave
        for (int i = threadIdx.x; i < cnt; i += 256) {
            const int c = t0 + i;
            s_pts[i] = c < narch ? ((const Pt *)archive)[(size_t)c] : ((const Pt *)bc)[(size_t)(c - narch)];
        }
        __syncthreads();
        for (int j = lane; j < cnt; j += 64) {
            spread(s_pts[j], a);
            const uint64_t ck = sort_key(distance(p, a, D));
            const int cs = t0 + j;
            if (ck < worst && cs != self) {         // (the candidate's combined slot is above every slot of the list: on equal keys it comes after)
#pragma unroll
                for (int i = KMAX - 1; i >= 1; i--) {
                    const bool shift = key[i - 1] > ck, here = key[i] > ck;
                    key[i] = shift ? key[i - 1] : here ? ck : key[i];
                    slot[i] = shift ? slot[i - 1] : here ? cs : slot[i];
                }
                if (key[0] > ck) { key[0] = ck; slot[0] = cs; }
#pragma unroll
                for (int i = 0; i < KMAX; i++) worst = i == kk - 1 ? key[i] : worst;
            }
        }
    }
    double sum = 0.0;
    for (int t = 0; t < kk; t++) {
        uint64_t bk = key[0];
        int bs = slot[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ok = (uint64_t)__shfl_xor((long long)bk, o);
            const int os = __shfl_xor(bs, o);
            if (ok < bk || (ok == bk && os < bs)) { bk = ok; bs = os; }
        }
        if (slot[0] == bs) {                        // a combined slot lives in one lane
#pragma unroll
            for (int i = 0; i < KMAX - 1; i++) { key[i] = key[i + 1]; slot[i] = slot[i + 1]; }
            key[KMAX - 1] = KEY_NONE; slot[KMAX - 1] = INT_MAX;
        }
        sum += key_value(bk);
    }
    if (lane == 0 && live) out[m] = sum / (double)kk;
}

// archive slot have + i = the BC of the last evaluation's member members[i], in the order given (indices may repeat); one thread per point,
// one load and one store of 4 D bytes
template <int D>
__global__ __launch_bounds__(256) void k_dense_archive_gather(const float *__restrict__ bc, const int32_t *__restrict__ members, int count,
                                                              float *__restrict__ dst) {
    typedef typename PointOf<D>::T Pt;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) ((Pt *)dst)[i] = ((const Pt *)bc)[members[i]];
}
#endif

}  // namespace dense_novelty
}  // namespace dne
