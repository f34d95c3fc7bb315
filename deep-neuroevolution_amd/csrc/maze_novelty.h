// maze_novelty.h -- nses.py:12-32 for the hard maze's behaviour characterisation, ONE float32 point (x, y) per member (MazeFinalState,
// tf_maze.py:64-66): the mean distance of a member to its k nearest archive points, as ONE __host__ __device__ text for the arithmetic, a
// CPU twin (behind dne_maze_novelty_host) and a kernel for gfx950, which agree bit for bit.  DESIGN.md section 12
// ("Novelty on the maze") holds the contract:
//   * d(p, a) = sqrt(dx * dx + dy * dy) with dx = (double)ax - (double)px, dy likewise: IEEE double operations, the sum unfused
//     (-ffp-contract=off on both passes), sqrt the correctly rounded one (as nv_distance of novelty.h relies on).  nses.py:12-20 on
//     trajectories of length 1 is this followed by sqrt(d**2 + 0**2), which is dropped;
//   * the order is (isnan, value, archive slot): every number, +inf included, before every NaN, ties to the lower slot.  A distance is
//     never negative and never -0.0, so its bit pattern as an unsigned integer orders as the value does; a NaN is sent to one pattern
//     above +inf's.  That integer is the key both sides sort by (sort_key);
//   * novelty = (the kk = min(k, narch) first distances of that order, added one by one in that order into a double that starts at 0.0) / kk.
// A plain C++ compiler can include this file (the kernels are behind __HIPCC__): tests/maze_novelty_asan_main.cpp does.
//
// The text has two forms.  The archive form (NS-ES, section 12) is the one above.  The pool form (GA-NS) scores member p of n
// members against the archive AND the population it belongs to, and differs in three things:
//   * the slots are the combined ones: the archive's points at 0 .. narch - 1, then the population's points at narch .. narch + n - 1, so on
//     equal distances an archive point comes before a population point;
//   * a point at combined slot c >= narch is member c - narch's;
//   * p's own combined slot narch + p is left out -- by index, not by value: another member, or an archive point, at exactly p's position
//     stays in at distance 0.
// Hence kk = min(k, narch + n - 1); a NaN member gets a NaN novelty and sorts last for the others; narch may be 0, and a pool with nothing in it
// (n = 1, narch = 0) has no novelty: the callers refuse it.  On the CPU the two forms are one body (novelty_host_body behind novelty_host /
// novelty_pool_host); on the device they are two kernels with the same scheme, k_maze_novelty and k_maze_novelty_pool -- one templated body
// behind both compiled to a slower k_maze_novelty, so the kernels stay as they were.  Host and device agree bit for
// bit; no [n][narch] or [n][narch + n] matrix exists on either side.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MZN_HD __host__ __device__ __forceinline__
#else
#define MZN_HD inline
#endif

namespace dne {
namespace maze_novelty {

constexpr int KMAX = 32;          // DNE_MAZE_NOVELTY_KMAX: neighbours a lane keeps in registers
constexpr int TILE = 1024;        // archive points staged in LDS at a time (8 KiB), shared by a workgroup's four members
constexpr uint64_t KEY_NAN = 0x7FF8000000000000ull;   // every NaN: above +inf (0x7FF0...), below KEY_NONE
constexpr uint64_t KEY_NONE = ~0ull;                  // an empty place of a lane's list: after every distance

MZN_HD double distance(float px, float py, float ax, float ay) {
    const double dx = (double)ax - (double)px, dy = (double)ay - (double)py;
    return sqrt(dx * dx + dy * dy);
}

MZN_HD uint64_t sort_key(double d) {
    if (d != d) return KEY_NAN;
    uint64_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = (uint64_t)__double_as_longlong(d);
#else
    memcpy(&u, &d, sizeof(u));
#endif
    return u;
}

MZN_HD double key_value(uint64_t key) {
    double d;
#if defined(__HIP_DEVICE_COMPILE__)
    d = __longlong_as_double((long long)key);
#else
    memcpy(&d, &key, sizeof(d));
#endif
    return d;
}

// ---- the CPU side: a plain partial sort on (key, slot), then the sum in that order ----------------------------------------------------------
// POOL: the entries are the combined slots 0 .. narch + n - 1 without narch + p (narch may be 0; narch + n - 1 >= 1), else the archive's slots
template <bool POOL>
inline void novelty_host_body(const float *xy, int n, const float *archive, int narch, int k, double *out) {
    const int total = POOL ? narch + n : narch, pool = POOL ? total - 1 : total, kk = k < pool ? k : pool;
    std::vector<std::pair<uint64_t, int32_t>> e((size_t)pool);
    for (int p = 0; p < n; p++) {
        size_t at = 0;
        for (int c = 0; c < total; c++) {
            if (POOL && c == narch + p) continue;
            const float *q = c < narch ? archive + 2 * (size_t)c : xy + 2 * (size_t)(c - narch);
            e[at++] = std::make_pair(sort_key(distance(xy[2 * p], xy[2 * p + 1], q[0], q[1])), (int32_t)c);
        }
        std::partial_sort(e.begin(), e.begin() + kk, e.end());
        double s = 0.0;
        for (int t = 0; t < kk; t++) s += key_value(e[t].first);
        out[p] = s / (double)kk;
    }
}

inline void novelty_host(const float *xy, int n, const float *archive, int narch, int k, double *out) { novelty_host_body<false>(xy, n, archive, narch, k, out); }
inline void novelty_pool_host(const float *xy, int n, const float *archive, int narch, int k, double *out) { novelty_host_body<true>(xy, n, archive, narch, k, out); }

#if defined(__HIPCC__)
// ---- the device side --------------------------------------------------------------------------------------------------------------------------
// grid ceil(n / 4), 256 threads: wave w of block b scores member 4b + w against the whole archive.  The archive goes through LDS in tiles of
// TILE points that the four waves share; a lane walks points lane, lane + 64, ... of each tile, so what it sees comes in ascending slot
// order, and keeps its KMAX best (key, slot) pairs sorted in registers: every index below is a compile-time constant after unrolling
// (a run-time index would send the list to scratch).  `worst` is the list's place kk - 1: a point that does not come before it can be
// none of this lane's kk best, so none of the wave's, and skips the insert.  After the last tile, kk rounds: the wave-wide minimum over
// (key, slot) of the lanes' heads is the next distance of the order; the lane that holds it drops its head; every lane adds the value to
// its own copy of the sum.  Spare waves of a partial last workgroup shadow the last member and write nothing; no wave leaves ahead of a barrier.
__global__ __launch_bounds__(256) void k_maze_novelty(const float *__restrict__ xy, int n, const float *__restrict__ archive, int narch, int kk,
                                                      double *__restrict__ out) {
    __shared__ float2 s_pts[TILE];
    const int lane = threadIdx.x & 63;
    int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = m < n;
    if (!live) m = n - 1;
    const float px = xy[2 * (size_t)m], py = xy[2 * (size_t)m + 1];
    uint64_t key[KMAX];
    int slot[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++) { key[i] = KEY_NONE; slot[i] = INT_MAX; }
    uint64_t worst = KEY_NONE;
    for (int t0 = 0; t0 < narch; t0 += TILE) {
        const int cnt = narch - t0 < TILE ? narch - t0 : TILE;
        __syncthreads();                            // the tile before this one has been read by every wave
        for (int i = threadIdx.x; i < cnt; i += 256) s_pts[i] = ((const float2 *)archive)[(size_t)t0 + i];
        __syncthreads();
        for (int j = lane; j < cnt; j += 64) {
            const float2 a = s_pts[j];
            const uint64_t ck = sort_key(distance(px, py, a.x, a.y));
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

// k_maze_novelty's scheme over the pool: the tiles run over the COMBINED slots 0 .. narch + n - 1, the archive first and the population behind
// it (a tile may hold the end of one and the start of the other), so a lane still sees its points in ascending combined slot and a candidate
// still comes after everything already in its list.  The member's own combined slot narch + m is passed over, by index.  kk <= narch + n - 1,
// so the kk rounds never reach an empty place.  archive is not read when narch == 0 (it may be null).  Same list, same compile-time indices.
__global__ __launch_bounds__(256) void k_maze_novelty_pool(const float *__restrict__ xy, int n, const float *__restrict__ archive, int narch, int kk,
                                                           double *__restrict__ out) {
    __shared__ float2 s_pts[TILE];
    const int lane = threadIdx.x & 63;
    int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = m < n;
    if (!live) m = n - 1;
    const float px = xy[2 * (size_t)m], py = xy[2 * (size_t)m + 1];
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
            s_pts[i] = c < narch ? ((const float2 *)archive)[(size_t)c] : ((const float2 *)xy)[(size_t)(c - narch)];
        }
        __syncthreads();
        for (int j = lane; j < cnt; j += 64) {
            const float2 a = s_pts[j];
            const uint64_t ck = sort_key(distance(px, py, a.x, a.y));
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

// archive slot have + i = the last evaluation's member members[i], in the order given (indices may repeat); one thread per point
__global__ __launch_bounds__(256) void k_maze_archive_gather(const float *__restrict__ xy, const int32_t *__restrict__ members, int count,
                                                             float *__restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) ((float2 *)dst)[i] = ((const float2 *)xy)[members[i]];
}
#endif

}  // namespace maze_novelty
}  // namespace dne
