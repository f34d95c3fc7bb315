// ram_novelty.h -- pool novelty (GA-NS) over Atari behaviour characterisations: ONE 128-byte RAM row per member (GAAtariPolicy.rollout's final
// RAM, policies.py:510), each member scored against the archive AND the other members of its generation.  One contract, a CPU twin (behind
// dne_ram_novelty_pool_host) and a kernel for gfx950 that agree bit for bit.  DESIGN.md section 18 ("GA-NS on Atari") holds the contract:
//   * S(x, y) = the sum of the 128 squared byte differences, an exact integer <= 128 * 255^2 = 8 323 200; d(x, y) = orc_bc_distance of two
//     one-row trajectories = nv_distance(S, 0) of novelty.h: a = sqrt((double)S), then sqrt(a * a + 0.0), the product unfused;
//   * the pool of member m: the archive at combined slots 0 .. A - 1, then the population at A .. A + n - 1, without slot A + m -- left out by
//     index, not by value: another member, or an archive point, with the same 128 bytes stays in at distance 0;
//   * the order is (S, combined slot), ties to the lower slot (d is monotone in S), so the sort key is the integer (S << 32) | slot;
//   * novelty = (the kk = min(k, A + n - 1) first distances of that order, added one by one into a double that starts at 0.0) / kk; the
//     neighbours of m are those kk combined slots in that order.
// A may be 0; a pool with nothing in it (n = 1, A = 0) has no novelty: the callers refuse it.  No [n][A + n] matrix exists on either side.
// A plain C++ compiler can include this file (the kernels are behind __HIPCC__): tests/atari_gans_asan_main.cpp does.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RNV_HD __host__ __device__ __forceinline__
#else
#define RNV_HD inline
#endif

namespace dne {
namespace ram_novelty {

constexpr int KMAX = 32;          // DNE_RAM_NOVELTY_KMAX: neighbours a lane keeps in registers
constexpr int ROW = 128;          // bytes of a point
constexpr int ROW_W = ROW / 4;    // ... in 32-bit words
constexpr int TILE = 256;         // DNE_RAM_NOVELTY_TILE: combined slots staged in LDS at a time
constexpr int MPW = 1;            // members a wave scores side by side (a staged row is read once for all of them)
constexpr int WAVES = 4;          // waves of a workgroup: at 144 VGPRs three workgroups share a CU, one wave per SIMD each
constexpr int THREADS = 64 * WAVES;
constexpr int MEMBERS = WAVES * MPW;   // DNE_RAM_NOVELTY_MEMBERS: members of a workgroup's tile
constexpr int PITCH = 36;         // LDS pitch of a staged row in words (novelty.h's NV_P): the 8 rows one ds_read_b128 lane group reads sit on 8 disjoint 16-B bank slots
constexpr uint64_t KEY_NONE = ~0ull;   // an empty place of a lane's list: after every (S, slot)

// orc_bc_distance on two one-row trajectories whose squared distance is S: nv_distance(S, 0)
RNV_HD double distance(uint32_t S) {
    const double a = sqrt((double)S);
    return sqrt(a * a + 0.0);
}

RNV_HD uint64_t sort_key(uint32_t S, uint32_t slot) { return ((uint64_t)S << 32) | slot; }

// ---- the CPU side: a plain loop for S, a partial sort on (S, slot), then the sum in that order -----------------------------------------------
// p [n][128], archive [narch][128] (not read when narch == 0; it may be null), narch + n - 1 >= 1, narch + n <= INT_MAX;
// neighbours (or null) [n][min(k, narch + n - 1)]
inline void novelty_pool_host(const uint8_t *p, int n, const uint8_t *archive, int narch, int k, double *out, int32_t *neighbours) {
    const int total = narch + n, pool = total - 1, kk = k < pool ? k : pool;
    std::vector<uint64_t> e((size_t)pool);
    for (int m = 0; m < n; m++) {
        const uint8_t *x = p + (size_t)m * ROW;
        size_t at = 0;
        for (int c = 0; c < total; c++) {
            if (c == narch + m) continue;
            const uint8_t *y = c < narch ? archive + (size_t)c * ROW : p + (size_t)(c - narch) * ROW;
            uint32_t S = 0;
            for (int b = 0; b < ROW; b++) {
                const int32_t d = (int32_t)x[b] - (int32_t)y[b];
                S += (uint32_t)(d * d);
            }
            e[at++] = sort_key(S, (uint32_t)c);
        }
        std::partial_sort(e.begin(), e.begin() + kk, e.end());
        double s = 0.0;
        for (int t = 0; t < kk; t++) {
            s += distance((uint32_t)(e[t] >> 32));
            if (neighbours) neighbours[(size_t)m * kk + t] = (int32_t)(uint32_t)e[t];
        }
        out[m] = s / (double)kk;
    }
}

#if defined(__HIPCC__)
// ---- the device side --------------------------------------------------------------------------------------------------------------------------
// grid ceil(n / MEMBERS), THREADS threads: wave w of block b scores members MEMBERS * b + MPW * w + {0 .. MPW - 1} against the whole pool.  The
// combined slots 0 .. A + n - 1 go through LDS in tiles of TILE rows that the WAVES waves share, the archive first and the population behind it
// (a tile may hold the end of one and the start of the other: each staging thread picks its source by c < A, and `archive` is not read when
// A == 0).  Eight consecutive threads stage one row as eight 16-byte pieces and leave its squared norm beside it (v_dot4_u32_u8 of each word
// with itself, summed over the eight by shuffles).  A lane walks rows lane, lane + 64, ... of each tile: it reads the row once, forms the
// cross terms with each of its wave's MPW members (whose rows are wave-uniform), S = |x|^2 + |y|^2 - 2 x.y in uint32 -- exact: every term is
// below 2^24 -- and keeps, per member, its KMAX smallest keys (S << 32) | slot sorted in registers: every index below is a compile-time
// constant after unrolling (a run-time index would send the lists to scratch).  worst[i] is member i's last list place: a key that does not
// come before it can be none of this lane's KMAX best, so none of the wave's kk <= KMAX, and skips the insert (the place kk - 1 would prune a
// little more, but picking it takes KMAX wave-uniform selects whose masks crowd the scalar registers the member's row lives in).  A member's own slot A + m is passed over,
// by index.  After the last tile, kk rounds per member: the wave-wide minimum of the lanes' heads is the next key of the order (keys are
// unique: the slot is part of them); the lane that holds it drops its head; every lane adds the distance to its own copy of the sum.
// kk <= A + n - 1, so the rounds never reach an empty place.  Doubles appear only there.  Spare members of a partial last tile shadow member
// n - 1 and write nothing; no wave leaves ahead of a barrier.
__global__ __launch_bounds__(THREADS) void k_ram_novelty_pool(const uint32_t *__restrict__ pts /*[n][32]*/, int n,
                                                          const uint32_t *__restrict__ archive /*[narch][32]*/, int narch, int kk,
                                                          double *__restrict__ out, int32_t *__restrict__ neighbours /*[n][kk] or null*/) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[TILE * PITCH];
    __shared__ uint32_t snorm[TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int total = narch + n;
    int mem[MPW];
    bool live[MPW];
    uint32_t x[MPW][ROW_W], xn[MPW];
    uint64_t key[MPW][KMAX], worst[MPW];
#pragma unroll
    for (int i = 0; i < MPW; i++) {
        mem[i] = blockIdx.x * MEMBERS + wave * MPW + i;
        live[i] = mem[i] < n;
        if (!live[i]) mem[i] = n - 1;
        const uint4 *src = (const uint4 *)(pts + (size_t)mem[i] * ROW_W);
        uint32_t nr = 0;
#pragma unroll
        for (int g = 0; g < ROW_W / 4; g++) {
            const uint4 v = src[g];
            x[i][4 * g] = v.x; x[i][4 * g + 1] = v.y; x[i][4 * g + 2] = v.z; x[i][4 * g + 3] = v.w;
            nr = __builtin_amdgcn_udot4(v.x, v.x, nr, false);
            nr = __builtin_amdgcn_udot4(v.y, v.y, nr, false);
            nr = __builtin_amdgcn_udot4(v.z, v.z, nr, false);
            nr = __builtin_amdgcn_udot4(v.w, v.w, nr, false);
        }
        xn[i] = nr;
#pragma unroll
        for (int j = 0; j < KMAX; j++) key[i][j] = KEY_NONE;
        worst[i] = KEY_NONE;
    }
    for (int t0 = 0; t0 < total; t0 += TILE) {
        const int cnt = total - t0 < TILE ? total - t0 : TILE;
        __syncthreads();                            // the tile before this one has been read by every wave
#pragma unroll
        for (int v = 0; v < TILE * 8 / THREADS; v++) {  // TILE rows x 8 pieces, 8 per thread; rows past cnt are staged as zeros and never scored
            const int u = tid + THREADS * v, r = u >> 3, part = u & 7, c = t0 + r;
            uint4 w = make_uint4(0, 0, 0, 0);
            if (r < cnt) {
                const uint32_t *src = c < narch ? archive + (size_t)c * ROW_W : pts + (size_t)(c - narch) * ROW_W;
                w = *(const uint4 *)(src + 4 * part);
            }
            *(uint4 *)(stage + r * PITCH + 4 * part) = w;
            uint32_t nr = __builtin_amdgcn_udot4(w.x, w.x, 0u, false);
            nr = __builtin_amdgcn_udot4(w.y, w.y, nr, false);
            nr = __builtin_amdgcn_udot4(w.z, w.z, nr, false);
            nr = __builtin_amdgcn_udot4(w.w, w.w, nr, false);
            nr += __shfl_xor(nr, 1); nr += __shfl_xor(nr, 2); nr += __shfl_xor(nr, 4);
            if (part == 0) snorm[r] = nr;
        }
        __syncthreads();
        for (int j = lane; j < cnt; j += 64) {
            const uint32_t *row = stage + j * PITCH;
            uint32_t dot[MPW];
#pragma unroll
            for (int i = 0; i < MPW; i++) dot[i] = 0;
#pragma unroll
            for (int g = 0; g < ROW_W / 4; g++) {
                const uint4 y = *(const uint4 *)(row + 4 * g);
#pragma unroll
                for (int i = 0; i < MPW; i++) {
                    uint32_t s = dot[i];
                    s = __builtin_amdgcn_udot4(x[i][4 * g], y.x, s, false);
                    s = __builtin_amdgcn_udot4(x[i][4 * g + 1], y.y, s, false);
                    s = __builtin_amdgcn_udot4(x[i][4 * g + 2], y.z, s, false);
                    s = __builtin_amdgcn_udot4(x[i][4 * g + 3], y.w, s, false);
                    dot[i] = s;
                }
            }
            const uint32_t yn = snorm[j], cs = (uint32_t)(t0 + j);
#pragma unroll
            for (int i = 0; i < MPW; i++) {
                const uint64_t ck = sort_key(xn[i] + yn - 2u * dot[i], cs);
                if (ck < worst[i] && cs != (uint32_t)(narch + mem[i])) {
                    uint64_t carry = ck;             // one pass down the list: each place keeps the smaller, the larger moves on
#pragma unroll
                    for (int q = 0; q < KMAX; q++) {
                        const bool before = carry < key[i][q];
                        const uint64_t lo = before ? carry : key[i][q], hi = before ? key[i][q] : carry;
                        key[i][q] = lo; carry = hi;
                    }
                    worst[i] = key[i][KMAX - 1];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MPW; i++) {
        double sum = 0.0;
        for (int t = 0; t < kk; t++) {
            uint64_t bk = key[i][0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t ok = (uint64_t)__shfl_xor((long long)bk, o);
                if (ok < bk) bk = ok;
            }
            if (key[i][0] == bk) {                  // a combined slot lives in one lane
#pragma unroll
                for (int q = 0; q < KMAX - 1; q++) key[i][q] = key[i][q + 1];
                key[i][KMAX - 1] = KEY_NONE;
            }
            sum += distance((uint32_t)(bk >> 32));
            if (neighbours && lane == 0 && live[i]) neighbours[(size_t)mem[i] * kk + t] = (int32_t)(uint32_t)bk;
        }
        if (lane == 0 && live[i]) out[mem[i]] = sum / (double)kk;
    }
}

// dst row i (128 bytes, the archive's pitch for width 128) = src row rows[i], in the order given (indices may repeat): one thread per
// 16-byte piece.  The archive gather of dne_archive_append_members, and the caller-order view of h->bc after an evaluation that reordered
// its members
__global__ __launch_bounds__(256) void k_ram_archive_gather(const uint32_t *__restrict__ src, const int32_t *__restrict__ rows, int count,
                                                            uint32_t *__restrict__ dst) {
    const int u = blockIdx.x * 256 + threadIdx.x, i = u >> 3, part = u & 7;
    if (i < count) ((uint4 *)dst)[(size_t)i * 8 + part] = ((const uint4 *)src)[(size_t)rows[i] * 8 + part];
}
#endif

}  // namespace ram_novelty
}  // namespace dne
