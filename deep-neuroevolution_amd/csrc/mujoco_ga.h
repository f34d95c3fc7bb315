// mujoco_ga.h -- Deep-GA (es_distributed/ga.py) on MujocoPolicy, for the two kinds that run it (DNE_KIND_PENDULUM, DNE_KIND_MJMAZE): the genome
// side as ONE __host__ __device__ text, a CPU twin of every entry point (colscale_host, genome_host, members_host, behind
// dne_mujoco_ga_colscale_host / _theta_host / _members_host) and four small kernels for gfx950, which agree bit for bit.  DESIGN.md section
// 16b holds the contract:
//   * the layout is pendulum::offsets / mjmaze::offsets (used, not copied): l0/w [OBS][H], l0/b, l1/w [H][H], l1/b, out/w [H][O], out/b;
//   * column scale (ga.py:256-260 -> policies.py reinitialize -> tf_util.py:122-130,149-158: _normalize(w, std=1.0) for ALL THREE layers, `out`
//     included): for a weight block [K][C] read at noise[idx0 + off + k C + c], ss_c = the float32 sum over k of fl(x * x), sc_c = 1.0f / sqrtf(ss_c);
//   * order of the sum = numpy's np.square(out).sum(axis=0) on the [K][C] view: sequential in k for C >= 2; for C == 1 (the pendulum's
//     continuous action) numpy sees one contiguous run of K and sums it pairwise -- K a multiple of 8, K <= 128: eight accumulators seeded with
//     elements 0..7, each adds its stride-8 elements, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); K > 128: split at K / 2 rounded down to
//     a multiple of 8, each half summed the same way, the halves added;
//   * root: theta_p = fl(noise[idx0 + p] * sc_col(p)) for weights, +0.0f for biases; a column whose squares sum to 0 is NaN throughout;
//   * chain (ga.py:262-263), per further seed in order: theta_p = theta_p + fl(sigma * noise[idx_j + p]) -- maze::perturbed, never fused
//     (-ffp-contract=off on both passes);
//   * member descriptor (parent, idx, power) against a bank of T parents -- maze_ga::member_param's arithmetic for the last two forms:
//       root   parent == -1, idx >= 0       the root rule above; power is not read
//       child  0 <= parent < T, idx >= 0    bank[parent][p] + fl(power * noise[idx + p])
//       kept   0 <= parent < T, idx < 0     bank[parent][p], bit for bit (promotion only)
// k_pendulum_rollout / k_mjmaze_rollout evaluate a child as it stands: (base slot, noise offset, scale) = (the parent's bank slot, idx, power).
// A root is written into a scratch slot by k_mujoco_ga_roots and evaluated there at scale 0 and the member's own idx: theta + fl(0 * eps) keeps
// every bit -- a bias is +0 and +0 + (+-0) is +0; a zero weight of a root carries eps's sign (sc > 0) and so does fl(0 * eps).
// A plain C++ compiler can include this file (the kernels are behind __HIPCC__): tests/mujoco_ga_asan_main.cpp does.
#pragma once
#include "dense_ga.h"
#include "mjmaze.h"

namespace dne {
namespace mujoco_ga {

using dense_ga::check_genomes;   // (P at run time; the words are the dense kind's)
using dense_ga::check_member;
using maze_ga::member_param;

constexpr int BLOCKS = 3, MAX_COLS = 2 * 256 + pendulum::MAX_OUT;   // weight blocks; H + H + O columns at the most

// the three weight blocks [K][C] at w[], their biases at b[], first column of each block among the H + H + O columns
struct Layout { int w[BLOCKS], b[BLOCKS], K[BLOCKS], C[BLOCKS], col0[BLOCKS], ncol, P; };

// obs: pendulum::OBS (3) or mjmaze::OBS (11) -- which of the two layouts
MZ_HD Layout layout(int obs, int H, int O) {
    Layout L;
    if (obs == mjmaze::OBS) {
        const mjmaze::Offsets o = mjmaze::offsets(H, O);
        L.w[0] = o.w1; L.b[0] = o.b1; L.w[1] = o.w2; L.b[1] = o.b2; L.w[2] = o.w3; L.b[2] = o.b3; L.P = o.P;
    } else {
        const pendulum::Offsets o = pendulum::offsets(H, O);
        L.w[0] = o.w1; L.b[0] = o.b1; L.w[1] = o.w2; L.b[1] = o.b2; L.w[2] = o.w3; L.b[2] = o.b3; L.P = o.P;
    }
    L.K[0] = obs; L.K[1] = H; L.K[2] = H;
    L.C[0] = H; L.C[1] = H; L.C[2] = O;
    L.col0[0] = 0; L.col0[1] = H; L.col0[2] = 2 * H;
    L.ncol = 2 * H + O;
    return L;
}

inline bool shape_ok(int obs, int H, int O) {
    if (!pendulum::hidden_ok(H)) return false;
    if (obs == pendulum::OBS) return O >= 1 && O <= pendulum::MAX_OUT;
    return obs == mjmaze::OBS && O >= mjmaze::ADIM && O <= mjmaze::MAX_OUT && O % mjmaze::ADIM == 0;
}

// the column (0 .. ncol - 1) parameter p belongs to, -1 for a bias
MZ_HD int col_of(const Layout &L, int p) {
    for (int l = 0; l < BLOCKS; l++) {
        if (p < L.b[l]) return L.col0[l] + (p - L.w[l]) % L.C[l];
        if (p < L.b[l] + L.C[l]) return -1;
    }
    return -1;
}

// ---- the sum of squares of one column -------------------------------------------------------------------------------------------------------
// C >= 2 (and any K): sequential in k; 16 rows are loaded ahead of the dependent adds (reduce.h's normc_column), rows past K guarded
MZ_HD float ss_rows(const float *x, int K, int C, int c) {
    float ss = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = k0 + j < K ? x[(size_t)(k0 + j) * C + c] : 0.0f;
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (k0 + j < K) { const float sq = v[j] * v[j]; ss = ss + sq; }
    }
    return ss;
}

// one contiguous run of n <= 128 squares, n a multiple of 8: numpy's unrolled pairwise block
MZ_HD float ss_block8(const float *x, int n) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = x[j] * x[j];
    for (int i = 8; i < n; i += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = x[i + j];
#pragma unroll
        for (int j = 0; j < 8; j++) { const float sq = v[j] * v[j]; r[j] = r[j] + sq; }
    }
    const float a = r[0] + r[1], b = r[2] + r[3], c = r[4] + r[5], d = r[6] + r[7];
    const float ab = a + b, cd = c + d;
    return ab + cd;
}

// C == 1: a contiguous run of K (64, 128 or 256: a multiple of 8, at most two blocks of 128)
MZ_HD float ss_run(const float *x, int K) {
    if (K <= 128) return ss_block8(x, K);
    int n2 = K / 2;
    n2 -= n2 % 8;
    const float lo = ss_block8(x, n2), hi = ss_block8(x + n2, K - n2);
    return lo + hi;
}

// sc of column c (0 .. ncol - 1) of the slice at noise + idx0
MZ_HD float col_scale(const float *slice, const Layout &L, int c) {
    const int l = c < L.col0[1] ? 0 : c < L.col0[2] ? 1 : 2;
    const float *x = slice + L.w[l];
    const float ss = L.C[l] == 1 ? ss_run(x, L.K[l]) : ss_rows(x, L.K[l], L.C[l], c - L.col0[l]);
    const float rt = sqrtf(ss);
    return 1.0f / rt;
}

// parameter p of the root at noise + idx0 under its column scales sc [ncol]
MZ_HD float root_param(const float *slice, const float *sc, const Layout &L, int p) {
    const int c = col_of(L, p);
    return c < 0 ? 0.0f : slice[p] * sc[c];
}

// parameter p of a genome: seeds[0] the root (its scales in sc), seeds[1 .. n) the mutations at powers[1 .. n) (powers[0] is not read)
MZ_HD float genome_param(const float *noise, const float *sc, const Layout &L, const int64_t *seeds, const float *powers, int nseeds, int p) {
    float v = root_param(noise + seeds[0], sc, L, p);
    for (int j = 1; j < nseeds; j++) v = maze::perturbed(v, powers[j], noise[seeds[j] + p]);
    return v;
}

// parameter p of a descriptor (sc: the scales of its root, read only when parent < 0); the forms were checked by check_member
MZ_HD float descriptor_param(const float *noise, const float *sc, const Layout &L, const float *bank, size_t stride, int parent, int64_t idx, float power,
                             int p) {
    if (parent < 0) return root_param(noise + idx, sc, L, p);
    return member_param(noise, nullptr, bank, stride, parent, idx, power, p);   // (child and kept: scale_by is not read)
}

// ---- the CPU side ------------------------------------------------------------------------------------------------------------------------------
inline void colscale_host(const float *noise, const Layout &L, int64_t idx0, float *sc) {
    for (int c = 0; c < L.ncol; c++) sc[c] = col_scale(noise + idx0, L, c);
}

inline void genome_host(const float *noise, const Layout &L, const int64_t *seeds, const float *powers, int nseeds, float *out) {
    float sc[MAX_COLS];
    colscale_host(noise, L, seeds[0], sc);
    for (int p = 0; p < L.P; p++) out[p] = genome_param(noise, sc, L, seeds, powers, nseeds, p);
}

// bank [T][P] packed, out [n][P]
inline void members_host(const float *noise, const Layout &L, const float *bank, const int32_t *parent, const int64_t *idx, const float *power, int n,
                         float *out) {
    float sc[MAX_COLS];
    for (int i = 0; i < n; i++) {
        if (parent[i] < 0) colscale_host(noise, L, idx[i], sc);
        for (int p = 0; p < L.P; p++) out[(size_t)i * L.P + p] = descriptor_param(noise, sc, L, bank, (size_t)L.P, parent[i], idx[i], power[i], p);
    }
}

#if defined(__HIPCC__)
// ---- the device side ---------------------------------------------------------------------------------------------------------------------------
// the column scales of every entry that has a root: grid (entries, ceil(ncol / 64)), 64 threads, one thread a column -- the threads of a wave
// read neighbouring floats of one table row, straight from the table.  root_idx[e] < 0: entry e has no root (a child, a kept parent)
__global__ __launch_bounds__(64) void k_mujoco_ga_colscale(const float *__restrict__ noise, Layout L, const int64_t *__restrict__ root_idx,
                                                           float *__restrict__ sc, int sc_stride) {
    const int c = blockIdx.y * 64 + threadIdx.x, e = blockIdx.x;
    const int64_t idx0 = root_idx[e];
    if (c >= L.ncol || idx0 < 0) return;
    sc[(size_t)e * sc_stride + c] = col_scale(noise + idx0, L, c);
}

// the three below: grid (entries, ceil(P / 256)), 256 threads; block (x, y) writes parameters [256 y, 256 y + 256) of entry x
// the roots among an evaluation's members, each into its own scratch slot: member i is a root when its base slot is root0 + i
__global__ __launch_bounds__(256) void k_mujoco_ga_roots(const float *__restrict__ noise, Layout L, const float *__restrict__ sc, int sc_stride,
                                                         const int32_t *__restrict__ m_slot, const int64_t *__restrict__ m_off, int root0,
                                                         float *__restrict__ mem, size_t stride) {
    const int p = blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
    if (p >= L.P || m_slot[i] != root0 + i) return;
    mem[(size_t)m_slot[i] * stride + p] = root_param(noise + m_off[i], sc + (size_t)i * sc_stride, L, p);
}

// the bank's parents from their genomes: dst slot j = genome j
__global__ __launch_bounds__(256) void k_mujoco_ga_build(const float *__restrict__ noise, Layout L, const float *__restrict__ sc, int sc_stride,
                                                         const int32_t *__restrict__ chain_offsets, const int64_t *__restrict__ seeds,
                                                         const float *__restrict__ powers, float *__restrict__ dst, size_t stride) {
    const int p = blockIdx.y * 256 + threadIdx.x, j = blockIdx.x;
    if (p >= L.P) return;
    const int s0 = chain_offsets[j];
    dst[(size_t)j * stride + p] = genome_param(noise, sc + (size_t)j * sc_stride, L, seeds + s0, powers + s0, chain_offsets[j + 1] - s0, p);
}

// promotion: new bank slot j = theta of descriptor j over the OLD bank (`src` and `dst` are the two halves of a double buffer, so a kept
// parent may move and two entries may name one source)
__global__ __launch_bounds__(256) void k_mujoco_ga_promote(const float *__restrict__ noise, Layout L, const float *__restrict__ sc, int sc_stride,
                                                           const float *__restrict__ src, float *__restrict__ dst, size_t stride,
                                                           const int32_t *__restrict__ parent, const int64_t *__restrict__ idx,
                                                           const float *__restrict__ power) {
    const int p = blockIdx.y * 256 + threadIdx.x, j = blockIdx.x;
    if (p >= L.P) return;
    dst[(size_t)j * stride + p] = descriptor_param(noise, sc + (size_t)j * sc_stride, L, src, stride, parent[j], idx[j], power[j], p);
}
#endif

}  // namespace mujoco_ga
}  // namespace dne
