// dense_ga.h -- Deep-GA on a dense policy of any small shape (gpu_implementation/ga.py over DNE_KIND_DENSE): maze_ga.h's device-resident bank
// of parents with P a run-time value.  The arithmetic is maze_ga.h's own (member_param, genome_param, root_param: used, not copied -- none of
// them depends on P); what is written here is what maze_ga.h bakes to 498: the checks, the CPU twins (genome_host, members_host, behind
// dne_dense_ga_theta_host / dne_dense_ga_members_host) and three small kernels for gfx950, which agree bit for bit.  DESIGN.md section 17a:
//   * genome (idx0, (idx1, power1), ...): theta_p = fl(noise[idx0 + p] * scale_by[p]), then per mutation, in order,
//     theta_p = theta_p + fl(power_j * noise[idx_j + p]) -- maze::perturbed, never fused (-ffp-contract=off on both passes);
//     scale_by is policies.dense_scale_by(env_kind, hidden, n_out);
//   * member descriptor (parent, idx, power) against a bank of T parents:
//       root   parent == -1, idx >= 0       fl(noise[idx + p] * scale_by[p]); power is not read
//       child  0 <= parent < T, idx >= 0    bank[parent][p] + fl(power * noise[idx + p])
//       kept   0 <= parent < T, idx < 0     bank[parent][p], bit for bit (promotion only)
// k_dense_run (csrc/dense.h) evaluates a child as it stands, in its episode mode: (base slot, noise offset, scale) = (the parent's bank slot,
// idx, power).  A root is written into a scratch slot by k_dense_ga_roots and evaluated there at scale 0 and the member's own idx:
// theta + fl(0 * eps) keeps every bit, since a zero parameter of a root carries eps's sign and so does fl(0 * eps) (k_dense_run stages theta
// with maze::perturbed, as k_maze_rollout does).
// A plain C++ compiler can include this file (the kernels are behind __HIPCC__): tests/dense_ga_asan_main.cpp does.
#pragma once
#include "dense.h"
#include "maze_ga.h"

namespace dne {
namespace dense_ga {

using maze_ga::genome_param;
using maze_ga::member_param;
using maze_ga::root_param;

// ---- what both sides refuse, by name (the engine's entry points and the host twins share these) ---------------------------------------------
inline std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    char buf[256];
    snprintf(buf, sizeof(buf), f, a, b, c, d);
    return buf;
}

inline bool in_table(int64_t idx, int P, size_t count) { return idx >= 0 && (uint64_t)idx + (uint64_t)P <= (uint64_t)count; }

// one descriptor against a bank of T parents of P parameters and a table of `count` floats; "" when it stands
inline std::string check_member(int i, int T, int P, size_t count, int parent, int64_t idx, bool kept_allowed) {
    if (parent < -1) return fmt("member %lld: parent %lld (-1 is a root, 0 .. T - 1 a parent)", i, parent);
    if (parent >= 0 && T < 1) return fmt("member %lld: parent %lld on an empty bank", i, parent);
    if (parent >= T) return fmt("member %lld: parent %lld, the bank holds %lld", i, parent, T);
    if (idx < 0) {
        if (parent < 0) return fmt("member %lld: a root needs a noise index, got %lld", i, (long long)idx);
        if (!kept_allowed) return fmt("member %lld: the kept form (parent %lld, idx %lld) is for promotion only, an evaluation takes power 0 at a real index", i, parent, (long long)idx);
        return "";
    }
    if (!in_table(idx, P, count)) return fmt("member %lld: noise index %lld + P = %lld outside the table of %lld", i, (long long)idx, P, (long long)count);
    return "";
}

// T genomes, chain_offsets [T + 1] into seeds / powers
inline std::string check_genomes(int T, int P, const int32_t *chain_offsets, const int64_t *seeds, size_t count) {
    for (int j = 0; j < T; j++) {
        if (chain_offsets[j + 1] <= chain_offsets[j]) return fmt("genome %lld: empty chain", j);
        for (int s = chain_offsets[j]; s < chain_offsets[j + 1]; s++)
            if (!in_table(seeds[s], P, count)) return fmt("genome %lld: noise index %lld + P = %lld outside the table of %lld", j, (long long)seeds[s], P, (long long)count);
    }
    return "";
}

// ---- the CPU side ------------------------------------------------------------------------------------------------------------------------------
inline void genome_host(const float *noise, const float *scale_by, int P, const int64_t *seeds, const float *powers, int nseeds, float *out) {
    for (int p = 0; p < P; p++) out[p] = genome_param(noise, scale_by, seeds, powers, nseeds, p);
}

// bank [T][P] packed, out [n][P]
inline void members_host(const float *noise, const float *scale_by, int P, const float *bank, const int32_t *parent, const int64_t *idx,
                         const float *power, int n, float *out) {
    for (int i = 0; i < n; i++)
        for (int p = 0; p < P; p++) out[(size_t)i * P + p] = member_param(noise, scale_by, bank, (size_t)P, parent[i], idx[i], power[i], p);
}

#if defined(__HIPCC__)
// ---- the device side: grid (count, ceil(P / 256)), 256 threads; block (x, y) writes parameters [256 y, 256 y + 256) of entry x ------------------
// the bank's first parents from their genomes (the start, load_population, a resume): dst slot j = genome j
__global__ __launch_bounds__(256) void k_dense_ga_build(const float *__restrict__ noise, const float *__restrict__ scale_by, int P,
                                                        const int32_t *__restrict__ chain_offsets, const int64_t *__restrict__ seeds,
                                                        const float *__restrict__ powers, float *__restrict__ dst, size_t stride) {
    const int p = blockIdx.y * 256 + threadIdx.x, j = blockIdx.x;
    if (p >= P) return;
    const int s0 = chain_offsets[j];
    dst[(size_t)j * stride + p] = genome_param(noise, scale_by, seeds + s0, powers + s0, chain_offsets[j + 1] - s0, p);
}

// promotion: new bank slot j = theta of descriptor j over the OLD bank (`src` and `dst` are the two halves of a double buffer, so a kept
// parent may move and two entries may name one source)
__global__ __launch_bounds__(256) void k_dense_ga_promote(const float *__restrict__ noise, const float *__restrict__ scale_by, int P,
                                                          const float *__restrict__ src, float *__restrict__ dst, size_t stride,
                                                          const int32_t *__restrict__ parent, const int64_t *__restrict__ idx,
                                                          const float *__restrict__ power) {
    const int p = blockIdx.y * 256 + threadIdx.x, j = blockIdx.x;
    if (p >= P) return;
    dst[(size_t)j * stride + p] = member_param(noise, scale_by, src, stride, parent[j], idx[j], power[j], p);
}

// the roots among an evaluation's members, each into its own scratch slot: member i is a root when its base slot is root0 + i
__global__ __launch_bounds__(256) void k_dense_ga_roots(const float *__restrict__ noise, const float *__restrict__ scale_by, int P,
                                                        const int32_t *__restrict__ m_slot, const int64_t *__restrict__ m_off, int root0,
                                                        float *__restrict__ mem, size_t stride) {
    const int p = blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
    if (p >= P || m_slot[i] != root0 + i) return;
    mem[(size_t)m_slot[i] * stride + p] = root_param(noise[m_off[i] + p], scale_by[p]);
}
#endif

}  // namespace dense_ga
}  // namespace dne
