// k_out<2, true> ALONE at full width: one launch over `pairs` antithetic pairs (default 2500, the bench's population) between two device
// events, the chip to itself, median / minimum over the repetitions.  The kernel is the library's own (csrc/forward.h is included,
// not copied); the inputs are synthetic -- its cost does not depend on their values: a 250 M-float noise table, one base vector, random
// slice offsets (a fresh set of offsets every launch, eight sets in rotation, so that the 46 MB of output-layer noise rows of a launch
// are not the ones the last launches left in the Infinity Cache), fc partial sums and batch-norm rows of the right shape, nobody finished.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I deep-neuroevolution_amd/csrc -o out_alone tools/micro/out_alone.hip
//   ./out_alone [pairs] [reps] [nact]
// -DOUT_STRIDED builds against a csrc tree from before the staged output layer (k_out<NV, HAS_BN>, no dynamic LDS): the A/B's other side.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "env_synth.h"
#include "forward.h"
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
using namespace dne;

__global__ void k_fill(float *p, size_t n, unsigned seed) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned x = (unsigned)i * 2654435761u + seed; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        p[i] = ((int)(x & 0xffff) - 32768) * (1.0f / 16384.0f);
    }
}

int main(int argc, char **argv) {
    const int pairs = argc > 1 ? atoi(argv[1]) : 2500, reps = argc > 2 ? atoi(argv[2]) : 200, nact = argc > 3 ? atoi(argv[3]) : 18;
    const int members = 2 * pairs, SETS = 8;
    const size_t N = 250000000;
    if (pairs < 1 || reps < 1 || nact < 1 || nact > OUT_NA) { printf("usage: out_alone [pairs] [reps] [nact <= %d]\n", OUT_NA); return 1; }
    Layout L = {};
    L.kind = 0; L.nact = nact;
    int o = 0;
    L.c1w = o; o += 8 * 8 * 4 * 16; L.c1b = o; o += 16; L.bn1b = o; o += 16; L.bn1g = o; o += 16;
    L.c2w = o; o += 4 * 4 * 16 * 32; L.c2b = o; o += 32; L.bn2b = o; o += 32; L.bn2g = o; o += 32;
    L.fcw = o; o += 3872 * 256; L.fcb = o; o += 256; L.bn3b = o; o += 256; L.bn3g = o; o += 256;
    L.ow = o; o += 256 * nact; L.ob = o; o += nact; L.P = o; L.c3w = L.c3b = -1;

    float *noise, *base, *scale, *bn, *y3t, *y3;
    int32_t *slot, *done, *actions;
    int *list;
    int64_t *off[SETS];
    CK(hipMalloc(&noise, N * 4)); CK(hipMalloc(&base, (size_t)L.P * 4)); CK(hipMalloc(&scale, members * 4)); CK(hipMalloc(&bn, (size_t)members * 608 * 4));
    CK(hipMalloc(&y3t, (size_t)members * 4 * 256 * 4)); CK(hipMalloc(&y3, (size_t)members * 256 * 4));
    CK(hipMalloc(&slot, members * 4)); CK(hipMalloc(&done, members * 4)); CK(hipMalloc(&actions, members * 4)); CK(hipMalloc(&list, pairs * 4));
    k_fill<<<4096, 256>>>(noise, N, 1u); k_fill<<<256, 256>>>(base, (size_t)L.P, 2u); k_fill<<<256, 256>>>(bn, (size_t)members * 608, 3u);
    k_fill<<<1024, 256>>>(y3t, (size_t)members * 4 * 256, 4u);
    CK(hipMemset(slot, 0, members * 4)); CK(hipMemset(done, 0, members * 4));
    std::mt19937_64 rng(12345);
    std::vector<float> hs(members);
    std::vector<int> hl(pairs);
    for (int g = 0; g < pairs; g++) { hs[2 * g] = 0.02f; hs[2 * g + 1] = -0.02f; hl[g] = g; }
    CK(hipMemcpy(scale, hs.data(), members * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(list, hl.data(), pairs * 4, hipMemcpyHostToDevice));
    for (int s = 0; s < SETS; s++) {
        std::vector<int64_t> ho(members);
        for (int g = 0; g < pairs; g++) ho[2 * g] = ho[2 * g + 1] = (int64_t)(rng() % (N - (size_t)L.P));
        CK(hipMalloc(&off[s], members * 8)); CK(hipMemcpy(off[s], ho.data(), members * 8, hipMemcpyHostToDevice));
    }
    FwdArgs A = {};
    A.noise = noise; A.bases = base; A.base_stride = (size_t)L.P; A.m_slot = slot; A.m_scale = scale; A.bn = bn; A.bn_mom = nullptr; A.done = done;
    A.zero_rows = nullptr; A.sub_sums = 0; A.L = L; A.tt.n = 0;
#ifdef OUT_STRIDED
    auto launch = [&]() { hipLaunchKernelGGL((k_out<2, true>), dim3(pairs), dim3(256), 0, 0, A, (const int *)list, (const float *)y3t, y3, actions, (float *)nullptr); };
    const char *form = "strided";
#else
    const size_t lds = out_stage_bytes(2, nact);
    CK(hipFuncSetAttribute((const void *)k_out<2, true, OUT_NA_ATARI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)out_stage_bytes(2, OUT_NA)));
    CK(hipFuncSetAttribute((const void *)k_out<2, true, OUT_NA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)out_stage_bytes(2, OUT_NA)));
    auto launch = [&]() {
        if (nact <= OUT_NA_ATARI) hipLaunchKernelGGL((k_out<2, true, OUT_NA_ATARI>), dim3(pairs), dim3(256), lds, 0, A, (const int *)list, (const float *)y3t, y3, actions, (float *)nullptr);
        else hipLaunchKernelGGL((k_out<2, true, OUT_NA>), dim3(pairs), dim3(256), lds, 0, A, (const int *)list, (const float *)y3t, y3, actions, (float *)nullptr);
    };
    const char *form = "staged";
#endif
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int r = -10; r < reps; r++) {   // ten warm-up launches
        A.m_off = off[(r + 10) % SETS];
        CK(hipEventRecord(e0, 0));
        launch();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) us.push_back(ms * 1e3f);
    }
    std::vector<int32_t> ha(members);
    CK(hipMemcpy(ha.data(), actions, members * 4, hipMemcpyDeviceToHost));
    long long asum = 0;
    for (int a : ha) asum += a;
    std::sort(us.begin(), us.end());
    printf("{\"tool\": \"out_alone\", \"form\": \"%s\", \"pairs\": %d, \"nact\": %d, \"reps\": %d, \"us_min\": %.2f, \"us_median\": %.2f, \"us_p90\": %.2f, \"us_max\": %.2f, \"action_sum\": %lld}\n",
           form, pairs, nact, reps, us.front(), us[us.size() / 2], us[us.size() * 9 / 10], us.back(), asum);
    return 0;
}
