// nses.py:12-32 on the device: k-NN novelty of n trajectories against the archive.
//
// k_knn_dist: one workgroup per tile of NV_T members x NV_T archive entries, both sides ordered by length on the host so
// that a tile walks few rows past its pairs' ends.  Rows are staged in LDS once per tile (each trajectory's row index
// clamped to its length - 1: the reference's "pad the shorter with its last row", and rows past a member's length --
// stale data of an earlier, longer evaluation -- are never read).  Per pair and row, |x - y|^2 = |x|^2 + |y|^2 - 2 x.y
// with the cross term from v_dot4_u32_u8 and the row norms taken while staging; rows < lo go to A, rows in [lo, hi) to
// B, rows >= hi are masked.  A and B are exact integers (int64), then sqrt(sqrt(A)^2 + sqrt(B)^2) in the oracle's order
// (orc_bc_distance; the Makefile's -ffp-contract=off keeps a*a + b*b unfused).
// k_knn_select: one wave per member takes its kk smallest distances in ascending order (by value, ties by archive
// slot) and sums them one by one: bit for bit "sort ascending, sum the first kk, divide".  Each of the kk steps is a
// pass over the member's narch distances, so its cost is O(kk * narch) per member: small at the drivers' k = 10,
// quadratic in the archive size when k approaches it.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdint>

namespace dne {

constexpr int NV_T = 32;       // members (and archive entries) per tile
constexpr int NV_R = 4;        // row steps staged per barrier: one per wave
constexpr int NV_W = 32;       // words per row step (a 128-byte chunk of a row; wider rows take several steps)
constexpr int NV_P = 36;       // LDS pitch in words: the 8 rows one ds_read_b128 lane group reads sit on 8 disjoint 16-B bank slots
constexpr int NV_FLUSH = 64;   // row steps per wave between flushes of the 32-bit partial sums (|X| <= 64 * 2 * 128 * 255^2 < 2^31)

// the 16 cross terms of one lane's 4 members x 4 archive entries over one staged row step, accumulated into acc
__device__ __forceinline__ void nv_row_dots(const uint32_t *__restrict__ sm, const uint32_t *__restrict__ sa, uint32_t (&acc)[4][4]) {
#pragma unroll 1
    for (int g = 0; g < NV_W / 4; g++) {
        uint4 xm[4], xa[4];
#pragma unroll
        for (int j = 0; j < 4; j++) xm[j] = *(const uint4 *)(sm + j * 8 * NV_P + 4 * g);
#pragma unroll
        for (int k = 0; k < 4; k++) xa[k] = *(const uint4 *)(sa + k * 8 * NV_P + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t s = acc[j][k];
                s = __builtin_amdgcn_udot4(xm[j].x, xa[k].x, s, false);
                s = __builtin_amdgcn_udot4(xm[j].y, xa[k].y, s, false);
                s = __builtin_amdgcn_udot4(xm[j].z, xa[k].z, s, false);
                s = __builtin_amdgcn_udot4(xm[j].w, xa[k].w, s, false);
                acc[j][k] = s;
            }
    }
}

// nses.py:20 on the exact sums: a = sqrt(A), b = sqrt(B), sqrt(a*a + b*b) (orc_bc_distance's three roundings)
__device__ __forceinline__ double nv_distance(unsigned long long A, unsigned long long B) {
    const double a = sqrt((double)A), b = sqrt((double)B);
    return sqrt(a * a + b * b);
}

// grid (ceil(n / NV_T), ceil(narch / NV_T), rsplit), 256 threads.  Both sides come in length order: slot s of a side is the
// trajectory of row0[s] (rows of pw words, pw a multiple of 4, zero-padded) with len[s] rows.  dist[m][a] is written in
// those orders; the selection kernel does not care about the archive's order and maps members back itself.  A small grid
// (few tiles, e.g. the one-trajectory call) splits each tile's row steps over rsplit workgroups: they add their sums to
// acc[n][narch][2] (zeroed by the caller) and k_knn_finish takes the square roots; with rsplit = 1, acc is unused.
__global__ __launch_bounds__(256) void k_knn_dist(const uint32_t *__restrict__ mrows, const int64_t *__restrict__ mrow0,
                                                  const int32_t *__restrict__ mlen, int n,
                                                  const uint32_t *__restrict__ arows, const int64_t *__restrict__ arow0,
                                                  const int32_t *__restrict__ alen, int narch, int pw,
                                                  unsigned long long *__restrict__ acc, double *__restrict__ dist /*[n][narch]*/) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[NV_R * 2 * NV_T * NV_P];   // [step][slot: members, then archive][NV_P]
    __shared__ uint32_t snorm[NV_R * 2 * NV_T];
    __shared__ int64_t srow0[2 * NV_T];
    __shared__ int32_t slen[2 * NV_T];
    __shared__ unsigned long long red[2 * NV_T * NV_T];                               // the tile's A, then B
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.x * NV_T, a0 = blockIdx.y * NV_T;
    const int nchunk = (pw + NV_W - 1) / NV_W;
    for (int p = tid; p < 2 * NV_T * NV_T; p += 256) red[p] = 0;
    if (tid < 2 * NV_T) {   // pad slots repeat the side's last trajectory; their pairs are computed and never written
        const bool mem = tid < NV_T;
        const int cnt = mem ? n : narch, i = (mem ? m0 : a0) + (tid & (NV_T - 1));
        const int s = i < cnt ? i : cnt - 1;
        srow0[tid] = mem ? mrow0[s] : arow0[s];
        slen[tid] = mem ? mlen[s] : alen[s];
    }
    __syncthreads();
    int mlo = INT_MAX, mhi = 0, alo = INT_MAX, ahi = 0;
    for (int s = 0; s < NV_T; s++) {
        mlo = min(mlo, slen[s]); mhi = max(mhi, slen[s]);
        alo = min(alo, slen[NV_T + s]); ahi = max(ahi, slen[NV_T + s]);
    }
    const int S = max(mhi, ahi) * nchunk;          // row steps: the tile's longest trajectory, one step per 128-byte chunk
    const int G = (S + NV_R - 1) / NV_R;
    const int gz = (G + (int)gridDim.z - 1) / (int)gridDim.z, gb = (int)blockIdx.z * gz, ge = min(G, gb + gz);   // this block's steps

    // staging: 4 steps x 64 slots x 8 uint4 = 2048 loads, 8 per thread; 8 consecutive lanes share a row (norm by shuffle)
    uint4 pre[8];
    auto load = [&](int g) {
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const int u = tid + 256 * v, slot = (u >> 3) & 63, part = u & 7, q = g * NV_R + (u >> 9);
            const int c = q % nchunk, w = c * NV_W + 4 * part;
            pre[v] = make_uint4(0, 0, 0, 0);
            if (q < S && w < pw) {
                const int i = q / nchunk, L = slen[slot];
                const int64_t row = srow0[slot] + (i < L ? i : L - 1);
                pre[v] = *(const uint4 *)((slot < NV_T ? mrows : arows) + row * pw + w);
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const int u = tid + 256 * v, rs = u >> 3, part = u & 7;   // rs = step * 64 + slot
            *(uint4 *)(stage + rs * NV_P + 4 * part) = pre[v];
            uint32_t nr = __builtin_amdgcn_udot4(pre[v].x, pre[v].x, 0u, false);
            nr = __builtin_amdgcn_udot4(pre[v].y, pre[v].y, nr, false);
            nr = __builtin_amdgcn_udot4(pre[v].z, pre[v].z, nr, false);
            nr = __builtin_amdgcn_udot4(pre[v].w, pre[v].w, nr, false);
            nr += __shfl_xor(nr, 1); nr += __shfl_xor(nr, 2); nr += __shfl_xor(nr, 4);
            if (part == 0) snorm[rs] = nr;
        }
    };

    // lane (mg, ag) owns members mg + 8j and archive entries ag + 8k, j, k < 4
    const int mg = lane >> 3, ag = lane & 7;
    int ml[4], al[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { ml[j] = slen[mg + 8 * j]; al[j] = slen[NV_T + ag + 8 * j]; }
    // Per pair and flush window, X = sum over the rows where the whole tile is in A (in B) of 2 x.y, minus the full
    // |x - y|^2 of the rows classified pair by pair; the norms of the first kind of row are summed per lane.  The window's
    // A (B) is then Nm + Na - X, added to the block's int64 sums in LDS.
    int32_t XA[4][4], XB[4][4];
    uint32_t NmA[4], NaA[4], NmB[4], NaB[4];
    auto reset = [&]() {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            NmA[j] = NaA[j] = NmB[j] = NaB[j] = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) XA[j][k] = XB[j][k] = 0;
        }
    };
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int p = (mg + 8 * j) * NV_T + ag + 8 * k;
                atomicAdd(red + p, (unsigned long long)((int64_t)NmA[j] + NaA[k] - XA[j][k]));
                atomicAdd(red + NV_T * NV_T + p, (unsigned long long)((int64_t)NmB[j] + NaB[k] - XB[j][k]));
            }
        reset();
    };
    reset();

    int since = 0;
    if (gb < ge) load(gb);
    for (int g = gb; g < ge; g++) {
        if (g > gb) __syncthreads();
        store();
        __syncthreads();
        if (g + 1 < ge) load(g + 1);                // in flight while this step computes
        const int q = g * NV_R + wave;
        if (q >= S) continue;                       // wave-uniform
        const int i = q / nchunk;
        const uint32_t *sm = stage + (wave * 2 * NV_T + mg) * NV_P, *sa = stage + (wave * 2 * NV_T + NV_T + ag) * NV_P;
        const uint32_t *nrm = snorm + wave * 2 * NV_T;
        uint32_t t[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) t[j][k] = 0;
        nv_row_dots(sm, sa, t);
        if (i < min(mlo, alo)) {                                          // every pair: i < lo
#pragma unroll
            for (int j = 0; j < 4; j++) {
                NmA[j] += nrm[mg + 8 * j]; NaA[j] += nrm[NV_T + ag + 8 * j];
#pragma unroll
                for (int k = 0; k < 4; k++) XA[j][k] += 2 * t[j][k];
            }
        } else if ((i >= mhi && i < alo) || (i >= ahi && i < mlo)) {      // every pair: lo <= i < hi
#pragma unroll
            for (int j = 0; j < 4; j++) {
                NmB[j] += nrm[mg + 8 * j]; NaB[j] += nrm[NV_T + ag + 8 * j];
#pragma unroll
                for (int k = 0; k < 4; k++) XB[j][k] += 2 * t[j][k];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int32_t nm = nrm[mg + 8 * j];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int32_t val = nm + (int32_t)nrm[NV_T + ag + 8 * k] - 2 * (int32_t)t[j][k];
                    const bool inm = i < ml[j], ina = i < al[k];
                    if (inm && ina) XA[j][k] -= val;
                    else if (inm != ina) XB[j][k] -= val;
                }
            }
        }
        if (++since == NV_FLUSH) { flush(); since = 0; }
    }
    flush();
    __syncthreads();
    for (int p = tid; p < NV_T * NV_T; p += 256) {
        const int m = m0 + p / NV_T, a = a0 + p % NV_T;
        if (m >= n || a >= narch) continue;
        const size_t q = (size_t)m * narch + a;
        if (gridDim.z == 1) {
            dist[q] = nv_distance(red[p], red[NV_T * NV_T + p]);
        } else {
            atomicAdd(acc + 2 * q, red[p]);
            atomicAdd(acc + 2 * q + 1, red[NV_T * NV_T + p]);
        }
    }
}

// after a split k_knn_dist: the distances from the summed A, B.  grid ceil(pairs / 256)
__global__ __launch_bounds__(256) void k_knn_finish(const unsigned long long *__restrict__ acc, size_t pairs, double *__restrict__ dist) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < pairs) dist[q] = nv_distance(acc[2 * q], acc[2 * q + 1]);
}

// grid ceil(n / 4), 256 threads: wave w of block b scores member slot 4b + w (length order) and writes out[morder[slot]]
__global__ __launch_bounds__(256) void k_knn_select(const double *__restrict__ dist, int n, int narch, int kk,
                                                    const int32_t *__restrict__ morder, double *__restrict__ out) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= n) return;                             // wave-uniform
    const double *d = dist + (size_t)m * narch;
    double pv = -1.0, s = 0.0;                      // distances are >= 0: every slot comes after (-1, -1)
    int pj = -1;
    for (int t = 0; t < kk; t++) {                  // the next (value, slot) after (pv, pj): ascending order, ties by slot
        double bv = INFINITY;
        int bj = INT_MAX;
        for (int j = lane; j < narch; j += 64) {
            const double v = d[j];
            if ((v > pv || (v == pv && j > pj)) && v < bv) { bv = v; bj = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oj = __shfl_xor(bj, o);
            if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
        }
        s += bv;                                    // nses.py:31, one by one in ascending order
        pv = bv; pj = bj;
    }
    if (lane == 0) out[morder[m]] = s / kk;
}

}  // namespace dne
