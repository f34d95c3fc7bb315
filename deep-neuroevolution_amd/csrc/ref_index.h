// ref_index.h -- the reference batch as unique convolution operands, built on the host from plain bytes: no HIP, no kernels, no handle.
// The F reference frames of virtual batch norm are consecutive observations of one rollout and stay fixed for a whole run, so most
// im2col rows of conv1 (8x8x4 patches of the zero-padded 88x88 image, as k_ref_to_float pads it) and of conv2 (4x4 windows of conv1
// positions, SAME(1,2)) are byte-identical to another row.  An output row of v_mfma_f32_16x16x4_f32 depends only on its own A row, B
// and the k order, so the reference pass computes every distinct row once per member and lays the values back out (forward.h:
// k_conv1_ref_uniq, k_bn1_gather, k_conv2_ref_uniq, k_y2_expand).  dne_set_ref_batch builds the index once; dne_debug_ref_index walks
// the same function without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace dne {

struct RefIndex {
    int F = 0, U1 = 0, U2 = 0;
    std::vector<int32_t> idx1;      // [F][441]: id of the conv1 patch at position oy * 21 + ox among the unique ones (first-seen order)
    std::vector<uint8_t> patches;   // [U1][256]: the unique patches, k = (kh * 8 + kw) * 4 + c -- the order k_conv1_ref_shared's B fragments assume
    std::vector<int32_t> idx2;      // [F][121]: id of the conv2 window at position oy * 11 + ox among the unique ones
    std::vector<int32_t> windows;   // [U2][16]: a window's sixteen conv1 patch ids in (kh, kw) order, -1 = SAME padding
};

constexpr int RI_N1 = 441, RI_N2 = 121, RI_K1 = 256, RI_K2 = 16;

// rows of NB bytes -> ids of the distinct ones in first-seen order (open addressing; equal hash is confirmed byte by byte)
template <int NB>
struct RowDedup {
    static_assert(NB % 8 == 0, "rows are hashed in 8-byte words");
    std::vector<int32_t> slot;
    std::vector<uint64_t> hash_of;   // per unique row
    std::vector<uint8_t> *rows;
    uint32_t mask;
    RowDedup(size_t max_rows, std::vector<uint8_t> *out) : rows(out) {
        size_t cap = 64;
        while (cap < 2 * max_rows) cap <<= 1;
        slot.assign(cap, -1);
        mask = (uint32_t)(cap - 1);
    }
    static uint64_t hash(const uint8_t *p) {
        uint64_t h = 0x243F6A8885A308D3ull;
        for (int i = 0; i < NB; i += 8) {
            uint64_t w;
            memcpy(&w, p + i, 8);
            h = (h ^ w) * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
        }
        return h;
    }
    int32_t id(const uint8_t *p) {
        const uint64_t h = hash(p);
        for (uint32_t s = (uint32_t)(h >> 20) & mask;; s = (s + 1) & mask) {
            const int32_t u = slot[s];
            if (u < 0) {
                const int32_t n = (int32_t)hash_of.size();
                slot[s] = n;
                hash_of.push_back(h);
                rows->insert(rows->end(), p, p + NB);
                return n;
            }
            if (hash_of[u] == h && memcmp(rows->data() + (size_t)u * NB, p, NB) == 0) return u;
        }
    }
};

// ref: [F][84][84][4] u8
inline void build_ref_index(const uint8_t *ref, int F, RefIndex *R) {
    R->F = F;
    R->idx1.assign((size_t)F * RI_N1, 0);
    R->idx2.assign((size_t)F * RI_N2, 0);
    R->patches.clear();
    R->windows.clear();
    std::vector<uint8_t> win_bytes;
    RowDedup<RI_K1> d1((size_t)F * RI_N1, &R->patches);
    RowDedup<RI_K2 * 4> d2((size_t)F * RI_N2, &win_bytes);
    std::vector<uint8_t> img(88 * 88 * 4);
    for (int f = 0; f < F; f++) {
        memset(img.data(), 0, img.size());   // a padding zero equals a pixel zero
        for (int r = 0; r < 84; r++) memcpy(&img[((r + 2) * 88 + 2) * 4], ref + ((size_t)f * 84 + r) * 84 * 4, 84 * 4);
        int32_t *i1 = &R->idx1[(size_t)f * RI_N1];
        for (int oy = 0; oy < 21; oy++)
            for (int ox = 0; ox < 21; ox++) {
                uint8_t patch[RI_K1];
                for (int kh = 0; kh < 8; kh++) memcpy(patch + kh * 32, &img[((4 * oy + kh) * 88 + 4 * ox) * 4], 32);
                i1[oy * 21 + ox] = d1.id(patch);
            }
        for (int oy = 0; oy < 11; oy++)
            for (int ox = 0; ox < 11; ox++) {
                int32_t w[RI_K2];
                for (int kh = 0; kh < 4; kh++)
                    for (int kw = 0; kw < 4; kw++) {
                        const int y = 2 * oy + kh - 1, x = 2 * ox + kw - 1;
                        w[kh * 4 + kw] = y >= 0 && y < 21 && x >= 0 && x < 21 ? i1[y * 21 + x] : -1;
                    }
                R->idx2[(size_t)f * RI_N2 + oy * 11 + ox] = d2.id((const uint8_t *)w);
            }
    }
    R->U1 = (int)(R->patches.size() / RI_K1);
    R->U2 = (int)(win_bytes.size() / (RI_K2 * 4));
    R->windows.resize((size_t)R->U2 * RI_K2);
    if (R->U2) memcpy(R->windows.data(), win_bytes.data(), win_bytes.size());
}

// Which route the reference pass takes on the default knobs.  The dedup route computes U1 + U2 rows and then pays two gather passes
// over every position; the dense kernels compute every position and gather nothing.  The constants are the kernels' own times alone,
// ms per 5000 members at F = 128 (profiles/r07_ref_dedup_ab.json): the dense kernels; the unique-row GEMMs
// scaled from the fraction they ran at (2.789 ms at U1p / N1 = 0.1304, 4.350 ms at U2p / N2 = 0.2645) to a table as long as the dense
// im2col; the two gather passes, whose work does not depend on U.  The route pays when its sum is below the dense sum: an all-unique
// batch would cost 21.4 + 16.4 + 5.1 = 42.9 ms against 29.8, conv1 alone breaks even at U1 / N1 = 0.78, conv2 alone at 0.49.
constexpr float REF_MS_CONV1_DENSE = 18.30f, REF_MS_CONV2_DENSE = 11.46f;   // k_conv1_ref_shared<16>, k_conv2_ref<16, true>
constexpr float REF_MS_CONV1_UNIQ = 21.4f, REF_MS_CONV2_UNIQ = 16.4f;       // k_conv1_ref_uniq / k_conv2_ref_uniq at U = N
constexpr float REF_MS_GATHER = 1.71f + 3.34f;                              // k_bn1_gather + k_y2_expand
constexpr int REF_U1_PAD = 32, REF_U2_PAD = 64;   // rows per step of k_conv1_ref_uniq / k_conv2_ref_uniq: the tables are padded to whole steps
inline int ref_pad(int u, int to) { return (u + to - 1) / to * to; }
// the route's scratch -- y1u [U1p][16] and y2u [U2p][32] per member -- lives where the dense route keeps y1 [F][441][16]: both must fit
inline bool ref_dedup_fits(int F, int U1, int U2) {
    return (size_t)ref_pad(U1, REF_U1_PAD) * 16 + (size_t)ref_pad(U2, REF_U2_PAD) * 32 <= (size_t)F * RI_N1 * 16;
}
inline bool ref_dedup_pays(int F, int U1, int U2) {
    const float f1 = (float)U1 / (float)(F * RI_N1), f2 = (float)U2 / (float)(F * RI_N2);
    return REF_MS_CONV1_UNIQ * f1 + REF_MS_CONV2_UNIQ * f2 + REF_MS_GATHER < REF_MS_CONV1_DENSE + REF_MS_CONV2_DENSE && ref_dedup_fits(F, U1, U2);
}

}   // namespace dne
