// Stand-alone host program over csrc/mujoco_ga.h for tests/test_mujoco_ga_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it once: for every shape the two kinds build (the pendulum: hidden 64 / 128 / 256
// with 1..16 outputs; the maze: the same widths with 2, 4, .. 16) the layout against offsets written out here, then colscale_host, genome_host
// and members_host on a table in an exactly sized heap buffer whose LAST P floats are one of the slices -- so that a read past the slice, a
// row guard that lets row K = 3 or K = 11 through, or a write past a result is reported.  One column of each weight block is zeroed in a
// second slice: NaN there, and nowhere else.  P at hidden 256 is 68 864 + 257 O on the maze.
// Prints "ok <shapes> <facts>"; a sanitizer finding or a wrong fact aborts it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mujoco_ga.h"

namespace G = dne::mujoco_ga;

static long long facts = 0;
#define FACT(c)                                                                          \
    do {                                                                                 \
        if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); }           \
        facts++;                                                                         \
    } while (0)

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static float draw() {   // a few hundred distinct values in (-2, 2), none of them 0
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const int v = (int)((rng >> 40) % 801) - 400;
    return (v == 0 ? 1 : v) * 0.005f;
}

static void shape(int obs, int H, int O) {
    const G::Layout L = G::layout(obs, H, O);
    // the offsets, written out
    const int w1 = 0, b1 = obs * H, w2 = b1 + H, b2 = w2 + H * H, w3 = b2 + H, b3 = w3 + H * O, P = b3 + O;
    FACT(L.w[0] == w1 && L.b[0] == b1 && L.w[1] == w2 && L.b[1] == b2 && L.w[2] == w3 && L.b[2] == b3 && L.P == P && L.ncol == 2 * H + O);
    FACT(L.K[0] == obs && L.K[1] == H && L.K[2] == H && L.C[0] == H && L.C[1] == H && L.C[2] == O);
    FACT(G::shape_ok(obs, H, O));
    FACT(G::col_of(L, 0) == 0 && G::col_of(L, b1 - 1) == H - 1 && G::col_of(L, b1) == -1 && G::col_of(L, w2) == H && G::col_of(L, b2) == -1 &&
         G::col_of(L, w3) == 2 * H && G::col_of(L, b3 - 1) == 2 * H + O - 1 && G::col_of(L, b3) == -1 && G::col_of(L, P - 1) == -1);
    // the table: P + 29 floats, slices at 0, 29 (the last P floats) and 13
    const size_t count = (size_t)P + 29;
    std::vector<float> noise(count);
    for (float &v : noise) v = draw();
    const int64_t last = (int64_t)count - P;
    std::vector<float> sc((size_t)L.ncol), th((size_t)P);
    for (int64_t idx0 : {(int64_t)0, last}) {
        G::colscale_host(noise.data(), L, idx0, sc.data());
        for (int c = 0; c < L.ncol; c++) FACT(sc[c] > 0.0f && std::isfinite(sc[c]));
        const int64_t seeds[3] = {idx0, last - idx0, 13};
        const float powers[3] = {0.0f, 0.02f, -0.02f};
        FACT(G::check_genomes(1, P, std::vector<int32_t>{0, 3}.data(), seeds, count).empty());
        for (int n = 1; n <= 3; n++) {
            G::genome_host(noise.data(), L, seeds, powers, n, th.data());
            if (n > 1) continue;
            // a root: biases +0, every column of norm 1 to a few ulps of the K-term sum (checked in double)
            for (int l = 0; l < G::BLOCKS; l++) {
                for (int c = 0; c < L.C[l]; c++) FACT(bits(th[L.b[l] + c]) == 0u);
                for (int c = 0; c < L.C[l]; c += (L.C[l] > 16 ? 37 : 1)) {
                    double ss = 0;
                    for (int k = 0; k < L.K[l]; k++) ss += (double)th[L.w[l] + k * L.C[l] + c] * th[L.w[l] + k * L.C[l] + c];
                    FACT(std::fabs(std::sqrt(ss) - 1.0) < 1e-5);
                }
            }
        }
    }
    // members over a bank of two: a root at the table's end, a child, a kept parent; the refusals by name
    std::vector<float> bank((size_t)2 * P), out((size_t)4 * P);
    {
        const int64_t s0[1] = {0}, s1[2] = {last, 5};
        const float p0[1] = {0.0f}, p1[2] = {0.0f, 0.02f};
        G::genome_host(noise.data(), L, s0, p0, 1, bank.data());
        G::genome_host(noise.data(), L, s1, p1, 2, bank.data() + P);
    }
    const int32_t parent[4] = {-1, 1, 0, 1};
    const int64_t idx[4] = {last, last, -1, -9};
    const float power[4] = {7.0f, 0.02f, 0.5f, 0.0f};
    for (int i = 0; i < 4; i++) FACT(G::check_member(i, 2, P, count, parent[i], idx[i], true).empty());
    FACT(!G::check_member(2, 2, P, count, parent[2], idx[2], false).empty());            // the kept form in an evaluation
    FACT(!G::check_member(0, 2, P, count, 2, 0, true).empty());                           // parent >= T
    FACT(!G::check_member(0, 0, P, count, 0, 0, true).empty());                           // an empty bank
    FACT(!G::check_member(0, 2, P, count, -1, last + 1, true).empty());                   // idx + P past the table
    {
        const int32_t co[2] = {0, 0};
        const int64_t none[1] = {0};
        FACT(!G::check_genomes(1, P, co, none, count).empty());                             // an empty chain
    }
    G::members_host(noise.data(), L, bank.data(), parent, idx, power, 4, out.data());
    for (int p = 0; p < P; p += 7) {
        FACT(bits(out[(size_t)2 * P + p]) == bits(bank[p]) && bits(out[(size_t)3 * P + p]) == bits(bank[(size_t)P + p]));
        const float v = 0.02f * noise[last + p];
        FACT(bits(out[(size_t)P + p]) == bits(bank[(size_t)P + p] + v));
    }
    // a zero column in every block of the slice at 13: NaN in that column, and only there
    const int zc[3] = {H - 1, 0, O - 1};
    for (int l = 0; l < G::BLOCKS; l++)
        for (int k = 0; k < L.K[l]; k++) noise[13 + L.w[l] + k * L.C[l] + zc[l]] = (k & 1) ? -0.0f : 0.0f;
    const int64_t s13[1] = {13};
    const float p13[1] = {0.0f};
    G::genome_host(noise.data(), L, s13, p13, 1, th.data());
    for (int p = 0; p < P; p++) {
        const int c = G::col_of(L, p);
        const bool zero = c >= 0 && (c == zc[0] || c == H + zc[1] || c == 2 * H + zc[2]);
        if (th[p] != th[p]) FACT(zero); else if (zero) FACT(false);
    }
}

int main() {
    int shapes = 0;
    for (int H : {64, 128, 256}) {
        for (int O = 1; O <= dne::pendulum::MAX_OUT; O++) { shape(dne::pendulum::OBS, H, O); shapes++; }
        for (int O = 2; O <= dne::mjmaze::MAX_OUT; O += 2) { shape(dne::mjmaze::OBS, H, O); shapes++; }
    }
    FACT(G::layout(dne::mjmaze::OBS, 256, 2).P == 69378 && G::layout(dne::mjmaze::OBS, 256, 16).P == 72976);   // 13 H + H^2 + 257 O: far past dense_ga's 9 218
    FACT(!G::shape_ok(dne::pendulum::OBS, 32, 1) && !G::shape_ok(dne::mjmaze::OBS, 64, 3) && !G::shape_ok(dne::pendulum::OBS, 64, 17) && !G::shape_ok(5, 64, 2));
    printf("ok %d %lld\n", shapes, facts);
    return 0;
}
