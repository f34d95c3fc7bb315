// Stand-alone host program over csrc/ram_novelty.h for tests/test_atari_gans_cpu.py, which builds it with -fsanitize=address,undefined and
// runs it: novelty_pool_host on the cases of the text file given as argv[1], each in exactly sized heap buffers so that any access past the
// members, the archive, the results or the neighbours is reported.  With narch == 0 there is no archive buffer at all: the function gets a
// null pointer.
// Per case one line "n narch k", then n * 128 member bytes and narch * 128 archive bytes as decimal numbers; prints per case one line: the n
// novelties as %a, then the n * min(k, narch + n - 1) neighbours.  The last line is "ok <cases>"; a sanitizer finding aborts the program.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "ram_novelty.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES_FILE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int W = dne::ram_novelty::ROW;
    int cases = 0, n, narch, k;
    while (in >> n >> narch >> k) {
        if (n < 1 || narch < 0 || k < 1 || narch + n - 1 < 1) { fprintf(stderr, "bad case header\n"); return 2; }
        const int kk = k < narch + n - 1 ? k : narch + n - 1;
        uint8_t *bc = new uint8_t[(size_t)n * W];
        uint8_t *arch = narch ? new uint8_t[(size_t)narch * W] : nullptr;
        int v;
        for (int i = 0; i < W * n; i++) { if (!(in >> v) || v < 0 || v > 255) { fprintf(stderr, "short case\n"); return 2; } bc[i] = (uint8_t)v; }
        for (int i = 0; i < W * narch; i++) { if (!(in >> v) || v < 0 || v > 255) { fprintf(stderr, "short case\n"); return 2; } arch[i] = (uint8_t)v; }
        double *out = new double[(size_t)n];
        int32_t *nb = new int32_t[(size_t)n * kk];
        dne::ram_novelty::novelty_pool_host(bc, n, arch, narch, k, out, nb);
        for (int i = 0; i < n; i++) printf("%a ", out[i]);
        for (int i = 0; i < n * kk; i++) printf("%d%c", nb[i], i + 1 < n * kk ? ' ' : '\n');
        delete[] bc;
        delete[] arch;
        delete[] out;
        delete[] nb;
        cases++;
    }
    printf("ok %d\n", cases);
    return 0;
}
