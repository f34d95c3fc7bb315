// Stand-alone host program over csrc/maze_novelty.h's pool form for tests/test_maze_gans_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: novelty_pool_host on the cases of the text file given as argv[1], each in
// exactly sized heap buffers (no archive buffer at all when narch is 0) so that any access past the members, the archive or the results is reported.
// The file: per case one line "n narch k", then n * 2 member coordinates and narch * 2 archive coordinates as strtof reads them (hex floats,
// "nan", "inf").  Prints per case one line of n results (%a; a NaN as "nan"), then "ok <cases>"; a sanitizer finding aborts it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "maze_novelty.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES_FILE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    auto number = [&](float *v) {
        std::string tok;
        if (!(in >> tok)) return false;
        char *end = nullptr;
        *v = strtof(tok.c_str(), &end);
        return end != tok.c_str() && *end == 0;
    };
    int cases = 0, n, narch, k;
    while (in >> n >> narch >> k) {
        if (n < 1 || narch < 0 || k < 1 || narch + n - 1 < 1) { fprintf(stderr, "bad case header\n"); return 2; }
        float *xy = new float[(size_t)n * 2];
        float *arch = narch ? new float[(size_t)narch * 2] : nullptr;
        for (int i = 0; i < 2 * n; i++) if (!number(&xy[i])) { fprintf(stderr, "short case\n"); return 2; }
        for (int i = 0; i < 2 * narch; i++) if (!number(&arch[i])) { fprintf(stderr, "short case\n"); return 2; }
        std::vector<double> out((size_t)n);
        dne::maze_novelty::novelty_pool_host(xy, n, arch, narch, k, out.data());
        for (int i = 0; i < n; i++) {
            if (out[i] != out[i]) printf("nan%c", i + 1 < n ? ' ' : '\n');
            else printf("%a%c", out[i], i + 1 < n ? ' ' : '\n');
        }
        delete[] xy;
        delete[] arch;
        cases++;
    }
    printf("ok %d\n", cases);
    return 0;
}
