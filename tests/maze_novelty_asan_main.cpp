// Stand-alone host program over csrc/maze_novelty.h for tests/test_maze_novelty_cpu.py and tests/test_maze_gans_cpu.py, which build it with
// -fsanitize=address,undefined,float-cast-overflow and run it: novelty_host (argv[1] "archive") or novelty_pool_host (argv[1] "pool") on the cases
// of the text file given as argv[2], each in exactly sized heap buffers (no archive buffer at all when narch is 0) so that any access past the
// members, the archive or the results is reported.
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
    if (argc != 3 || (strcmp(argv[1], "archive") && strcmp(argv[1], "pool"))) { fprintf(stderr, "usage: %s archive|pool CASES_FILE\n", argv[0]); return 2; }
    const bool pool = !strcmp(argv[1], "pool");
    std::ifstream in(argv[2]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    auto number = [&](float *v) {
        std::string tok;
        if (!(in >> tok)) return false;
        char *end = nullptr;
        *v = strtof(tok.c_str(), &end);
        return end != tok.c_str() && *end == 0;
    };
    int cases = 0, n, narch, k;
    while (in >> n >> narch >> k) {
        if (n < 1 || k < 1 || (pool ? narch < 0 || narch + n - 1 < 1 : narch < 1)) { fprintf(stderr, "bad case header\n"); return 2; }
        float *xy = new float[(size_t)n * 2];
        float *arch = narch ? new float[(size_t)narch * 2] : nullptr;
        for (int i = 0; i < 2 * n; i++) if (!number(&xy[i])) { fprintf(stderr, "short case\n"); return 2; }
        for (int i = 0; i < 2 * narch; i++) if (!number(&arch[i])) { fprintf(stderr, "short case\n"); return 2; }
        std::vector<double> out((size_t)n);
        (pool ? dne::maze_novelty::novelty_pool_host : dne::maze_novelty::novelty_host)(xy, n, arch, narch, k, out.data());
        for (int i = 0; i < n; i++) {
            if (out[i] != out[i]) printf("nan%c", i + 1 < n ? ' ' : '\n');
            else printf("%a%c", out[i], i + 1 < n ? ' ' : '\n');
        }
        // the key round trip on what no distance produces
        const double odd[4] = {-0.0, -1.0, -INFINITY, 5e-324};
        for (double d : odd) (void)dne::maze_novelty::key_value(dne::maze_novelty::sort_key(d));
        delete[] xy;
        delete[] arch;
        cases++;
    }
    printf("ok %d\n", cases);
    return 0;
}
