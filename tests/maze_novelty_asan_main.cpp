// Stand-alone host program over csrc/maze_novelty.h for tests/test_maze_novelty_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: novelty_host on the cases of the text file given as argv[1], each in
// exactly sized heap buffers so that any access past the members, the archive or the results is reported.
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
        if (n < 1 || narch < 1 || k < 1) { fprintf(stderr, "bad case header\n"); return 2; }
        std::vector<float> xy((size_t)n * 2), arch((size_t)narch * 2);
        for (float &v : xy) if (!number(&v)) { fprintf(stderr, "short case\n"); return 2; }
        for (float &v : arch) if (!number(&v)) { fprintf(stderr, "short case\n"); return 2; }
        std::vector<double> out((size_t)n);
        dne::maze_novelty::novelty_host(xy.data(), n, arch.data(), narch, k, out.data());
        for (int i = 0; i < n; i++) {
            if (out[i] != out[i]) printf("nan%c", i + 1 < n ? ' ' : '\n');
            else printf("%a%c", out[i], i + 1 < n ? ' ' : '\n');
        }
        // the key round trip on what no distance produces
        const double odd[4] = {-0.0, -1.0, -INFINITY, 5e-324};
        for (double d : odd) (void)dne::maze_novelty::key_value(dne::maze_novelty::sort_key(d));
        cases++;
    }
    printf("ok %d\n", cases);
    return 0;
}
