// Stand-alone host program over csrc/dense_novelty.h's pool form for tests/test_dense_gans_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: novelty_pool_host on the cases of the text file given as argv[1], each in
// exactly sized heap buffers so that any access past the members, the archive or the results is reported.  With narch == 0 there is no
// archive buffer at all: the function gets a null pointer.
// Per case one line "D n narch k", then n * D member coordinates and narch * D archive coordinates as strtod reads them (hex floats, "nan",
// "inf"); prints per case one line of n results, a value as %a, a NaN as "nan".  The last line is "ok <cases>"; a sanitizer finding aborts
// the program.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "dense_novelty.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES_FILE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    auto number = [&](double *v) {
        std::string tok;
        if (!(in >> tok)) return false;
        char *end = nullptr;
        *v = strtod(tok.c_str(), &end);
        return end != tok.c_str() && *end == 0;
    };
    int cases = 0, D, n, narch, k;
    while (in >> D >> n >> narch >> k) {
        if ((D != 2 && D != 4) || n < 1 || narch < 0 || k < 1 || narch + n - 1 < 1) { fprintf(stderr, "bad case header\n"); return 2; }
        float *bc = new float[(size_t)n * D];
        float *arch = narch ? new float[(size_t)narch * D] : nullptr;
        double v;
        for (int i = 0; i < D * n; i++) { if (!number(&v)) { fprintf(stderr, "short case\n"); return 2; } bc[i] = (float)v; }
        for (int i = 0; i < D * narch; i++) { if (!number(&v)) { fprintf(stderr, "short case\n"); return 2; } arch[i] = (float)v; }
        double *out = new double[(size_t)n];
        dne::dense_novelty::novelty_pool_host(bc, n, arch, narch, D, k, out);
        for (int i = 0; i < n; i++) {
            if (out[i] != out[i]) printf("nan%c", i + 1 < n ? ' ' : '\n');
            else printf("%a%c", out[i], i + 1 < n ? ' ' : '\n');
        }
        delete[] bc;
        delete[] arch;
        delete[] out;
        cases++;
    }
    printf("ok %d\n", cases);
    return 0;
}
