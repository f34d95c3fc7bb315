// Stand-alone host program over csrc/dense_novelty.h for tests/test_dense_novelty_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it: novelty_host (argv[1] "novelty") or bc_host (argv[1] "bc") on the cases of the
// text file given as argv[2], each in exactly sized heap buffers so that any access past the members, the archive, the records or the results
// is reported.
// "novelty": per case one line "D n narch k", then n * D member coordinates and narch * D archive coordinates as strtod reads them (hex
// floats, "nan", "inf"); prints per case one line of n results.  "bc": per case one line "env n", then n * S record doubles; prints per case one
// line of n * D floats.  A value is printed as %a, a NaN as "nan".  The last line is "ok <cases>"; a sanitizer finding aborts the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "dense_novelty.h"

static void print_row(const double *v, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (v[i] != v[i]) printf("nan%c", i + 1 < n ? ' ' : '\n');
        else printf("%a%c", v[i], i + 1 < n ? ' ' : '\n');
    }
}

int main(int argc, char **argv) {
    if (argc != 3 || (strcmp(argv[1], "novelty") && strcmp(argv[1], "bc"))) { fprintf(stderr, "usage: %s novelty|bc CASES_FILE\n", argv[0]); return 2; }
    const bool bc_mode = !strcmp(argv[1], "bc");
    std::ifstream in(argv[2]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    auto number = [&](double *v) {
        std::string tok;
        if (!(in >> tok)) return false;
        char *end = nullptr;
        *v = strtod(tok.c_str(), &end);
        return end != tok.c_str() && *end == 0;
    };
    int cases = 0;
    if (bc_mode) {
        int env, n;
        while (in >> env >> n) {
            if (n < 1 || env < dne::dense::KIND_MAZE || env > dne::dense::KIND_PENDULUM) { fprintf(stderr, "bad case header\n"); return 2; }
            const size_t S = env == dne::dense::KIND_MAZE ? 7 : env == dne::dense::KIND_CARTPOLE ? 4 : 2, D = (size_t)dne::dense_novelty::bc_dim(env);
            double *rec = new double[(size_t)n * S];
            float *bc = new float[(size_t)n * D];
            for (size_t i = 0; i < (size_t)n * S; i++) if (!number(&rec[i])) { fprintf(stderr, "short case\n"); return 2; }
            dne::dense_novelty::bc_host(env, rec, n, bc);
            std::vector<double> wide((size_t)n * D);
            for (size_t i = 0; i < wide.size(); i++) wide[i] = (double)bc[i];
            print_row(wide.data(), wide.size());
            delete[] rec;
            delete[] bc;
            cases++;
        }
    } else {
        int D, n, narch, k;
        while (in >> D >> n >> narch >> k) {
            if ((D != 2 && D != 4) || n < 1 || narch < 1 || k < 1) { fprintf(stderr, "bad case header\n"); return 2; }
            float *bc = new float[(size_t)n * D];
            float *arch = new float[(size_t)narch * D];
            double v;
            for (int i = 0; i < D * n; i++) { if (!number(&v)) { fprintf(stderr, "short case\n"); return 2; } bc[i] = (float)v; }
            for (int i = 0; i < D * narch; i++) { if (!number(&v)) { fprintf(stderr, "short case\n"); return 2; } arch[i] = (float)v; }
            double *out = new double[(size_t)n];
            dne::dense_novelty::novelty_host(bc, n, arch, narch, D, k, out);
            print_row(out, (size_t)n);
            delete[] bc;
            delete[] arch;
            delete[] out;
            cases++;
        }
    }
    printf("ok %d\n", cases);
    return 0;
}
