// Stand-alone host program over csrc/dense_ga.h for tests/test_dense_ga_cpu.py, which builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it once per shape: check_genomes + genome_host and check_member + members_host
// with P read at run time, on the cases of the text file given as argv[1], every array in an exactly sized heap buffer so that any access
// past the table, the bank, the descriptors or the results is reported.
// The file: "count P", count noise floats, P scale_by floats (as strtof reads them: hex floats), then cases, each either
//   G nseeds            then nseeds pairs "idx power"
//   M T n               then T * P bank floats, then n triples "parent idx power"
// Prints per case one line: "refused <why>" or the P (G) / n * P (M) results as %a ("nan" for a NaN), then "ok <cases>"; a sanitizer
// finding aborts it.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "dense_ga.h"

namespace G = dne::dense_ga;

static void print_row(const std::vector<float> &out) {
    for (size_t i = 0; i < out.size(); i++) {
        if (out[i] != out[i]) printf("nan%c", i + 1 < out.size() ? ' ' : '\n');
        else printf("%a%c", (double)out[i], i + 1 < out.size() ? ' ' : '\n');
    }
}

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
    long long count = 0;
    int P = 0;
    if (!(in >> count >> P) || count < 1 || P < 1 || P > dne::dense::MAX_P) { fprintf(stderr, "bad table size or P\n"); return 2; }
    std::vector<float> noise((size_t)count), scale_by((size_t)P);
    for (float &v : noise) if (!number(&v)) { fprintf(stderr, "short table\n"); return 2; }
    for (float &v : scale_by) if (!number(&v)) { fprintf(stderr, "short scale_by\n"); return 2; }
    int cases = 0;
    std::string kind;
    while (in >> kind) {
        if (kind == "G") {
            int nseeds;
            if (!(in >> nseeds) || nseeds < 0) { fprintf(stderr, "bad genome header\n"); return 2; }
            std::vector<int64_t> seeds((size_t)nseeds);
            std::vector<float> powers((size_t)nseeds);
            for (int j = 0; j < nseeds; j++) {
                long long s;
                if (!(in >> s) || !number(&powers[j])) { fprintf(stderr, "short genome\n"); return 2; }
                seeds[j] = s;
            }
            const int32_t co[2] = {0, nseeds};
            const std::string bad = G::check_genomes(1, P, co, seeds.data(), noise.size());
            if (!bad.empty()) printf("refused %s\n", bad.c_str());
            else {
                std::vector<float> out((size_t)P);
                G::genome_host(noise.data(), scale_by.data(), P, seeds.data(), powers.data(), nseeds, out.data());
                print_row(out);
            }
        } else if (kind == "M") {
            int T, n;
            if (!(in >> T >> n) || T < 0 || n < 1) { fprintf(stderr, "bad member header\n"); return 2; }
            std::vector<float> bank((size_t)T * P), power((size_t)n);
            std::vector<int32_t> parent((size_t)n);
            std::vector<int64_t> idx((size_t)n);
            for (float &v : bank) if (!number(&v)) { fprintf(stderr, "short bank\n"); return 2; }
            for (int i = 0; i < n; i++) {
                long long a, b;
                if (!(in >> a >> b) || !number(&power[i])) { fprintf(stderr, "short members\n"); return 2; }
                parent[i] = (int32_t)a; idx[i] = b;
            }
            std::string bad;
            for (int i = 0; i < n && bad.empty(); i++) bad = G::check_member(i, T, P, noise.size(), parent[i], idx[i], true);
            if (!bad.empty()) printf("refused %s\n", bad.c_str());
            else {
                std::vector<float> out((size_t)n * P);
                G::members_host(noise.data(), scale_by.data(), P, T ? bank.data() : nullptr, parent.data(), idx.data(), power.data(), n, out.data());
                print_row(out);
            }
        } else { fprintf(stderr, "bad case kind %s\n", kind.c_str()); return 2; }
        cases++;
    }
    printf("ok %d\n", cases);
    return 0;
}
