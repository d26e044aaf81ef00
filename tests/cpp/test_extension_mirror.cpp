// The C++ host mirror of the extension columns (ms::build_extension_columns, prover.hpp) over Fp -> Fq3 and Fp -> Fp, and
// ms::DeepPolyComposer<ms::Fp> with a NON-NULL extension matrix (an Fq = Fp AIR with interaction columns): the program prints the words it
// gets; tests/test_extension_mirror.py builds the same inputs and compares them with the Python mirror's, word for word.
#include <cstdio>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

static uint64_t lcg_state = 42;
static uint64_t next_word() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (lcg_state >> 1) % ms::gl::P; }
static std::vector<uint64_t> words(size_t n) { std::vector<uint64_t> w(n); for (auto& x : w) x = next_word(); return w; }
static void print_words(const char* tag, unsigned k, const std::vector<uint64_t>& w) {
    printf("%s %u", tag, k);
    for (uint64_t x : w) printf(" %llu", (unsigned long long)x);
    printf("\n");
}

int main() {
    ms::Planner& pl = ms::get_planner();
    const size_t n = 300;                                   // the scan takes any length
    ms::Matrix<ms::Fp> base;
    for (int c = 0; c < 4; c++) base.columns.emplace_back(pl, words(n));
    const ms::GpuVec<ms::Fq3> chal3(pl, words(3 * 4));
    const ms::GpuVec<ms::Fp> chal1(pl, words(4));
    std::vector<ms::ExtColumn> columns(3);
    columns[0].init = MS_EXT_INIT_ONE;                      // a masked running product  P' = P (c0 - c1 x0 - c2 x1')
    columns[0].a_terms = {{+1, 0, MS_EXT_NONE, 0}, {-1, 1, 0, 0}, {-1, 2, 1, 1}};
    columns[0].mask = MS_EXT_IF_NONZERO; columns[0].mask_col = 3;
    columns[1].init = MS_EXT_INIT_CHALLENGE; columns[1].init_chal = 1;      // a running evaluation  E' = c3 E + x0', inclusive
    columns[1].a_terms = {{+1, 3, MS_EXT_NONE, 0}};
    columns[1].b_terms = {{+1, MS_EXT_NONE, 0, 1}};
    columns[1].inclusive = true;
    columns[2].b_terms = {{-1, MS_EXT_NONE, 2, -7}, {+1, MS_EXT_NONE, MS_EXT_NONE, 0}};      // a running sum with the literal 1
    const ms::Matrix<ms::Fq3> ext3 = ms::build_extension_columns<ms::Fq3>(base, &chal3, columns);
    const ms::Matrix<ms::Fp> ext1 = ms::build_extension_columns<ms::Fp>(base, &chal1, columns);
    for (unsigned c = 0; c < 3; c++) { print_words("fq3", c, ext3.columns[c].to_host()); print_words("fp", c, ext1.columns[c].to_host()); }

    // DeepPolyComposer<Fp> with an extension matrix: 256 coefficients per column
    const size_t m = 256;
    ms::Matrix<ms::Fp> bp, ep, cp;
    for (int c = 0; c < 4; c++) bp.columns.emplace_back(pl, words(m));
    for (int c = 0; c < 2; c++) ep.columns.emplace_back(pl, words(m));
    cp.columns.emplace_back(pl, words(m));
    std::vector<std::pair<unsigned, int>> args;
    for (unsigned c = 0; c < 6; c++) for (int o = 0; o < 2; o++) args.push_back({c, o});
    ms::FqVal z; z.c[0] = next_word();
    ms::DeepPolyComposer<ms::Fp> composer(args, m, z, bp, &ep, cp);
    const auto ood = composer.get_ood_evals();
    if (ood.first.size() != args.size() || ood.second.size() != 1) { printf("FAILED: out-of-domain values missing\n"); return 1; }
    std::vector<uint64_t> ex, co;
    for (auto& v : ood.first) ex.push_back(v.c[0]);
    for (auto& v : ood.second) co.push_back(v.c[0]);
    print_words("ood_exec", 0, ex);
    print_words("ood_comp", 0, co);
    ms::DeepCompositionCoeffs coeffs;
    for (size_t k = 0; k < args.size(); k++) { ms::FqVal v; v.c[0] = next_word(); coeffs.execution_trace.push_back(v); }
    { ms::FqVal v; v.c[0] = next_word(); coeffs.composition_trace.push_back(v); }
    coeffs.degree[0].c[0] = next_word(); coeffs.degree[1].c[0] = next_word();
    print_words("deep", 0, composer.into_deep_poly(coeffs).to_host());
    printf("extension host mirror ok\n");
    return 0;
}
