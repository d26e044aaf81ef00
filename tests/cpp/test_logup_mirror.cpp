// The C++ host mirror of the LogUp lookup columns (ms::build_logup_columns, prover.hpp) over Fp -> Fq3 and Fp -> Fp: the program prints
// the words it gets; tests/test_logup_mirror.py builds the same inputs and compares them with the Python mirror's, word for word.
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
    for (int c = 0; c < 5; c++) {
        std::vector<uint64_t> w = words(n);
        if (c == 4) for (size_t i = 0; i < n; i++) if (i % 3 == 0) w[i] = 0;        // a column with zeros: a mask and a denominator
        base.columns.emplace_back(pl, w);
    }
    const ms::GpuVec<ms::Fq3> chal3(pl, words(3 * 4));
    const ms::GpuVec<ms::Fp> chal1(pl, words(4));
    std::vector<ms::LogUpColumn> columns(3);
    // the lookup rule  S' = S + x4 / (c0 - x2 - c1 x3) - 1 / (c0 - x0 - c1 x1)
    columns[0].fractions.push_back(ms::LogUpFraction{{{+1, MS_EXT_NONE, 4, 0}}, {{+1, 0, MS_EXT_NONE, 0}, {-1, MS_EXT_NONE, 2, 0}, {-1, 1, 3, 0}}});
    columns[0].fractions.push_back(ms::LogUpFraction{{{-1, MS_EXT_NONE, MS_EXT_NONE, 0}}, {{+1, 0, MS_EXT_NONE, 0}, {-1, MS_EXT_NONE, 0, 0}, {-1, 1, 1, 0}}});
    // 1 / x4 with its zeros, from a challenge, inclusive, under a mask
    columns[1].init = MS_EXT_INIT_CHALLENGE; columns[1].init_chal = 2;
    columns[1].fractions.push_back(ms::LogUpFraction{{}, {{+1, MS_EXT_NONE, 4, 1}}});
    columns[1].mask = MS_EXT_IF_NONZERO; columns[1].mask_col = 4;
    columns[1].inclusive = true;
    // no fraction: the init everywhere
    columns[2].init = MS_EXT_INIT_ONE;
    const ms::Matrix<ms::Fq3> ext3 = ms::build_logup_columns<ms::Fq3>(base, &chal3, columns);
    const ms::Matrix<ms::Fp> ext1 = ms::build_logup_columns<ms::Fp>(base, &chal1, columns);
    if (ext3.columns.size() != 3 || ext1.columns.size() != 3) { printf("FAILED: columns missing\n"); return 1; }
    for (unsigned c = 0; c < 3; c++) { print_words("fq3", c, ext3.columns[c].to_host()); print_words("fp", c, ext1.columns[c].to_host()); }
    // a refusal surfaces as the library's error
    bool refused = false;
    std::vector<ms::LogUpColumn> bad(1);
    bad[0].fractions.push_back(ms::LogUpFraction{{{+1, MS_EXT_NONE, 0, 0}}, {}});        // nd = 0
    try { ms::build_logup_columns<ms::Fp>(base, &chal1, bad); } catch (const std::exception& e) { refused = std::string(e.what()).find("nd = 0") != std::string::npos; }
    if (!refused) { printf("FAILED: an empty denominator was accepted\n"); return 1; }
    printf("logup host mirror ok\n");
    return 0;
}
