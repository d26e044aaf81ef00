// The C++ mirror of the canonical-form scan and of checked mode (ministark_amd/csrc/host/ministark.hpp: Matrix<F>::check_canonical,
// Planner::set_checked) on the cases tests/test_canonical_mirror.py states: a deterministic matrix per field, clean and with planted
// values.  Prints one JSON line per case (the report, or the refusal's message); the Python test compares them with what it works out.
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"

using namespace ms;

static const uint64_t GL_P = 0xFFFFFFFF00000001ull, P3 = 0x0800000000000011ull;
// word w of column c: a fixed mix, canonical for every field (Goldilocks: below p; 252-bit: limb 3 below p's)
static uint64_t word(unsigned c, size_t w, unsigned words) {
    uint64_t x = (uint64_t)(c + 1) * 0x9E3779B97F4A7C15ull + (uint64_t)w * 0xD1B54A32D192ED03ull;
    x ^= x >> 29;
    if (words == 4 && w % 4 == 3) return x % P3;
    return x % GL_P;
}
template <class F>
static Matrix<F> matrix(Planner& pl, size_t n, unsigned ncols, const std::vector<std::vector<uint64_t>>& plants) {   // plant: {col, word index, value}
    Matrix<F> m;
    for (unsigned c = 0; c < ncols; c++) {
        std::vector<uint64_t> w(n * F::words);
        for (size_t i = 0; i < w.size(); i++) w[i] = word(c, i, F::words);
        for (auto& p : plants) if (p[0] == c) w[p[1]] = p[2];
        m.columns.emplace_back(pl, w);
    }
    return m;
}
static std::string esc(const std::string& s) {
    std::string o;
    for (char ch : s) { if (ch == '"' || ch == '\\') { o += '\\'; o += ch; } else o += ch; }
    return o;
}
template <class F>
static void report(const char* name, const Matrix<F>& m) {
    const ms_canon_report r = m.check_canonical();
    printf("{\"case\": \"%s\", \"count\": %llu, \"first_col\": %u, \"first_row\": %llu, \"first_word\": %u}\n", name, (unsigned long long)r.count,
           r.count ? r.first_col : 0u, (unsigned long long)(r.count ? r.first_row : 0), r.count ? r.first_word : 0u);
}
template <class F, class Fn>
static void refusal(const char* name, Planner& pl, const Matrix<F>& m, Fn&& fn) {
    std::vector<std::vector<uint64_t>> before;
    for (auto& c : m.columns) before.push_back(c.to_host());
    std::string thrown;
    try { fn(); } catch (const std::runtime_error& e) { thrown = e.what(); }
    pl.sync();
    bool same = true;
    for (size_t c = 0; c < m.columns.size(); c++) same = same && m.columns[c].to_host() == before[c];
    printf("{\"case\": \"%s\", \"thrown\": \"%s\", \"inputs_unchanged\": %s}\n", name, esc(thrown).c_str(), same ? "true" : "false");
}

int main() {
    Planner pl(0);
    printf("{\"case\": \"default\", \"checked\": %s}\n", pl.checked() ? "true" : "false");
    const size_t n = 1 << 9;
    report("fp_clean", matrix<Fp>(pl, n, 3, {}));
    report("fp_planted", matrix<Fp>(pl, n, 3, {{2, 5, ~0ull}, {1, 400, GL_P}, {1, 401, GL_P + 1}}));
    report("fq3_clean", matrix<Fq3>(pl, n, 2, {}));
    report("fq3_planted", matrix<Fq3>(pl, n, 2, {{1, 3 * 100 + 2, GL_P}, {1, 3 * 100 + 1, ~0ull}, {1, 3 * 7 + 0, GL_P}}));
    report("f252_clean", matrix<Fp252>(pl, n, 2, {}));
    report("f252_planted", matrix<Fp252>(pl, n, 2, {{0, 4 * 511 + 3, P3}, {0, 4 * 511 + 1, 9}, {1, 4 * 2 + 3, P3 + 1}}));
    // checked mode: the refusal is the mirror's exception, before anything is written (the transform is in place)
    Matrix<Fp> bad = matrix<Fp>(pl, n, 3, {{1, 400, GL_P}});
    pl.set_checked(true);
    printf("{\"case\": \"switched_on\", \"checked\": %s}\n", pl.checked() ? "true" : "false");
    refusal("fp_into_polynomials", pl, bad, [&] { bad.into_polynomials(Radix2EvaluationDomain(n)); });
    refusal("fp_sum_columns", pl, bad, [&] { bad.sum_columns(); });
    Matrix<Fp> good = matrix<Fp>(pl, n, 3, {});
    refusal("fp_clean_sum_columns", pl, good, [&] { good.sum_columns(); });
    pl.set_checked(false);
    refusal("fp_unchecked_sum_columns", pl, bad, [&] { bad.sum_columns(); });
    printf("cpp canonical mirror ok\n");
    return 0;
}
