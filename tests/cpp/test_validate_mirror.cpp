// The C++ mirror of validate_constraints (ministark_amd/csrc/host/expr.hpp) on the cases tests/test_validate_mirror.py runs through the
// Python mirror: the fib AIR on a valid trace and with corrupted cells, and a running-product AIR over Fq3.  Prints one JSON line per
// case (report + message); the Python test compares them with its own.
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/expr.hpp"

using namespace ms;
using namespace ms::expr;

static std::vector<std::vector<uint64_t>> fib_trace(size_t n) {              // canonical values (examples/fib gen_trace)
    std::vector<std::vector<uint64_t>> cols(8, std::vector<uint64_t>(n));
    uint64_t v[8];
    v[0] = 1; v[1] = 2;
    for (int k = 2; k < 8; k++) v[k] = gl::mul(v[k - 2], v[k - 1]);
    for (size_t r = 0; r < n; r++) {
        for (int k = 0; k < 8; k++) cols[k][r] = v[k];
        uint64_t w[8];
        w[0] = gl::mul(v[6], v[7]); w[1] = gl::mul(v[7], w[0]);
        for (int k = 2; k < 8; k++) w[k] = gl::mul(w[k - 2], w[k - 1]);
        for (int k = 0; k < 8; k++) v[k] = w[k];
    }
    return cols;
}
static std::vector<E> fib_air(size_t n) {                                    // pipeline.fib_air_constraints
    E x = X();
    const uint64_t last = gl::pow(Radix2EvaluationDomain(n).group_gen, n - 1);
    uint64_t v[8] = {1, 2, 2};
    for (int k = 3; k < 8; k++) v[k] = gl::mul(v[k - 2], v[k - 1]);
    std::vector<E> cs;
    for (unsigned k = 0; k < 8; k++) cs.push_back((Trace(k, 0) - Constant(v[k])) / (x - Constant(1)));
    cs.push_back((Trace(7, 0) - Hint(0)) / (x - Constant(last)));
    std::vector<E> tr{Trace(0, 1) - Trace(6, 0) * Trace(7, 0), Trace(1, 1) - Trace(7, 0) * Trace(0, 1)};
    for (unsigned k = 2; k < 8; k++) tr.push_back(Trace(k, 1) - Trace(k - 2, 1) * Trace(k - 1, 1));
    E zer = (x - Constant(last)) / (pow(x, (uint32_t)n) - Constant(1));
    for (auto& t : tr) cs.push_back(t * zer);
    return cs;
}
static std::vector<E> ext_air(size_t n) {                                    // tests/test_validate_constraints.py _ext_air
    E x = X();
    const uint64_t last = gl::pow(Radix2EvaluationDomain(n).group_gen, n - 1);
    E zer = (x - Constant(last)) / (pow(x, (uint32_t)n) - Constant(1));
    return {(Trace(1, 1) - Trace(1, 0) * (Challenge(0) - Trace(0, 0) * Challenge(1))) * zer, (Trace(1, 0) - Constant(1)) / (x - Constant(1))};
}
static Matrix<Fp> fp_matrix(Planner& pl, const std::vector<std::vector<uint64_t>>& cols) {
    Matrix<Fp> m;
    for (auto& c : cols) { std::vector<uint64_t> w(c.size()); for (size_t i = 0; i < c.size(); i++) w[i] = gl::to_mont(c[i]); m.columns.emplace_back(pl, w); }
    return m;
}
static std::string esc(const std::string& s) {
    std::string o;
    for (char ch : s) { if (ch == '\n') o += "\\n"; else if (ch == '"' || ch == '\\') { o += '\\'; o += ch; } else o += ch; }
    return o;
}
static std::string list(const std::vector<unsigned>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}
static void emit(const char* name, const ValidationReport& r, const std::string& thrown) {
    std::string f = "[";
    for (size_t i = 0; i < r.failures.size(); i++)
        f += (i ? ", " : "") + std::string("[") + std::to_string(r.failures[i].constraint) + ", " + std::to_string(r.failures[i].first_row) + ", " +
             std::to_string(r.failures[i].rows_failed) + "]";
    printf("{\"case\": \"%s\", \"failures\": %s], \"unused_columns\": %s, \"unused_challenges\": %s, \"unused_hints\": %s, \"message\": \"%s\", \"thrown\": \"%s\"}\n",
           name, f.c_str(), list(r.unused_columns).c_str(), list(r.unused_challenges).c_str(), list(r.unused_hints).c_str(), esc(r.message).c_str(), esc(thrown).c_str());
}
template <class Fq>
static void run(const char* name, const std::vector<E>& cs, const std::vector<uint64_t>& ch, const std::vector<uint64_t>& hints, const Matrix<Fp>& base,
                const Matrix<Fq3>* ext) {
    ValidationReport r = validate_constraints<Fq>(cs, ch, hints, base, ext, false);
    std::string thrown;
    try { validate_constraints<Fq>(cs, ch, hints, base, ext, true); } catch (const std::runtime_error& e) { thrown = e.what(); }
    emit(name, r, thrown);
}

int main() {
    Planner& pl = get_planner();
    {   // case 1: the fib AIR on a valid 2^10-row trace, one challenge and one hint no constraint reads
        const size_t n = 1 << 10;
        auto cols = fib_trace(n);
        run<Fp>("fib_valid", fib_air(n), {99}, {cols[7][n - 1], 12345}, fp_matrix(pl, cols), nullptr);
    }
    {   // case 2: corrupted cells at row 0, an interior row, row n - 1, and a cell only a `next` offset reads
        const size_t n = 1 << 8;
        const std::pair<unsigned, size_t> bad[] = {{7, 0}, {6, n / 2 + 1}, {7, n - 1}, {2, n / 2 + 9}};
        for (auto [col, row] : bad) {
            auto cols = fib_trace(n);
            const uint64_t claimed = cols[7][n - 1];
            cols[col][row] = (cols[col][row] + 1) % gl::P;
            const std::string name = "fib_corrupt_" + std::to_string(col) + "_" + std::to_string(row);
            run<Fp>(name.c_str(), fib_air(n), {}, {claimed}, fp_matrix(pl, cols), nullptr);
        }
    }
    {   // case 4: a running product over Fq3, valid and with one component of one cell corrupted
        const size_t n = 1 << 8;
        const uint64_t g0[3] = {11, 22, 33}, g1[3] = {44, 55, 66};
        std::vector<uint64_t> b(n), e(3 * n);
        for (size_t r = 0; r < n; r++) b[r] = (r * 2654435761ull + 12345) % ((uint64_t)1 << 62);
        // Fq3 = Fp[x] / (x^3 - 2) on canonical values: e[r + 1] = e[r] * (g0 - b[r] g1)
        auto mul3 = [](const uint64_t* a, const uint64_t* c, uint64_t* o) {
            auto m = [](uint64_t u, uint64_t v) { return gl::mul(u, v); };
            auto ad = [](uint64_t u, uint64_t v) { return (uint64_t)(((unsigned __int128)u + v) % gl::P); };
            const uint64_t t0 = ad(m(a[0], c[0]), m(2, ad(m(a[1], c[2]), m(a[2], c[1]))));
            const uint64_t t1 = ad(ad(m(a[0], c[1]), m(a[1], c[0])), m(2, m(a[2], c[2])));
            const uint64_t t2 = ad(ad(m(a[0], c[2]), m(a[1], c[1])), m(a[2], c[0]));
            o[0] = t0; o[1] = t1; o[2] = t2;
        };
        uint64_t acc[3] = {1, 0, 0};
        for (size_t r = 0; r < n; r++) {
            for (int w = 0; w < 3; w++) e[3 * r + w] = gl::to_mont(acc[w]);
            uint64_t f[3], nx[3];
            for (int w = 0; w < 3; w++) f[w] = (g0[w] + gl::P - gl::mul(g1[w], b[r])) % gl::P;
            mul3(acc, f, nx);
            for (int w = 0; w < 3; w++) acc[w] = nx[w];
        }
        Matrix<Fp> base = fp_matrix(pl, {b});
        const std::vector<uint64_t> ch{g0[0], g0[1], g0[2], g1[0], g1[1], g1[2]};
        for (long row : {-1L, 0L, 77L, (long)n - 1}) {
            std::vector<uint64_t> em = e;
            if (row >= 0) em[3 * row + 1] = gl::to_mont((gl::from_mont(em[3 * row + 1]) + 1) % gl::P);
            Matrix<Fq3> ext;
            ext.columns.emplace_back(pl, em);
            const std::string name = row < 0 ? std::string("ext_valid") : "ext_corrupt_" + std::to_string(row);
            run<Fq3>(name.c_str(), ext_air(n), ch, {}, base, &ext);
        }
    }
    printf("cpp validate mirror ok\n");
    return 0;
}
