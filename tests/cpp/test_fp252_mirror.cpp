// The C++ host mirror over the 252-bit field, and the Fq = Fp composer with extension columns:
//   * DeepPolyComposer<Fp252>: into_deep_evaluations (whole LDE domain and a row shard) against into_deep_poly followed by the LDE;
//   * apply_drp_rows<Fp252>: the shards' folds concatenate to apply_drp's layer;
//   * DeepPolyComposer<Fp> with a non-null extension matrix: out-of-domain values against Horner sums computed here.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

namespace f252 = ms::f252;
#define REQUIRE(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static uint64_t next64(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
// n elements below 2^251 < p: any such four words are the Montgomery form of some element
static std::vector<uint64_t> rnd252(size_t n, uint64_t seed) {
    std::vector<uint64_t> v(4 * n);
    for (size_t i = 0; i < n; i++) { for (int w = 0; w < 4; w++) v[4 * i + w] = next64(seed); v[4 * i + 3] &= (1ull << 59) - 1; }
    return v;
}
static f252::E elem(uint64_t seed) { const auto w = rnd252(1, seed); f252::E e; memcpy(e.l, w.data(), 32); return e; }
static std::vector<uint64_t> rndgl(size_t n, uint64_t seed) { std::vector<uint64_t> v(n); for (auto& x : v) x = next64(seed) % ms::gl::P; return v; }

static ms::Matrix<ms::Fp252> lde252(ms::Planner& pl, const ms::Matrix<ms::Fp252>& polys, unsigned log_n, unsigned log_N) {
    std::vector<ms::GpuVec<ms::Fp252>> out;
    std::vector<const void*> in; std::vector<void*> o;
    for (auto& c : polys.columns) { in.push_back(c.ptr()); out.emplace_back(pl, (size_t)1 << log_N); }
    for (auto& c : out) o.push_back(c.ptr());
    const auto off = ms::offset_words<ms::Fp252>(3);
    ms::check(ms_evaluate(pl.ctx(), ms::Fp252::id, log_n, log_N, off.data(), in.data(), o.data(), (unsigned)in.size(), 1));
    return ms::Matrix<ms::Fp252>(std::move(out));
}
static ms::Matrix<ms::Fp252> rows_of(ms::Planner& pl, const ms::Matrix<ms::Fp252>& m, size_t first, size_t count) {
    std::vector<ms::GpuVec<ms::Fp252>> out;
    for (auto& c : m.columns) { const auto h = c.to_host(); out.emplace_back(pl, std::vector<uint64_t>(h.begin() + 4 * first, h.begin() + 4 * (first + count))); }
    return ms::Matrix<ms::Fp252>(std::move(out));
}

int main() {
    ms::Planner& pl = ms::get_planner();
    {   // the 252-bit composer: rows form against coefficient form
        const unsigned log_n = 6, log_N = 8;
        const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N;
        std::vector<ms::GpuVec<ms::Fp252>> b, c;
        for (int k = 0; k < 3; k++) b.emplace_back(pl, rnd252(n, 100 + k));
        for (int k = 0; k < 2; k++) c.emplace_back(pl, rnd252(n, 200 + k));
        ms::Matrix<ms::Fp252> base(std::move(b)), comp(std::move(c));
        const std::vector<std::pair<unsigned, int>> args = {{0, 0}, {0, 1}, {1, 0}, {2, 1}, {2, -1}};
        ms::DeepPolyComposer<ms::Fp252> composer(args, n, elem(7), base, comp);
        const auto ood = composer.get_ood_evals();
        REQUIRE(ood.first.size() == args.size() && ood.second.size() == 2);
        {   // one out-of-domain value against Horner on the host
            const auto coef = base.columns[2].to_host();
            const f252::E x = composer.point(-1);
            f252::E acc = f252::zero();
            for (size_t i = n; i-- > 0;) { f252::E ci; memcpy(ci.l, &coef[4 * i], 32); acc = f252::add(f252::mul(acc, x), ci); }
            REQUIRE(f252::eq(acc, ood.first[4]));
        }
        ms::DeepCompositionCoeffs252 co;
        for (size_t k = 0; k < args.size(); k++) co.execution_trace.push_back(elem(300 + k));
        for (int k = 0; k < 2; k++) co.composition_trace.push_back(elem(400 + k));
        co.degree[0] = elem(500); co.degree[1] = elem(501);
        std::vector<ms::GpuVec<ms::Fp252>> q; q.push_back(composer.into_deep_poly(co));
        const auto want = lde252(pl, ms::Matrix<ms::Fp252>(std::move(q)), log_n, log_N).columns[0].to_host();
        const auto bl = lde252(pl, base, log_n, log_N), cl = lde252(pl, comp, log_n, log_N);
        REQUIRE(composer.into_deep_evaluations(co, bl, cl).to_host() == want);
        const size_t first = N / 4 + 3, count = N / 2;
        const auto got = composer.into_deep_evaluations(co, rows_of(pl, bl, first, count), rows_of(pl, cl, first, count), N, first).to_host();
        REQUIRE(got == std::vector<uint64_t>(want.begin() + 4 * first, want.begin() + 4 * (first + count)));
    }
    for (unsigned ff : {2u, 4u, 8u, 16u}) {   // row-sharded fold
        const unsigned log_n = 9;
        const size_t n = (size_t)1 << log_n, m = n / ff;
        const auto words = rnd252(n, 900 + ff);
        const auto alpha = rnd252(1, 950 + ff);
        ms::GpuVec<ms::Fp252> layer(pl, words);
        const auto want = ms::apply_drp<ms::Fp252>(layer, alpha, ff, 3).to_host();
        REQUIRE(want.size() == 4 * m);
        std::vector<uint64_t> got;
        const size_t cuts[4] = {0, m / 4, m / 4 + 1, m};
        for (int k = 0; k < 3; k++) {
            ms::GpuVec<ms::Fp252> shard(pl, std::vector<uint64_t>(words.begin() + 4 * ff * cuts[k], words.begin() + 4 * ff * cuts[k + 1]));
            const auto part = ms::apply_drp_rows<ms::Fp252>(shard, alpha, ff, log_n, cuts[k], 3).to_host();
            got.insert(got.end(), part.begin(), part.end());
        }
        REQUIRE(got == want);
    }
    {   // an Fq = Fp composer whose AIR has extension columns (over Fp): their out-of-domain values must be evaluated too
        const size_t n = 256;
        std::vector<std::vector<uint64_t>> polys;                       // canonical coefficients: 2 base, 2 extension, 1 composition
        for (int k = 0; k < 5; k++) polys.push_back(rndgl(n, 600 + k));
        auto mat = [&](int from, int to) { std::vector<ms::GpuVec<ms::Fp>> v; for (int k = from; k < to; k++) { auto w = polys[k]; for (auto& x : w) x = ms::gl::to_mont(x); v.emplace_back(pl, w); } return ms::Matrix<ms::Fp>(std::move(v)); };
        const auto base = mat(0, 2), ext = mat(2, 4), comp = mat(4, 5);
        const std::vector<std::pair<unsigned, int>> args = {{0, 0}, {2, 0}, {1, 1}, {3, 1}, {3, -1}, {2, 1}};
        ms::FqVal z; z.c[0] = 0x123456789ABCDEFull % ms::gl::P;
        ms::DeepPolyComposer<ms::Fp> composer(args, n, z, base, &ext, comp);
        const auto ood = composer.get_ood_evals();
        REQUIRE(ood.first.size() == args.size() && ood.second.size() == 1);
        const uint64_t g = ms::Radix2EvaluationDomain(n).group_gen, g_inv = ms::gl::inv(g);
        auto horner = [&](const std::vector<uint64_t>& c, uint64_t x) { uint64_t acc = 0; for (size_t i = c.size(); i-- > 0;) acc = ms::gl::add(ms::gl::mul(acc, x), c[i]); return acc; };
        for (size_t k = 0; k < args.size(); k++) {
            const int o = args[k].second;
            const uint64_t x = ms::gl::mul(z.c[0], ms::gl::pow(o >= 0 ? g : g_inv, (uint64_t)(o >= 0 ? o : -o)));
            REQUIRE(ood.first[k].c[0] == horner(polys[args[k].first], x) && ood.first[k].c[1] == 0 && ood.first[k].c[2] == 0);
        }
        REQUIRE(ood.second[0].c[0] == horner(polys[4], z.c[0]));
    }
    printf("fp252 host mirror ok\n");
    return 0;
}
