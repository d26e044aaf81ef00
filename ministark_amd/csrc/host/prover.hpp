// prover.hpp -- the remaining data-parallel pieces of default_prove (src/prover.rs:25-174) over the C ABI:
//   apply_drp                         src/fri.rs:526-567
//   DeepPolyComposer                  src/composer.rs:17-188
//   scan_affine / running_product     examples/brainfuck/trace.rs:108-289 (extension-column loops)
//   ExtColumn / build_extension_columns   src/trace.rs build_extension_columns: every extension column in one call (ministark_hip_ext.h)
//   LookupTuple / lookup_multiplicities   the m column of a LogUp lookup, counted on the device (ministark_hip_lookup.h)
//   SortKey / sort_rows / permute_columns   the rows of a table in key order (examples/brainfuck/vm.rs sort_by_key), on the device (ministark_hip_sort.h)
//   join_rows / fetch_columns         for every row, the table row that holds its key, and that row's other columns: instruction fetch, ROM reads (ministark_hip_join.h)
//   LimbSpec / limb_decompose / RangeSet / range_multiplicities   range checks: the limbs of a value column and the multiplicities of the table 0 .. 2^bits - 1 (ministark_hip_range.h)
//   BitwiseSpec / bitwise_columns / bitwise_table / BitwiseSet / bitwise_multiplicities   a AND / OR / XOR b as a column, the table over limb pairs and its multiplicities (ministark_hip_bitwise.h)
//   GapSpec / gap_plan / gap_fill     derive_memory_rows and pad_*_rows (examples/brainfuck/vm.rs:282-380): select, fill clock gaps, pad, on the device (ministark_hip_gaps.h)
//   Queries                           src/trace.rs:113-157
//   grind_proof_of_work               src/random.rs:48-55
//   PublicCoin                        src/random.rs:61-141, as ProverChannel uses it (src/channel.rs:46-100); state on the device
//   RpoCoin                           the same calls on the algebraic RPO-256 coin (ministark_hip_rpo_coin.h)
//   PoseidonCoin                      the same calls on the algebraic coin of the 252-bit field (ministark_hip_hades_coin.h)
//   GpuRpo256ColumnMajor / RowMajor / gen_rpo_merkle_tree   gpu/src/plan.rs:32-174
// Host values of Fq are canonical integers: FqVal{c0,c1,c2} (c1 = c2 = 0 when Fq = Fp).
#pragma once
#include "ministark.hpp"
#include "../../../include/ministark_hip_transcript.h"
#include "../../../include/ministark_hip_ext.h"
#include "../../../include/ministark_hip_logup.h"
#include "../../../include/ministark_hip_rpo_coin.h"
#include "../../../include/ministark_hip_hades_coin.h"
#include "../../../include/ministark_hip_lookup.h"
#include "../../../include/ministark_hip_sort.h"
#include "../../../include/ministark_hip_gaps.h"
#include "../../../include/ministark_hip_join.h"
#include "../../../include/ministark_hip_range.h"
#include "../../../include/ministark_hip_bitwise.h"
#include <cstring>
#include <stdint.h>
// host arithmetic of the 252-bit field (points and offsets of its composer): the library's own fp252.h, kept inside ms:: so that its
// Goldilocks namespace does not meet ms::gl in a program that says `using namespace ms`
namespace ms { namespace lib252 {
#include "../fp252.h"
} namespace f252 = lib252::f252; }

namespace ms {

struct FqVal {
    uint64_t c[3] = {0, 0, 0};
    bool operator==(const FqVal& o) const { return c[0] == o.c[0] && c[1] == o.c[1] && c[2] == o.c[2]; }
    bool operator<(const FqVal& o) const { return std::lexicographical_compare(c, c + 3, o.c, o.c + 3); }
};
namespace fq {          // Fq3 = Fp[x]/(x^3 - 2) on canonical values: bookkeeping of evaluation points only
inline uint64_t addp(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + b) % gl::P); }
inline FqVal mul(const FqVal& a, const FqVal& b) {
    auto m = gl::mul;
    return {{addp(m(a.c[0], b.c[0]), m(2, addp(m(a.c[1], b.c[2]), m(a.c[2], b.c[1])))),
             addp(addp(m(a.c[0], b.c[1]), m(a.c[1], b.c[0])), m(2, m(a.c[2], b.c[2]))),
             addp(addp(m(a.c[0], b.c[2]), m(a.c[1], b.c[1])), m(a.c[2], b.c[0]))}};
}
inline FqVal mul_base(const FqVal& a, uint64_t s) { return {{gl::mul(a.c[0], s), gl::mul(a.c[1], s), gl::mul(a.c[2], s)}}; }
inline FqVal pow(FqVal a, uint64_t e) { FqVal r{{1, 0, 0}}; while (e) { if (e & 1) r = mul(r, a); a = mul(a, a); e >>= 1; } return r; }
template <class F> inline void push_words(std::vector<uint64_t>& out, const FqVal& v) { for (unsigned w = 0; w < F::words; w++) out.push_back(gl::to_mont(v.c[w])); }
inline uint64_t from_mont(uint64_t m) { return gl::mul(m, gl::pow(0xFFFFFFFFull, gl::P - 2)); }
template <class F> inline FqVal from_words(const uint64_t* w) { FqVal v; for (unsigned k = 0; k < F::words; k++) v.c[k] = from_mont(w[k]); return v; }
}  // namespace fq

// a domain offset (a small canonical integer) as the Montgomery words of F's FFT field: one word, or four for Fp252
template <class F>
inline std::array<uint64_t, 4> offset_words(uint64_t domain_offset) {
    if constexpr (F::words == 4) { const f252::E m = f252::to_mont(f252::E{{domain_offset, 0, 0, 0}}); return {{m.l[0], m.l[1], m.l[2], m.l[3]}}; }
    else return {{gl::to_mont(domain_offset), 0, 0, 0}};
}
// apply_drp(evals, domain_offset, alpha, folding_factor): `evals` in bit-reversed order; returns the next layer
// (bit-reversed).  alpha: Montgomery words of one element of F.
template <class F>
inline GpuVec<F> apply_drp(const GpuVec<F>& evals, const std::vector<uint64_t>& alpha, unsigned folding_factor, uint64_t domain_offset = 1) {
    if (alpha.size() != F::words) throw std::invalid_argument("alpha has the wrong number of limbs");
    GpuVec<F> out(evals.planner(), evals.len() / folding_factor);
    unsigned log_n = 0; while (((size_t)1 << log_n) < evals.len()) log_n++;
    const auto off = offset_words<F>(domain_offset);
    check(ms_fri_fold(evals.planner().ctx(), F::id, log_n, folding_factor, alpha.data(), off.data(), evals.ptr(), out.ptr()));
    return out;
}
// the same fold with the challenge where the device-resident coin drew it (PublicCoin::draw): one element of F in device memory,
// read by the kernel (ms_fri_fold_dev) -- no host wait between a layer's commitment and its fold
template <class F>
inline GpuVec<F> apply_drp(const GpuVec<F>& evals, const GpuVec<F>& alpha, unsigned folding_factor, uint64_t domain_offset = 1) {
    if (alpha.len() != 1) throw std::invalid_argument("apply_drp: a device alpha is one element");
    GpuVec<F> out(evals.planner(), evals.len() / folding_factor);
    unsigned log_n = 0; while (((size_t)1 << log_n) < evals.len()) log_n++;
    const auto off = offset_words<F>(domain_offset);
    check(ms_fri_fold_dev(evals.planner().ctx(), F::id, log_n, folding_factor, alpha.ptr(), off.data(), evals.ptr(), out.ptr()));
    return out;
}
// the same fold on a row shard of a layer of 2^log_n evaluations: `shard` holds chunks [first_chunk, first_chunk + shard.len() / folding_factor)
// of the bit-reversed layer and the result is those chunks of the next one (ms_fri_fold_rows; Fp, Fq3 and Fp252)
template <class F>
inline GpuVec<F> apply_drp_rows(const GpuVec<F>& shard, const std::vector<uint64_t>& alpha, unsigned folding_factor, unsigned log_n, size_t first_chunk,
                                uint64_t domain_offset = 1) {
    if (alpha.size() != F::words) throw std::invalid_argument("alpha has the wrong number of limbs");
    if (shard.len() % folding_factor) throw std::invalid_argument("apply_drp_rows: a shard holds whole chunks");
    const size_t nchunks = shard.len() / folding_factor;
    GpuVec<F> out(shard.planner(), nchunks);
    const auto off = offset_words<F>(domain_offset);
    check(ms_fri_fold_rows(shard.planner().ctx(), F::id, log_n, folding_factor, alpha.data(), off.data(), first_chunk, nchunks, shard.ptr(), out.ptr()));
    return out;
}

// state = init; for every row: out[row] = state; state = a[row]*state + b[row]   (a or b may be null)
template <class F>
inline GpuVec<F> scan_affine(const GpuVec<F>* a, const GpuVec<F>* b, const std::vector<uint64_t>& init, bool inclusive = false) {
    const GpuVec<F>* ref = a ? a : b;
    if (!ref) throw std::invalid_argument("scan_affine: neither multipliers nor addends given");
    if (init.size() != F::words) throw std::invalid_argument("init has the wrong number of limbs");
    GpuVec<F> out(ref->planner(), ref->len());
    check(ms_scan_affine(ref->planner().ctx(), F::id, ref->len(), a ? a->ptr() : nullptr, b ? b->ptr() : nullptr, init.data(), inclusive ? 1 : 0, out.ptr()));
    return out;
}
template <class F> inline GpuVec<F> running_product(const GpuVec<F>& factors, const std::vector<uint64_t>& init) { return scan_affine<F>(&factors, nullptr, init); }

// Trace::build_extension_columns(&challenges) in one asynchronous call (ms_build_extension_columns): per column
//     state = init;  for row i: out[i] = state;  if active(i): state = A(i) * state + B(i),   A(i) = sum_t sign_t coef_t base[col_t][(i + off_t) mod n]
// chal: an index into the challenge vector, or MS_EXT_NONE for the literal 1; col: an index into the base matrix, or MS_EXT_NONE for a constant term
struct ExtTerm { int sign; int chal; int col; int off = 0; };
struct ExtColumn {
    int init = MS_EXT_INIT_ZERO, init_chal = 0;                  // MS_EXT_INIT_ZERO / _ONE / _CHALLENGE (the state starts as challenges[init_chal])
    std::vector<ExtTerm> a_terms, b_terms;                       // an empty A is 1, an empty B is 0
    int mask = MS_EXT_ALWAYS, mask_col = 0;                      // MS_EXT_IF_NONZERO / MS_EXT_IF_ZERO: active where base[mask_col][i] != 0 / == 0
    bool inclusive = false;                                      // out[i] is the state AFTER row i
};
// base: columns of B (Fp or Fp252); challenges: elements of FqT on the device (e.g. PublicCoin::draw), or null when nothing names one.
// Pairs Fp -> Fq3, Fp -> Fp, Fp252 -> Fp252.  Enqueues and returns.
template <class FqT, class B>
inline Matrix<FqT> build_extension_columns(const Matrix<B>& base, const GpuVec<FqT>* challenges, const std::vector<ExtColumn>& columns) {
    Planner& pl = base.planner();
    const size_t n = base.num_rows();
    std::vector<ms_ext_column> recs;
    std::vector<ms_ext_term> terms;
    for (auto& c : columns) {
        recs.push_back({c.init, c.init_chal, c.mask, c.mask_col, c.inclusive ? 1 : 0, (uint32_t)c.a_terms.size(), (uint32_t)c.b_terms.size(), 0});
        for (auto* list : {&c.a_terms, &c.b_terms}) for (auto& t : *list) terms.push_back({t.col, t.off, t.chal, t.sign});
    }
    std::vector<const void*> in;
    for (auto& c : base.columns) in.push_back(c.ptr());
    Matrix<FqT> out;
    std::vector<void*> outs;
    for (size_t e = 0; e < columns.size(); e++) { out.columns.emplace_back(pl, n); outs.push_back(out.columns.back().ptr()); }
    check(ms_build_extension_columns(pl.ctx(), B::id, FqT::id, n, in.data(), (unsigned)in.size(), challenges ? challenges->ptr() : nullptr,
                                     challenges ? (unsigned)challenges->len() : 0u, recs.data(), terms.data(), (unsigned)columns.size(), outs.data()));
    return out;
}

// LogUp lookup columns in one asynchronous call (ms_build_logup_columns): per column
//     state = init;  for row i: out[i] = state;  if active(i): state = state + sum_f N_f(i) * inv(D_f(i)),   inv(0) = 0
// N_f, D_f: sums of ExtTerms (an empty numerator is the literal 1; a denominator has at least one term)
struct LogUpFraction { std::vector<ExtTerm> numerator, denominator; };
struct LogUpColumn {
    int init = MS_EXT_INIT_ZERO, init_chal = 0;                  // as ExtColumn's
    std::vector<LogUpFraction> fractions;                        // none: the column holds its init everywhere
    int mask = MS_EXT_ALWAYS, mask_col = 0;
    bool inclusive = false;
};
template <class FqT, class B>
inline Matrix<FqT> build_logup_columns(const Matrix<B>& base, const GpuVec<FqT>* challenges, const std::vector<LogUpColumn>& columns) {
    Planner& pl = base.planner();
    const size_t n = base.num_rows();
    std::vector<ms_logup_column> recs;
    std::vector<ms_logup_fraction> fracs;
    std::vector<ms_ext_term> terms;
    for (auto& c : columns) {
        recs.push_back({c.init, c.init_chal, c.mask, c.mask_col, c.inclusive ? 1 : 0, (uint32_t)c.fractions.size(), 0, 0});
        for (auto& f : c.fractions) {
            fracs.push_back({(uint32_t)f.numerator.size(), (uint32_t)f.denominator.size()});
            for (auto* list : {&f.numerator, &f.denominator}) for (auto& t : *list) terms.push_back({t.col, t.off, t.chal, t.sign});
        }
    }
    std::vector<const void*> in;
    for (auto& c : base.columns) in.push_back(c.ptr());
    Matrix<FqT> out;
    std::vector<void*> outs;
    for (size_t e = 0; e < columns.size(); e++) { out.columns.emplace_back(pl, n); outs.push_back(out.columns.back().ptr()); }
    check(ms_build_logup_columns(pl.ctx(), B::id, FqT::id, n, in.data(), (unsigned)in.size(), challenges ? challenges->ptr() : nullptr,
                                 challenges ? (unsigned)challenges->len() : 0u, recs.data(), fracs.data(), terms.data(), (unsigned)columns.size(), outs.data()));
    return out;
}

// The m column of a lookup in one asynchronous call (ms_lookup_multiplicities): m[j] = how many active rows of the `lookups` hold the tuple
// of table row j (equal table rows: the first takes the credit).  cols: 1 .. MS_LOOKUP_MAX_WIDTH indices into the base matrix, the same
// number in the table and in every set; mask as ExtColumn's.  m: n elements, possibly a column of `base` that no tuple and no mask names.
struct LookupTuple { std::vector<int> cols; int mask = MS_EXT_ALWAYS, mask_col = 0; };
struct LookupReport {
    GpuVec<Fp> buf;                                              // the ms_lookup_report where the call wrote it
    ms_lookup_report read() const { const std::vector<uint64_t> w = buf.to_host(); ms_lookup_report r; memcpy(&r, w.data(), sizeof r); return r; }   // a host wait
};
template <class B>
inline LookupReport lookup_multiplicities(const Matrix<B>& base, const LookupTuple& table, const std::vector<LookupTuple>& lookups, GpuVec<B>& m) {
    Planner& pl = base.planner();
    auto record = [&](const LookupTuple& t) {
        if (t.cols.empty() || t.cols.size() > (size_t)MS_LOOKUP_MAX_WIDTH || t.cols.size() != table.cols.size())
            throw std::invalid_argument("lookup_multiplicities: a tuple has 1 .. 4 columns, as many as the table");
        ms_lookup_tuple r = {{0, 0, 0, 0}, t.mask, t.mask_col, 0, 0};
        for (size_t c = 0; c < t.cols.size(); c++) r.cols[c] = t.cols[c];
        return r;
    };
    const ms_lookup_tuple trec = record(table);
    std::vector<ms_lookup_tuple> lrecs;
    for (auto& t : lookups) lrecs.push_back(record(t));
    std::vector<const void*> in;
    for (auto& c : base.columns) in.push_back(c.ptr());
    LookupReport rep{GpuVec<Fp>(pl, sizeof(ms_lookup_report) / 8)};
    check(ms_lookup_multiplicities(pl.ctx(), B::id, base.num_rows(), in.data(), (unsigned)in.size(), (unsigned)table.cols.size(), &trec,
                                   lrecs.empty() ? nullptr : lrecs.data(), (unsigned)lrecs.size(), m.ptr(), rep.buf.ptr()));
    return rep;
}

// The permutation that sorts the first n rows of `base` (all of them by default) in one asynchronous call (ms_sort_rows): the active rows in
// ascending order of the canonical values of cols[0] (most significant) .. cols[nkeys-1], rows of equal keys in their original order, then
// the inactive rows in their original order.  cols: 1 .. MS_SORT_MAX_KEYS indices into the base matrix; mask as ExtColumn's.
struct SortKey { std::vector<int> cols; int mask = MS_EXT_ALWAYS, mask_col = 0; };
struct RowOrder {
    GpuVec<Fp> index;                                            // n x uint32 where the call wrote them (two to a word)
    GpuVec<Fp> report;                                           // the ms_sort_report
    size_t n = 0;
    std::vector<uint32_t> to_host() const {                      // a host wait
        const std::vector<uint64_t> w = index.to_host();
        std::vector<uint32_t> out(n);
        if (n) memcpy(out.data(), w.data(), n * 4);
        return out;
    }
    ms_sort_report read() const { const std::vector<uint64_t> w = report.to_host(); ms_sort_report r; memcpy(&r, w.data(), sizeof r); return r; }   // a host wait
};
template <class B>
inline RowOrder sort_rows(const Matrix<B>& base, const SortKey& key, size_t n = (size_t)-1) {
    Planner& pl = base.planner();
    if (key.cols.empty() || key.cols.size() > (size_t)MS_SORT_MAX_KEYS) throw std::invalid_argument("sort_rows: a key has 1 .. 4 columns");
    if (n == (size_t)-1) n = base.num_rows();
    if (n > base.num_rows()) throw std::invalid_argument("sort_rows: more rows than the columns hold");
    ms_sort_key rec = {{0, 0, 0, 0}, key.mask, key.mask_col, 0, 0};
    for (size_t c = 0; c < key.cols.size(); c++) rec.cols[c] = key.cols[c];
    std::vector<const void*> in;
    for (auto& c : base.columns) in.push_back(c.ptr());
    RowOrder out{GpuVec<Fp>(pl, (n + 1) / 2), GpuVec<Fp>(pl, sizeof(ms_sort_report) / 8), n};
    check(ms_sort_rows(pl.ctx(), B::id, n, in.data(), (unsigned)in.size(), (unsigned)key.cols.size(), &rec, out.index.ptr(), out.report.ptr()));
    return out;
}
// dst[c][i] = src[c][index[i]] for i < n_out (ms_permute_columns; a zero element where index[i] is no row of src): `order.n` entries by default
template <class F>
inline Matrix<F> permute_columns(const Matrix<F>& src, const RowOrder& order, size_t n_out = (size_t)-1) {
    Planner& pl = src.planner();
    if (n_out == (size_t)-1) n_out = order.n;
    if (n_out > order.n) throw std::invalid_argument("permute_columns: more entries than the index holds");
    Matrix<F> out;
    std::vector<const void*> in;
    std::vector<void*> to;
    for (auto& c : src.columns) { in.push_back(c.ptr()); out.columns.emplace_back(pl, n_out); }
    for (auto& c : out.columns) to.push_back(c.ptr());
    check(ms_permute_columns(pl.ctx(), F::id, src.num_rows(), in.data(), to.data(), (unsigned)in.size(), order.index.ptr(), n_out));
    return out;
}

// Rows joined against a table in one asynchronous call (ms_join_rows): match[s][i] = the smallest active row of `table` whose key
// (`table_key`, indices into `table`) equals the key of row i of `base` under keys[s] (indices into `base`), or MS_JOIN_NONE for an inactive
// row and for a key the table does not hold.  The two matrices may be the same one.  The matches are RowOrders: permute_columns reads them.
struct JoinReport {
    std::vector<RowOrder> matches;                               // one per key set; .report is not written (the join has one report: buf)
    GpuVec<Fp> buf;                                              // the ms_join_report where the call wrote it
    ms_join_report read() const { const std::vector<uint64_t> w = buf.to_host(); ms_join_report r; memcpy(&r, w.data(), sizeof r); return r; }   // a host wait
};
template <class B>
inline JoinReport join_rows(const Matrix<B>& table, const LookupTuple& table_key, const Matrix<B>& base, const std::vector<LookupTuple>& keys) {
    Planner& pl = base.planner();
    auto record = [&](const LookupTuple& t) {
        if (t.cols.empty() || t.cols.size() > (size_t)MS_JOIN_MAX_WIDTH || t.cols.size() != table_key.cols.size())
            throw std::invalid_argument("join_rows: a key has 1 .. 4 columns, as many as the table key");
        ms_lookup_tuple r = {{0, 0, 0, 0}, t.mask, t.mask_col, 0, 0};
        for (size_t c = 0; c < t.cols.size(); c++) r.cols[c] = t.cols[c];
        return r;
    };
    if (keys.size() > (size_t)MS_JOIN_MAX_SETS) throw std::invalid_argument("join_rows: at most 8 key sets in one call");
    const ms_lookup_tuple trec = record(table_key);
    std::vector<ms_lookup_tuple> krecs;
    for (auto& t : keys) krecs.push_back(record(t));
    std::vector<const void*> tin, in;
    for (auto& c : table.columns) tin.push_back(c.ptr());
    for (auto& c : base.columns) in.push_back(c.ptr());
    const size_t n = base.num_rows();
    JoinReport rep{{}, GpuVec<Fp>(pl, sizeof(ms_join_report) / 8)};
    std::vector<void*> to;
    for (size_t s = 0; s < keys.size(); s++) rep.matches.push_back(RowOrder{GpuVec<Fp>(pl, (n + 1) / 2), GpuVec<Fp>(pl, sizeof(ms_sort_report) / 8), n});
    for (auto& m : rep.matches) to.push_back(m.index.ptr());
    check(ms_join_rows(pl.ctx(), B::id, table.num_rows(), tin.data(), (unsigned)tin.size(), &trec, n, in.data(), (unsigned)in.size(),
                       (unsigned)table_key.cols.size(), krecs.empty() ? nullptr : krecs.data(), (unsigned)krecs.size(), to.empty() ? nullptr : to.data(), rep.buf.ptr()));
    return rep;
}
// The `payload` columns (indices into `table`) of the table row that holds each base row's key: join_rows for the one set `key`, then
// permute_columns by the match; zero elements where the row is inactive or its key is not in the table.  -> (the columns, the join's report)
template <class B>
inline std::pair<Matrix<B>, JoinReport> fetch_columns(const Matrix<B>& table, const LookupTuple& table_key, const Matrix<B>& base, const LookupTuple& key,
                                                      const std::vector<int>& payload) {
    if (payload.empty()) throw std::invalid_argument("fetch_columns: no payload column");
    Planner& pl = base.planner();
    std::vector<const void*> in;
    for (int c : payload) {
        if (c < 0 || (size_t)c >= table.columns.size()) throw std::invalid_argument("fetch_columns: a payload column is an index into the table");
        in.push_back(table.columns[c].ptr());
    }
    JoinReport rep = join_rows<B>(table, table_key, base, {key});
    const size_t n = base.num_rows();
    Matrix<B> out;
    std::vector<void*> to;
    for (size_t c = 0; c < in.size(); c++) out.columns.emplace_back(pl, n);
    for (auto& c : out.columns) to.push_back(c.ptr());
    check(ms_permute_columns(pl.ctx(), B::id, table.num_rows(), in.data(), to.data(), (unsigned)in.size(), rep.matches[0].index.ptr(), n));
    return {std::move(out), std::move(rep)};
}

// The limb columns of a range check in one asynchronous call (ms_limb_decompose): for every spec, columns dst0 .. dst0 + nlimbs - 1 of `trace`
// get the limbs of column src -- limb j the bits [j * bits, (j + 1) * bits) of the canonical value -- and an inactive row zero limbs.  A value
// that does not fit is counted in the report and still gets its low limbs.  mask as ExtColumn's.
struct LimbSpec { int src = 0, dst0 = 0, nlimbs = 1, bits = 16, mask = MS_EXT_ALWAYS, mask_col = 0; };
struct LimbReport {
    GpuVec<Fp> buf;                                              // the ms_limb_report where the call wrote it
    ms_limb_report read() const { const std::vector<uint64_t> w = buf.to_host(); ms_limb_report r; memcpy(&r, w.data(), sizeof r); return r; }   // a host wait
};
template <class B>
inline LimbReport limb_decompose(Matrix<B>& trace, const std::vector<LimbSpec>& specs) {
    Planner& pl = trace.planner();
    if (specs.size() > (size_t)MS_RANGE_MAX_SPECS) throw std::invalid_argument("limb_decompose: at most 64 specs in one call");
    std::vector<ms_limb_spec> recs;
    for (auto& sp : specs) {
        if (sp.bits < 1 || sp.bits > MS_RANGE_MAX_LIMB_BITS || sp.nlimbs < 1 || sp.nlimbs > MS_RANGE_MAX_LIMBS || (unsigned)(sp.nlimbs * sp.bits) > 64u * B::words)
            throw std::invalid_argument("limb_decompose: 1 .. 256 limbs of 1 .. 32 bits, together no more than the bits of an element's words");
        recs.push_back(ms_limb_spec{sp.src, sp.dst0, sp.nlimbs, sp.bits, sp.mask, sp.mask_col, 0, 0});
    }
    std::vector<void*> cols;
    for (auto& c : trace.columns) cols.push_back(c.ptr());
    LimbReport rep{GpuVec<Fp>(pl, sizeof(ms_limb_report) / 8)};
    check(ms_limb_decompose(pl.ctx(), B::id, trace.num_rows(), cols.data(), (unsigned)cols.size(), recs.empty() ? nullptr : recs.data(), (unsigned)recs.size(), rep.buf.ptr()));
    return rep;
}

// The m column of a range check in one asynchronous call (ms_range_multiplicities): m[j] = how many active rows of the `sets` hold the value
// j, j < 2^bits, and zero from there to the end of m -- by direct indexing: no table column, no hash table.  A value that is not below 2^bits
// is counted as missing in the report (an ms_lookup_report; duplicate_table_rows is 0).  m: at least 2^bits elements, possibly a column of
// `trace` that no set and no mask names.
struct RangeSet { int col = 0, mask = MS_EXT_ALWAYS, mask_col = 0; };
using RangeReport = LookupReport;
template <class B>
inline RangeReport range_multiplicities(const Matrix<B>& trace, unsigned bits, const std::vector<RangeSet>& sets, GpuVec<B>& m) {
    Planner& pl = trace.planner();
    if (bits < 1 || bits > (unsigned)MS_RANGE_MAX_TABLE_BITS) throw std::invalid_argument("range_multiplicities: bits is 1 .. 24");
    if (sets.size() > (size_t)MS_RANGE_MAX_SETS) throw std::invalid_argument("range_multiplicities: at most 64 sets in one call");
    if (m.len() < ((size_t)1 << bits)) throw std::invalid_argument("range_multiplicities: m holds fewer elements than the table has rows");
    std::vector<ms_range_set> recs;
    for (auto& st : sets) recs.push_back(ms_range_set{st.col, st.mask, st.mask_col, 0});
    std::vector<const void*> in;
    for (auto& c : trace.columns) in.push_back(c.ptr());
    RangeReport rep{GpuVec<Fp>(pl, sizeof(ms_lookup_report) / 8)};
    check(ms_range_multiplicities(pl.ctx(), B::id, trace.num_rows(), in.data(), (unsigned)in.size(), bits, recs.empty() ? nullptr : recs.data(), (unsigned)recs.size(),
                                  m.len(), m.ptr(), rep.buf.ptr()));
    return rep;
}

// The result columns of bitwise operations in one asynchronous call (ms_bitwise_columns): for every spec, column dst of `trace` gets
// (a mod 2^width) op (b mod 2^width) on the canonical integers of columns a and b -- op MS_BIT_AND, MS_BIT_OR or MS_BIT_XOR, a == b allowed --
// and an inactive row zero.  An operand that does not fit `width` bits is counted in the report (an ms_limb_report).  mask as ExtColumn's.
struct BitwiseSpec { int op = MS_BIT_XOR, a = 0, b = 0, dst = 0, width = 32, mask = MS_EXT_ALWAYS, mask_col = 0; };
template <class B> inline unsigned bitwise_wmax() { return B::words == 1 ? 63u : 251u; }          // 2^wmax: the widest power of two below the modulus
template <class B>
inline LimbReport bitwise_columns(Matrix<B>& trace, const std::vector<BitwiseSpec>& specs) {
    Planner& pl = trace.planner();
    if (specs.size() > (size_t)MS_BITWISE_MAX_SPECS) throw std::invalid_argument("bitwise_columns: at most 64 specs in one call");
    std::vector<ms_bitwise_spec> recs;
    for (auto& sp : specs) {
        if (sp.width < 1 || (unsigned)sp.width > bitwise_wmax<B>()) throw std::invalid_argument("bitwise_columns: an operand has 1 .. 63 bits over Fp, 1 .. 251 over Fp252");
        recs.push_back(ms_bitwise_spec{sp.op, sp.a, sp.b, sp.dst, sp.width, sp.mask, sp.mask_col, 0});
    }
    std::vector<void*> cols;
    for (auto& c : trace.columns) cols.push_back(c.ptr());
    LimbReport rep{GpuVec<Fp>(pl, sizeof(ms_limb_report) / 8)};
    check(ms_bitwise_columns(pl.ctx(), B::id, trace.num_rows(), cols.data(), (unsigned)cols.size(), recs.empty() ? nullptr : recs.data(), (unsigned)recs.size(), rep.buf.ptr()));
    return rep;
}

// The table (op, x, y, x op y) over all pairs of `bits`-bit limbs, op by op in the order of `ops`, written where it is used
// (ms_bitwise_table) and padded to the columns' length by repeating its last row.  top: the op column, or null for none.
inline size_t bitwise_table_rows(unsigned bits, const std::vector<int>& ops) {
    if (bits < 1 || bits > (unsigned)MS_BITWISE_MAX_BITS || ops.empty() || ops.size() > (size_t)MS_BITWISE_MAX_OPS || (ops.size() << (2 * bits)) > ((size_t)1 << MS_BITWISE_MAX_TABLE_LOG))
        throw std::invalid_argument("bitwise table: bits is 1 .. 12, 1 .. 3 ops, at most 2^24 rows");
    return ops.size() << (2 * bits);
}
template <class B>
inline void bitwise_table(unsigned bits, const std::vector<int>& ops, GpuVec<B>* top, GpuVec<B>& tx, GpuVec<B>& ty, GpuVec<B>& tz) {
    Planner& pl = tx.planner();
    const size_t T = bitwise_table_rows(bits, ops), n_t = tx.len();
    if (n_t < T || ty.len() != n_t || tz.len() != n_t || (top && top->len() != n_t)) throw std::invalid_argument("bitwise_table: columns of one length, at least the table's rows");
    std::vector<int32_t> codes(ops.begin(), ops.end());
    check(ms_bitwise_table(pl.ctx(), B::id, bits, codes.data(), (unsigned)codes.size(), n_t, top ? top->ptr() : nullptr, tx.ptr(), ty.ptr(), tz.ptr()));
}

// The m column of a bitwise lookup in one asynchronous call (ms_bitwise_multiplicities): m[slot * 4^bits + (x << bits) + y] = how many
// limb pairs (x, y) the active rows of the `sets` whose op stands at `slot` of `ops` hold, counted from the word columns a, b (and checked
// against c, unless c is -1); zero from the table's end to the end of m.  A row with an operand not below 2^(nlimbs * bits), or with
// c != a op b, is counted as missing in the report (an ms_lookup_report) and none of its limbs is counted.
struct BitwiseSet { int op = MS_BIT_XOR, a = 0, b = 0, c = -1, nlimbs = 1, mask = MS_EXT_ALWAYS, mask_col = 0; };
using BitwiseReport = LookupReport;
template <class B>
inline BitwiseReport bitwise_multiplicities(const Matrix<B>& trace, unsigned bits, const std::vector<int>& ops, const std::vector<BitwiseSet>& sets, GpuVec<B>& m) {
    Planner& pl = trace.planner();
    const size_t T = bitwise_table_rows(bits, ops);
    if (sets.size() > (size_t)MS_BITWISE_MAX_SETS) throw std::invalid_argument("bitwise_multiplicities: at most 64 sets in one call");
    if (m.len() < T) throw std::invalid_argument("bitwise_multiplicities: m holds fewer elements than the table has rows");
    std::vector<ms_bitwise_set> recs;
    for (auto& st : sets) {
        if (st.nlimbs < 1 || st.nlimbs > MS_BITWISE_MAX_LIMBS || (unsigned)st.nlimbs * bits > bitwise_wmax<B>())
            throw std::invalid_argument("bitwise_multiplicities: 1 .. 256 limbs, together no more than 63 bits over Fp, 251 over Fp252");
        recs.push_back(ms_bitwise_set{st.op, st.a, st.b, st.c, st.nlimbs, st.mask, st.mask_col, 0});
    }
    std::vector<int32_t> codes(ops.begin(), ops.end());
    std::vector<const void*> in;
    for (auto& c : trace.columns) in.push_back(c.ptr());
    BitwiseReport rep{GpuVec<Fp>(pl, sizeof(ms_lookup_report) / 8)};
    check(ms_bitwise_multiplicities(pl.ctx(), B::id, trace.num_rows(), in.data(), (unsigned)in.size(), bits, codes.data(), (unsigned)codes.size(),
                                    recs.empty() ? nullptr : recs.data(), (unsigned)recs.size(), m.len(), m.ptr(), rep.buf.ptr()));
    return rep;
}

// A table whose row count differs from its source's, derived where the source lies (ms_gap_plan, ms_gap_fill): the rows the mask lets
// through, a dummy row for every counter value missing between two consecutive rows that agree on the group columns, the last row repeated
// up to n_out.  group: 0 .. MS_GAP_MAX_GROUP indices into the base matrix; counter: the clock column or -1 for no gaps; mask as ExtColumn's.
struct GapSpec { std::vector<int> group; int counter = -1; int mask = MS_EXT_ALWAYS, mask_col = 0; };
struct GapPlan {
    GpuVec<Fp> start;                                            // (n + 1) x uint64: the prefix sums
    GpuVec<Fp> report;                                           // the ms_gap_report
    const RowOrder* order = nullptr;                             // the permutation the plan went through, or null; the caller keeps it alive
    size_t n = 0;
    std::vector<uint64_t> to_host() const { return start.to_host(); }   // a host wait
    ms_gap_report read() const { const std::vector<uint64_t> w = report.to_host(); ms_gap_report r; memcpy(&r, w.data(), sizeof r); return r; }   // a host wait
};
template <class B>
inline GapPlan gap_plan(const Matrix<B>& base, const GapSpec& spec, const RowOrder* order = nullptr, size_t n = (size_t)-1) {
    Planner& pl = base.planner();
    if (spec.group.size() > (size_t)MS_GAP_MAX_GROUP) throw std::invalid_argument("gap_plan: a group has 0 .. 3 columns");
    const size_t held = order ? order->n : base.num_rows();
    if (n == (size_t)-1) n = held;
    if (n > held) throw std::invalid_argument("gap_plan: more positions than the index or the columns hold");
    ms_gap_spec rec = {{0, 0, 0}, (int32_t)spec.group.size(), spec.counter, spec.mask, spec.mask_col, 0};
    for (size_t c = 0; c < spec.group.size(); c++) rec.group[c] = spec.group[c];
    std::vector<const void*> in;
    for (auto& c : base.columns) in.push_back(c.ptr());
    GapPlan out{GpuVec<Fp>(pl, n + 1), GpuVec<Fp>(pl, sizeof(ms_gap_report) / 8), order, n};
    check(ms_gap_plan(pl.ctx(), B::id, base.num_rows(), in.data(), (unsigned)in.size(), &rec, order ? order->index.ptr() : nullptr, n, out.start.ptr(),
                      out.report.ptr()));
    return out;
}
// columns: (MS_GAP_COPY | MS_GAP_ZERO | MS_GAP_COUNTER | MS_GAP_FLAG, source column); n_out: by default the least power of two >= max(rows_out, 1),
// which reads the report (the only host wait)
template <class B>
inline Matrix<B> gap_fill(const Matrix<B>& base, const GapPlan& plan, const std::vector<ms_gap_column>& columns, size_t n_out = (size_t)-1) {
    Planner& pl = base.planner();
    if (columns.empty() || columns.size() > (size_t)MS_GAP_MAX_COLUMNS) throw std::invalid_argument("gap_fill: 1 .. 128 columns");
    if (n_out == (size_t)-1) {
        const uint64_t rows = plan.read().rows_out;
        for (n_out = 1; n_out < rows; n_out *= 2) {}
    }
    Matrix<B> out;
    std::vector<const void*> in;
    std::vector<void*> to;
    for (auto& c : base.columns) in.push_back(c.ptr());
    for (size_t c = 0; c < columns.size(); c++) out.columns.emplace_back(pl, n_out);
    for (auto& c : out.columns) to.push_back(c.ptr());
    check(ms_gap_fill(pl.ctx(), B::id, base.num_rows(), in.data(), (unsigned)in.size(), plan.order ? plan.order->index.ptr() : nullptr, plan.n, plan.start.ptr(),
                      columns.data(), to.data(), (unsigned)columns.size(), n_out));
    return out;
}

// `fold_positions` (src/fri.rs:615-622): strictly increasing positions -> their cosets, deduplicated
inline std::vector<size_t> fold_positions(const std::vector<size_t>& positions, unsigned folding_factor) {
    std::vector<size_t> out;
    for (size_t i = 1; i < positions.size(); i++)          // the reference's precondition (src/fri.rs:613), asserted by the Python mirror too
        if (positions[i] <= positions[i - 1]) throw std::invalid_argument("fold_positions: positions must be strictly increasing");
    for (size_t p : positions) if (out.empty() || out.back() != p / folding_factor) out.push_back(p / folding_factor);
    return out;
}
// rows `positions` of Matrix::from_arrays(evaluations.as_chunks::<N>()) (src/fri.rs:213-215): N consecutive evaluations each,
// gathered on the device as 32-byte records (FriProver::into_proof, src/fri.rs:148-165)
template <class F>
inline Pending fri_layer_rows_launch(const GpuVec<F>& layer, unsigned folding_factor, const std::vector<size_t>& positions, GatherArena* arena = nullptr) {
    const size_t words = (size_t)folding_factor * F::words;
    if (words % 4) throw std::invalid_argument("fri_layer_rows_launch: rows shorter than a 32-byte record");
    Planner& pl = layer.planner();
    Pending out(pl, positions.size() * words * 8, arena);
    if (!out.bytes()) return out;
    const size_t per = words / 4;
    std::vector<uint64_t> ids;
    for (size_t p : positions) for (size_t k = 0; k < per; k++) ids.push_back(p * per + k);
    gather_digests_into(pl, layer.ptr(), layer.len() * F::words / 4, ids, out.ptr(), arena);
    return out;
}
template <class F>
inline std::vector<uint64_t> fri_layer_rows(const GpuVec<F>& layer, unsigned folding_factor, const std::vector<size_t>& positions) {
    const size_t words = (size_t)folding_factor * F::words;
    if (words % 4) {                                       // rows shorter than a record: tiny layers only
        std::vector<uint64_t> out(positions.size() * words);
        if (out.empty()) return out;
        const auto all = layer.to_host();
        for (size_t i = 0; i < positions.size(); i++) memcpy(&out[i * words], &all[positions[i] * words], words * 8);
        return out;
    }
    return fri_layer_rows_launch(layer, folding_factor, positions).template fetch<uint64_t>();
}

// Queries::new: rows of the three LDE matrices at the query positions + batched openings of the three trees.  With an arena
// the constructor only launches the gathers (into the arena) and fetch() fills the fields, so that a prover can put the
// FRI layer openings into the same arena and download everything once.
template <class FqT>
struct Queries {
    std::vector<uint64_t> base_trace_values, extension_trace_values, composition_trace_values;
    MerkleTree::MerkleView base_trace_proof, extension_trace_proof, composition_trace_proof;
    Queries(const Matrix<Fp>& base_lde, const Matrix<FqT>* extension_lde, const Matrix<FqT>& composition_lde,
            const MerkleTree& base_tree, const MerkleTree* extension_tree, const MerkleTree& composition_tree, const std::vector<size_t>& positions,
            GatherArena* arena = nullptr) : has_ext_tree_(extension_tree), has_ext_lde_(extension_lde) {
        std::vector<uint64_t> pos(positions.begin(), positions.end());
        // every gather first, then the downloads: one wait for the device instead of eight
        bp_ = base_tree.prove_launch(positions, arena);
        if (extension_tree) ep_ = extension_tree->prove_launch(positions, arena);
        cp_ = composition_tree.prove_launch(positions, arena);
        bv_ = base_lde.get_rows_launch(pos, arena);
        cv_ = composition_lde.get_rows_launch(pos, arena);
        if (extension_lde) ev_ = extension_lde->get_rows_launch(pos, arena);
        if (!arena) fetch();
    }
    void fetch() {
        if (fetched_) return;
        fetched_ = true;
        base_trace_proof = bp_.fetch();
        if (has_ext_tree_) extension_trace_proof = ep_.fetch();
        composition_trace_proof = cp_.fetch();
        base_trace_values = bv_.template fetch<uint64_t>();
        if (has_ext_lde_) extension_trace_values = ev_.template fetch<uint64_t>();
        composition_trace_values = cv_.template fetch<uint64_t>();
    }
private:
    MerkleTree::PendingView bp_, ep_, cp_;
    Pending bv_, ev_, cv_;
    bool has_ext_tree_, has_ext_lde_, fetched_ = false;
};

// PublicCoin::grind_proof_of_work(bits): the smallest nonce >= 1 with `bits` leading zero bits of H(seed || nonce_be),
// H = SHA-256 (Hash::Sha256, also what an RPO-256 prover grinds with), BLAKE2s-256 (Hash::Blake2s), Keccak-256, SHA3-256 or BLAKE3 (Hash::Blake3_256)
inline uint64_t grind_proof_of_work(Planner& pl, const std::array<uint8_t, 32>& seed, unsigned proof_of_work_bits, uint64_t max_nonce = (uint64_t)1 << 40,
                                    Hash h = Hash::Sha256) {
    uint64_t nonce = 0;
    check(hash_pow_grind(pl.ctx(), h, seed.data(), proof_of_work_bits, max_nonce, &nonce));
    return nonce;
}

// What the three device-resident coins below share: every method is one entry point of the family's table on the coin's handle.  The reseeds
// and draw() enqueue and return; draw_queries, grind and state wait for the device.  state(): the family's ms_*_coin_state, as stored.
struct CoinAbi {
    int (*destroy)(ms_ctx*, void*);
    int (*read)(ms_ctx*, const void*, void*);
    int (*reseed_digest)(ms_ctx*, void*, const void*);
    int (*reseed_int)(ms_ctx*, void*, uint64_t);
    int (*reseed_elements)(ms_ctx*, void*, int, const void*, size_t);
    int (*reseed_elements_host)(ms_ctx*, void*, int, const void*, size_t);
    int (*draw)(ms_ctx*, void*, int, size_t, void*);
    int (*draw_queries)(ms_ctx*, void*, size_t, size_t, uint64_t*, size_t*);
    int (*pow_grind)(ms_ctx*, void*, unsigned, uint64_t, uint64_t*);
};
template <class State>
class Coin {
public:
    ~Coin() { if (coin_) abi_.destroy(pl_->ctx(), coin_); }
    Coin(const Coin&) = delete; Coin& operator=(const Coin&) = delete;
    void reseed_digest(const void* d_digest) { check(abi_.reseed_digest(pl_->ctx(), coin_, d_digest)); }          // e.g. tree.root_ptr() of a tree of the coin's hash
    void reseed_int(uint64_t value) { check(abi_.reseed_int(pl_->ctx(), coin_, value)); }
    template <class F> void reseed_elements(const GpuVec<F>& elems, size_t count) { check(abi_.reseed_elements(pl_->ctx(), coin_, F::id, elems.ptr(), count)); }
    template <class F> void reseed_elements(const GpuVec<F>& elems) { reseed_elements(elems, elems.len()); }
    template <class F> void reseed_elements(const std::vector<uint64_t>& mont_words) {                            // host elements, Montgomery words
        check(abi_.reseed_elements_host(pl_->ctx(), coin_, F::id, mont_words.data(), mont_words.size() / F::words));
    }
    template <class F> GpuVec<F> draw(size_t count = 1) { GpuVec<F> out(*pl_, count); check(abi_.draw(pl_->ctx(), coin_, F::id, count, out.ptr())); return out; }
    std::vector<size_t> draw_queries(size_t max_n, size_t domain_size) {
        std::vector<uint64_t> pos(max_n ? max_n : 1);
        size_t n = 0;
        check(abi_.draw_queries(pl_->ctx(), coin_, max_n, domain_size, pos.data(), &n));
        return std::vector<size_t>(pos.begin(), pos.begin() + n);
    }
    uint64_t grind(unsigned bits, uint64_t max_nonce = (uint64_t)1 << 40) { uint64_t nonce = 0; check(abi_.pow_grind(pl_->ctx(), coin_, bits, max_nonce, &nonce)); return nonce; }
    State state() const { State st; check(abi_.read(pl_->ctx(), coin_, &st)); return st; }
protected:
    Coin(Planner& pl, const CoinAbi& abi) : pl_(&pl), abi_(abi) {}                                                // the family's constructor creates coin_
    Planner* pl_;
    const CoinAbi& abi_;
    void* coin_ = nullptr;
};

// PublicCoinImpl<F, H> (src/random.rs:61-141) with its state in device memory (ms_coin_*): H = SHA-256, or BLAKE2s-256 / Keccak-256 /
// SHA3-256 / BLAKE3 for Hash::Blake2s / Keccak256 / Sha3_256 / Blake3_256 (ids 0, 1, 3, 4, 6; an RPO-256 prover's coin is SHA-256 unless it asks for RpoCoin, below; ids 2 and 5 stay unknown).
class PublicCoin : public Coin<ms_coin_state> {
    static constexpr CoinAbi abi = {ms_coin_destroy, ms_coin_read, ms_coin_reseed_digest, ms_coin_reseed_int, ms_coin_reseed_elements, ms_coin_reseed_elements_host,
                                    ms_coin_draw, ms_coin_draw_queries, ms_coin_pow_grind};
public:
    PublicCoin(Planner& pl, const std::array<uint8_t, 32>& seed, Hash h = Hash::Sha256) : Coin(pl, abi) {          // PublicCoin::new
        const int id = h == Hash::Blake2s ? MS_HASH_BLAKE2S : h == Hash::Keccak256 ? MS_HASH_KECCAK256 : h == Hash::Sha3_256 ? MS_HASH_SHA3_256 : h == Hash::Blake3_256 ? MS_HASH_BLAKE3 : MS_HASH_SHA256;
        check(ms_coin_create(pl.ctx(), id, seed.data(), &coin_));
    }
};

// The RPO-256 public coin (ms_rpo_coin_*, include/ministark_hip_rpo_coin.h): PublicCoin's methods over a 12-element sponge that absorbs and
// draws Goldilocks elements (Fp or Fq3), for a prover whose verifier runs inside another proof.  seed: four canonical integers below p.
// state(): Montgomery words.
class RpoCoin : public Coin<ms_rpo_coin_state> {
    static constexpr CoinAbi abi = {ms_rpo_coin_destroy, ms_rpo_coin_read, ms_rpo_coin_reseed_digest, ms_rpo_coin_reseed_int, ms_rpo_coin_reseed_elements,
                                    ms_rpo_coin_reseed_elements_host, ms_rpo_coin_draw, ms_rpo_coin_draw_queries, ms_rpo_coin_pow_grind};
public:
    RpoCoin(Planner& pl, const std::array<uint64_t, 4>& seed) : Coin(pl, abi) {
        uint64_t m[4];
        for (int q = 0; q < 4; q++) { if (seed[q] >= gl::P) throw std::invalid_argument("RpoCoin: seed words are below p"); m[q] = gl::to_mont(seed[q]); }
        check(ms_rpo_coin_create(pl.ctx(), m, &coin_));
    }
};

// The Poseidon public coin of the 252-bit field (ms_hades_coin_*, include/ministark_hip_hades_coin.h): RpoCoin's methods over one field
// element and a draw counter, for an Fp252 prover that commits with Hash::Poseidon252 and whose verifier runs inside another proof.
// seed: one element below p as four canonical little-endian words.  state(): the digest in Montgomery words.
class PoseidonCoin : public Coin<ms_hades_coin_state> {
    static constexpr CoinAbi abi = {ms_hades_coin_destroy, ms_hades_coin_read, ms_hades_coin_reseed_digest, ms_hades_coin_reseed_int, ms_hades_coin_reseed_elements,
                                    ms_hades_coin_reseed_elements_host, ms_hades_coin_draw, ms_hades_coin_draw_queries, ms_hades_coin_pow_grind};
public:
    PoseidonCoin(Planner& pl, const std::array<uint64_t, 4>& seed) : Coin(pl, abi) {
        lib252::f252::E e;
        for (int q = 0; q < 4; q++) e.l[q] = seed[q];
        if (lib252::f252::geq_p(e)) throw std::invalid_argument("PoseidonCoin: the seed is below p");
        check(ms_hades_coin_create(pl.ctx(), seed.data(), &coin_));
    }
};

// DeepPolyComposer::new(air, z, base_trace_polys, extension_trace_polys, composition_trace_polys)
// trace_arguments: the AIR's (column, offset) pairs (air.trace_arguments()).  Polynomials are coefficient-form
// matrices on the device (what interpolate / into_polynomials return).  FqT = Fq3 or Fp (Fq = Fp AIRs).
struct DeepCompositionCoeffs { std::vector<FqVal> execution_trace, composition_trace; FqVal degree[2]; };   // src/composer.rs:191-198
template <class FqT>
class DeepPolyComposer {
public:
    DeepPolyComposer(std::vector<std::pair<unsigned, int>> trace_arguments, size_t trace_len, FqVal z, const Matrix<Fp>& base_polys,
                     const Matrix<FqT>* extension_polys, const Matrix<FqT>& composition_polys)
        : args_(std::move(trace_arguments)), n_(trace_len), z_(z), base_(base_polys), ext_(extension_polys), comp_(composition_polys) {
        Radix2EvaluationDomain d(trace_len);
        g_ = d.group_gen; g_inv_ = gl::pow(g_, gl::P - 2);
        nbase_ = (unsigned)base_.num_cols();
    }
    // -> (execution trace values in trace_arguments order, composition trace values)   src/composer.rs:43-86
    std::pair<std::vector<FqVal>, std::vector<FqVal>> get_ood_evals() {
        std::vector<unsigned> bq_col, eq_col; std::vector<FqVal> bq_pt, eq_pt;
        for (auto& a : args_) { if (a.first < nbase_) { bq_col.push_back(a.first); bq_pt.push_back(point(a.second)); } else { eq_col.push_back(a.first - nbase_); eq_pt.push_back(point(a.second)); } }
        const FqVal z_n = fq::pow(z_, comp_.num_cols());
        std::vector<unsigned> cc; std::vector<FqVal> cp;
        for (unsigned c = 0; c < comp_.num_cols(); c++) { cc.push_back(c); cp.push_back(z_n); }
        // matrices over the same field with the same number of rows share ONE launch and one download (every call is a wait of the host for
        // the device and of the device for the host's next launch): the composition-trace polynomials ride with the trace polynomials of
        // their field -- the base trace's when Fq = Fp, the extension trace's otherwise
        std::vector<FqVal> bv, ev, cv;
        bool comp_done = false;
        if constexpr (FqT::words == 1) {
            if (comp_.num_rows() == base_.num_rows() && base_.num_cols() + comp_.num_cols() <= 96 && !bq_col.empty()) {
                auto cols = ptrs_of(base_); for (auto& c : comp_.columns) cols.push_back(c.ptr());
                auto qc = bq_col; auto qp = bq_pt;
                for (unsigned c : cc) qc.push_back((unsigned)base_.num_cols() + c);
                qp.insert(qp.end(), cp.begin(), cp.end());
                const auto all = horner_cols<Fp>(base_.planner(), base_.num_rows(), cols, qc, qp);
                bv.assign(all.begin(), all.begin() + bq_col.size()); cv.assign(all.begin() + bq_col.size(), all.end());
                if (ext_) ev = horner(*ext_, eq_col, eq_pt);      // an Fq = Fp AIR may still carry extension columns (over Fp): their own launch
                comp_done = true;
            }
        } else if (ext_ && comp_.num_rows() == ext_->num_rows() && ext_->num_cols() + comp_.num_cols() <= 96 && !eq_col.empty()) {
            auto cols = ptrs_of(*ext_); for (auto& c : comp_.columns) cols.push_back(c.ptr());
            auto qc = eq_col; auto qp = eq_pt;
            for (unsigned c : cc) qc.push_back((unsigned)ext_->num_cols() + c);
            qp.insert(qp.end(), cp.begin(), cp.end());
            const auto all = horner_cols<FqT>(base_.planner(), ext_->num_rows(), cols, qc, qp);
            ev.assign(all.begin(), all.begin() + eq_col.size()); cv.assign(all.begin() + eq_col.size(), all.end());
            bv = horner(base_, bq_col, bq_pt);
            comp_done = true;
        }
        if (!comp_done) {
            bv = horner(base_, bq_col, bq_pt);
            if (ext_) ev = horner(*ext_, eq_col, eq_pt);
            cv = horner(comp_, cc, cp);
        }
        size_t bi = 0, ei = 0;
        std::vector<FqVal> execution;
        for (auto& a : args_) execution.push_back(a.first < nbase_ ? bv[bi++] : ev[ei++]);
        ood_exec_ = execution; ood_comp_ = cv; have_ood_ = true;
        return {ood_exec_, ood_comp_};
    }
    GpuVec<FqT> into_deep_poly(const DeepCompositionCoeffs& coeffs) {           // src/composer.rs:89-188
        std::vector<const void*> bp, ep;
        for (auto& c : base_.columns) bp.push_back(c.ptr());
        auto& second = FqT::words == 1 ? bp : ep;                    // Fq = Fp: everything is a base column
        if (ext_) for (auto& c : ext_->columns) second.push_back(c.ptr());
        for (auto& c : comp_.columns) second.push_back(c.ptr());
        unsigned log_n = 0; while (((size_t)1 << log_n) < n_) log_n++;
        return compose(coeffs, bp, ep, n_, [&](Planner& pl, const Terms& t, void* out) {
            return ms_deep_compose(pl.ctx(), FqT::id, log_n, nullptr, bp.empty() ? nullptr : bp.data(), (unsigned)bp.size(), ep.empty() ? nullptr : ep.data(), (unsigned)ep.size(),
                                   t.pts.data(), t.npoints, t.tcol.data(), t.tpoint.data(), t.al.data(), t.od.data(), (unsigned)t.tcol.size(), t.da.data(), t.db.data(), out); });
    }
    // into_deep_poly(coeffs) followed by into_bit_reversed_evaluations(lde_domain) (src/prover.rs:149-152) in one step: the polynomial's
    // values on the LDE domain (domain_size points, offset 7) computed from the committed LDE matrices themselves (ms_deep_rows) -- the
    // same field elements, without the coset transforms, the inverse transform and the LDE.  Goldilocks fields.
    GpuVec<FqT> into_deep_evaluations(const DeepCompositionCoeffs& coeffs, const Matrix<Fp>& base_lde, const Matrix<FqT>* ext_lde, const Matrix<FqT>& comp_lde) {
        const size_t N = base_lde.num_rows();
        if (comp_lde.num_rows() != N || (ext_lde && ext_lde->num_rows() != N)) throw std::invalid_argument("into_deep_evaluations: LDE matrices of different heights");
        std::vector<const void*> bp, ep;
        for (auto& c : base_lde.columns) bp.push_back(c.ptr());
        auto& second = FqT::words == 1 ? bp : ep;
        if (ext_lde) for (auto& c : ext_lde->columns) second.push_back(c.ptr());
        for (auto& c : comp_lde.columns) second.push_back(c.ptr());
        unsigned log_N = 0; while (((size_t)1 << log_N) < N) log_N++;
        return compose(coeffs, bp, ep, N, [&](Planner& pl, const Terms& t, void* out) {
            return ms_deep_rows(pl.ctx(), FqT::id, log_N, nullptr, 0, N, bp.empty() ? nullptr : bp.data(), (unsigned)bp.size(), ep.empty() ? nullptr : ep.data(), (unsigned)ep.size(),
                                t.pts.data(), t.npoints, t.tcol.data(), t.tpoint.data(), t.al.data(), t.od.data(), (unsigned)t.tcol.size(), t.da.data(), t.db.data(), out); });
    }
private:
    struct Terms { std::vector<unsigned> tcol, tpoint; std::vector<uint64_t> pts, al, od, da, db; unsigned npoints = 0; };
    template <class Call>
    GpuVec<FqT> compose(const DeepCompositionCoeffs& coeffs, const std::vector<const void*>&, const std::vector<const void*>&, size_t out_len, Call call) {
        if (!have_ood_) get_ood_evals();
        Planner& pl = base_.planner();
        std::vector<FqVal> points;
        auto pid = [&](const FqVal& p) { for (size_t k = 0; k < points.size(); k++) if (points[k] == p) return (unsigned)k; points.push_back(p); return (unsigned)points.size() - 1; };
        const FqVal z_n = fq::pow(z_, comp_.num_cols());
        const unsigned next = ext_ ? (unsigned)ext_->num_cols() : 0;
        Terms t;
        std::vector<FqVal> talpha, tood;
        for (unsigned c = 0; c < comp_.num_cols(); c++) { t.tcol.push_back(nbase_ + next + c); t.tpoint.push_back(pid(z_n)); talpha.push_back(coeffs.composition_trace.at(c)); tood.push_back(ood_comp_[c]); }
        for (size_t k = 0; k < args_.size(); k++) { t.tcol.push_back(args_[k].first); t.tpoint.push_back(pid(point(args_[k].second))); talpha.push_back(coeffs.execution_trace.at(k)); tood.push_back(ood_exec_[k]); }
        auto flat = [](const std::vector<FqVal>& v) { std::vector<uint64_t> o; for (auto& q : v) fq::push_words<FqT>(o, q); return o; };
        t.pts = flat(points); t.al = flat(talpha); t.od = flat(tood); t.da = flat({coeffs.degree[0]}); t.db = flat({coeffs.degree[1]});
        t.npoints = (unsigned)points.size();
        GpuVec<FqT> out(pl, out_len);
        check(call(pl, t, out.ptr()));
        return out;
    }
    FqVal point(int offset) const { return fq::mul_base(z_, gl::pow(offset >= 0 ? g_ : g_inv_, (uint64_t)(offset >= 0 ? offset : -offset))); }
    template <class CF> static std::vector<const void*> ptrs_of(const Matrix<CF>& m) { std::vector<const void*> in; for (auto& c : m.columns) in.push_back(c.ptr()); return in; }
    template <class CF>
    static std::vector<FqVal> horner_cols(Planner& pl, size_t nrows, const std::vector<const void*>& in, const std::vector<unsigned>& qcol, const std::vector<FqVal>& qpt) {
        std::vector<FqVal> res;
        if (qcol.empty()) return res;
        std::vector<uint64_t> pts, out(qcol.size() * FqT::words);
        for (auto& p : qpt) fq::push_words<FqT>(pts, p);
        check(ms_horner_eval(pl.ctx(), CF::id, FqT::id, nrows, in.data(), (unsigned)in.size(), qcol.data(), pts.data(), (unsigned)qcol.size(), out.data()));
        for (size_t k = 0; k < qcol.size(); k++) res.push_back(fq::from_words<FqT>(&out[k * FqT::words]));
        return res;
    }
    template <class CF>
    std::vector<FqVal> horner(const Matrix<CF>& m, const std::vector<unsigned>& qcol, const std::vector<FqVal>& qpt) {
        if (qcol.empty()) return {};
        return horner_cols<CF>(m.planner(), m.num_rows(), ptrs_of(m), qcol, qpt);
    }
    std::vector<std::pair<unsigned, int>> args_;
    size_t n_; FqVal z_; const Matrix<Fp>& base_; const Matrix<FqT>* ext_; const Matrix<FqT>& comp_;
    uint64_t g_ = 1, g_inv_ = 1; unsigned nbase_ = 0;
    std::vector<FqVal> ood_exec_, ood_comp_; bool have_ood_ = false;
};

// ---- the composer over the 252-bit field (Fq = Fp = Fp252: no extension, every column a base column).  Host values are Montgomery
// words (f252::E): what the C ABI takes and what f252:: multiplies.  Same methods as above; the LDE offset defaults to the field's generator 3.
struct DeepCompositionCoeffs252 { std::vector<f252::E> execution_trace, composition_trace; f252::E degree[2]; };
template <>
class DeepPolyComposer<Fp252> {
public:
    DeepPolyComposer(std::vector<std::pair<unsigned, int>> trace_arguments, size_t trace_len, f252::E z, const Matrix<Fp252>& base_polys,
                     const Matrix<Fp252>& composition_polys)
        : args_(std::move(trace_arguments)), n_(trace_len), z_(z), base_(base_polys), comp_(composition_polys) {
        unsigned log_n = 0; while (((size_t)1 << log_n) < trace_len) log_n++;
        g_ = f252::root_of_unity(log_n); g_inv_ = f252::inv(g_);
        nbase_ = (unsigned)base_.num_cols();
    }
    f252::E point(int offset) const { return f252::mul(z_, f252::pow_u64(offset >= 0 ? g_ : g_inv_, (uint64_t)(offset >= 0 ? offset : -offset))); }
    f252::E composition_point() const { return f252::pow_u64(z_, comp_.num_cols()); }
    std::pair<std::vector<f252::E>, std::vector<f252::E>> get_ood_evals() {
        std::vector<const void*> cols;
        for (auto& c : base_.columns) cols.push_back(c.ptr());
        std::vector<unsigned> qc; std::vector<uint64_t> pts;
        auto push = [&](unsigned col, const f252::E& p) { qc.push_back(col); pts.insert(pts.end(), p.l, p.l + 4); };
        for (auto& a : args_) push(a.first, point(a.second));
        const bool together = comp_.num_rows() == base_.num_rows() && base_.num_cols() + comp_.num_cols() <= 96;   // one launch, one download
        std::vector<uint64_t> out((args_.size() + comp_.num_cols()) * 4);
        if (together) {
            for (auto& c : comp_.columns) cols.push_back(c.ptr());
            for (unsigned c = 0; c < comp_.num_cols(); c++) push(nbase_ + c, composition_point());
            check(ms_horner_eval(base_.planner().ctx(), Fp252::id, Fp252::id, base_.num_rows(), cols.data(), (unsigned)cols.size(), qc.data(), pts.data(), (unsigned)qc.size(), out.data()));
        } else {
            if (!qc.empty()) check(ms_horner_eval(base_.planner().ctx(), Fp252::id, Fp252::id, base_.num_rows(), cols.data(), (unsigned)cols.size(), qc.data(), pts.data(), (unsigned)qc.size(), out.data()));
            std::vector<const void*> cc; std::vector<unsigned> cq; std::vector<uint64_t> cp;
            const f252::E zn = composition_point();
            for (unsigned c = 0; c < comp_.num_cols(); c++) { cc.push_back(comp_.columns[c].ptr()); cq.push_back(c); cp.insert(cp.end(), zn.l, zn.l + 4); }
            check(ms_horner_eval(base_.planner().ctx(), Fp252::id, Fp252::id, comp_.num_rows(), cc.data(), (unsigned)cc.size(), cq.data(), cp.data(), (unsigned)cq.size(), out.data() + args_.size() * 4));
        }
        auto at = [&](size_t k) { f252::E e; memcpy(e.l, &out[4 * k], 32); return e; };
        ood_exec_.clear(); ood_comp_.clear();
        for (size_t k = 0; k < args_.size(); k++) ood_exec_.push_back(at(k));
        for (size_t c = 0; c < comp_.num_cols(); c++) ood_comp_.push_back(at(args_.size() + c));
        have_ood_ = true;
        return {ood_exec_, ood_comp_};
    }
    GpuVec<Fp252> into_deep_poly(const DeepCompositionCoeffs252& coeffs) {
        unsigned log_n = 0; while (((size_t)1 << log_n) < n_) log_n++;
        return compose(coeffs, base_, comp_, n_, [&](Planner& pl, const std::vector<const void*>& cols, const Terms& t, void* out) {
            return ms_deep_compose(pl.ctx(), Fp252::id, log_n, nullptr, cols.data(), (unsigned)cols.size(), nullptr, 0, t.pts.data(), t.npoints, t.tcol.data(), t.tpoint.data(),
                                   t.al.data(), t.od.data(), (unsigned)t.tcol.size(), t.da.data(), t.db.data(), out); });
    }
    // the polynomial's values at rows [first, first + base_lde.num_rows()) of the bit-reversed LDE domain of domain_size points (0: the
    // matrices hold the whole domain), from those rows of the committed LDE matrices (ms_deep_rows): a whole first FRI layer or a row shard
    GpuVec<Fp252> into_deep_evaluations(const DeepCompositionCoeffs252& coeffs, const Matrix<Fp252>& base_lde, const Matrix<Fp252>& comp_lde,
                                        size_t domain_size = 0, size_t first = 0, const f252::E* offset = nullptr) {
        const size_t count = base_lde.num_rows();
        if (comp_lde.num_rows() != count) throw std::invalid_argument("into_deep_evaluations: LDE matrices of different heights");
        if (!domain_size) domain_size = count;
        unsigned log_N = 0; while (((size_t)1 << log_N) < domain_size) log_N++;
        return compose(coeffs, base_lde, comp_lde, count, [&](Planner& pl, const std::vector<const void*>& cols, const Terms& t, void* out) {
            return ms_deep_rows(pl.ctx(), Fp252::id, log_N, offset ? offset->l : nullptr, first, count, cols.data(), (unsigned)cols.size(), nullptr, 0, t.pts.data(), t.npoints,
                                t.tcol.data(), t.tpoint.data(), t.al.data(), t.od.data(), (unsigned)t.tcol.size(), t.da.data(), t.db.data(), out); });
    }
private:
    struct Terms { std::vector<unsigned> tcol, tpoint; std::vector<uint64_t> pts, al, od, da, db; unsigned npoints = 0; };
    template <class Call>
    GpuVec<Fp252> compose(const DeepCompositionCoeffs252& coeffs, const Matrix<Fp252>& b, const Matrix<Fp252>& c, size_t out_len, Call call) {
        if (!have_ood_) get_ood_evals();
        std::vector<const void*> cols;
        for (auto& v : b.columns) cols.push_back(v.ptr());
        for (auto& v : c.columns) cols.push_back(v.ptr());
        std::vector<f252::E> points;
        auto pid = [&](const f252::E& p) { for (size_t k = 0; k < points.size(); k++) if (f252::eq(points[k], p)) return (unsigned)k; points.push_back(p); return (unsigned)points.size() - 1; };
        Terms t;
        auto put = [](std::vector<uint64_t>& o, const f252::E& e) { o.insert(o.end(), e.l, e.l + 4); };
        for (unsigned k = 0; k < comp_.num_cols(); k++) { t.tcol.push_back(nbase_ + k); t.tpoint.push_back(pid(composition_point())); put(t.al, coeffs.composition_trace.at(k)); put(t.od, ood_comp_[k]); }
        for (size_t k = 0; k < args_.size(); k++) { t.tcol.push_back(args_[k].first); t.tpoint.push_back(pid(point(args_[k].second))); put(t.al, coeffs.execution_trace.at(k)); put(t.od, ood_exec_[k]); }
        for (auto& p : points) put(t.pts, p);
        put(t.da, coeffs.degree[0]); put(t.db, coeffs.degree[1]);
        t.npoints = (unsigned)points.size();
        Planner& pl = b.planner();
        GpuVec<Fp252> out(pl, out_len);
        check(call(pl, cols, t, out.ptr()));
        return out;
    }
    std::vector<std::pair<unsigned, int>> args_;
    size_t n_; f252::E z_; const Matrix<Fp252>& base_; const Matrix<Fp252>& comp_;
    f252::E g_, g_inv_; unsigned nbase_ = 0;
    std::vector<f252::E> ood_exec_, ood_comp_; bool have_ood_ = false;
};

// ---- RPO-256 front-ends (gpu/src/plan.rs:32-174); digests are 4 Fp elements, Montgomery form
class GpuRpo256ColumnMajor {                      // ::new(n, requires_padding); update(col) per column; finish()
public:
    GpuRpo256ColumnMajor(Planner& pl, size_t n) : pl_(&pl), n_(n) {}
    void update(const GpuVec<Fp>& col) { if (col.len() != n_) throw std::invalid_argument("column length differs from n"); cols_.push_back(col.ptr()); }
    GpuVec<Fp> finish() {
        GpuVec<Fp> digests(*pl_, n_ * 4);
        check(ms_rpo256_rows(pl_->ctx(), n_, cols_.data(), (unsigned)cols_.size(), digests.ptr()));
        pl_->sync();
        return digests;
    }
private:
    Planner* pl_; size_t n_; std::vector<const void*> cols_;
};
inline GpuVec<Fp> rpo256_rows_row_major(const GpuVec<Fp>& rows, unsigned ncols = 8) {      // GpuRpo256RowMajor: update(rows) + finish()
    GpuVec<Fp> digests(rows.planner(), rows.len() / ncols * 4);
    check(ms_rpo256_rows_row_major(rows.planner().ctx(), rows.len() / ncols, ncols, rows.ptr(), digests.ptr()));
    return digests;
}
inline GpuVec<Fp> gen_rpo_merkle_tree(const GpuVec<Fp>& leaves) {                          // nodes, [n][4] Fp
    GpuVec<Fp> nodes(leaves.planner(), leaves.len());
    check(ms_rpo256_merkle(leaves.planner().ctx(), leaves.len() / 4, leaves.ptr(), nodes.ptr()));
    return nodes;
}

}  // namespace ms
