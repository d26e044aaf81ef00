// The C++ host mirror of the range check (ms::limb_decompose, ms::range_multiplicities, prover.hpp) over Fp and Fp252 against values the
// Python reference dumped: tests/test_range_mirror.py writes, per field, the trace's columns (Montgomery words), the specs and sets, and
// the columns, the m column and the two reports that tests/range_ref.py expects; the program runs the calls and compares.
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

static bool read_u64(FILE* f, unsigned long long* v) { return fscanf(f, "%llu", v) == 1; }
static bool read_ints(FILE* f, int* out, unsigned count) {
    unsigned long long v = 0;
    for (unsigned k = 0; k < count; k++) { if (!read_u64(f, &v)) return false; out[k] = (int)v; }
    return true;
}
static bool read_words(FILE* f, std::vector<uint64_t>* w) {
    unsigned long long v = 0;
    for (auto& x : *w) { if (!read_u64(f, &v)) return false; x = v; }
    return true;
}

template <class B>
static int run(FILE* f, const char* tag) {
    ms::Planner& pl = ms::get_planner();
    unsigned long long n = 0, nbase = 0, nspecs = 0, bits = 0, nsets = 0, n_m = 0;
    if (!read_u64(f, &n) || !read_u64(f, &nbase) || !read_u64(f, &nspecs) || !read_u64(f, &bits) || !read_u64(f, &nsets) || !read_u64(f, &n_m)) {
        printf("FAILED: %s: header\n", tag); return 1;
    }
    std::vector<ms::LimbSpec> specs(nspecs);
    for (auto& sp : specs) {
        int w[6];
        if (!read_ints(f, w, 6)) { printf("FAILED: %s: specs\n", tag); return 1; }
        sp.src = w[0]; sp.dst0 = w[1]; sp.nlimbs = w[2]; sp.bits = w[3]; sp.mask = w[4]; sp.mask_col = w[5];
    }
    std::vector<ms::RangeSet> sets(nsets);
    for (auto& st : sets) {
        int w[3];
        if (!read_ints(f, w, 3)) { printf("FAILED: %s: sets\n", tag); return 1; }
        st.col = w[0]; st.mask = w[1]; st.mask_col = w[2];
    }
    ms::Matrix<B> trace;
    std::vector<std::vector<uint64_t>> want(nbase, std::vector<uint64_t>(n * B::words));
    for (unsigned c = 0; c < nbase; c++) {
        std::vector<uint64_t> w(n * B::words);
        if (!read_words(f, &w)) { printf("FAILED: %s: columns\n", tag); return 1; }
        trace.columns.emplace_back(pl, w);
    }
    for (auto& w : want) if (!read_words(f, &w)) { printf("FAILED: %s: expected columns\n", tag); return 1; }
    unsigned long long lrep[4], rrep[3];
    for (auto& x : lrep) if (!read_u64(f, &x)) { printf("FAILED: %s: limb report\n", tag); return 1; }
    std::vector<uint64_t> want_m(n_m * B::words);
    if (!read_words(f, &want_m)) { printf("FAILED: %s: expected m\n", tag); return 1; }
    for (auto& x : rrep) if (!read_u64(f, &x)) { printf("FAILED: %s: range report\n", tag); return 1; }

    const ms::LimbReport limbs = ms::limb_decompose<B>(trace, specs);
    const ms_limb_report lr = limbs.read();
    for (unsigned c = 0; c < nbase; c++) if (trace.columns[c].to_host() != want[c]) { printf("FAILED: %s: column %u differs\n", tag, c); return 1; }
    if (lr.overflow != lrep[0] || lr.first_overflow_spec != lrep[1] || lr.first_overflow_row != lrep[2] || lr.active != lrep[3]) {
        printf("FAILED: %s: limb report %llu %u %llu %llu\n", tag, (unsigned long long)lr.overflow, lr.first_overflow_spec, (unsigned long long)lr.first_overflow_row,
               (unsigned long long)lr.active);
        return 1;
    }
    ms::GpuVec<B> m(pl, n_m);
    const ms::RangeReport counts = ms::range_multiplicities<B>(trace, (unsigned)bits, sets, m);
    const ms_lookup_report rr = counts.read();
    if (m.to_host() != want_m) { printf("FAILED: %s: m differs\n", tag); return 1; }
    if (rr.missing != rrep[0] || rr.first_missing_set != rrep[1] || rr.first_missing_row != rrep[2] || rr.duplicate_table_rows != 0) {
        printf("FAILED: %s: range report %llu %u %llu\n", tag, (unsigned long long)rr.missing, rr.first_missing_set, (unsigned long long)rr.first_missing_row);
        return 1;
    }
    // refusals surface as the library's errors, or before the call: a destination on its source, a set out of range, an m shorter than the table
    bool refused = false;
    std::vector<ms::LimbSpec> bad = specs;
    bad[0].dst0 = bad[0].src;
    try { ms::limb_decompose<B>(trace, bad); } catch (const std::exception& e) { refused = std::string(e.what()).find("overlap") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a destination on its source was accepted\n", tag); return 1; }
    refused = false;
    std::vector<ms::RangeSet> stray = sets;
    stray[0].col = (int)nbase;
    try { ms::range_multiplicities<B>(trace, (unsigned)bits, stray, m); } catch (const std::exception& e) { refused = std::string(e.what()).find("out of range") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a set column out of range was accepted\n", tag); return 1; }
    refused = false;
    ms::GpuVec<B> too_short(pl, ((size_t)1 << bits) - 1);
    try { ms::range_multiplicities<B>(trace, (unsigned)bits, sets, too_short); } catch (const std::invalid_argument&) { refused = true; }
    if (!refused) { printf("FAILED: %s: an m shorter than the table was accepted\n", tag); return 1; }
    printf("%s rows %llu active %llu overflow %llu missing %llu\n", tag, n, (unsigned long long)lr.active, (unsigned long long)lr.overflow, (unsigned long long)rr.missing);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: test_range_mirror <file the Python driver wrote>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAILED: cannot open %s\n", argv[1]); return 1; }
    int rc = run<ms::Fp>(f, "fp");
    if (rc == 0) rc = run<ms::Fp252>(f, "fp252");
    fclose(f);
    if (rc == 0) printf("range host mirror ok\n");
    return rc;
}
