// The C++ host mirror of the bitwise-operation columns (ms::bitwise_columns, ms::bitwise_table, ms::bitwise_multiplicities, prover.hpp) over
// Fp and Fp252 against values the Python reference dumped: tests/test_bitwise_mirror.py writes, per field, the trace's columns (Montgomery
// words), the specs, ops and sets, and the columns, the table, the m column and the two reports that tests/bitwise_ref.py expects; the
// program runs the calls and compares.
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

static bool read_u64(FILE* f, unsigned long long* v) { return fscanf(f, "%llu", v) == 1; }
static bool read_ints(FILE* f, int* out, unsigned count) {
    long long v = 0;
    for (unsigned k = 0; k < count; k++) { if (fscanf(f, "%lld", &v) != 1) return false; out[k] = (int)v; }
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
    unsigned long long n = 0, nbase = 0, nspecs = 0, bits = 0, nops = 0, nsets = 0, n_m = 0;
    if (!read_u64(f, &n) || !read_u64(f, &nbase) || !read_u64(f, &nspecs) || !read_u64(f, &bits) || !read_u64(f, &nops) || !read_u64(f, &nsets) || !read_u64(f, &n_m)) {
        printf("FAILED: %s: header\n", tag); return 1;
    }
    std::vector<ms::BitwiseSpec> specs(nspecs);
    for (auto& sp : specs) {
        int w[7];
        if (!read_ints(f, w, 7)) { printf("FAILED: %s: specs\n", tag); return 1; }
        sp.op = w[0]; sp.a = w[1]; sp.b = w[2]; sp.dst = w[3]; sp.width = w[4]; sp.mask = w[5]; sp.mask_col = w[6];
    }
    std::vector<int> ops(nops);
    if (!read_ints(f, ops.data(), (unsigned)nops)) { printf("FAILED: %s: ops\n", tag); return 1; }
    std::vector<ms::BitwiseSet> sets(nsets);
    for (auto& st : sets) {
        int w[7];
        if (!read_ints(f, w, 7)) { printf("FAILED: %s: sets\n", tag); return 1; }
        st.op = w[0]; st.a = w[1]; st.b = w[2]; st.c = w[3]; st.nlimbs = w[4]; st.mask = w[5]; st.mask_col = w[6];
    }
    ms::Matrix<B> trace;
    std::vector<std::vector<uint64_t>> want(nbase, std::vector<uint64_t>(n * B::words));
    for (unsigned c = 0; c < nbase; c++) {
        std::vector<uint64_t> w(n * B::words);
        if (!read_words(f, &w)) { printf("FAILED: %s: columns\n", tag); return 1; }
        trace.columns.emplace_back(pl, w);
    }
    for (auto& w : want) if (!read_words(f, &w)) { printf("FAILED: %s: expected columns\n", tag); return 1; }
    unsigned long long crep[4], mrep[3];
    for (auto& x : crep) if (!read_u64(f, &x)) { printf("FAILED: %s: column report\n", tag); return 1; }
    std::vector<std::vector<uint64_t>> want_t(4, std::vector<uint64_t>(n_m * B::words));
    for (auto& w : want_t) if (!read_words(f, &w)) { printf("FAILED: %s: expected table\n", tag); return 1; }
    std::vector<uint64_t> want_m(n_m * B::words);
    if (!read_words(f, &want_m)) { printf("FAILED: %s: expected m\n", tag); return 1; }
    for (auto& x : mrep) if (!read_u64(f, &x)) { printf("FAILED: %s: count report\n", tag); return 1; }

    const ms::LimbReport cols = ms::bitwise_columns<B>(trace, specs);
    const ms_limb_report cr = cols.read();
    for (unsigned c = 0; c < nbase; c++) if (trace.columns[c].to_host() != want[c]) { printf("FAILED: %s: column %u differs\n", tag, c); return 1; }
    if (cr.overflow != crep[0] || cr.first_overflow_spec != crep[1] || cr.first_overflow_row != crep[2] || cr.active != crep[3]) {
        printf("FAILED: %s: column report %llu %u %llu %llu\n", tag, (unsigned long long)cr.overflow, cr.first_overflow_spec, (unsigned long long)cr.first_overflow_row,
               (unsigned long long)cr.active);
        return 1;
    }
    ms::GpuVec<B> top(pl, n_m), tx(pl, n_m), ty(pl, n_m), tz(pl, n_m);
    ms::bitwise_table<B>((unsigned)bits, ops, &top, tx, ty, tz);
    if (top.to_host() != want_t[0] || tx.to_host() != want_t[1] || ty.to_host() != want_t[2] || tz.to_host() != want_t[3]) { printf("FAILED: %s: the table differs\n", tag); return 1; }
    ms::GpuVec<B> tz2(pl, n_m);
    ms::bitwise_table<B>((unsigned)bits, ops, nullptr, tx, ty, tz2);                 // no op column
    if (tz2.to_host() != want_t[3]) { printf("FAILED: %s: the table without its op column differs\n", tag); return 1; }
    ms::GpuVec<B> m(pl, n_m);
    const ms::BitwiseReport counts = ms::bitwise_multiplicities<B>(trace, (unsigned)bits, ops, sets, m);
    const ms_lookup_report mr = counts.read();
    if (m.to_host() != want_m) { printf("FAILED: %s: m differs\n", tag); return 1; }
    if (mr.missing != mrep[0] || mr.first_missing_set != mrep[1] || mr.first_missing_row != mrep[2] || mr.duplicate_table_rows != 0) {
        printf("FAILED: %s: count report %llu %u %llu\n", tag, (unsigned long long)mr.missing, mr.first_missing_set, (unsigned long long)mr.first_missing_row);
        return 1;
    }
    // refusals surface as the library's errors, or before the call: a destination on an operand, a set column out of range, an op the table
    // does not have, an m shorter than the table
    bool refused = false;
    std::vector<ms::BitwiseSpec> bad = specs;
    bad[0].dst = bad[0].a;
    try { ms::bitwise_columns<B>(trace, bad); } catch (const std::exception& e) { refused = std::string(e.what()).find("overlap") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a destination on its operand was accepted\n", tag); return 1; }
    refused = false;
    std::vector<ms::BitwiseSet> stray = sets;
    stray[0].b = (int)nbase;
    try { ms::bitwise_multiplicities<B>(trace, (unsigned)bits, ops, stray, m); } catch (const std::exception& e) { refused = std::string(e.what()).find("out of range") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a set column out of range was accepted\n", tag); return 1; }
    refused = false;
    try { ms::bitwise_multiplicities<B>(trace, (unsigned)bits, std::vector<int>{sets[0].op == MS_BIT_OR ? MS_BIT_AND : MS_BIT_OR}, sets, m); }
    catch (const std::exception& e) { refused = std::string(e.what()).find("not one of the table's ops") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a set whose op the table does not have was accepted\n", tag); return 1; }
    refused = false;
    ms::GpuVec<B> too_short(pl, (nops << (2 * bits)) - 1);
    try { ms::bitwise_multiplicities<B>(trace, (unsigned)bits, ops, sets, too_short); } catch (const std::invalid_argument&) { refused = true; }
    if (!refused) { printf("FAILED: %s: an m shorter than the table was accepted\n", tag); return 1; }
    printf("%s rows %llu active %llu overflow %llu missing %llu\n", tag, n, (unsigned long long)cr.active, (unsigned long long)cr.overflow, (unsigned long long)mr.missing);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: test_bitwise_mirror <file the Python driver wrote>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAILED: cannot open %s\n", argv[1]); return 1; }
    int rc = run<ms::Fp>(f, "fp");
    if (rc == 0) rc = run<ms::Fp252>(f, "fp252");
    fclose(f);
    if (rc == 0) printf("bitwise host mirror ok\n");
    return rc;
}
