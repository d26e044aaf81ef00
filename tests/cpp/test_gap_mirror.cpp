// The C++ host mirror of the padded-table layer (ms::gap_plan, ms::gap_fill, prover.hpp) over Fp and Fp252 against values the Python
// references dumped: tests/test_gap_mirror.py writes, per field, the processor table (Montgomery words: cycle, mp, mem_val, instr), and the
// start, report and filled columns that tests/gaps_ref.py expects of the memory table; the program sorts the rows whose instr is not zero by
// (mp, cycle), plans through that order, fills, and compares every word.
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

static bool read_u64(FILE* f, unsigned long long* v) { return fscanf(f, "%llu", v) == 1; }

template <class B>
static int run(FILE* f, const char* tag) {
    ms::Planner& pl = ms::get_planner();
    unsigned long long n = 0, nbase = 0, ncols = 0, n_out = 0, v = 0;
    if (!read_u64(f, &n) || !read_u64(f, &nbase) || !read_u64(f, &ncols) || !read_u64(f, &n_out)) { printf("FAILED: %s: header\n", tag); return 1; }
    ms::Matrix<B> base;
    for (unsigned c = 0; c < nbase; c++) {
        std::vector<uint64_t> w(n * B::words);
        for (auto& x : w) { if (!read_u64(f, &v)) { printf("FAILED: %s: base\n", tag); return 1; } x = v; }
        base.columns.emplace_back(pl, w);
    }
    std::vector<uint64_t> want_start(n + 1);
    for (auto& x : want_start) { if (!read_u64(f, &v)) { printf("FAILED: %s: start\n", tag); return 1; } x = v; }
    unsigned long long rep[8];
    for (auto& x : rep) if (!read_u64(f, &x)) { printf("FAILED: %s: report\n", tag); return 1; }
    std::vector<ms_gap_column> columns(ncols);
    for (auto& c : columns) {
        unsigned long long kind = 0, src = 0;
        if (!read_u64(f, &kind) || !read_u64(f, &src)) { printf("FAILED: %s: columns\n", tag); return 1; }
        c.kind = (int32_t)kind; c.src = (int32_t)src;
    }
    std::vector<std::vector<uint64_t>> want(ncols, std::vector<uint64_t>(n_out * B::words));
    for (auto& col : want) for (auto& x : col) { if (!read_u64(f, &v)) { printf("FAILED: %s: expected columns\n", tag); return 1; } x = v; }

    ms::SortKey key;
    key.cols = {1, 0}; key.mask = MS_EXT_IF_NONZERO; key.mask_col = 3;
    const ms::RowOrder order = ms::sort_rows<B>(base, key);
    ms::GapSpec spec;
    spec.group = {1}; spec.counter = 0; spec.mask = MS_EXT_IF_NONZERO; spec.mask_col = 3;
    const ms::GapPlan plan = ms::gap_plan<B>(base, spec, &order);
    if (plan.to_host() != want_start) { printf("FAILED: %s: start differs\n", tag); return 1; }
    const ms_gap_report r = plan.read();
    const unsigned long long got[8] = {r.active, r.rows_out, r.gaps, r.max_gap, r.unordered, r.first_unordered, r.saturated, r.pad0};
    for (int k = 0; k < 8; k++) if (got[k] != rep[k]) { printf("FAILED: %s: report word %d: %llu for %llu\n", tag, k, got[k], rep[k]); return 1; }
    const ms::Matrix<B> table = ms::gap_fill<B>(base, plan, columns, n_out);
    for (unsigned c = 0; c < ncols; c++)
        if (table.columns[c].to_host() != want[c]) { printf("FAILED: %s: filled column %u\n", tag, c); return 1; }
    // the default length: the least power of two that holds the table
    const ms::Matrix<B> sized = ms::gap_fill<B>(base, plan, columns);
    size_t pow2 = 1;
    while (pow2 < r.rows_out) pow2 *= 2;
    if (sized.num_rows() != pow2) { printf("FAILED: %s: default length %zu for %zu\n", tag, sized.num_rows(), pow2); return 1; }
    const std::vector<uint64_t> head = sized.columns[0].to_host();
    for (size_t i = 0; i < std::min<size_t>(pow2, n_out) * B::words; i++) if (head[i] != want[0][i]) { printf("FAILED: %s: default length, word %zu\n", tag, i); return 1; }
    // without an order: the identity
    const ms::GapPlan plain = ms::gap_plan<B>(base, ms::GapSpec{});
    if (plain.read().rows_out != n || plain.to_host()[n] != n) { printf("FAILED: %s: a plan without mask and counter\n", tag); return 1; }
    // a refusal surfaces as the library's error: a counter column out of range
    bool refused = false;
    ms::GapSpec bad = spec;
    bad.counter = (int)nbase;
    try { ms::gap_plan<B>(base, bad, &order); } catch (const std::exception& e) { refused = std::string(e.what()).find("out of range") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a counter column out of range was accepted\n", tag); return 1; }
    printf("%s rows %llu active %llu rows_out %llu gaps %llu\n", tag, n, (unsigned long long)r.active, (unsigned long long)r.rows_out, (unsigned long long)r.gaps);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: test_gap_mirror <file the Python driver wrote>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAILED: cannot open %s\n", argv[1]); return 1; }
    int rc = run<ms::Fp>(f, "fp");
    if (rc == 0) rc = run<ms::Fp252>(f, "fp252");
    fclose(f);
    if (rc == 0) printf("gap host mirror ok\n");
    return rc;
}
