// The C++ host mirror of the lookup multiplicities (ms::lookup_multiplicities, prover.hpp) over Fp and Fp252 against values the Python
// reference dumped: tests/test_lookup_mirror.py writes, per field, the base columns (Montgomery words), the tuples, and the m column and
// report that tests/lookup_ref.py expects; the program runs the call -- m in place, in the base matrix's last column -- and compares.
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

static bool read_u64(FILE* f, unsigned long long* v) { return fscanf(f, "%llu", v) == 1; }
static bool read_tuple(FILE* f, unsigned width, ms::LookupTuple* t) {
    unsigned long long v = 0;
    for (unsigned c = 0; c < width; c++) { if (!read_u64(f, &v)) return false; t->cols.push_back((int)v); }
    if (!read_u64(f, &v)) return false;
    t->mask = (int)v;
    if (!read_u64(f, &v)) return false;
    t->mask_col = (int)v;
    return true;
}

template <class B>
static int run(FILE* f, const char* tag) {
    ms::Planner& pl = ms::get_planner();
    unsigned long long n = 0, nbase = 0, width = 0, nsets = 0, v = 0;
    if (!read_u64(f, &n) || !read_u64(f, &nbase) || !read_u64(f, &width) || !read_u64(f, &nsets)) { printf("FAILED: %s: header\n", tag); return 1; }
    ms::LookupTuple table;
    std::vector<ms::LookupTuple> lookups(nsets);
    if (!read_tuple(f, (unsigned)width, &table)) { printf("FAILED: %s: table\n", tag); return 1; }
    for (auto& t : lookups) if (!read_tuple(f, (unsigned)width, &t)) { printf("FAILED: %s: lookups\n", tag); return 1; }
    ms::Matrix<B> base;
    for (unsigned c = 0; c < nbase; c++) {
        std::vector<uint64_t> w(n * B::words);
        for (auto& x : w) { if (!read_u64(f, &v)) { printf("FAILED: %s: base\n", tag); return 1; } x = v; }
        base.columns.emplace_back(pl, w);
    }
    std::vector<uint64_t> want(n * B::words);
    for (auto& x : want) { if (!read_u64(f, &v)) { printf("FAILED: %s: m\n", tag); return 1; } x = v; }
    unsigned long long rep[4];
    for (auto& x : rep) if (!read_u64(f, &x)) { printf("FAILED: %s: report\n", tag); return 1; }
    ms::GpuVec<B>& m = base.columns.back();
    const ms::LookupReport report = ms::lookup_multiplicities<B>(base, table, lookups, m);
    const ms_lookup_report r = report.read();
    if (m.to_host() != want) { printf("FAILED: %s: m differs\n", tag); return 1; }
    if (r.missing != rep[0] || r.first_missing_set != rep[1] || r.first_missing_row != rep[2] || r.duplicate_table_rows != rep[3]) {
        printf("FAILED: %s: report %llu %u %llu %llu\n", tag, (unsigned long long)r.missing, r.first_missing_set, (unsigned long long)r.first_missing_row,
               (unsigned long long)r.duplicate_table_rows);
        return 1;
    }
    // a refusal surfaces as the library's error: m over a column the table names
    bool refused = false;
    try { ms::lookup_multiplicities<B>(base, table, lookups, base.columns[table.cols[0]]); } catch (const std::exception& e) { refused = std::string(e.what()).find("overlap") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: an overlapping m was accepted\n", tag); return 1; }
    printf("%s rows %llu missing %llu duplicates %llu\n", tag, n, (unsigned long long)r.missing, (unsigned long long)r.duplicate_table_rows);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: test_lookup_mirror <file the Python driver wrote>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAILED: cannot open %s\n", argv[1]); return 1; }
    int rc = run<ms::Fp>(f, "fp");
    if (rc == 0) rc = run<ms::Fp252>(f, "fp252");
    fclose(f);
    if (rc == 0) printf("lookup host mirror ok\n");
    return rc;
}
