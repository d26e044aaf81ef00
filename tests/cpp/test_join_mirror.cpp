// The C++ host mirror of the row join (ms::join_rows, ms::fetch_columns, prover.hpp) over Fp and Fp252 against values the Python reference
// dumped: tests/test_join_mirror.py writes, per field, the table's and the base's columns (Montgomery words), the keys, and the match
// arrays, the report and the fetched payload column that tests/join_ref.py expects; the program runs the calls and compares.
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
static bool read_matrix(FILE* f, ms::Planner& pl, size_t rows, unsigned ncols, ms::Matrix<B>* m) {
    unsigned long long v = 0;
    for (unsigned c = 0; c < ncols; c++) {
        std::vector<uint64_t> w(rows * B::words);
        for (auto& x : w) { if (!read_u64(f, &v)) return false; x = v; }
        m->columns.emplace_back(pl, w);
    }
    return true;
}

template <class B>
static int run(FILE* f, const char* tag) {
    ms::Planner& pl = ms::get_planner();
    unsigned long long n_table = 0, ntc = 0, n = 0, nbase = 0, width = 0, nsets = 0, payload = 0, v = 0;
    if (!read_u64(f, &n_table) || !read_u64(f, &ntc) || !read_u64(f, &n) || !read_u64(f, &nbase) || !read_u64(f, &width) || !read_u64(f, &nsets) || !read_u64(f, &payload)) {
        printf("FAILED: %s: header\n", tag); return 1;
    }
    ms::LookupTuple table_key;
    std::vector<ms::LookupTuple> keys(nsets);
    if (!read_tuple(f, (unsigned)width, &table_key)) { printf("FAILED: %s: table key\n", tag); return 1; }
    for (auto& t : keys) if (!read_tuple(f, (unsigned)width, &t)) { printf("FAILED: %s: keys\n", tag); return 1; }
    ms::Matrix<B> table, base;
    if (!read_matrix<B>(f, pl, n_table, (unsigned)ntc, &table) || !read_matrix<B>(f, pl, n, (unsigned)nbase, &base)) { printf("FAILED: %s: columns\n", tag); return 1; }
    std::vector<std::vector<uint32_t>> want(nsets, std::vector<uint32_t>(n));
    for (auto& m : want) for (auto& x : m) { if (!read_u64(f, &v)) { printf("FAILED: %s: matches\n", tag); return 1; } x = (uint32_t)v; }
    unsigned long long rep[6];
    for (auto& x : rep) if (!read_u64(f, &x)) { printf("FAILED: %s: report\n", tag); return 1; }
    std::vector<uint64_t> fetched(n * B::words);
    for (auto& x : fetched) { if (!read_u64(f, &v)) { printf("FAILED: %s: fetched\n", tag); return 1; } x = v; }

    const ms::JoinReport report = ms::join_rows<B>(table, table_key, base, keys);
    const ms_join_report r = report.read();
    for (size_t s = 0; s < nsets; s++) if (report.matches[s].to_host() != want[s]) { printf("FAILED: %s: the matches of set %zu differ\n", tag, s); return 1; }
    if (r.matched != rep[0] || r.missing != rep[1] || r.first_missing_set != rep[2] || r.first_missing_row != rep[3] || r.duplicate_table_rows != rep[4] || r.table_active != rep[5]) {
        printf("FAILED: %s: report %llu %llu %u %llu %llu %llu\n", tag, (unsigned long long)r.matched, (unsigned long long)r.missing, r.first_missing_set,
               (unsigned long long)r.first_missing_row, (unsigned long long)r.duplicate_table_rows, (unsigned long long)r.table_active);
        return 1;
    }
    // the payload of set 0's matches, zero where there is none; the report of that one set comes with it
    const auto got = ms::fetch_columns<B>(table, table_key, base, keys[0], {(int)payload});
    const ms::JoinReport& one = got.second;
    if (got.first.columns.size() != 1 || got.first.columns[0].to_host() != fetched) { printf("FAILED: %s: the fetched column differs\n", tag); return 1; }
    if (one.matches.size() != 1 || one.matches[0].to_host() != want[0] || one.read().table_active != rep[5]) { printf("FAILED: %s: fetch_columns' report\n", tag); return 1; }
    // a refusal surfaces as the library's error: a key column out of the table's range
    bool refused = false;
    ms::LookupTuple bad = table_key;
    bad.cols[0] = (int)ntc;
    try { ms::join_rows<B>(table, bad, base, keys); } catch (const std::exception& e) { refused = std::string(e.what()).find("d_table") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a table key column out of range was accepted\n", tag); return 1; }
    printf("%s rows %llu table %llu matched %llu missing %llu duplicates %llu\n", tag, n, n_table, (unsigned long long)r.matched, (unsigned long long)r.missing,
           (unsigned long long)r.duplicate_table_rows);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: test_join_mirror <file the Python driver wrote>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAILED: cannot open %s\n", argv[1]); return 1; }
    int rc = run<ms::Fp>(f, "fp");
    if (rc == 0) rc = run<ms::Fp252>(f, "fp252");
    fclose(f);
    if (rc == 0) printf("join host mirror ok\n");
    return rc;
}
