// The C++ host mirror of the row sort (ms::sort_rows, ms::permute_columns, prover.hpp) over Fp and Fp252 against values the Python reference
// dumped: tests/test_sort_mirror.py writes, per field, the base columns (Montgomery words), the key, and the permutation and report that
// tests/sort_ref.py expects; the program sorts, compares, gathers every column through the permutation and compares those words too.
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

static bool read_u64(FILE* f, unsigned long long* v) { return fscanf(f, "%llu", v) == 1; }

template <class B>
static int run(FILE* f, const char* tag) {
    ms::Planner& pl = ms::get_planner();
    unsigned long long n = 0, nbase = 0, nkeys = 0, v = 0;
    if (!read_u64(f, &n) || !read_u64(f, &nbase) || !read_u64(f, &nkeys)) { printf("FAILED: %s: header\n", tag); return 1; }
    ms::SortKey key;
    for (unsigned c = 0; c < nkeys; c++) { if (!read_u64(f, &v)) { printf("FAILED: %s: key\n", tag); return 1; } key.cols.push_back((int)v); }
    if (!read_u64(f, &v)) { printf("FAILED: %s: key\n", tag); return 1; }
    key.mask = (int)v;
    if (!read_u64(f, &v)) { printf("FAILED: %s: key\n", tag); return 1; }
    key.mask_col = (int)v;
    ms::Matrix<B> base;
    std::vector<std::vector<uint64_t>> host;
    for (unsigned c = 0; c < nbase; c++) {
        std::vector<uint64_t> w(n * B::words);
        for (auto& x : w) { if (!read_u64(f, &v)) { printf("FAILED: %s: base\n", tag); return 1; } x = v; }
        base.columns.emplace_back(pl, w);
        host.push_back(w);
    }
    std::vector<uint32_t> want(n);
    for (auto& x : want) { if (!read_u64(f, &v)) { printf("FAILED: %s: perm\n", tag); return 1; } x = (uint32_t)v; }
    unsigned long long rep[2];
    for (auto& x : rep) if (!read_u64(f, &x)) { printf("FAILED: %s: report\n", tag); return 1; }
    const ms::RowOrder order = ms::sort_rows<B>(base, key);
    const ms_sort_report r = order.read();
    if (order.to_host() != want) { printf("FAILED: %s: the permutation differs\n", tag); return 1; }
    if (r.active != rep[0] || r.varying_bytes != rep[1]) { printf("FAILED: %s: report %llu %llu\n", tag, (unsigned long long)r.active, (unsigned long long)r.varying_bytes); return 1; }
    const ms::Matrix<B> sorted = ms::permute_columns<B>(base, order);
    for (unsigned c = 0; c < nbase; c++) {
        const std::vector<uint64_t> got = sorted.columns[c].to_host();
        for (size_t i = 0; i < n; i++)
            for (unsigned l = 0; l < B::words; l++)
                if (got[i * B::words + l] != host[c][(size_t)want[i] * B::words + l]) { printf("FAILED: %s: permuted column %u, row %zu\n", tag, c, i); return 1; }
    }
    const ms::Matrix<B> head = ms::permute_columns<B>(base, order, 10);
    const std::vector<uint64_t> whole = sorted.columns[0].to_host();
    if (head.num_rows() != 10 || head.columns[0].to_host() != std::vector<uint64_t>(whole.begin(), whole.begin() + 10 * B::words)) {
        printf("FAILED: %s: a head of the index\n", tag); return 1;
    }
    // a refusal surfaces as the library's error: a key column out of range
    bool refused = false;
    ms::SortKey bad = key;
    bad.cols[0] = (int)nbase;
    try { ms::sort_rows<B>(base, bad); } catch (const std::exception& e) { refused = std::string(e.what()).find("out of range") != std::string::npos; }
    if (!refused) { printf("FAILED: %s: a key column out of range was accepted\n", tag); return 1; }
    printf("%s rows %llu active %llu varying %llu\n", tag, n, (unsigned long long)r.active, (unsigned long long)r.varying_bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: test_sort_mirror <file the Python driver wrote>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAILED: cannot open %s\n", argv[1]); return 1; }
    int rc = run<ms::Fp>(f, "fp");
    if (rc == 0) rc = run<ms::Fp252>(f, "fp252");
    fclose(f);
    if (rc == 0) printf("sort host mirror ok\n");
    return rc;
}
