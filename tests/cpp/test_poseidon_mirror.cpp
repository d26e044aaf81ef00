// The C++ host mirror of the Poseidon commitments (Hash::Poseidon252 in ministark.hpp) and of ms::poseidon252_permute against expected
// values dumped by tests/test_poseidon_mirror.py from tests/poseidon_ref.py.  The data file holds, in Montgomery words:
//   nrows ncols                 then ncols lines of 4 nrows words (the columns), then one line of 4 nrows words: every node of the tree
//   nlayer ff                   then one line of 4 nlayer words (a FRI layer), then one line of 4 (nlayer / ff) words: every node
//   nstates                     then one line of 12 nstates words (the states), then one line of 12 nstates words: their permutations
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"

using namespace ms;

static std::vector<uint64_t> line(std::ifstream& f, size_t n) {
    std::vector<uint64_t> v(n);
    for (auto& w : v) f >> w;
    return v;
}
static int fails = 0;
static void expect(bool ok, const char* what) { if (!ok) { printf("FAIL %s\n", what); fails++; } }

// leaves_ / nodes_ are private: the root and an opening of every leaf are what the mirror shows of a tree
static void check_tree(const MerkleTree& t, const std::vector<uint64_t>& nodes, const std::vector<uint64_t>& leaves, const char* what) {
    const size_t n = t.num_leaves();
    expect(nodes.size() == 4 * n && leaves.size() == 4 * n, what);
    expect(memcmp(t.root().data(), nodes.data() + 4, 32) == 0, what);
    std::vector<size_t> all(n);
    for (size_t i = 0; i < n; i++) all[i] = i;
    const auto view = t.prove(all);                                          // every leaf, no sibling, no node
    expect(view.initial_leaves.size() == n && view.sibling_leaves.empty() && view.nodes.empty(), what);
    for (size_t i = 0; i < n && i < view.initial_leaves.size(); i++) expect(memcmp(view.initial_leaves[i].data(), leaves.data() + 4 * i, 32) == 0, what);
    const auto one = t.prove({n - 1});                                       // one leaf: its sibling and one node per level above
    expect(one.sibling_leaves.size() == 1 && memcmp(one.sibling_leaves[0].data(), leaves.data() + 4 * (n - 2), 32) == 0, what);
    size_t k = (2 * n - 1) >> 1;
    for (const auto& d : one.nodes) { expect(memcmp(d.data(), nodes.data() + 4 * (k ^ 1), 32) == 0, what); k >>= 1; }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    Planner& pl = get_planner();
    size_t nrows, ncols;
    f >> nrows >> ncols;
    Matrix<Fp252> m;
    for (size_t c = 0; c < ncols; c++) m.columns.emplace_back(pl, line(f, 4 * nrows));
    const auto leaves = line(f, 4 * nrows), nodes = line(f, 4 * nrows);
    check_tree(MerkleTree::from_matrix(m, Hash::Poseidon252), nodes, leaves, "from_matrix");
    printf("matrix rows %zu cols %zu\n", nrows, ncols);

    size_t nlayer, ff;
    f >> nlayer >> ff;
    GpuVec<Fp252> layer(pl, line(f, 4 * nlayer));
    const auto lleaves = line(f, 4 * (nlayer / ff)), lnodes = line(f, 4 * (nlayer / ff));
    check_tree(MerkleTree::from_fri_layer(layer, (unsigned)ff, Hash::Poseidon252), lnodes, lleaves, "from_fri_layer");
    printf("layer %zu folding %zu\n", nlayer, ff);

    size_t nstates;
    f >> nstates;
    GpuVec<Fp252> states(pl, line(f, 12 * nstates));
    const auto want = line(f, 12 * nstates);
    expect(poseidon252_permute(states).to_host() == want, "poseidon252_permute");
    printf("states %zu\n", nstates);

    // a Goldilocks matrix is refused with a clear error, before the library is called
    bool refused = false;
    try {
        Matrix<Fp> g;
        g.columns.emplace_back(pl, std::vector<uint64_t>(8, 1));
        MerkleTree::from_matrix(g, Hash::Poseidon252);
    } catch (const std::invalid_argument& e) { refused = strstr(e.what(), "252-bit field") != nullptr; }
    expect(refused, "Goldilocks matrix refused");
    if (!f) { printf("FAIL short data file\n"); fails++; }
    if (fails) return 1;
    printf("poseidon host mirror ok\n");
    return 0;
}
