// The C++ host mirror of the Poseidon public coin of the 252-bit field: three FRI layers committed with Hash::Poseidon252, absorbed,
// challenged and folded through ms::PoseidonCoin, MerkleTree::root_ptr and the apply_drp overload that takes alpha from device memory.
// Prints every root and alpha, the remainder, the coin's state, the nonce, three draws and the positions for
// tests/test_hades_coin_cpp_mirror.py to replay with tests/hades_coin_ref.py, and checks here that each fold equals the host-alpha
// fold of the downloaded challenge.  All printed elements are Montgomery words.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

#define REQUIRE(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static void print_words(const char* tag, const uint64_t* p, size_t n) {
    printf("%s", tag);
    for (size_t i = 0; i < n; i++) printf(" %llu", (unsigned long long)p[i]);
    printf("\n");
}

int main() {
    ms::Planner& pl = ms::get_planner();
    bool refused = false;
    try { ms::PoseidonCoin bad(pl, {{1, 0, 0, 0x0800000000000011ull}}); } catch (const std::invalid_argument&) { refused = true; }   // the seed p
    REQUIRE(refused);
    ms::PoseidonCoin coin(pl, {{5, 6, 7, 8}});
    const unsigned ff = 4;
    const size_t n = (size_t)1 << 8;
    std::vector<uint64_t> words(4 * n);
    uint64_t s = 42;
    for (size_t i = 0; i < n; i++) {                                          // canonical Montgomery words: the top word below 2^59
        for (int q = 0; q < 4; q++) { s = s * 6364136223846793005ull + 1442695040888963407ull; words[4 * i + q] = q == 3 ? s >> 6 : s; }
    }
    ms::GpuVec<ms::Fp252> cur(pl, words);
    for (int layer = 0; layer < 3; layer++) {
        const ms::MerkleTree tree = ms::MerkleTree::from_fri_layer(cur, ff, ms::Hash::Poseidon252);
        coin.reseed_digest(tree.root_ptr());
        const ms::GpuVec<ms::Fp252> alpha = coin.draw<ms::Fp252>();
        ms::GpuVec<ms::Fp252> next = ms::apply_drp<ms::Fp252>(cur, alpha, ff, 3);
        // nothing above waited for the device; now look
        const auto root = tree.root();
        const auto a = alpha.to_host();
        print_words("root", (const uint64_t*)root.data(), 4);
        print_words("alpha", a.data(), 4);
        REQUIRE(next.to_host() == ms::apply_drp<ms::Fp252>(cur, a, ff, 3).to_host());
        cur = std::move(next);
    }
    coin.reseed_elements(cur);
    const ms_hades_coin_state st = coin.state();
    REQUIRE(st.n_draws == 0);
    for (int q = 0; q < 4; q++) REQUIRE(st.pad[q] == 0);
    print_words("remainder", cur.to_host().data(), 4 * cur.len());
    print_words("state", st.digest, 4);
    const uint64_t nonce = coin.grind(8);
    coin.reseed_int(nonce);
    printf("nonce %llu\n", (unsigned long long)nonce);
    const ms::GpuVec<ms::Fp252> e = coin.draw<ms::Fp252>(3);
    print_words("draws", e.to_host().data(), 12);
    REQUIRE(coin.state().n_draws == 3);
    for (size_t p : coin.draw_queries(8, n)) printf("position %zu\n", p);
    bool unsupported = false;
    try { coin.draw<ms::Fp>(1); } catch (const std::exception&) { unsupported = true; }                 // Goldilocks draws from RpoCoin
    REQUIRE(unsupported);
    printf("hades coin host mirror ok\n");
    return 0;
}
