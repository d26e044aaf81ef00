// The C++ host mirror of the RPO-256 public coin: three FRI layers committed with RPO-256, absorbed, challenged and folded through
// ms::RpoCoin, MerkleTree::root_ptr and the apply_drp overload that takes alpha from device memory.  Prints every root and alpha, the
// remainder, the coin's state, the nonce and the positions for tests/test_rpo_coin_cpp_mirror.py to replay with tests/rpo_coin_ref.py,
// and checks here that each fold equals the host-alpha fold of the downloaded challenge.
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
    ms::RpoCoin coin(pl, {{5, 6, 7, ms::gl::P - 1}});
    const unsigned ff = 4;
    std::vector<uint64_t> words((size_t)1 << 9);
    uint64_t s = 42;
    for (auto& w : words) { s = s * 6364136223846793005ull + 1442695040888963407ull; w = (s >> 1) % ms::gl::P; }
    ms::GpuVec<ms::Fp> cur(pl, words);
    for (int layer = 0; layer < 3; layer++) {
        const ms::MerkleTree tree = ms::MerkleTree::from_fri_layer(cur, ff, ms::Hash::Rpo256);
        coin.reseed_digest(tree.root_ptr());
        const ms::GpuVec<ms::Fp> alpha = coin.draw<ms::Fp>();
        ms::GpuVec<ms::Fp> next = ms::apply_drp<ms::Fp>(cur, alpha, ff, 7);
        // nothing above waited for the device; now look
        const auto root = tree.root();
        const auto a = alpha.to_host();
        print_words("root", (const uint64_t*)root.data(), 4);
        print_words("alpha", a.data(), 1);
        REQUIRE(next.to_host() == ms::apply_drp<ms::Fp>(cur, a, ff, 7).to_host());
        cur = std::move(next);
    }
    coin.reseed_elements(cur);
    const ms_rpo_coin_state st = coin.state();
    REQUIRE(st.pos == 4);
    for (int q = 0; q < 7; q++) REQUIRE(st.pad[q] == 0);
    print_words("remainder", cur.to_host().data(), cur.len());
    print_words("state", st.s, 12);
    const uint64_t nonce = coin.grind(8);
    coin.reseed_int(nonce);
    printf("nonce %llu\n", (unsigned long long)nonce);
    const ms::GpuVec<ms::Fq3> e = coin.draw<ms::Fq3>(2);
    print_words("fq3", e.to_host().data(), 6);
    for (size_t p : coin.draw_queries(8, (size_t)1 << 9)) printf("position %zu\n", p);
    printf("rpo coin host mirror ok\n");
    return 0;
}
