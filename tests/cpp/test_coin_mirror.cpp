// The C++ host mirror of the device-resident public coin: three FRI layers committed, absorbed, challenged and folded through
// ms::PublicCoin, MerkleTree::root_ptr and the apply_drp overload that takes alpha from device memory.  Prints every root and alpha
// (and the coin's final seed) for tests/test_coin_cpp_mirror.py to replay with tests/coin_ref.py, and checks here that each fold
// equals the host-alpha fold of the downloaded challenge.   usage: test_coin_mirror sha256|blake2s
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

#define REQUIRE(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static void print_hex(const char* tag, const uint8_t* p, size_t n) {
    printf("%s ", tag);
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    const ms::Hash h = argc > 1 && !strcmp(argv[1], "blake2s") ? ms::Hash::Blake2s : ms::Hash::Sha256;
    ms::Planner& pl = ms::get_planner();
    std::array<uint8_t, 32> seed;
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 1);
    ms::PublicCoin coin(pl, seed, h);
    const unsigned ff = 4;
    std::vector<uint64_t> words((size_t)1 << 9);
    uint64_t s = 42;
    for (auto& w : words) { s = s * 6364136223846793005ull + 1442695040888963407ull; w = (s >> 1) % ms::gl::P; }
    ms::GpuVec<ms::Fp> cur(pl, words);
    for (int layer = 0; layer < 3; layer++) {
        const ms::MerkleTree tree = ms::MerkleTree::from_fri_layer(cur, ff, h);
        coin.reseed_digest(tree.root_ptr());
        const ms::GpuVec<ms::Fp> alpha = coin.draw<ms::Fp>();
        ms::GpuVec<ms::Fp> next = ms::apply_drp<ms::Fp>(cur, alpha, ff, 7);
        // nothing above waited for the device; now look
        const auto root = tree.root();
        const auto a = alpha.to_host();
        print_hex("root", root.data(), 32);
        printf("alpha %llu\n", (unsigned long long)a[0]);
        REQUIRE(next.to_host() == ms::apply_drp<ms::Fp>(cur, a, ff, 7).to_host());
        cur = std::move(next);
    }
    coin.reseed_elements(cur);
    const ms_coin_state st = coin.state();
    REQUIRE(st.counter == 0 && st.nbytes == 0);
    print_hex("remainder", (const uint8_t*)cur.to_host().data(), cur.len() * 8);
    print_hex("seed", st.seed, 32);
    const uint64_t nonce = coin.grind(8);
    coin.reseed_int(nonce);
    printf("nonce %llu\n", (unsigned long long)nonce);
    for (size_t p : coin.draw_queries(8, (size_t)1 << 9)) printf("position %zu\n", p);
    printf("coin host mirror ok\n");
    return 0;
}
