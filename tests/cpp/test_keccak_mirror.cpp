// The C++ mirror of the Keccak-256 / SHA3-256 commitments (Hash::Keccak256 and Hash::Sha3_256 in ministark.hpp, grind_proof_of_work's
// hash and PublicCoin's id mapping in prover.hpp) on the cases tests/test_keccak_prover.py builds through the Python mirror: column-major
// Fp and Fq3 matrices, a row-major FRI layer, proof-of-work nonces from a host seed and from the coin, and one draw.  The inputs are
// splitmix64 words reduced below p, taken as Montgomery words.  Prints one JSON line per case.
#include <array>
#include <cstdio>
#include <string>
#include <vector>
#include "../../ministark_amd/csrc/host/ministark.hpp"
#include "../../ministark_amd/csrc/host/prover.hpp"

using namespace ms;

static std::vector<uint64_t> words(size_t n, uint64_t seed) {               // splitmix64, reduced below the Goldilocks prime
    std::vector<uint64_t> out(n);
    uint64_t s = seed;
    for (auto& w : out) {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        w = (z ^ (z >> 31)) % gl::P;
    }
    return out;
}
static std::string hex(const std::array<uint8_t, 32>& d) {
    std::string s;
    char b[3];
    for (uint8_t x : d) { snprintf(b, sizeof b, "%02x", x); s += b; }
    return s;
}
template <class F>
static void matrix_case(Planner& pl, Hash h, const char* variant, const char* name, size_t nrows, unsigned ncols, uint64_t seed) {
    Matrix<F> m;
    for (unsigned c = 0; c < ncols; c++) m.columns.emplace_back(pl, words(nrows * F::words, seed + c));
    const auto root = MerkleTree::from_matrix(m, h).root();
    printf("{\"case\": \"%s_%s\", \"root\": \"%s\"}\n", variant, name, hex(root).c_str());
}

int main() {
    Planner& pl = get_planner();
    const Hash hashes[2] = {Hash::Keccak256, Hash::Sha3_256};
    const char* names[2] = {"keccak256", "sha3_256"};
    for (int k = 0; k < 2; k++) {
        const Hash h = hashes[k];
        matrix_case<Fp>(pl, h, names[k], "fp_1x256", 256, 1, 11);
        matrix_case<Fp>(pl, h, names[k], "fp_17x256", 256, 17, 21);
        matrix_case<Fq3>(pl, h, names[k], "fq3_6x128", 128, 6, 41);
        GpuVec<Fp> ev(pl, words((size_t)1 << 10, 51));
        printf("{\"case\": \"%s_fri_fp_8\", \"root\": \"%s\"}\n", names[k], hex(MerkleTree::from_fri_layer(ev, 8, h).root()).c_str());
        std::array<uint8_t, 32> seed{};
        for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(i * 13 + 1);
        const uint64_t nonce = grind_proof_of_work(pl, seed, 9, (uint64_t)1 << 40, h);
        const uint64_t sha = grind_proof_of_work(pl, seed, 9);                  // the default stays SHA-256
        PublicCoin coin(pl, seed, h);
        coin.reseed_int(5);
        const uint64_t coin_nonce = coin.grind(9);
        const uint64_t word = coin.draw<Fp>().to_host()[0];
        printf("{\"case\": \"%s_pow\", \"nonce\": %llu, \"sha256\": %llu, \"coin_nonce\": %llu, \"coin_word\": %llu}\n", names[k],
               (unsigned long long)nonce, (unsigned long long)sha, (unsigned long long)coin_nonce, (unsigned long long)word);
    }
    printf("cpp keccak mirror ok\n");
    return 0;
}
