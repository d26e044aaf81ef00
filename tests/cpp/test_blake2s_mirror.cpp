// The C++ mirror of the BLAKE2s-256 commitments (Hash::Blake2s in ministark.hpp, grind_proof_of_work's hash in prover.hpp) on the cases
// tests/test_blake2s_mirror.py builds through the Python mirror: column-major Fp and Fq3 matrices, row-major FRI layers and proof-of-work
// nonces.  The inputs are splitmix64 words reduced below p, taken as Montgomery words.  Prints one JSON line per case.
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
static void matrix_case(Planner& pl, const char* name, size_t nrows, unsigned ncols, uint64_t seed) {
    Matrix<F> m;
    for (unsigned c = 0; c < ncols; c++) m.columns.emplace_back(pl, words(nrows * F::words, seed + c));
    const auto root = MerkleTree::from_matrix(m, Hash::Blake2s).root();
    printf("{\"case\": \"%s\", \"root\": \"%s\"}\n", name, hex(root).c_str());
}
template <class F>
static void fri_case(Planner& pl, const char* name, size_t n, unsigned folding, uint64_t seed) {
    GpuVec<F> ev(pl, words(n * F::words, seed));
    const auto root = MerkleTree::from_fri_layer(ev, folding, Hash::Blake2s).root();
    printf("{\"case\": \"%s\", \"root\": \"%s\"}\n", name, hex(root).c_str());
}

int main() {
    Planner& pl = get_planner();
    matrix_case<Fp>(pl, "fp_1x1024", 1024, 1, 11);
    matrix_case<Fp>(pl, "fp_8x1024", 1024, 8, 21);
    matrix_case<Fp>(pl, "fp_9x512", 512, 9, 31);
    matrix_case<Fq3>(pl, "fq3_3x512", 512, 3, 41);
    fri_case<Fp>(pl, "fri_fp_8", 1 << 11, 8, 51);
    fri_case<Fq3>(pl, "fri_fq3_4", 1 << 10, 4, 61);
    for (unsigned k = 0; k < 3; k++) {
        std::array<uint8_t, 32> seed{};
        for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(i * 13 + 5 * k + 1);
        const uint64_t b2 = grind_proof_of_work(pl, seed, 10, (uint64_t)1 << 40, Hash::Blake2s);
        const uint64_t sha = grind_proof_of_work(pl, seed, 10);                  // the default stays SHA-256
        printf("{\"case\": \"pow_%u\", \"blake2s\": %llu, \"sha256\": %llu}\n", k, (unsigned long long)b2, (unsigned long long)sha);
    }
    printf("cpp blake2s mirror ok\n");
    return 0;
}
