// The C++ mirror of the BLAKE3 commitments (Hash::Blake3_256 in ministark.hpp, grind_proof_of_work's hash and PublicCoin's id mapping in
// prover.hpp) on the cases tests/test_blake3_prover.py builds through the Python mirror and recomputes with tests/blake3_ref.py:
// column-major Fp, Fq3 and Fp252 matrices -- one of them with rows longer than a chunk -- a row-major FRI layer, proof-of-work nonces from
// a host seed and from the coin, and one draw.  The inputs are splitmix64 words reduced below p, taken as Montgomery words (Fp252: with
// the top limb cut to 59 bits, so that the element is below its prime).  Prints one JSON line per case.
//   usage: test_blake3_mirror [digests.txt]     lines "<case> <root as hex>" written by the test from tests/blake3_ref.py: every root
//                                               computed here must be the one the file gives for its case, or the program fails
#include <array>
#include <cstdio>
#include <fstream>
#include <map>
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
template <class F>
static std::vector<uint64_t> elements(size_t n, uint64_t seed) {
    std::vector<uint64_t> w = words(n * F::words, seed);
    if (F::words == 4)
        for (size_t i = 3; i < w.size(); i += 4) w[i] >>= 5;                 // below 2^251 < p
    return w;
}
static std::string hex(const std::array<uint8_t, 32>& d) {
    std::string s;
    char b[3];
    for (uint8_t x : d) { snprintf(b, sizeof b, "%02x", x); s += b; }
    return s;
}
static std::map<std::string, std::string> expected;                         // empty: nothing to compare with
static int mismatches = 0;
static void report(const char* name, const std::string& root) {
    printf("{\"case\": \"%s\", \"root\": \"%s\"}\n", name, root.c_str());
    if (expected.empty()) return;
    auto it = expected.find(name);
    if (it == expected.end() || it->second != root) {
        fprintf(stderr, "%s: root %s, the helper gives %s\n", name, root.c_str(), it == expected.end() ? "nothing" : it->second.c_str());
        mismatches++;
    }
}
template <class F>
static void matrix_case(Planner& pl, const char* name, size_t nrows, unsigned ncols, uint64_t seed) {
    Matrix<F> m;
    for (unsigned c = 0; c < ncols; c++) m.columns.emplace_back(pl, elements<F>(nrows, seed + c));
    report(name, hex(MerkleTree::from_matrix(m, Hash::Blake3_256).root()));
}

int main(int argc, char** argv) {
    if (argc > 1) {
        std::ifstream in(argv[1]);
        std::string name, root;
        while (in >> name >> root) expected[name] = root;
        if (expected.empty()) { fprintf(stderr, "%s: no digests\n", argv[1]); return 2; }
    }
    Planner& pl = get_planner();
    const Hash h = Hash::Blake3_256;
    matrix_case<Fp>(pl, "fp_1x256", 256, 1, 11);
    matrix_case<Fp>(pl, "fp_17x256", 256, 17, 21);
    matrix_case<Fq3>(pl, "fq3_43x64", 64, 43, 41);                           // 1 032 bytes a row: two chunks
    matrix_case<Fp252>(pl, "fp252_97x32", 32, 97, 61);                       // 3 104 bytes a row: four chunks
    GpuVec<Fp> ev(pl, words((size_t)1 << 10, 51));
    report("fri_fp_8", hex(MerkleTree::from_fri_layer(ev, 8, h).root()));
    std::array<uint8_t, 32> seed{};
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(i * 13 + 1);
    const uint64_t nonce = grind_proof_of_work(pl, seed, 9, (uint64_t)1 << 40, h);
    const uint64_t sha = grind_proof_of_work(pl, seed, 9);                  // the default stays SHA-256
    PublicCoin coin(pl, seed, h);
    coin.reseed_int(5);
    const uint64_t coin_nonce = coin.grind(9);
    const uint64_t word = coin.draw<Fp>().to_host()[0];
    printf("{\"case\": \"pow\", \"nonce\": %llu, \"sha256\": %llu, \"coin_nonce\": %llu, \"coin_word\": %llu}\n",
           (unsigned long long)nonce, (unsigned long long)sha, (unsigned long long)coin_nonce, (unsigned long long)word);
    if (mismatches) return 1;
    printf("cpp blake3 mirror ok\n");
    return 0;
}
