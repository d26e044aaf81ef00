/* ministark_hip_keccak.h -- Keccak-256 and SHA3-256 commitments, proof-of-work and public coin, on top of ministark_hip.h and
 * ministark_hip_transcript.h (same conventions, same library).  H = the Keccak sponge, rate 136 bytes, capacity 512 bits, 32-byte
 * digest, behind the reference's HashFn / ElementHashFn seam (src/hash.rs:9-41) for MatrixMerkleTreeImpl<H>
 * (src/merkle.rs:296-361, 412-508) and PublicCoinImpl<F, H> (src/random.rs:48-58, 61-141).  The two members differ in the domain byte
 * appended to the message and nothing else:
 *   MS_KECCAK256  0x01  the original submission's padding: sha3::Keccak256, the EVM's KECCAK256 -- the hash an on-chain verifier
 *                       recomputes with one opcode
 *   MS_SHA3_256   0x06  FIPS 202: sha3::Sha3_256, hashlib.sha3_256
 * Sponge rules: lanes are little-endian; the domain byte goes at offset L mod 136 of the last block and 0x80 is ORed into that block's
 * byte 135; a message whose length L is a multiple of 136 gets one more block that holds only padding; the digest is the first 32
 * bytes of the state.  These entry points have a header -- and generated bindings, rust/gpu/src/hip/sys_keccak.rs,
 * ministark_amd/_lib.py `keccak_sigs` -- of their own, as the transcript layer has.
 *
 * Each entry point is the twin of its ms_blake2s_* namesake, with `variant` in front and the same rules:
 * ms_keccak_rows            leaf[r] = H( ||_c canonical little-endian bytes of M[c][r] ): the bytes ms_sha256_rows / ms_blake2s_rows
 *                           hash (Fp 8 bytes, Fq3 c0||c1||c2, Fp252 32 bytes); columns in Montgomery form, d_leaves nrows x 32 bytes.
 *                           ncols <= 128, else MS_ERR_UNSUPPORTED; ncols = 0 gives H("") in every row; nrows = 0 does nothing.
 * ms_keccak_rows_row_major  the same leaves for a row-major matrix (a FRI layer: row r = ncols consecutive elements), ncols in 1..128,
 *                           else MS_ERR_UNSUPPORTED.
 * ms_keccak_merkle          nodes[k] = H(nodes[2k] || nodes[2k+1]) over nleaves = 2^k >= 2 leaves of 32 bytes: nodes[1] is the root,
 *                           nodes[0] is zero, d_nodes holds nleaves x 32 bytes.  A merge is one permutation.
 * ms_keccak_pow_grind       grind_proof_of_work (src/random.rs:48-58): the smallest nonce n >= 1 with `bits` leading zero bits of
 *                           H(seed || n as 8 big-endian bytes), byte 0's high bit first.  bits > 64, or no nonce up to max_nonce:
 *                           MS_ERR_INVALID.  Blocks.
 * Refused with MS_ERR_INVALID before anything is enqueued: null pointers (a null column included), an unknown field, an unknown variant.
 *
 * Checked mode (ms_ctx_set_checked): ms_keccak_rows and ms_keccak_rows_row_major take field data out of Montgomery form, so with
 * checked mode on they refuse non-canonical input exactly as ms_blake2s_rows does -- MS_ERR_INVALID, ms_last_error() naming the entry
 * point, the argument, the column, row and component, before anything is enqueued and with d_leaves untouched.  ms_keccak_merkle and
 * ms_keccak_pow_grind only move bytes and are not checked.
 *
 * The coin: ms_coin_create accepts MS_HASH_KECCAK256 and MS_HASH_SHA3_256 as `hash`; every ms_coin_* entry point and ms_fri_fold_dev
 * then work as for the other hashes (ms_coin_pow_grind included; every message of the coin is one block).  Id 2 stays unknown: it is
 * left for an RPO-256 coin. */
#ifndef MINISTARK_HIP_KECCAK_H
#define MINISTARK_HIP_KECCAK_H
#include "ministark_hip_transcript.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_KECCAK256 = 0, MS_SHA3_256 = 1 };             /* variant: domain byte 0x01 / 0x06 */
enum { MS_HASH_KECCAK256 = 3, MS_HASH_SHA3_256 = 4 };   /* ms_coin_create's `hash`; 2 stays unknown */
int ms_keccak_rows(ms_ctx* ctx, int variant, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves);
int ms_keccak_rows_row_major(ms_ctx* ctx, int variant, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves);
int ms_keccak_merkle(ms_ctx* ctx, int variant, size_t nleaves, const void* d_leaves, void* d_nodes);
int ms_keccak_pow_grind(ms_ctx* ctx, int variant, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_KECCAK_H */
