/* ministark_hip_blake3.h -- BLAKE3 commitments, proof-of-work and public coin, on top of ministark_hip.h and
 * ministark_hip_transcript.h (same conventions, same library).  H = unkeyed BLAKE3 in its default hash mode with a 32-byte digest
 * (blake3::hash; Winterfell's Blake3_256), behind the reference's HashFn / ElementHashFn seam (src/hash.rs:9-41) for
 * MatrixMerkleTreeImpl<H> (src/merkle.rs:296-361, 412-508) and PublicCoinImpl<F, H> (src/random.rs:48-58, 61-141).
 * Hash rules: words are little-endian; the input is cut into chunks of 1024 bytes (the empty input is one empty chunk) and a chunk
 * into 64-byte blocks, the last one zero-padded; every block of chunk c is compressed with counter c, its count of real bytes and
 * the flags CHUNK_START (1) on a chunk's first block, CHUNK_END (2) on its last; two subtrees are joined by a parent compression
 * (flag PARENT = 4, counter 0, 64 bytes, chaining value IV), the left one taking the largest power of two of chunks below the chunk
 * count; ROOT (8) goes on the last compression only.  The compression is BLAKE2s's G with 7 rounds.  These entry points have a
 * header -- and generated bindings, rust/gpu/src/hip/sys_blake3.rs, ministark_amd/_lib.py `blake3_sigs` -- of their own, as the
 * Keccak layer has.
 *
 * Each entry point is the twin of its ms_blake2s_* namesake, with the same rules:
 * ms_blake3_rows            leaf[r] = H( ||_c canonical little-endian bytes of M[c][r] ): the bytes ms_sha256_rows / ms_blake2s_rows
 *                           hash (Fp 8 bytes, Fq3 c0||c1||c2, Fp252 32 bytes); columns in Montgomery form, d_leaves nrows x 32 bytes.
 *                           ncols <= 128, else MS_ERR_UNSUPPORTED -- a row is at most 4 chunks; ncols = 0 gives H("") in every row;
 *                           nrows = 0 does nothing.
 * ms_blake3_rows_row_major  the same leaves for a row-major matrix (a FRI layer: row r = ncols consecutive elements), ncols in 1..128,
 *                           else MS_ERR_UNSUPPORTED.
 * ms_blake3_merkle          nodes[k] = H(nodes[2k] || nodes[2k+1]) over nleaves = 2^k >= 2 leaves of 32 bytes: nodes[1] is the root,
 *                           nodes[0] is zero, d_nodes holds nleaves x 32 bytes.  A merge is the plain hash of 64 bytes -- one
 *                           compression with flags CHUNK_START | CHUNK_END | ROOT -- as for every other H behind HashFn::merge; it is
 *                           not BLAKE3's parent-node mode.
 * ms_blake3_pow_grind       grind_proof_of_work (src/random.rs:48-58): the smallest nonce n >= 1 with `bits` leading zero bits of
 *                           H(seed || n as 8 big-endian bytes), byte 0's high bit first.  bits > 64, or no nonce up to max_nonce:
 *                           MS_ERR_INVALID.  Blocks.
 * Refused with MS_ERR_INVALID before anything is enqueued: null pointers (a null column included), an unknown field, a leaf count
 * that is not a power of two >= 2.
 *
 * Checked mode (ms_ctx_set_checked): ms_blake3_rows and ms_blake3_rows_row_major take field data out of Montgomery form, so with
 * checked mode on they refuse non-canonical input exactly as ms_blake2s_rows does -- MS_ERR_INVALID, ms_last_error() naming the entry
 * point, the argument, the column, row and component, before anything is enqueued and with d_leaves untouched.  ms_blake3_merkle and
 * ms_blake3_pow_grind only move bytes and are not checked.
 *
 * The coin: ms_coin_create accepts MS_HASH_BLAKE3 as `hash`; every ms_coin_* entry point and ms_fri_fold_dev then work as for the
 * other hashes (ms_coin_pow_grind included; every message of the coin is one block).  Ids 2 and 5 stay unknown.  Keyed hashing,
 * key derivation and extended output are not offered. */
#ifndef MINISTARK_HIP_BLAKE3_H
#define MINISTARK_HIP_BLAKE3_H
#include "ministark_hip_transcript.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_HASH_BLAKE3 = 6 };   /* ms_coin_create's `hash`; 2 and 5 stay unknown */
int ms_blake3_rows(ms_ctx* ctx, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves);
int ms_blake3_rows_row_major(ms_ctx* ctx, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves);
int ms_blake3_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes);
int ms_blake3_pow_grind(ms_ctx* ctx, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_BLAKE3_H */
