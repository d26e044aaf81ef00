/* ministark_hip_poseidon.h -- Starknet's Poseidon over the 252-bit field: the bulk permutation and algebraic commitments, on top of
 * ministark_hip.h (same conventions, same library).  The field is MS_STARK252_FP, p = 2^251 + 17 * 2^192 + 1; the function is the
 * Hades permutation with t = 3, S-box x^3, 8 full and 83 partial rounds -- the Cairo `poseidon` builtin and the `poseidon3` commitment
 * hash, which a verifier written in Cairo recomputes in-field:
 *   rc[i] = sha256("Hades<i>") as a big-endian integer, mod p, i = 0 .. 272
 *   round r = 0 .. 90:  s[j] += rc[3r + j];  x -> x^3 on all three elements when r < 4 or r >= 87, on s[2] alone otherwise;
 *                       mix with M = [[3, 1, 1], [1, -1, 1], [1, 1, -2]]
 *   hash2(x, y)  = permute(x, y, 2)[0]                                             a Merkle node
 *   hash_many(v) = append 1 to v, and 0 as well if the length is then odd; start from (0, 0, 0); for each pair (a, b):
 *                  s0 += a, s1 += b, permute; the result is s0.  hash_many([]) is one permutation of (1, 0, 0).       a leaf
 * Elements are the library's Fp252 form everywhere: 4 little-endian u64 in Montgomery form (radix 2^256).  A DIGEST IS ONE ELEMENT in
 * that form, 32 bytes, so a level of digests is a column of Fp252 and ms_gather_digests[_multi], ms_merkle_view_ids and the proofs keep
 * their shapes.  These entry points have a header -- and generated bindings, rust/gpu/src/hip/sys_poseidon.rs, ministark_amd/_lib.py
 * `poseidon_sigs` -- of their own, as the Keccak layer has.
 *
 * ms_poseidon252_permute         d_out[i] = permute(d_in[i]) over n states of 3 elements, row-major [n][3] (96 bytes a state): the bulk
 *                                primitive of a Poseidon-builtin trace generator.  d_out == d_in is allowed; any other overlap of the
 *                                two ranges is MS_ERR_INVALID ("overlap").  n = 0 does nothing.
 * ms_poseidon252_rows            leaf[r] = hash_many(row r of the column-major matrix d_cols[0 .. ncols)), d_leaves nrows x 32 bytes.
 *                                ncols <= 128, else MS_ERR_UNSUPPORTED; ncols = 0 gives hash_many([]) in every row; nrows = 0 does nothing.
 * ms_poseidon252_rows_row_major  the same leaves for a row-major matrix (a FRI layer: row r = ncols consecutive elements), ncols in
 *                                1 .. 128, else MS_ERR_UNSUPPORTED.
 * ms_poseidon252_merkle          nodes[k] = hash2(nodes[2k], nodes[2k+1]) over nleaves = 2^k >= 2 leaves of 32 bytes: nodes[1] is the
 *                                root, nodes[0] is zero, d_nodes holds nleaves x 32 bytes -- the layout of the other trees.
 * Refused with MS_ERR_INVALID before anything is enqueued and with the outputs untouched: null pointers (a null column included,
 * "null column <c>"), nleaves that is not a power of two >= 2.
 *
 * Checked mode (ms_ctx_set_checked): all four do arithmetic on their inputs, so with checked mode on they scan first and refuse
 * non-canonical elements (a word pattern >= p) as ms_rpo256_rows_field and ms_rpo256_merkle do -- MS_ERR_INVALID, ms_last_error()
 * naming the entry point, the argument, the column, row and component, before anything is enqueued and with the outputs untouched.
 * Without it a non-canonical element gives an unspecified (but in-bounds) result.
 *
 * Not here: a Poseidon public coin and Poseidon proof-of-work -- a prover that commits with Poseidon draws from the byte coin and
 * grinds with SHA-256 over the root's 32 bytes, as an RPO-256 prover without the RPO coin does. */
#ifndef MINISTARK_HIP_POSEIDON_H
#define MINISTARK_HIP_POSEIDON_H
#include "ministark_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int ms_poseidon252_permute(ms_ctx* ctx, size_t n, const void* d_in, void* d_out);
int ms_poseidon252_rows(ms_ctx* ctx, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves);
int ms_poseidon252_rows_row_major(ms_ctx* ctx, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves);
int ms_poseidon252_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_POSEIDON_H */
