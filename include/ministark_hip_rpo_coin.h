/* ministark_hip_rpo_coin.h -- the RPO-256 public coin: an algebraic Fiat-Shamir transcript and proof-of-work, on top of
 * ministark_hip_transcript.h (same conventions, same library).  A prover that commits with RPO-256 so that its verifier is cheap inside
 * another proof draws its challenges here, and that verifier never hashes a byte.  The coin is a 12-element sponge over Goldilocks on
 * the permutation of ms_rpo256_rows / ms_rpo256_merkle: capacity s[0..4), rate s[4..12).  It absorbs field elements directly and draws
 * them without rejection, so its state is not ms_coin_state and its handles are not ms_coin_create's: the family has entry points --
 * and generated bindings, rust/gpu/src/hip/sys_rpo_coin.rs, ministark_amd/_lib.py `rpo_coin_sigs` -- of its own.  ms_coin_create's
 * hash id 2 stays unknown.  The transcript rules are this project's own, modelled on Miden's RpoRandomCoin (no parity with it is
 * claimed); the permutation is pinned by Miden's known answers.
 *
 * All values are Goldilocks elements; in device memory and in this ABI they are Montgomery words, like every column.  "x as an
 * integer" means the canonical value.  The state record is ms_rpo_coin_state, 128 bytes, 8-byte aligned: `pos` in 4..12 is the index of
 * the next unread rate element (12: nothing unread), `pad` is zero.  d_coin is the handle ms_rpo_coin_create returns: the device
 * address of that record; it and the record travel as void*, like ms_coin_state.
 *
 * ms_rpo_coin_create        h_seed4: four words < p.  s = 0; s[4..8) = seed; permute; pos = 4.  A word >= p: MS_ERR_INVALID.
 * ms_rpo_coin_destroy       a null d_coin is MS_OK.
 * ms_rpo_coin_read / _write the record, to and from the host (tests, checkpoints).  _read blocks.  _write refuses pos outside 4..12,
 *                           non-zero pad and any s[i] >= p -- host words, so always, not only in checked mode.
 * ms_rpo_coin_reseed_digest d_digest4: four elements of device memory, 8-byte aligned, e.g. d_nodes + 32, the root of a tree
 *                           ms_rpo256_merkle built.  s[4+i] += d[i] for i < 4; permute; pos = 4.
 * ms_rpo_coin_reseed_int    any u64 (the proof-of-work nonce): s[4] += value mod 2^32, s[5] += value >> 32; permute; pos = 4.
 * ms_rpo_coin_reseed_elements  field = MS_GOLDILOCKS_FP or MS_GOLDILOCKS_FQ3 (MS_STARK252_FP: MS_ERR_UNSUPPORTED).  The base-field
 *                           words in memory order (c0, c1, c2 of each Fq3 element), then a single 1, then zeros up to a multiple of 8;
 *                           for each block of 8: s[4+j] += w[j], permute; finally pos = 4.  count = 0 changes nothing, pos included.
 *                           _host takes the elements from host memory through the staging ring; h_elems may be reused at once.
 * ms_rpo_coin_draw          count elements of `field` into d_out (which must not overlap the state): for each base-field word, if
 *                           pos == 12 then permute and pos = 4; the word is s[pos++].  An Fq3 element is three consecutive words.  No
 *                           rejection.  MS_STARK252_FP: MS_ERR_UNSUPPORTED.
 * ms_rpo_coin_draw_queries  domain_size a power of two in 1..2^32, else MS_ERR_INVALID.  max_n samples of (one drawn word as an
 *                           integer) & (domain_size - 1), returned distinct and ascending in h_positions (room for max_n), their
 *                           number in *npos.  Blocks.
 * ms_rpo_coin_pow_grind     the smallest nonce n in 1..max_nonce such that t = permute(s with s[4] += n mod 2^32, s[5] += n >> 32) has
 *                           t[0], as an integer, with its low `bits` bits zero.  bits in 0..63 (0 gives 1); bits > 63 or no such nonce:
 *                           MS_ERR_INVALID.  Blocks; does not reseed -- the caller absorbs the nonce with ms_rpo_coin_reseed_int, after
 *                           which the state IS t.  The condition is on a capacity element because capacity is never drawn: on t[4] it
 *                           would clear the low bits of the first query position.
 * The reseeds and ms_rpo_coin_draw are asynchronous: one single-wave launch on the context's stream, no host wait.  Refused with
 * MS_ERR_INVALID before anything is enqueued, the state left as it was: null pointers, a d_coin that ms_rpo_coin_create did not return
 * on this context (a handle of ms_coin_create included), an unknown field.
 *
 * Checked mode (ms_ctx_set_checked): ms_rpo_coin_reseed_elements, _reseed_elements_host and _reseed_digest refuse non-canonical input
 * as ms_coin_reseed_elements does -- MS_ERR_INVALID, ms_last_error() naming the entry point and the argument, before anything is
 * enqueued. */
#ifndef MINISTARK_HIP_RPO_COIN_H
#define MINISTARK_HIP_RPO_COIN_H
#include "ministark_hip_transcript.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ms_rpo_coin_state { uint64_t s[12]; uint32_t pos; uint32_t pad[7]; } ms_rpo_coin_state;
int ms_rpo_coin_create(ms_ctx* ctx, const void* h_seed4, void** d_coin);
int ms_rpo_coin_destroy(ms_ctx* ctx, void* d_coin);
int ms_rpo_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state);
int ms_rpo_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state);
int ms_rpo_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest4);
int ms_rpo_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value);
int ms_rpo_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count);
int ms_rpo_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count);
int ms_rpo_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out);
int ms_rpo_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos);
int ms_rpo_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_RPO_COIN_H */
