/* ministark_hip_hades_coin.h -- the algebraic public coin of the 252-bit field: a Fiat-Shamir transcript and proof-of-work on the Hades
 * permutation (t = 3, x^3, 8 + 83 rounds) of the library's algebraic 252-bit commitment, on top of ministark_hip_transcript.h (same
 * conventions, same library).  A prover that commits over MS_STARK252_FP with that permutation so that its verifier is cheap inside
 * another proof draws its challenges here, and that verifier never hashes a byte.  The coin is not a sponge: it keeps ONE field element
 * and a draw counter, as ms_coin_state keeps (seed, counter).  Absorbing is serial; every draw of a call is an independent permutation
 * (one launch, a lane per element); the proof-of-work search has the same shape.  Its state is neither ms_coin_state nor
 * ms_rpo_coin_state and its handles are neither family's: the entry points -- and generated bindings,
 * rust/gpu/src/hip/sys_hades_coin.rs, ministark_amd/_lib.py `hades_coin_sigs` -- are its own.  The transcript rules are this project's
 * own (no parity with another implementation is claimed); the permutation is pinned by known answers.
 *
 * Below, permute(a, b, c) is the permutation of the state (a, b, c); hash2(x, y) = permute(x, y, 2)[0], the Merkle node of the
 * commitment; hash_many(v) appends 1, then 0 if that leaves the length odd, and from (0, 0, 0) runs s0 += a, s1 += b, permute for each
 * pair (a, b), giving s0.  All values are elements of the 252-bit field; in device memory and in this ABI an element is four
 * little-endian u64 Montgomery words, like every Fp252 column and every digest of the commitment.  "x as an integer" means the canonical
 * value.  The third state element is a domain tag: 2 absorb, 3 draw, 4 proof-of-work.  The state record is ms_hades_coin_state, 56 bytes,
 * 8-byte aligned: `digest` (Montgomery words), `n_draws`, `pad` zero.  d_coin is the handle ms_hades_coin_create returns: the device
 * address of that record; it and the record travel as void*, like ms_coin_state.
 *
 * ms_hades_coin_create      h_seed4: ONE element < p as four canonical little-endian host words.  digest = seed; n_draws = 0; no
 *                           permutation.  A seed >= p: MS_ERR_INVALID.
 * ms_hades_coin_destroy     a null d_coin is MS_OK.
 * ms_hades_coin_read / _write  the record, to and from the host (tests, checkpoints).  _read blocks.  _write refuses non-zero pad and a
 *                           digest >= p -- host words, so always, not only in checked mode.
 * ms_hades_coin_reseed_digest  d_digest: one element of device memory, 8-byte aligned, e.g. d_nodes + 32, the root of a tree of the
 *                           algebraic 252-bit commitment.  digest = hash2(digest, d); n_draws = 0.
 * ms_hades_coin_reseed_int  any u64 (the proof-of-work nonce): digest = hash2(digest, value); n_draws = 0.
 * ms_hades_coin_reseed_elements  field = MS_STARK252_FP (the Goldilocks fields: MS_ERR_UNSUPPORTED).  digest = hash2(digest,
 *                           hash_many(elements)); n_draws = 0.  count = 0 changes nothing, n_draws included.  _host takes the elements
 *                           from host memory through the staging ring; h_elems may be reused at once.
 * ms_hades_coin_draw        count elements of MS_STARK252_FP (the Goldilocks fields: MS_ERR_UNSUPPORTED) into d_out, which must not
 *                           overlap the state: out[i] = permute(digest, n_draws + i, 3)[0] for i < count; then n_draws += count.  No
 *                           rejection.  A call one of whose counters n_draws + i does not fit a u64 is refused with MS_ERR_INVALID (a draw
 *                           that ends exactly on counter 2^64 - 1 is served, and n_draws wraps to 0).
 * ms_hades_coin_draw_queries  domain_size a power of two in 1..2^32, else MS_ERR_INVALID.  max_n draws as above, each giving (the element
 *                           as an integer) & (domain_size - 1), returned distinct and ascending in h_positions (room for max_n), their
 *                           number in *npos.  Blocks.
 * ms_hades_coin_pow_grind   the smallest nonce n in 1..max_nonce such that permute(digest, n, 4)[0], as an integer, has its low `bits`
 *                           bits zero.  bits in 0..63 (0 gives 1); bits > 63 or no such nonce: MS_ERR_INVALID.  Blocks; does not reseed --
 *                           the caller absorbs the nonce with ms_hades_coin_reseed_int.  The digest after that reseed is another
 *                           permutation's output (tag 2, not 4), so the condition clears no bit of the first query position.
 * The reseeds and ms_hades_coin_draw are asynchronous: launches on the context's stream, no host wait (a reseed is one single-lane
 * launch; a draw of up to 256 elements is one launch, a longer one is followed by a single-lane launch that advances n_draws).  Refused
 * with MS_ERR_INVALID before anything is enqueued, the state left as it was: null pointers, a d_coin that ms_hades_coin_create did not
 * return on this context (a handle of ms_coin_create or ms_rpo_coin_create included), an unknown field.
 *
 * Checked mode (ms_ctx_set_checked): ms_hades_coin_reseed_elements, _reseed_elements_host and _reseed_digest refuse non-canonical input
 * as ms_rpo_coin_reseed_elements does -- MS_ERR_INVALID, ms_last_error() naming the entry point and the argument, before anything is
 * enqueued. */
#ifndef MINISTARK_HIP_HADES_COIN_H
#define MINISTARK_HIP_HADES_COIN_H
#include "ministark_hip_transcript.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ms_hades_coin_state { uint64_t digest[4]; uint64_t n_draws; uint32_t pad[4]; } ms_hades_coin_state;
int ms_hades_coin_create(ms_ctx* ctx, const void* h_seed4, void** d_coin);
int ms_hades_coin_destroy(ms_ctx* ctx, void* d_coin);
int ms_hades_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state);
int ms_hades_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state);
int ms_hades_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest);
int ms_hades_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value);
int ms_hades_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count);
int ms_hades_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count);
int ms_hades_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out);
int ms_hades_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos);
int ms_hades_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_HADES_COIN_H */
