/* ministark_hip_transcript.h -- the Fiat-Shamir layer of the C ABI, on top of ministark_hip.h (same conventions, same library):
 * the public coin with its state in device memory, and the FRI fold that reads its challenge there.  Together they let a prover
 * enqueue the whole FRI commit phase -- commit, reseed with the root, draw alpha, fold, per layer -- without a host wait.
 * ministark_hip.h is the reference's gpu-poly boundary (crate ministark-gpu); these entry points stand in for items of the main
 * crate (src/random.rs, src/channel.rs, src/fri.rs), which is why they have a header -- and generated bindings,
 * rust/gpu/src/hip/sys_transcript.rs, ministark_amd/_lib.py `transcript_sigs` -- of their own. */
#ifndef MINISTARK_HIP_TRANSCRIPT_H
#define MINISTARK_HIP_TRANSCRIPT_H
#include "ministark_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- public coin: PublicCoinImpl<F, H> (src/random.rs:61-141) with its state in device memory, for the calls ProverChannel makes
 * (src/channel.rs:46-100, src/fri.rs:217-247).  H = SHA-256 (MS_HASH_SHA256) or BLAKE2s-256 (MS_HASH_BLAKE2S).  The state is a 32-byte
 * seed, a u64 counter and the unread bytes of the last digest (ms_coin_state: `nbytes` unread bytes in bytes[0..nbytes), consumed from
 * the END; bytes past nbytes and `pad` are zero).  d_coin is the handle ms_coin_create returns: the device address of that record; it
 * and ms_coin_state travel as void*, like ms_canon_report.  Rules (restated from the reference's dependencies):
 *   words       when nothing is unread: counter += 1, unread = H(seed || counter as 8 big-endian bytes).  A word is 8 bytes popped
 *               from the end (Iterator::next on the byte vector, next_u64 = from_be_bytes; src/random.rs:88-96, 147-169): a digest D yields LE64(D[24..32]),
 *               LE64(D[16..24]), LE64(D[8..16]), LE64(D[0..8]).  Every consumer takes whole words.
 * ms_coin_create           PublicCoin::new(seed): counter 0, nothing unread (src/random.rs:102-109)
 * ms_coin_read / _write    the state record, to and from the host (tests, checkpoints).  _read blocks.  _write refuses nbytes outside
 *                          {0, 8, 16, 24, 32}.
 * ms_coin_reseed_digest    reseed_with_digest (src/random.rs:111-115, src/channel.rs:46-63): seed = H(seed || digest) (HashFn::merge),
 *                          counter = 0, nothing unread.  d_digest32: 32 bytes of device memory, 4-byte aligned, e.g. d_nodes + 32, the
 *                          root of a tree ms_*_merkle built.  An RPO-256 digest (4 Fp elements in Montgomery form) is absorbed as the
 *                          32 bytes it occupies in memory.
 * ms_coin_reseed_int       reseed_with_int (src/random.rs:123-127; the proof-of-work nonce, src/channel.rs:86-93):
 *                          seed = H(seed || value as 8 big-endian bytes) (merge_with_int), counter = 0, nothing unread
 * ms_coin_reseed_elements  reseed_with_field_elements (src/random.rs:70-75, 117-121; OOD evaluations src/channel.rs:65-74, the FRI remainder
 *                          src/fri.rs:240-247): for each element in order seed = H(seed || H(bytes(e))), bytes(e) = the canonical
 *                          little-endian bytes ms_sha256_rows hashes for a one-column row (Fp 8, Fq3 c0||c1||c2, Fp252 32); elements
 *                          are in Montgomery form.  count = 0 changes nothing, counter and unread bytes included.  _host takes the
 *                          elements from host memory through the staging ring; h_elems may be reused at once.
 * ms_coin_draw             draw() x count (src/random.rs:134-136) into d_out (count elements of `field`, Montgomery form, which must
 *                          not overlap the state).  The sampler is ark-ff 0.4.2's Standard distribution: N words as limbs 0..N-1
 *                          (N = 1, or 4 for Fp252), the top 64 N - bits(p) bits of the last limb cleared (0 / 4), the integer accepted
 *                          when it is < p, otherwise all N words are discarded and the sample repeats; the accepted limbs ARE the
 *                          Montgomery representation.  Fq3 draws c0, c1, c2 in that order.
 * ms_coin_draw_queries     draw_queries(max_n, domain_size) (src/random.rs:138-140): max_n samples of rand 0.8.5's
 *                          gen_range(0..domain_size) -- zone = (range << clz64(range)) - 1; take words v until lo64(v * range) <= zone,
 *                          the sample is hi64(v * range) -- returned distinct and ascending (a BTreeSet) in h_positions (room for
 *                          max_n), their number in *npos.  Blocks.
 * ms_coin_pow_grind        grind_proof_of_work (src/random.rs:48-58): ms_sha256_pow_grind / ms_blake2s_pow_grind with the seed read
 *                          from the coin on the device.  Blocks; does not reseed -- the caller absorbs the nonce with
 *                          ms_coin_reseed_int (src/channel.rs:76-93).
 * The reseeds and ms_coin_draw are asynchronous: one single-wave launch on the context's stream, no host wait.  Refused with
 * MS_ERR_INVALID before anything is enqueued, the state left as it was: null pointers, a d_coin this context did not create, an unknown
 * hash or field, domain_size = 0, bits > 64. */
enum { MS_HASH_SHA256 = 0, MS_HASH_BLAKE2S = 1 };
typedef struct ms_coin_state { uint8_t seed[32]; uint64_t counter; uint32_t nbytes; uint32_t pad; uint8_t bytes[32]; } ms_coin_state;
int ms_coin_create(ms_ctx* ctx, int hash, const void* h_seed32, void** d_coin);
int ms_coin_destroy(ms_ctx* ctx, void* d_coin);
int ms_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state);
int ms_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state);
int ms_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest32);
int ms_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value);
int ms_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count);
int ms_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count);
int ms_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out);
int ms_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos);
int ms_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce);

/* ---- FRI fold with the challenge in device memory: apply_drp (src/fri.rs:526-567) as build_layer calls it right after
 * channel.draw_fri_alpha (src/fri.rs:199-231). */
/* ms_fri_fold_dev: ms_fri_fold with the challenge taken from DEVICE memory -- d_alpha is one element of `field` (8-byte aligned), read by
 * the kernel when it runs, e.g. where ms_coin_draw has just put it (channel.draw_fri_alpha, src/fri.rs:225-227): commit, reseed,
 * draw and fold of a FRI layer are then enqueued on the stream without a host wait.  Every other rule is ms_fri_fold's, and the words
 * are those ms_fri_fold writes for the same alpha.  d_out must overlap neither d_evals nor the element at d_alpha (MS_ERR_INVALID). */
int ms_fri_fold_dev(ms_ctx* ctx, int field, unsigned log_n, unsigned folding_factor, const void* d_alpha,
                    const void* h_offset, const void* d_evals, void* d_out);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_TRANSCRIPT_H */
