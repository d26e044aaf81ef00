// Keccak-256 / SHA3-256 commitments and proof-of-work grinding (src/hash.rs:9-41, src/merkle.rs:296-361, 412-508, src/random.rs:48-58,
// 61-141): the traits of commit_host.h, which holds the host logic of every byte hash, and the four entry points.  The traits carry the
// domain byte that `variant` selects; every kernel takes it as a launch argument.  Kernels: keccak_kernels.h; declarations:
// include/ministark_hip_keccak.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_keccak.h"
#include "commit_host.h"
#include "keccak_kernels.h"

namespace {
struct KeccakCommit {
    using RowsParams = mskec::RowsParams;
    using PowParams = mskec::PowParams;
    static constexpr int NT = mskec::NT, MAXCOLS = mskec::MAXCOLS;
    static constexpr bool SEED_BIG_ENDIAN = false;
    static constexpr const char *ROWS = "keccak_rows", *LEVEL = "keccak_merkle_level", *TOP = "keccak_merkle_top", *GRIND = "keccak_pow_grind";
    uint32_t domain = 0;                                    // 0x01 Keccak-256, 0x06 SHA3-256
    void rows_hook(RowsParams& P, unsigned) const { P.domain = domain; }
    void pow_hook(PowParams& P) const { P.domain = domain; }
    template <int V> void launch_rows(dim3 grid, dim3 block, hipStream_t st, const RowsParams& P) const { hipLaunchKernelGGL(mskec::keccak_rows<V>, grid, block, 0, st, P); }
    void launch_level(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* dst, size_t count) const { hipLaunchKernelGGL(mskec::keccak_merge_level, grid, block, 0, st, src, dst, count, domain); }
    template <int PER> void launch_top(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* nodes, unsigned count) const { hipLaunchKernelGGL(mskec::keccak_merkle_top<PER>, grid, block, 0, st, src, nodes, count, domain); }
    void launch_grind(dim3 grid, dim3 block, hipStream_t st, const PowParams& P) const { hipLaunchKernelGGL(mskec::keccak_pow_grind, grid, block, 0, st, P); }
};
}  // namespace

// the wrappers look `variant` up before anything else, so an unknown variant is reported ahead of a null argument (both MS_ERR_INVALID)
static int keccak_variant(const char* entry, int variant, KeccakCommit* t) {
    if (variant == MS_KECCAK256) { t->domain = mskec::DOMAIN_KECCAK; return MS_OK; }
    if (variant == MS_SHA3_256) { t->domain = mskec::DOMAIN_SHA3; return MS_OK; }
    return fail(MS_ERR_INVALID, "%s: unknown variant %d (MS_KECCAK256 = 0, MS_SHA3_256 = 1)", entry, variant);
}

extern "C" int ms_keccak_rows(ms_ctx* ctx, int variant, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    KeccakCommit t;
    MSCHK(keccak_variant("ms_keccak_rows", variant, &t));
    return mscommit::rows(ctx, t, "ms_keccak_rows", field, nrows, d_cols, ncols, d_leaves);
}
extern "C" int ms_keccak_rows_row_major(ms_ctx* ctx, int variant, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    KeccakCommit t;
    MSCHK(keccak_variant("ms_keccak_rows_row_major", variant, &t));
    return mscommit::rows_row_major(ctx, t, "ms_keccak_rows_row_major", field, nrows, ncols, d_matrix, d_leaves);
}
extern "C" int ms_keccak_merkle(ms_ctx* ctx, int variant, size_t nleaves, const void* d_leaves, void* d_nodes) {
    KeccakCommit t;
    MSCHK(keccak_variant("ms_keccak_merkle", variant, &t));
    return mscommit::merkle(ctx, t, "ms_keccak_merkle", nleaves, d_leaves, d_nodes);
}
extern "C" int ms_keccak_pow_grind(ms_ctx* ctx, int variant, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    KeccakCommit t;
    MSCHK(keccak_variant("ms_keccak_pow_grind", variant, &t));
    return mscommit::pow_grind(ctx, t, "ms_keccak_pow_grind", h_seed32, bits, max_nonce, nonce);
}
