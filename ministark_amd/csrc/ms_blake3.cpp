// BLAKE3 commitments and proof-of-work grinding (src/hash.rs:9-41, src/merkle.rs:296-361, 412-508, src/random.rs:48-58, 61-141): the
// traits of commit_host.h, which holds the host logic of every byte hash, and the four entry points.  Kernels: blake3_kernels.h;
// declarations: include/ministark_hip_blake3.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_blake3.h"
#include "commit_host.h"
#include "blake3_kernels.h"

namespace {
struct Blake3Commit {
    using RowsParams = msb3::RowsParams;
    using PowParams = msb3::PowParams;
    static constexpr int NT = msb3::NT, MAXCOLS = msb3::MAXCOLS;
    static constexpr bool SEED_BIG_ENDIAN = false;
    static constexpr const char *ROWS = "blake3_rows", *LEVEL = "blake3_merkle_level", *TOP = "blake3_merkle_top", *GRIND = "blake3_pow_grind";
    void rows_hook(RowsParams&, unsigned) const {}
    void pow_hook(PowParams&) const {}
    template <int V> void launch_rows(dim3 grid, dim3 block, hipStream_t st, const RowsParams& P) const { hipLaunchKernelGGL(msb3::blake3_rows<V>, grid, block, 0, st, P); }
    void launch_level(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* dst, size_t count) const { hipLaunchKernelGGL(msb3::blake3_merge_level, grid, block, 0, st, src, dst, count); }
    template <int PER> void launch_top(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* nodes, unsigned count) const { hipLaunchKernelGGL(msb3::blake3_merkle_top<PER>, grid, block, 0, st, src, nodes, count); }
    void launch_grind(dim3 grid, dim3 block, hipStream_t st, const PowParams& P) const { hipLaunchKernelGGL(msb3::blake3_pow_grind, grid, block, 0, st, P); }
};
}  // namespace

extern "C" int ms_blake3_rows(ms_ctx* ctx, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    return mscommit::rows(ctx, Blake3Commit{}, "ms_blake3_rows", field, nrows, d_cols, ncols, d_leaves);
}
extern "C" int ms_blake3_rows_row_major(ms_ctx* ctx, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    return mscommit::rows_row_major(ctx, Blake3Commit{}, "ms_blake3_rows_row_major", field, nrows, ncols, d_matrix, d_leaves);
}
extern "C" int ms_blake3_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes) {
    return mscommit::merkle(ctx, Blake3Commit{}, "ms_blake3_merkle", nleaves, d_leaves, d_nodes);
}
extern "C" int ms_blake3_pow_grind(ms_ctx* ctx, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    return mscommit::pow_grind(ctx, Blake3Commit{}, "ms_blake3_pow_grind", h_seed32, bits, max_nonce, nonce);
}
