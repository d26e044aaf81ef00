// BLAKE2s-256 commitments and proof-of-work grinding (src/hash.rs:9-41, src/merkle.rs:296-361, src/random.rs:61-141): the traits of
// commit_host.h, which holds the host logic of every byte hash, and the four entry points.  Kernels: blake2s_kernels.h.
#include "ms_internal.h"
#include "commit_host.h"
#include "blake2s_kernels.h"

namespace {
struct Blake2sCommit {
    using RowsParams = msb2s::RowsParams;
    using PowParams = msb2s::PowParams;
    static constexpr int NT = msb2s::NT, MAXCOLS = msb2s::MAXCOLS;
    static constexpr bool SEED_BIG_ENDIAN = false;
    static constexpr const char *ROWS = "blake2s_rows", *LEVEL = "blake2s_merkle_level", *TOP = "blake2s_merkle_top", *GRIND = "blake2s_pow_grind";
    void rows_hook(RowsParams&, unsigned) const {}
    void pow_hook(PowParams&) const {}
    template <int V> void launch_rows(dim3 grid, dim3 block, hipStream_t st, const RowsParams& P) const { hipLaunchKernelGGL(msb2s::blake2s_rows<V>, grid, block, 0, st, P); }
    void launch_level(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* dst, size_t count) const { hipLaunchKernelGGL(msb2s::blake2s_merge_level, grid, block, 0, st, src, dst, count); }
    template <int PER> void launch_top(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* nodes, unsigned count) const { hipLaunchKernelGGL(msb2s::blake2s_merkle_top<PER>, grid, block, 0, st, src, nodes, count); }
    void launch_grind(dim3 grid, dim3 block, hipStream_t st, const PowParams& P) const { hipLaunchKernelGGL(msb2s::blake2s_pow_grind, grid, block, 0, st, P); }
};
}  // namespace

extern "C" int ms_blake2s_rows(ms_ctx* ctx, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    return mscommit::rows(ctx, Blake2sCommit{}, "ms_blake2s_rows", field, nrows, d_cols, ncols, d_leaves);
}
extern "C" int ms_blake2s_rows_row_major(ms_ctx* ctx, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    return mscommit::rows_row_major(ctx, Blake2sCommit{}, "ms_blake2s_rows_row_major", field, nrows, ncols, d_matrix, d_leaves);
}
extern "C" int ms_blake2s_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes) {
    return mscommit::merkle(ctx, Blake2sCommit{}, "ms_blake2s_merkle", nleaves, d_leaves, d_nodes);
}
extern "C" int ms_blake2s_pow_grind(ms_ctx* ctx, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    return mscommit::pow_grind(ctx, Blake2sCommit{}, "ms_blake2s_pow_grind", h_seed32, bits, max_nonce, nonce);
}
