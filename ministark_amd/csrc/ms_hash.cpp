// SHA-256 and RPO-256 commitments, proof-of-work grinding (src/merkle.rs:412-508, src/hash.rs:58-100, gpu/src/plan.rs:32-174,
// src/channel.rs:76-93).  The SHA-256 host logic is commit_host.h's, shared with BLAKE2s and Keccak; RPO-256 is a different shape
// (digests of field elements, no LDS top) and keeps its own.
#include "ms_internal.h"
#include "commit_host.h"
#include "sha256_kernels.h"
#include "rpo_kernels.h"

// ---------------------------------------------------------------------------------------
// SHA-256 commitments and proof-of-work: the traits of commit_host.h and the four entry points
// ---------------------------------------------------------------------------------------
namespace {
struct Sha256Commit {
    using RowsParams = mssha::RowsParams;
    using PowParams = mssha::PowParams;
    static constexpr int NT = mssha::NT, MAXCOLS = mssha::MAXCOLS;
    static constexpr bool SEED_BIG_ENDIAN = true;
    static constexpr const char *ROWS = "sha256_rows", *LEVEL = "sha256_merkle_level", *TOP = "sha256_merkle_top", *GRIND = "sha256_pow_grind";
    // the kernel reads V at run time; a row that is a whole number of blocks ends in a constant padding block, folded into round constants
    void rows_hook(RowsParams& P, unsigned V) const {
        P.V = V;
        if (P.ncols && (P.ncols * V) % 8 == 0) { P.fold_last = 1; mssha::sha256_fold_pad_block((uint64_t)P.ncols * V * 64, P.kw_last); }
    }
    void pow_hook(PowParams&) const {}
    // V is ignored: sha256_rows takes it from P.V, so the three instantiations that rows_launch names are the same launch
    template <int V> void launch_rows(dim3 grid, dim3 block, hipStream_t st, const RowsParams& P) const { hipLaunchKernelGGL(mssha::sha256_rows, grid, block, 0, st, P); }
    void launch_level(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* dst, size_t count) const { hipLaunchKernelGGL(mssha::sha256_merge_level, grid, block, 0, st, src, dst, count); }
    template <int PER> void launch_top(dim3 grid, dim3 block, hipStream_t st, const uint8_t* src, uint8_t* nodes, unsigned count) const { hipLaunchKernelGGL(mssha::sha256_merkle_top<PER>, grid, block, 0, st, src, nodes, count); }
    void launch_grind(dim3 grid, dim3 block, hipStream_t st, const PowParams& P) const { hipLaunchKernelGGL(mssha::sha256_pow_grind, grid, block, 0, st, P); }
};
}  // namespace

extern "C" int ms_sha256_rows(ms_ctx* ctx, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    return mscommit::rows(ctx, Sha256Commit{}, "ms_sha256_rows", field, nrows, d_cols, ncols, d_leaves);
}
extern "C" int ms_sha256_rows_row_major(ms_ctx* ctx, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    return mscommit::rows_row_major(ctx, Sha256Commit{}, "ms_sha256_rows_row_major", field, nrows, ncols, d_matrix, d_leaves);
}
extern "C" int ms_sha256_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes) {
    return mscommit::merkle(ctx, Sha256Commit{}, "ms_sha256_merkle", nleaves, d_leaves, d_nodes);
}
extern "C" int ms_sha256_pow_grind(ms_ctx* ctx, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    return mscommit::pow_grind(ctx, Sha256Commit{}, "ms_sha256_pow_grind", h_seed32, bits, max_nonce, nonce);
}

// ---------------------------------------------------------------------------------------
// RPO-256 commitments
// ---------------------------------------------------------------------------------------
static int rpo_rows(ms_ctx* ctx, size_t nrows, const uint64_t* const* cols, unsigned ncols, unsigned stride, void* d_digests) {
    if (ncols == 0) return fail(MS_ERR_INVALID, "the zero-length input is not allowed");          // plan.rs:72
    if (ncols > (unsigned)msrpo::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "at most %d columns per commitment", msrpo::MAXCOLS);
    if (nrows == 0) return MS_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    msrpo::RowsParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = cols[c];
    P.digests = (uint64_t*)d_digests; P.nrows = nrows; P.ncols = ncols; P.row_stride = stride;
    ProfScope ps(ctx, "rpo256_rows", 8.0 * nrows * (ncols + 4));
    hipLaunchKernelGGL(msrpo::rpo256_rows, dim3((unsigned)((nrows + msrpo::NT - 1) / msrpo::NT)), dim3(msrpo::NT), 0, ctx->stream, P);
    HIPCHK(hipGetLastError());
    return MS_OK;
}
extern "C" int ms_rpo256_rows(ms_ctx* ctx, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_digests) {
    if (!ctx || !d_cols || !d_digests) return fail(MS_ERR_INVALID, "ms_rpo256_rows: null argument");
    if (ncols && ncols <= (unsigned)msrpo::MAXCOLS) MSCHK(canon_cols(ctx, "ms_rpo256_rows", "d_cols", MS_GOLDILOCKS_FP, nrows, d_cols, ncols));
    std::vector<const uint64_t*> cols(ncols);
    for (unsigned c = 0; c < ncols; c++) {
        if (!d_cols[c]) return fail(MS_ERR_INVALID, "null column %u", c);        // (canon_cols scans nothing when a column is null)
        cols[c] = (const uint64_t*)d_cols[c];
    }
    return rpo_rows(ctx, nrows, cols.data(), ncols, 1, d_digests);
}
// rows of a column-major matrix of `field`: an Fq3 column contributes its components c0, c1, c2 in the order
// the SHA-256 leaves serialise them (src/hash.rs:93-98) -- the column pointers are simply taken at word stride 3
extern "C" int ms_rpo256_rows_field(ms_ctx* ctx, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_digests) {
    if (!ctx || !d_cols || !d_digests) return fail(MS_ERR_INVALID, "ms_rpo256_rows_field: null argument");
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V != 1 && V != 3) return fail(MS_ERR_UNSUPPORTED, "RPO-256 absorbs Goldilocks elements (Fp or Fq3 columns)");
    if (ncols && ncols * V <= (unsigned)msrpo::MAXCOLS) MSCHK(canon_cols(ctx, "ms_rpo256_rows_field", "d_cols", field, nrows, d_cols, ncols));
    std::vector<const uint64_t*> cols;
    for (unsigned c = 0; c < ncols; c++) {
        if (!d_cols[c]) return fail(MS_ERR_INVALID, "null column %u", c);
        for (unsigned k = 0; k < V; k++) cols.push_back((const uint64_t*)d_cols[c] + k);
    }
    return rpo_rows(ctx, nrows, cols.data(), (unsigned)cols.size(), V, d_digests);
}
extern "C" int ms_rpo256_rows_row_major(ms_ctx* ctx, size_t nrows, unsigned ncols, const void* d_matrix, void* d_digests) {
    if (!ctx || !d_matrix || !d_digests) return fail(MS_ERR_INVALID, "ms_rpo256_rows_row_major: null argument");
    if (ncols && ncols <= (unsigned)msrpo::MAXCOLS) MSCHK(canon_rows(ctx, "ms_rpo256_rows_row_major", "d_matrix", MS_GOLDILOCKS_FP, nrows, ncols, d_matrix));
    std::vector<const uint64_t*> cols(ncols);
    for (unsigned c = 0; c < ncols; c++) cols[c] = (const uint64_t*)d_matrix + c;
    return rpo_rows(ctx, nrows, cols.data(), ncols, ncols, d_digests);
}
extern "C" int ms_rpo256_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes) {
    if (!ctx || !d_leaves || !d_nodes) return fail(MS_ERR_INVALID, "ms_rpo256_merkle: null argument");
    if (nleaves < 2 || (nleaves & (nleaves - 1))) return fail(MS_ERR_INVALID, "number of leaves must be a power of two >= 2");
    MSCHK(canon_rows(ctx, "ms_rpo256_merkle", "d_leaves", MS_GOLDILOCKS_FP, nleaves, 4, d_leaves));      // a digest is a row of four Fp elements
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t* nodes = (uint64_t*)d_nodes;
    HIPCHK(hipMemsetAsync(nodes, 0, 32, ctx->stream));
    const uint64_t* src = (const uint64_t*)d_leaves;
    for (size_t count = nleaves / 2; count >= 1; count >>= 1) {
        uint64_t* dst = nodes + count * 4;
        ProfScope ps(ctx, "rpo256_merkle_level", 96.0 * count);
        if (count <= ((size_t)1 << 15))      // few nodes: sixteen lanes per node (latency of one element's chains, not of twelve)
            hipLaunchKernelGGL(msrpo::rpo256_merge_level_wide, dim3((unsigned)((count + 3) / 4)), dim3(msrpo::NTW), 0, ctx->stream, src, dst, count);
        else
            hipLaunchKernelGGL(msrpo::rpo256_merge_level, dim3((unsigned)((count + msrpo::NT - 1) / msrpo::NT)), dim3(msrpo::NT), 0, ctx->stream, src, dst, count);
        src = dst;
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}
