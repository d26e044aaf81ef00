// Starknet's Poseidon over the 252-bit field: the bulk permutation and the commitments built on it -- a sponge over the rows of a
// matrix (either layout, one kernel through a row stride), the two-to-one hash of a Merkle level, and the levels of at most
// mspos::TOP nodes in one launch.  Digests are Fp252 elements, so, like RPO-256 (ms_hash.cpp), this is not one of commit_host.h's byte
// hashes.  Kernels: poseidon252_kernels.h; declarations: include/ministark_hip_poseidon.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_poseidon.h"
#include "poseidon252_kernels.h"

static inline dim3 pos_blocks(size_t n) { return dim3((unsigned)((n + mspos::NT - 1) / mspos::NT)); }

extern "C" int ms_poseidon252_permute(ms_ctx* ctx, size_t n, const void* d_in, void* d_out) {
    if (!ctx || !d_in || !d_out) return fail(MS_ERR_INVALID, "ms_poseidon252_permute: null argument");
    if (d_in != d_out && ranges_overlap(d_in, n * 96, d_out, n * 96))
        return fail(MS_ERR_INVALID, "ms_poseidon252_permute: d_in and d_out overlap without being the same buffer");
    if (n == 0) return MS_OK;
    MSCHK(canon_rows(ctx, "ms_poseidon252_permute", "d_in", MS_STARK252_FP, n, 3, d_in));       // a state is a row of three elements
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    ProfScope ps(ctx, "poseidon252_permute", 192.0 * n);
    hipLaunchKernelGGL(mspos::poseidon252_permute, pos_blocks(n), dim3(mspos::NT), 0, ctx->stream, (const uint64_t*)d_in, (uint64_t*)d_out, n);
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// `stride`: elements between the rows of one column
static int poseidon_rows(ms_ctx* ctx, size_t nrows, mspos::RowsParams& P, unsigned ncols, unsigned stride, void* d_leaves) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    P.leaves = (uint64_t*)d_leaves; P.nrows = nrows; P.ncols = ncols; P.row_stride = stride;
    ProfScope ps(ctx, "poseidon252_rows", 32.0 * nrows * (ncols + 1));
    hipLaunchKernelGGL(mspos::poseidon252_rows, pos_blocks(nrows), dim3(mspos::NT), 0, ctx->stream, P);
    HIPCHK(hipGetLastError());
    return MS_OK;
}
extern "C" int ms_poseidon252_rows(ms_ctx* ctx, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    if (!ctx || (!d_cols && ncols) || !d_leaves) return fail(MS_ERR_INVALID, "ms_poseidon252_rows: null argument");
    if (ncols > (unsigned)mspos::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "at most %d columns per commitment", mspos::MAXCOLS);
    for (unsigned c = 0; c < ncols; c++)
        if (!d_cols[c]) return fail(MS_ERR_INVALID, "ms_poseidon252_rows: null column %u", c);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_cols(ctx, "ms_poseidon252_rows", "d_cols", MS_STARK252_FP, nrows, d_cols, ncols));
    mspos::RowsParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_cols[c];
    return poseidon_rows(ctx, nrows, P, ncols, 1, d_leaves);
}
extern "C" int ms_poseidon252_rows_row_major(ms_ctx* ctx, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    if (!ctx || !d_matrix || !d_leaves) return fail(MS_ERR_INVALID, "ms_poseidon252_rows_row_major: null argument");
    if (ncols == 0 || ncols > (unsigned)mspos::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "1..%d columns per row", mspos::MAXCOLS);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_rows(ctx, "ms_poseidon252_rows_row_major", "d_matrix", MS_STARK252_FP, nrows, ncols, d_matrix));
    mspos::RowsParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_matrix + 4 * (size_t)c;
    return poseidon_rows(ctx, nrows, P, ncols, ncols, d_leaves);
}

// one launch per level above mspos::TOP parents, then ONE launch for every level of at most TOP parents (2 TOP - 1 nodes, nine levels)
extern "C" int ms_poseidon252_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes) {
    if (!ctx || !d_leaves || !d_nodes) return fail(MS_ERR_INVALID, "ms_poseidon252_merkle: null argument");
    if (nleaves < 2 || (nleaves & (nleaves - 1))) return fail(MS_ERR_INVALID, "number of leaves must be a power of two >= 2");
    MSCHK(canon_rows(ctx, "ms_poseidon252_merkle", "d_leaves", MS_STARK252_FP, nleaves, 1, d_leaves));     // a digest is one element
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t* nodes = (uint64_t*)d_nodes;
    HIPCHK(hipMemsetAsync(nodes, 0, 32, ctx->stream));
    const uint64_t* src = (const uint64_t*)d_leaves;
    size_t count = nleaves / 2;
    for (; count > mspos::TOP; count >>= 1) {
        uint64_t* dst = nodes + 4 * count;
        ProfScope ps(ctx, "poseidon252_merkle_level", 96.0 * count);
        hipLaunchKernelGGL(mspos::poseidon252_merge_level, pos_blocks(count), dim3(mspos::NT), 0, ctx->stream, src, dst, count);
        src = dst;
    }
    {
        ProfScope ps(ctx, "poseidon252_merkle_top", 96.0 * (2 * count - 1));
        hipLaunchKernelGGL(mspos::poseidon252_merkle_top, dim3(1), dim3(mspos::TOP), 0, ctx->stream, src, nodes, (unsigned)count);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}
