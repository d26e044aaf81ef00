// BLAKE2s-256 commitments and proof-of-work grinding: the entry points of ms_hash.cpp's SHA-256 twins, with H = BLAKE2s
// (src/hash.rs:9-41, src/merkle.rs:296-361, src/random.rs:61-141; kernels in blake2s_kernels.h).
#include "ms_internal.h"
#include "blake2s_kernels.h"

static int blake2s_rows_launch(ms_ctx* ctx, unsigned V, msb2s::RowsParams& P) {
    const size_t nrows = P.nrows;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "blake2s_rows", (double)nrows * P.ncols * V * 8 + 32.0 * nrows);
        const dim3 grid((unsigned)((nrows + msb2s::NT - 1) / msb2s::NT)), block(msb2s::NT);
        if (V == 1) hipLaunchKernelGGL(msb2s::blake2s_rows<1>, grid, block, 0, ctx->stream, P);
        else if (V == 3) hipLaunchKernelGGL(msb2s::blake2s_rows<3>, grid, block, 0, ctx->stream, P);
        else hipLaunchKernelGGL(msb2s::blake2s_rows<4>, grid, block, 0, ctx->stream, P);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_blake2s_rows(ms_ctx* ctx, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    if (!ctx || (!d_cols && ncols) || !d_leaves) return fail(MS_ERR_INVALID, "ms_blake2s_rows: null argument");
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols > (unsigned)msb2s::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "at most %d columns per commitment", msb2s::MAXCOLS);
    for (unsigned c = 0; c < ncols; c++)
        if (!d_cols[c]) return fail(MS_ERR_INVALID, "ms_blake2s_rows: null column %u", c);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_cols(ctx, "ms_blake2s_rows", "d_cols", field, nrows, d_cols, ncols));
    msb2s::RowsParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_cols[c];
    P.leaves = (uint8_t*)d_leaves; P.nrows = nrows; P.ncols = ncols; P.row_stride = V;
    return blake2s_rows_launch(ctx, V, P);
}

extern "C" int ms_blake2s_rows_row_major(ms_ctx* ctx, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    if (!ctx || !d_matrix || !d_leaves) return fail(MS_ERR_INVALID, "ms_blake2s_rows_row_major: null argument");
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols == 0 || ncols > (unsigned)msb2s::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "1..%d columns per row", msb2s::MAXCOLS);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_rows(ctx, "ms_blake2s_rows_row_major", "d_matrix", field, nrows, ncols, d_matrix));
    msb2s::RowsParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_matrix + (size_t)c * V;
    P.leaves = (uint8_t*)d_leaves; P.nrows = nrows; P.ncols = ncols; P.row_stride = ncols * V;
    return blake2s_rows_launch(ctx, V, P);
}

// the level / subtree split of ms_sha256_merkle: level launches above 2^17 parents, then subtrees of NT parents climbed in LDS
extern "C" int ms_blake2s_merkle(ms_ctx* ctx, size_t nleaves, const void* d_leaves, void* d_nodes) {
    if (!ctx || !d_leaves || !d_nodes) return fail(MS_ERR_INVALID, "ms_blake2s_merkle: null argument");
    if (nleaves < 2 || (nleaves & (nleaves - 1))) return fail(MS_ERR_INVALID, "number of leaves must be a power of two >= 2");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t* nodes = (uint8_t*)d_nodes;                       // (nodes[0] is cleared by the launch that writes the root)
    const uint8_t* src = (const uint8_t*)d_leaves;
    const size_t NT = msb2s::NT;
    for (size_t count = nleaves / 2; count >= 1;) {
        uint8_t* dst = nodes + count * 32;
        if (count <= NT) {                                     // the remaining levels in one launch
            ProfScope ps(ctx, "blake2s_merkle_top", 96.0 * (2 * count - 1));
            hipLaunchKernelGGL(msb2s::blake2s_merkle_top<1>, dim3(1), dim3(msb2s::NT), 0, ctx->stream, src, nodes, (unsigned)count);
            break;
        }
        if (count <= ((size_t)1 << 17)) {                      // log2(NT) + 1 levels at once: count / NT subtrees, one workgroup each
            const unsigned per = nleaves <= ((size_t)1 << 21) && count / NT > 256 && count % (2 * NT) == 0 ? 2u : 1u;
            ProfScope ps(ctx, "blake2s_merkle_top", 96.0 * (2 * count - count / (per * NT)));
            if (per == 2) hipLaunchKernelGGL(msb2s::blake2s_merkle_top<2>, dim3((unsigned)(count / (2 * NT))), dim3(msb2s::NT), 0, ctx->stream, src, nodes, (unsigned)count);
            else hipLaunchKernelGGL(msb2s::blake2s_merkle_top<1>, dim3((unsigned)(count / NT)), dim3(msb2s::NT), 0, ctx->stream, src, nodes, (unsigned)count);
            const size_t last = count / (per * NT);            // the level the subtrees end in
            src = nodes + last * 32;
            count = last / 2;
            continue;
        }
        ProfScope ps(ctx, "blake2s_merkle_level", 96.0 * count);
        hipLaunchKernelGGL(msb2s::blake2s_merge_level, dim3((unsigned)((count + NT - 1) / NT)), dim3(msb2s::NT), 0, ctx->stream, src, dst, count);
        src = dst;
        count >>= 1;
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_blake2s_pow_grind(ms_ctx* ctx, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    if (!ctx || !h_seed32 || !nonce) return fail(MS_ERR_INVALID, "ms_blake2s_pow_grind: null argument");
    if (bits > 64) return fail(MS_ERR_INVALID, "proof-of-work bits must be <= 64");
    void* d_found = nullptr;
    PoolGuard pooled(ctx);                                 // temporaries go back to the pool on every exit path
    MSCHK(pooled.alloc(8, &d_found));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    msb2s::PowParams P;
    const uint8_t* sb = (const uint8_t*)h_seed32;
    for (int q = 0; q < 8; q++) P.seed[q] = sb[4 * q] | ((uint32_t)sb[4 * q + 1] << 8) | ((uint32_t)sb[4 * q + 2] << 16) | ((uint32_t)sb[4 * q + 3] << 24);
    P.bits = bits; P.found = (unsigned long long*)d_found;
    unsigned long long window = 1ull << 12;             // grows to 2^24 nonces per launch
    unsigned long long none = ~0ull, found = ~0ull;
    int rc = MS_OK;
    for (unsigned long long base = 1; base <= max_nonce && rc == MS_OK; base += P.count, window = std::min(window * 4, 1ull << 24)) {
        P.base = base; P.count = std::min<unsigned long long>(window, max_nonce - base + 1);
        if (hipMemcpyAsync(d_found, &none, 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = fail(MS_ERR_HIP, "pow: memcpy"); break; }
        {
            ProfScope ps(ctx, "blake2s_pow_grind", 0.0);
            hipLaunchKernelGGL(msb2s::blake2s_pow_grind, dim3((unsigned)((P.count + msb2s::NT - 1) / msb2s::NT)), dim3(msb2s::NT), 0, ctx->stream, P);
        }
        if (hipMemcpyAsync(&found, d_found, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = fail(MS_ERR_HIP, "pow: readback"); break; }
        if (found != none) break;
    }
    if (rc != MS_OK) return rc;
    if (found == none) return fail(MS_ERR_INVALID, "no nonce below %llu has %u leading zero bits", (unsigned long long)max_nonce, bits);
    *nonce = found;
    return MS_OK;
}
