// Keccak-256 / SHA3-256 commitments and proof-of-work grinding: the entry points of ms_blake2s.cpp with H = the Keccak sponge and the
// domain byte chosen by `variant` (src/hash.rs:9-41, src/merkle.rs:296-361, 412-508, src/random.rs:48-58, 61-141; kernels in
// keccak_kernels.h; declarations in include/ministark_hip_keccak.h).
#include "ms_internal.h"
#include "../../include/ministark_hip_keccak.h"
#include "keccak_kernels.h"

static int keccak_domain(const char* entry, int variant, uint32_t* domain) {
    if (variant == MS_KECCAK256) { *domain = mskec::DOMAIN_KECCAK; return MS_OK; }
    if (variant == MS_SHA3_256) { *domain = mskec::DOMAIN_SHA3; return MS_OK; }
    return fail(MS_ERR_INVALID, "%s: unknown variant %d (MS_KECCAK256 = 0, MS_SHA3_256 = 1)", entry, variant);
}

static int keccak_rows_launch(ms_ctx* ctx, unsigned V, mskec::RowsParams& P) {
    const size_t nrows = P.nrows;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "keccak_rows", (double)nrows * P.ncols * V * 8 + 32.0 * nrows);
        const dim3 grid((unsigned)((nrows + mskec::NT - 1) / mskec::NT)), block(mskec::NT);
        if (V == 1) hipLaunchKernelGGL(mskec::keccak_rows<1>, grid, block, 0, ctx->stream, P);
        else if (V == 3) hipLaunchKernelGGL(mskec::keccak_rows<3>, grid, block, 0, ctx->stream, P);
        else hipLaunchKernelGGL(mskec::keccak_rows<4>, grid, block, 0, ctx->stream, P);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_keccak_rows(ms_ctx* ctx, int variant, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    if (!ctx || (!d_cols && ncols) || !d_leaves) return fail(MS_ERR_INVALID, "ms_keccak_rows: null argument");
    mskec::RowsParams P;
    memset(&P, 0, sizeof P);
    MSCHK(keccak_domain("ms_keccak_rows", variant, &P.domain));
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols > (unsigned)mskec::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "at most %d columns per commitment", mskec::MAXCOLS);
    for (unsigned c = 0; c < ncols; c++)
        if (!d_cols[c]) return fail(MS_ERR_INVALID, "ms_keccak_rows: null column %u", c);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_cols(ctx, "ms_keccak_rows", "d_cols", field, nrows, d_cols, ncols));
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_cols[c];
    P.leaves = (uint8_t*)d_leaves; P.nrows = nrows; P.ncols = ncols; P.row_stride = V;
    return keccak_rows_launch(ctx, V, P);
}

extern "C" int ms_keccak_rows_row_major(ms_ctx* ctx, int variant, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    if (!ctx || !d_matrix || !d_leaves) return fail(MS_ERR_INVALID, "ms_keccak_rows_row_major: null argument");
    mskec::RowsParams P;
    memset(&P, 0, sizeof P);
    MSCHK(keccak_domain("ms_keccak_rows_row_major", variant, &P.domain));
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols == 0 || ncols > (unsigned)mskec::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "1..%d columns per row", mskec::MAXCOLS);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_rows(ctx, "ms_keccak_rows_row_major", "d_matrix", field, nrows, ncols, d_matrix));
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_matrix + (size_t)c * V;
    P.leaves = (uint8_t*)d_leaves; P.nrows = nrows; P.ncols = ncols; P.row_stride = ncols * V;
    return keccak_rows_launch(ctx, V, P);
}

// the level / subtree split of ms_blake2s_merkle: level launches above 2^17 parents, then subtrees of NT parents climbed in LDS
extern "C" int ms_keccak_merkle(ms_ctx* ctx, int variant, size_t nleaves, const void* d_leaves, void* d_nodes) {
    if (!ctx || !d_leaves || !d_nodes) return fail(MS_ERR_INVALID, "ms_keccak_merkle: null argument");
    uint32_t domain = 0;
    MSCHK(keccak_domain("ms_keccak_merkle", variant, &domain));
    if (nleaves < 2 || (nleaves & (nleaves - 1))) return fail(MS_ERR_INVALID, "number of leaves must be a power of two >= 2");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t* nodes = (uint8_t*)d_nodes;                       // (nodes[0] is cleared by the launch that writes the root)
    const uint8_t* src = (const uint8_t*)d_leaves;
    const size_t NT = mskec::NT;
    for (size_t count = nleaves / 2; count >= 1;) {
        uint8_t* dst = nodes + count * 32;
        if (count <= NT) {                                     // the remaining levels in one launch
            ProfScope ps(ctx, "keccak_merkle_top", 96.0 * (2 * count - 1));
            hipLaunchKernelGGL(mskec::keccak_merkle_top<1>, dim3(1), dim3(mskec::NT), 0, ctx->stream, src, nodes, (unsigned)count, domain);
            break;
        }
        if (count <= ((size_t)1 << 17)) {                      // log2(NT) + 1 levels at once: count / NT subtrees, one workgroup each
            const unsigned per = nleaves <= ((size_t)1 << 21) && count / NT > 256 && count % (2 * NT) == 0 ? 2u : 1u;
            ProfScope ps(ctx, "keccak_merkle_top", 96.0 * (2 * count - count / (per * NT)));
            if (per == 2) hipLaunchKernelGGL(mskec::keccak_merkle_top<2>, dim3((unsigned)(count / (2 * NT))), dim3(mskec::NT), 0, ctx->stream, src, nodes, (unsigned)count, domain);
            else hipLaunchKernelGGL(mskec::keccak_merkle_top<1>, dim3((unsigned)(count / NT)), dim3(mskec::NT), 0, ctx->stream, src, nodes, (unsigned)count, domain);
            const size_t last = count / (per * NT);            // the level the subtrees end in
            src = nodes + last * 32;
            count = last / 2;
            continue;
        }
        ProfScope ps(ctx, "keccak_merkle_level", 96.0 * count);
        hipLaunchKernelGGL(mskec::keccak_merge_level, dim3((unsigned)((count + NT - 1) / NT)), dim3(mskec::NT), 0, ctx->stream, src, dst, count, domain);
        src = dst;
        count >>= 1;
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_keccak_pow_grind(ms_ctx* ctx, int variant, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    if (!ctx || !h_seed32 || !nonce) return fail(MS_ERR_INVALID, "ms_keccak_pow_grind: null argument");
    mskec::PowParams P;
    MSCHK(keccak_domain("ms_keccak_pow_grind", variant, &P.domain));
    if (bits > 64) return fail(MS_ERR_INVALID, "proof-of-work bits must be <= 64");
    void* d_found = nullptr;
    PoolGuard pooled(ctx);                                 // temporaries go back to the pool on every exit path
    MSCHK(pooled.alloc(8, &d_found));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
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
            ProfScope ps(ctx, "keccak_pow_grind", 0.0);
            hipLaunchKernelGGL(mskec::keccak_pow_grind, dim3((unsigned)((P.count + mskec::NT - 1) / mskec::NT)), dim3(mskec::NT), 0, ctx->stream, P);
        }
        if (hipMemcpyAsync(&found, d_found, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = fail(MS_ERR_HIP, "pow: readback"); break; }
        if (found != none) break;
    }
    if (rc != MS_OK) return rc;
    if (found == none) return fail(MS_ERR_INVALID, "no nonce below %llu has %u leading zero bits", (unsigned long long)max_nonce, bits);
    *nonce = found;
    return MS_OK;
}
