// The host side of a byte-hash commitment, written once: row hashing in its two layouts, the Merkle level / subtree schedule and the
// windowed proof-of-work search.  ms_hash.cpp (SHA-256), ms_blake2s.cpp and ms_keccak.cpp each supply a traits object T and four thin
// extern "C" wrappers; ms_coin.cpp uses the search alone.  T holds what really differs between the hashes:
//   NT, MAXCOLS, RowsParams, PowParams      the constants and launch structures of the hash's kernel header
//   ROWS, LEVEL, TOP, GRIND                 the ProfScope labels
//   SEED_BIG_ENDIAN                         the byte order of PowParams::seed[]'s words
//   rows_hook(P, V), pow_hook(P)            what the hash adds to the common fill (SHA-256: V and the folded last block; Keccak: domain)
//   launch_rows<V>, launch_level, launch_top<PER>, launch_grind     the kernel launches (Keccak's carry the domain byte; SHA-256's rows
//                                           kernel reads V at run time, so its three launch_rows<V> are one launch)
// Host-only: no kernel lives here.  `entry` is the entry point's name, for the error strings.
#pragma once
#include "ms_internal.h"

namespace mscommit {

static inline dim3 blocks_of(unsigned long long n, unsigned nt) { return dim3((unsigned)((n + nt - 1) / nt)); }

// the common tail of the two row layouts: P.cols[], P.row_stride and the counts are set; one launch, one ProfScope
template <class T>
static int rows_launch(ms_ctx* ctx, const T& t, unsigned V, typename T::RowsParams& P, void* d_leaves, size_t nrows, unsigned ncols) {
    P.leaves = (uint8_t*)d_leaves; P.nrows = nrows; P.ncols = ncols;
    t.rows_hook(P, V);
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, T::ROWS, (double)nrows * ncols * V * 8 + 32.0 * nrows);
        const dim3 grid = blocks_of(nrows, T::NT), block(T::NT);
        if (V == 1) t.template launch_rows<1>(grid, block, ctx->stream, P);
        else if (V == 3) t.template launch_rows<3>(grid, block, ctx->stream, P);
        else t.template launch_rows<4>(grid, block, ctx->stream, P);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// leaf[r] = H(the canonical bytes of row r) of a column-major matrix: d_cols[c] is column c, dense
template <class T>
static int rows(ms_ctx* ctx, const T& t, const char* entry, int field, size_t nrows, const void* const* d_cols, unsigned ncols, void* d_leaves) {
    if (!ctx || (!d_cols && ncols) || !d_leaves) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols > (unsigned)T::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "at most %d columns per commitment", T::MAXCOLS);
    for (unsigned c = 0; c < ncols; c++)
        if (!d_cols[c]) return fail(MS_ERR_INVALID, "%s: null column %u", entry, c);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_cols(ctx, entry, "d_cols", field, nrows, d_cols, ncols));
    typename T::RowsParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_cols[c];
    P.row_stride = V;
    return rows_launch(ctx, t, V, P, d_leaves, nrows, ncols);
}

// the same leaves from a row-major matrix of nrows x ncols elements (a FRI layer): column c starts at element c
template <class T>
static int rows_row_major(ms_ctx* ctx, const T& t, const char* entry, int field, size_t nrows, unsigned ncols, const void* d_matrix, void* d_leaves) {
    if (!ctx || !d_matrix || !d_leaves) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols == 0 || ncols > (unsigned)T::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "1..%d columns per row", T::MAXCOLS);
    if (nrows == 0) return MS_OK;
    MSCHK(canon_rows(ctx, entry, "d_matrix", field, nrows, ncols, d_matrix));
    typename T::RowsParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) P.cols[c] = (const uint64_t*)d_matrix + (size_t)c * V;
    P.row_stride = ncols * V;
    return rows_launch(ctx, t, V, P, d_leaves, nrows, ncols);
}

// nodes[k] = H(nodes[2k] || nodes[2k+1]): level launches above 2^17 parents, then subtrees of NT parents climbed in LDS, one closing launch
template <class T>
static int merkle(ms_ctx* ctx, const T& t, const char* entry, size_t nleaves, const void* d_leaves, void* d_nodes) {
    if (!ctx || !d_leaves || !d_nodes) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    if (nleaves < 2 || (nleaves & (nleaves - 1))) return fail(MS_ERR_INVALID, "number of leaves must be a power of two >= 2");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t* nodes = (uint8_t*)d_nodes;                       // (nodes[0] is cleared by the launch that writes the root: the top kernel)
    const uint8_t* src = (const uint8_t*)d_leaves;
    const size_t NT = T::NT;
    const dim3 block(T::NT);
    for (size_t count = nleaves / 2; count >= 1;) {
        uint8_t* dst = nodes + count * 32;
        if (count <= NT) {                                     // the remaining levels in one launch
            ProfScope ps(ctx, T::TOP, 96.0 * (2 * count - 1));
            t.template launch_top<1>(dim3(1), block, ctx->stream, src, nodes, (unsigned)count);
            break;
        }
        if (count <= ((size_t)1 << 17)) {                      // log2(NT) + 1 levels at once: count / NT subtrees, one workgroup each
            // more subtrees than CUs: two parents per lane, so that every wave keeps a SIMD to itself (sha256_kernels.h)
            // Measured per SHA-256 tree (scripts/merkle_top_probe.py, same box): 2^18 leaves 123 -> 105 us, 2^21 120 -> 108; 2^23 / 2^24 leaves 116 -> 119
            // (after the long level launches of a big tree the 512-workgroup form is the faster one), hence the bound on the tree's size.
            const unsigned per = nleaves <= ((size_t)1 << 21) && count / NT > 256 && count % (2 * NT) == 0 ? 2u : 1u;
            ProfScope ps(ctx, T::TOP, 96.0 * (2 * count - count / (per * NT)));
            if (per == 2) t.template launch_top<2>(dim3((unsigned)(count / (2 * NT))), block, ctx->stream, src, nodes, (unsigned)count);
            else t.template launch_top<1>(dim3((unsigned)(count / NT)), block, ctx->stream, src, nodes, (unsigned)count);
            const size_t last = count / (per * NT);            // the level the subtrees end in
            src = nodes + last * 32;
            count = last / 2;
            continue;
        }
        ProfScope ps(ctx, T::LEVEL, 96.0 * count);
        t.launch_level(blocks_of(count, T::NT), block, ctx->stream, src, dst, count);
        src = dst;
        count >>= 1;
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// The smallest nonce in [1, max_nonce] that a launch reports, searched in windows: 2^12 nonces in the first launch, four times as many in
// the next, up to 2^24.  launch(base, count, found) enqueues one kernel over [base, base + count) that keeps its smallest hit in *found
// with atomicMin; a window costs one 8-byte reset, that launch and one 8-byte readback.
template <class Launch>
static int grind_windows(ms_ctx* ctx, unsigned bits, uint64_t max_nonce, const char* label, Launch launch, uint64_t* nonce) {
    if (bits > 64) return fail(MS_ERR_INVALID, "proof-of-work bits must be <= 64");
    void* d_found = nullptr;
    PoolGuard pooled(ctx);                                 // temporaries go back to the pool on every exit path
    MSCHK(pooled.alloc(8, &d_found));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long window = 1ull << 12, count = 0;
    unsigned long long none = ~0ull, found = ~0ull;
    for (unsigned long long base = 1; base <= max_nonce; base += count, window = std::min(window * 4, 1ull << 24)) {
        count = std::min<unsigned long long>(window, max_nonce - base + 1);
        if (hipMemcpyAsync(d_found, &none, 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail(MS_ERR_HIP, "pow: memcpy");
        {
            ProfScope ps(ctx, label, 0.0);
            launch(base, count, (unsigned long long*)d_found);
        }
        if (hipMemcpyAsync(&found, d_found, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
            return fail(MS_ERR_HIP, "pow: readback");
        if (found != none) break;
    }
    if (found == none) return fail(MS_ERR_INVALID, "no nonce below %llu has %u leading zero bits", (unsigned long long)max_nonce, bits);
    *nonce = found;
    return MS_OK;
}

// the search over H(seed32 || nonce as 8 big-endian bytes), the seed carried in PowParams
template <class T>
static int pow_grind(ms_ctx* ctx, const T& t, const char* entry, const void* h_seed32, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    if (!ctx || !h_seed32 || !nonce) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    typename T::PowParams P;
    const uint8_t* sb = (const uint8_t*)h_seed32;
    for (int q = 0; q < 8; q++) {
        const uint32_t le = sb[4 * q] | ((uint32_t)sb[4 * q + 1] << 8) | ((uint32_t)sb[4 * q + 2] << 16) | ((uint32_t)sb[4 * q + 3] << 24);
        P.seed[q] = T::SEED_BIG_ENDIAN ? __builtin_bswap32(le) : le;
    }
    P.bits = bits;
    t.pow_hook(P);
    return grind_windows(ctx, bits, max_nonce, T::GRIND, [&](unsigned long long base, unsigned long long count, unsigned long long* found) {
        P.base = base; P.count = count; P.found = found;
        t.launch_grind(blocks_of(count, T::NT), dim3(T::NT), ctx->stream, P);
    }, nonce);
}

}  // namespace mscommit
