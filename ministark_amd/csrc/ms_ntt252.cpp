// The transforms of the 252-bit field: the radix-2 sequence (fp252_kernels.h) and the tiled passes (fp252_ntt_kernels.h) of a plan
// built by ms_ntt_plan.cpp.  The entry points that route here are in ms_ntt.cpp.
#include "ms_internal.h"
#include "fp252_kernels.h"
#include "fp252_ntt_kernels.h"

static_assert(NTT252_TILE_LOG == ms252::TILE_LOG, "plan_build252 gives the tiled passes to every plan of at least one tile");

// Tiled passes (fp252_ntt_kernels.h).  log_zero_ext: the source holds only the first n >> log_zero_ext elements, the rest
// of the domain is implicit zeros (needs 2^log_zero_ext <= R_0); bitrev_out: bit-reversed order, fused into the last pass.
int plan_run252_tiled(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols, unsigned log_zero_ext, bool bitrev_out) {
    ms_ctx* ctx = p->ctx;
    hipStream_t st = ctx->stream;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << p->log_n, col_bytes = n * 32;
    const int np = p->np252;
    if (log_zero_ext > p->lr252[0]) return fail(MS_ERR_INVALID, "internal: zero extension 2^%u beyond the first radix", log_zero_ext);
    unsigned group = (unsigned)std::max<size_t>(1, std::min<size_t>(msntt::MAXC, ctx->group_bytes / col_bytes));
    group = std::min(group, ncols);
    void* scratch = nullptr;
    MSCHK(ctx_scratch(ctx, (size_t)group * col_bytes, &scratch));
    static const char* const names[3] = {"ntt252_pass1", "ntt252_pass2", "ntt252_pass3"};
    if (getenv("MS_NTT_DEBUG"))
        fprintf(stderr, "[ms_ntt] Fp252 log_n=%u tiled: %d passes, radices 2^%u 2^%u 2^%u, zero extension 2^%u, bitrev %d\n", p->log_n, np,
                p->lr252[0], p->lr252[1], p->lr252[2], log_zero_ext, (int)bitrev_out);
    for (unsigned c0 = 0; c0 < ncols; c0 += group) {
        const unsigned nc = std::min(group, ncols - c0);
        unsigned done = 0;                                        // log2 of R_0 .. R_(q-1)
        for (int q = 0; q < np; q++) {
            ms252::PassParams P;
            memset(&P, 0, sizeof P);
            const bool last = q == np - 1;
            for (unsigned c = 0; c < nc; c++) {
                uint64_t* scr = (uint64_t*)((char*)scratch + (size_t)c * col_bytes);
                P.src[c] = q == 0 ? (const uint64_t*)src[c0 + c] : scr;
                P.dst[c] = last ? (uint64_t*)dst[c0 + c] : scr;
            }
            P.twr = p->d252_twr[q]; P.tw_lo = p->d252_tw_lo; P.tw_hi = p->d252_tw_hi; P.sc_lo = p->d252_sc_lo; P.sc_hi = p->d252_sc_hi;
            P.log_n = p->log_n; P.lo_bits = p->lo_bits;
            P.log_r = p->lr252[q]; P.log_c = ms252::TILE_LOG - P.log_r;
            P.log_s = p->log_n - done - P.log_r; P.log_tw = done;
            P.valid_rows = (1u << p->lr252[0]) >> log_zero_ext;
            P.log_r0 = p->lr252[0]; P.log_r1 = np == 3 ? p->lr252[1] : 0;
            P.scale_in = p->scale_in252; P.scale_out = p->scale_out252; P.bitrev_out = bitrev_out ? 1 : 0;
            const dim3 grid((unsigned)(n >> ms252::TILE_LOG), nc), block(ms252::NT2);
            ProfScope ps(ctx, names[q], 2.0 * col_bytes * nc);
            if (q == 0) hipLaunchKernelGGL((ms252::ntt252_strided_pass<ms252::NT2, true>), grid, block, 0, st, P);
            else if (!last) hipLaunchKernelGGL((ms252::ntt252_strided_pass<ms252::NT2, false>), grid, block, 0, st, P);
            else hipLaunchKernelGGL((ms252::ntt252_last_pass<ms252::NT2>), grid, block, 0, st, P);
            done += P.log_r;
        }
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

int plan_run252(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols) {
    if (p->np252) return plan_run252_tiled(p, src, dst, ncols, 0, false);
    ms_ctx* ctx = p->ctx;
    hipStream_t st = ctx->stream;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << p->log_n;
    for (unsigned c = 0; c < ncols; c++)
        if (src[c] != dst[c]) HIPCHK(hipMemcpyAsync(dst[c], src[c], n * 32, hipMemcpyDeviceToDevice, st));
    MSCHK(bit_reverse_run(ctx, 4, p->log_n, (const void* const*)dst, dst, ncols));
    for (unsigned c = 0; c < ncols; c++) {
        ms252::Params P;
        memset(&P, 0, sizeof P);
        P.col = (uint64_t*)dst[c]; P.tw_lo = p->d252_tw_lo; P.tw_hi = p->d252_tw_hi; P.sc_lo = p->d252_sc_lo; P.sc_hi = p->d252_sc_hi;
        P.log_n = p->log_n; P.lo_bits = p->lo_bits; P.scale_in = p->scale_in252; P.scale_out = p->scale_out252;
        const unsigned clog = std::min<unsigned>(p->log_n, ms252::CHUNK_LOG);
        {
            ProfScope ps(ctx, "ntt252_local", 64.0 * n);
            hipLaunchKernelGGL(ms252::ntt252_local, dim3((unsigned)(n >> clog)), dim3(ms252::NT), 0, st, P);
        }
        for (unsigned s = clog; s < p->log_n;) {                 // stages s+1 .. s+R per launch
            const unsigned R = std::min(ms252::MAX_FUSED_STAGES, p->log_n - s);
            P.stage = s;
            const dim3 g((unsigned)(((n >> R) + ms252::NT - 1) / ms252::NT));
            ProfScope ps(ctx, "ntt252_stages", 64.0 * n);
            if (R == 1) hipLaunchKernelGGL(ms252::ntt252_stages<1>, g, dim3(ms252::NT), 0, st, P);
            else hipLaunchKernelGGL(ms252::ntt252_stages<2>, g, dim3(ms252::NT), 0, st, P);
            s += R;
        }
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}
