// Constraint validation on the trace domain (Stark::validate_constraints, src/stark.rs:66-75; src/debug.rs:10-127):
// program validation on the host and the launches of csrc/validate_kernels.h.
#include "ms_internal.h"
#include "validate_kernels.h"

static int validate_locked(ms_ctx* ctx, int base_field, const uint32_t* h_prog, unsigned ninstr, const void* h_consts, unsigned nconst_words,
                           unsigned log_n, const void* const* d_base_cols, unsigned nbase, const void* const* d_ext_cols, unsigned next,
                           const void* const* d_periodic, const unsigned* periodic_len, unsigned nperiodic, unsigned nconstraints,
                           uint64_t* h_first_row, uint64_t* h_rows_failed) {
    using namespace mseval;
    using msvalidate::VK;
    using msvalidate::VGRID;
    if (!h_prog || !ninstr || (nconst_words && !h_consts) || !h_first_row || !h_rows_failed) return fail(MS_ERR_INVALID, "ms_validate_constraints: null argument");
    if (base_field != MS_GOLDILOCKS_FP && base_field != MS_STARK252_FP) return fail(MS_ERR_INVALID, "ms_validate_constraints: base_field must be MS_GOLDILOCKS_FP or MS_STARK252_FP");
    if (nconstraints == 0) return fail(MS_ERR_INVALID, "ms_validate_constraints: no constraints");
    if (nbase > (unsigned)MAXCOLS || next > (unsigned)MAXCOLS) return fail(MS_ERR_INVALID, "ms_validate_constraints: at most %d base and %d extension columns", MAXCOLS, MAXCOLS);
    if (nperiodic > 16u) return fail(MS_ERR_INVALID, "ms_validate_constraints: at most 16 periodic columns");
    if ((nbase && !d_base_cols) || (next && !d_ext_cols) || (nperiodic && (!d_periodic || !periodic_len)))
        return fail(MS_ERR_INVALID, "ms_validate_constraints: null column table");
    for (unsigned c = 0; c < nbase; c++) if (!d_base_cols[c]) return fail(MS_ERR_INVALID, "ms_validate_constraints: base column %u is null", c);
    for (unsigned c = 0; c < next; c++) if (!d_ext_cols[c]) return fail(MS_ERR_INVALID, "ms_validate_constraints: extension column %u is null", c);
    for (unsigned c = 0; c < nperiodic; c++) if (!d_periodic[c] || !periodic_len[c]) return fail(MS_ERR_INVALID, "ms_validate_constraints: periodic column %u is null or empty", c);
    if (log_n < 1 || log_n > 32) return fail(MS_ERR_INVALID, "ms_validate_constraints: log_n must be in 1 .. 32");
    const bool is252 = base_field == MS_STARK252_FP;
    if (is252 && next) return fail(MS_ERR_INVALID, "ms_validate_constraints: the 252-bit field has no extension columns");
    const unsigned PW = is252 ? 4 : 1;
    // ---- validate: public opcodes only, every register written before it is read, operands in range, each constraint stored at most once
    unsigned maxp = 0, maxq = 0;
    std::vector<char> pw(256, 0), qw(128, 0), seen(nconstraints, 0);
    const Instr* prog = (const Instr*)h_prog;
    auto P_ok = [&](uint32_t r) { return r < 256 && pw[r]; };
    auto Q_ok = [&](uint32_t r) { return r < 128 && qw[r]; };
    for (unsigned k = 0; k < ninstr; k++) {
        const Instr I = prog[k];
        bool ok = true, dp = false, dq = false;
        switch (I.op) {
        case OP_X_P: dp = true; break;
        case OP_CONST_P: ok = (uint64_t)I.a + PW <= nconst_words; dp = true; break;
        case OP_CONST_Q: ok = (uint64_t)I.a + 3 <= nconst_words; dq = true; break;
        case OP_TRACE_P: ok = I.a < nbase; dp = true; break;
        case OP_TRACE_Q: ok = I.a < next; dq = true; break;
        case OP_PERIODIC_P: case OP_PERIODIC_Q: ok = I.a < nperiodic; (I.op == OP_PERIODIC_P ? dp : dq) = true; break;
        case OP_NEG_P: case OP_INV_P: case OP_POW_P: ok = P_ok(I.a); dp = true; break;
        case OP_NEG_Q: case OP_INV_Q: case OP_POW_Q: ok = Q_ok(I.a); dq = true; break;
        case OP_ADD_PP: case OP_MUL_PP: ok = P_ok(I.a) && P_ok(I.b); dp = true; break;
        case OP_ADD_QQ: case OP_MUL_QQ: ok = Q_ok(I.a) && Q_ok(I.b); dq = true; break;
        case OP_ADD_QP: case OP_MUL_QP: ok = Q_ok(I.a) && P_ok(I.b); dq = true; break;
        case OP_EMBED: ok = P_ok(I.a); dq = true; break;
        case OP_STORE_Q: case OP_STORE_P:
            ok = (I.op == OP_STORE_Q ? Q_ok(I.a) : P_ok(I.a)) && I.b < nconstraints && !seen[I.b];
            if (ok) seen[I.b] = 1;
            break;
        default: ok = false;              // the internal opcodes of the rewriting passes included
        }
        if (is252 && (dq || I.op == OP_STORE_Q)) ok = false;
        if (dp) { if (I.dst >= 256) ok = false; else { pw[I.dst] = 1; maxp = std::max(maxp, I.dst + 1); } }
        if (dq) { if (I.dst >= 128) ok = false; else { qw[I.dst] = 1; maxq = std::max(maxq, I.dst + 1); } }
        if (!ok) return fail(MS_ERR_INVALID, "ms_validate_constraints: invalid instruction %u (op %u dst %u a %u b %u)", k, I.op, I.dst, I.a, I.b);
    }
    const size_t n = (size_t)1 << log_n;
    HIPCHK(hipSetDevice(ctx->device));
    // ---- the device image: program | constants (+ the domain offset one, Fp252) | partials | results
    std::vector<uint64_t> consts((const uint64_t*)h_consts, (const uint64_t*)h_consts + nconst_words);
    const unsigned one_slot = (unsigned)consts.size();
    if (is252) { const f252::E one = f252::one(); consts.insert(consts.end(), one.l, one.l + 4); }
    const unsigned grid = (unsigned)std::min<size_t>(VGRID, (n + NT - 1) / NT);
    const size_t pbytes = ((size_t)ninstr * sizeof(Instr) + 15) & ~(size_t)15, cbytes = (consts.size() * 8 + 15) & ~(size_t)15;
    const size_t partw = (size_t)grid * VK, total = pbytes + cbytes + 2 * partw * 8 + 2 * (size_t)nconstraints * 8;
    LockedPoolGuard pooled(ctx);
    void* buf = nullptr;
    MSCHK(pooled.alloc(total, &buf));
    {
        std::vector<char> image(pbytes + cbytes, 0);
        memcpy(image.data(), prog, (size_t)ninstr * sizeof(Instr));
        if (!consts.empty()) memcpy(image.data() + pbytes, consts.data(), consts.size() * 8);
        MSCHK(stage_upload(ctx, buf, image.data(), image.size()));
    }
    uint64_t* part_first = (uint64_t*)((char*)buf + pbytes + cbytes);
    uint64_t* part_count = part_first + partw;
    uint64_t* d_first = part_count + partw;
    uint64_t* d_count = d_first + nconstraints;
    EvalParams E;
    memset(&E, 0, sizeof E);
    E.prog = (const Instr*)buf;
    E.consts = (const uint64_t*)((char*)buf + pbytes);
    for (unsigned c = 0; c < nbase; c++) E.base_cols[c] = (const uint64_t*)d_base_cols[c];
    for (unsigned c = 0; c < next; c++) E.ext_cols[c] = (const uint64_t*)d_ext_cols[c];
    for (unsigned c = 0; c < nperiodic; c++) { E.periodic[c] = (const uint64_t*)d_periodic[c]; E.periodic_len[c] = periodic_len[c]; }
    E.n = n; E.ninstr = ninstr; E.log_n = log_n; E.lde_step = 1; E.bitrev = 0;
    {   // x_i = w_n^i from the twiddle tables of the forward plan (the trace domain is a subgroup: offset one)
        ms_ntt_plan* plan = nullptr;
        if (is252) {
            MSCHK(plan252_cached(ctx, log_n, false, f252::one(), &plan));
            E.tw_lo = plan->d252_tw_lo; E.tw_hi = plan->d252_tw_hi; E.lo_bits = plan->lo_bits;
            E.h_mont = one_slot; E.xshift = 0;
        } else {
            const unsigned table_log = std::max(log_n, 12u);
            MSCHK(ctx_plan(ctx, 1, table_log, false, 1, &plan));
            E.tw_lo = plan->d_tw_lo; E.tw_hi = plan->d_tw_hi; E.lo_bits = plan->lo_bits;
            E.h_mont = gl::ONE_MONT; E.xshift = table_log - log_n;
        }
    }
    // ---- one launch per VK constraints (one for every AIR of up to VK constraints), then the partials folded
    for (unsigned k0 = 0; k0 < nconstraints; k0 += VK) {
        msvalidate::ValParams V;
        V.part_first = part_first; V.part_count = part_count;
        V.k0 = k0; V.nk = std::min<unsigned>(VK, nconstraints - k0);
        {
            ProfScope ps(ctx, is252 ? "validate_program252" : "validate_program", 0.0);
            if (is252) {
                if (maxp <= 16) hipLaunchKernelGGL((msvalidate::validate_program252<16>), dim3(grid), dim3(NT), 0, ctx->stream, E, V);
                else if (maxp <= 64) hipLaunchKernelGGL((msvalidate::validate_program252<64>), dim3(grid), dim3(NT), 0, ctx->stream, E, V);
                else hipLaunchKernelGGL((msvalidate::validate_program252<256>), dim3(grid), dim3(NT), 0, ctx->stream, E, V);
            } else {
                if (maxp <= 16 && maxq <= 8) hipLaunchKernelGGL((msvalidate::validate_program<16, 8>), dim3(grid), dim3(NT), 0, ctx->stream, E, V);
                else if (maxp <= 64 && maxq <= 32) hipLaunchKernelGGL((msvalidate::validate_program<64, 32>), dim3(grid), dim3(NT), 0, ctx->stream, E, V);
                else hipLaunchKernelGGL((msvalidate::validate_program<256, 128>), dim3(grid), dim3(NT), 0, ctx->stream, E, V);
            }
            HIPCHK(hipGetLastError());
        }
        {
            ProfScope ps(ctx, "validate_finish", 0.0);
            hipLaunchKernelGGL(msvalidate::validate_finish, dim3(V.nk), dim3(NT), 0, ctx->stream, (const uint64_t*)part_first, (const uint64_t*)part_count,
                               grid, d_first + k0, d_count + k0);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipMemcpyAsync(h_first_row, d_first, (size_t)nconstraints * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_rows_failed, d_count, (size_t)nconstraints * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MS_OK;
}

extern "C" int ms_validate_constraints(ms_ctx* ctx, int base_field, const uint32_t* h_prog, unsigned ninstr,
                                       const void* h_consts, unsigned nconst_words, unsigned log_n,
                                       const void* const* d_base_cols, unsigned nbase, const void* const* d_ext_cols, unsigned next,
                                       const void* const* d_periodic, const unsigned* periodic_len, unsigned nperiodic,
                                       unsigned nconstraints, uint64_t* h_first_row, uint64_t* h_rows_failed) {
    if (!ctx) return fail(MS_ERR_INVALID, "ms_validate_constraints: null argument");
    MSCHK(canon_program(ctx, "ms_validate_constraints", base_field == MS_STARK252_FP, h_prog, ninstr, h_consts, nconst_words, log_n, nullptr, nullptr,
                        d_base_cols, nbase, d_ext_cols, next, d_periodic, periodic_len, nperiodic));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return validate_locked(ctx, base_field, h_prog, ninstr, h_consts, nconst_words, log_n, d_base_cols, nbase, d_ext_cols, next,
                           d_periodic, periodic_len, nperiodic, nconstraints, h_first_row, h_rows_failed);
}
