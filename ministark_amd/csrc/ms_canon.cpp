// Canonical-form scan and the checked mode built on it (include/ministark_hip.h "checked mode"; kernels in canon_kernels.h): the one
// documented precondition of the ABI -- every element handed in is < p -- made checkable (ms_check_canonical, ms_check_canonical_host) and,
// with ms_ctx_set_checked, checked by every entry point that does arithmetic on field data before it enqueues anything.
#include "ms_internal.h"
#include "canon_kernels.h"
#include "stage_kernels.h"
#include "eval_kernels.h"

// ---------------------------------------------------------------------------------------
// host scan
// ---------------------------------------------------------------------------------------
// index of the first bad component of element e (V words), or V when the element is canonical
static unsigned host_bad_word(const uint64_t* e, unsigned V) {
    if (V == 4) return mscanon::f252_bad(e[0], e[1], e[2], e[3]) ? 0u : 4u;
    for (unsigned k = 0; k < V; k++) if (mscanon::gl_bad(e[k])) return k;
    return V;
}
extern "C" int ms_check_canonical_host(int field, const void* h_elems, size_t count, size_t* first_bad) {
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (!first_bad || (count && !h_elems)) return fail(MS_ERR_INVALID, "ms_check_canonical_host: null argument");
    const uint64_t* w = (const uint64_t*)h_elems;
    size_t i = 0;
    for (; i < count; i++) if (host_bad_word(w + i * V, V) != V) break;
    *first_bad = i;
    return MS_OK;
}

// ---------------------------------------------------------------------------------------
// device scan
// ---------------------------------------------------------------------------------------
// the caller holds ctx->mu; blocks
static int scan_locked(ms_ctx* ctx, unsigned V, size_t n, const void* const* d_cols, unsigned ncols, ms_canon_report* out) {
    using namespace mscanon;
    memset(out, 0, sizeof *out);
    if (n == 0 || ncols == 0) return MS_OK;
    if (n > ((size_t)1 << 50) / V) return fail(MS_ERR_UNSUPPORTED, "ms_check_canonical: column too long");     // keys: 4096 columns x words per column < 2^64
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t nwords = (uint64_t)n * V;
    const uint64_t tiles = V == 4 ? (n + TILE_ELEMS - 1) / TILE_ELEMS : (nwords + 1 + 2 * TILE_PAIRS - 1) / (2 * (uint64_t)TILE_PAIRS);
    const unsigned nchunks = (ncols + MAXCOLS_PER_LAUNCH - 1) / MAXCOLS_PER_LAUNCH;
    LockedPoolGuard pooled(ctx);
    void* buf = nullptr;
    MSCHK(pooled.alloc(((size_t)MAX_GRID + nchunks) * sizeof(Partial), &buf));
    Partial* d_parts = (Partial*)buf;
    Partial* d_res = d_parts + MAX_GRID;
    for (unsigned k = 0; k < nchunks; k++) {
        const unsigned c0 = k * MAXCOLS_PER_LAUNCH, nc = std::min<unsigned>(MAXCOLS_PER_LAUNCH, ncols - c0);
        const void* d_tab = nullptr;
        MSCHK(stage_view(ctx, d_cols + c0, (size_t)nc * sizeof(void*), &d_tab, pooled));
        // a grid that is a multiple of the column count keeps every workgroup on one column (canon_kernels.h)
        uint64_t G = nc <= MAX_GRID ? (uint64_t)(MAX_GRID / nc) * nc : MAX_GRID;
        G = std::min<uint64_t>(G, tiles * nc);
        ScanParams P;
        memset(&P, 0, sizeof P);
        P.cols = (const uint64_t* const*)d_tab; P.partials = d_parts; P.nwords = nwords; P.tiles = tiles;
        P.ncols = nc; P.dq = (unsigned)(G / nc); P.dr = (unsigned)(G % nc);
        {
            ProfScope ps(ctx, "canon_scan", 8.0 * (double)nwords * nc);
            if (V == 1) hipLaunchKernelGGL(canon_scan_gl<1>, dim3((unsigned)G), dim3(NT), 0, ctx->stream, P);
            else if (V == 3) hipLaunchKernelGGL(canon_scan_gl<3>, dim3((unsigned)G), dim3(NT), 0, ctx->stream, P);
            else hipLaunchKernelGGL(canon_scan_252, dim3((unsigned)G), dim3(NT), 0, ctx->stream, P);
        }
        HIPCHK(hipGetLastError());
        {
            ProfScope ps(ctx, "canon_fold", 16.0 * (double)G);
            hipLaunchKernelGGL(canon_fold, dim3(1), dim3(NT), 0, ctx->stream, (const Partial*)d_parts, (unsigned)G, d_res + k);
        }
        HIPCHK(hipGetLastError());
    }
    std::vector<Partial> res(nchunks);
    MSCHK(ms_download(ctx, res.data(), d_res, (size_t)nchunks * sizeof(Partial)));      // through the landing buffer; waits for the stream
    bool found = false;
    for (unsigned k = 0; k < nchunks; k++) {
        out->count += res[k].count;
        if (res[k].count && !found) {
            found = true;
            const uint64_t w = res[k].key % nwords;
            out->first_col = k * MAXCOLS_PER_LAUNCH + (uint32_t)(res[k].key / nwords);
            out->first_row = w / V;
            out->first_word = (uint32_t)(w % V);
        }
    }
    return MS_OK;
}
extern "C" int ms_check_canonical(ms_ctx* ctx, int field, size_t n, const void* const* d_cols, unsigned ncols, void* out_report) {
    ms_canon_report* out = (ms_canon_report*)out_report;
    if (!ctx || !out) return fail(MS_ERR_INVALID, "ms_check_canonical: null argument");
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols && !d_cols) return fail(MS_ERR_INVALID, "ms_check_canonical: null column table");
    if (n) for (unsigned c = 0; c < ncols; c++) if (!d_cols[c]) return fail(MS_ERR_INVALID, "ms_check_canonical: null column %u", c);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return scan_locked(ctx, V, n, d_cols, ncols, out);
}

// ---------------------------------------------------------------------------------------
// checked mode
// ---------------------------------------------------------------------------------------
extern "C" int ms_ctx_set_checked(ms_ctx* ctx, int on) {
    if (!ctx) return fail(MS_ERR_INVALID, "ms_ctx_set_checked: null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->checked = on != 0;
    return MS_OK;
}
extern "C" int ms_ctx_get_checked(ms_ctx* ctx, int* on) {
    if (!ctx || !on) return fail(MS_ERR_INVALID, "ms_ctx_get_checked: null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    *on = ctx->checked ? 1 : 0;
    return MS_OK;
}
static int refuse(const char* entry, const char* arg, unsigned V, uint64_t col, uint64_t row, unsigned word) {
    if (V == 3)
        return fail(MS_ERR_INVALID, "%s: %s holds an element that is not canonical (>= p): column %llu, row %llu, component %u; nothing was enqueued (checked mode)",
                    entry, arg, (unsigned long long)col, (unsigned long long)row, word);
    return fail(MS_ERR_INVALID, "%s: %s holds an element that is not canonical (>= p): column %llu, row %llu; nothing was enqueued (checked mode)",
                entry, arg, (unsigned long long)col, (unsigned long long)row);
}
// The helpers below are called by the entry points WITHOUT ctx->mu, after their own argument checks and before anything is enqueued; with
// the mode off they return at once.  A null table or column is left to the entry point's own validation.
int canon_cols(ms_ctx* ctx, const char* entry, const char* arg, int field, size_t n, const void* const* d_cols, unsigned ncols) {
    if (!ctx || !ctx->checked || !d_cols || !n || !ncols) return MS_OK;
    unsigned V = 0;
    if (field_words(field, &V) != MS_OK) return MS_OK;
    for (unsigned c = 0; c < ncols; c++) if (!d_cols[c]) return MS_OK;
    ms_canon_report r;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        MSCHK(scan_locked(ctx, V, n, d_cols, ncols, &r));
    }
    return r.count ? refuse(entry, arg, V, r.first_col, r.first_row, r.first_word) : MS_OK;
}
int canon_col(ms_ctx* ctx, const char* entry, const char* arg, int field, size_t n, const void* d_col) {
    const void* tab[1] = {d_col};
    return canon_cols(ctx, entry, arg, field, n, tab, 1);
}
// the columns of d_base a call names, over Fp or Fp252: only what the call reads is scanned (an output may be a column of d_base, of any
// content), and the column reported is the caller's index, not the one in the table scanned
int canon_named(ms_ctx* ctx, const char* entry, int field, size_t n, const void* const* d_base, const std::vector<unsigned>& used, const char* arg) {
    if (!ctx || !ctx->checked || !n || used.empty()) return MS_OK;
    unsigned V = 0;
    if (field_words(field, &V) != MS_OK) return MS_OK;
    std::vector<const void*> tab;
    for (unsigned c : used) tab.push_back(d_base[c]);
    ms_canon_report r;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        MSCHK(scan_locked(ctx, V, n, tab.data(), (unsigned)tab.size(), &r));
    }
    return r.count ? refuse(entry, arg, V, used[r.first_col], r.first_row, r.first_word) : MS_OK;
}
// a row-major matrix [nrows][ncols]: scanned as one run of nrows * ncols elements
int canon_rows(ms_ctx* ctx, const char* entry, const char* arg, int field, size_t nrows, unsigned ncols, const void* d_matrix) {
    if (!ctx || !ctx->checked || !d_matrix || !nrows || !ncols) return MS_OK;
    unsigned V = 0;
    if (field_words(field, &V) != MS_OK) return MS_OK;
    const void* tab[1] = {d_matrix};
    ms_canon_report r;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        MSCHK(scan_locked(ctx, V, nrows * ncols, tab, 1, &r));
    }
    return r.count ? refuse(entry, arg, V, r.first_row % ncols, r.first_row / ncols, r.first_word) : MS_OK;
}
// host constants: `count` packed elements; reported as column 0, row = the element's index
int canon_host(ms_ctx* ctx, const char* entry, const char* arg, int field, const void* h_elems, size_t count) {
    if (!ctx || !ctx->checked || !h_elems || !count) return MS_OK;
    unsigned V = 0;
    if (field_words(field, &V) != MS_OK) return MS_OK;
    const uint64_t* w = (const uint64_t*)h_elems;
    for (size_t i = 0; i < count; i++) {
        const unsigned k = host_bad_word(w + i * V, V);
        if (k != V) return refuse(entry, arg, V, 0, i, k);
    }
    return MS_OK;
}
// the inputs of a constraint program (ms_eval_program[_ex], ms_validate_constraints).  Runs before the entry point's own validation, so it
// looks only at what is well-formed enough to be read (the entry point reports the rest); is252: every element is an Fp252 one.
int canon_program(ms_ctx* ctx, const char* entry, bool is252, const uint32_t* h_prog, unsigned ninstr, const void* h_consts, unsigned nconst_words,
                  unsigned log_n, const void* h_domain_offset, const void* d_x_lde, const void* const* d_base_cols, unsigned nbase,
                  const void* const* d_ext_cols, unsigned next, const void* const* d_periodic, const unsigned* periodic_len, unsigned nperiodic) {
    if (!ctx || !ctx->checked || !h_prog || log_n > 32 || nperiodic > 16u || (nconst_words && !h_consts)) return MS_OK;
    if ((nbase && !d_base_cols) || (next && !d_ext_cols) || (nperiodic && (!d_periodic || !periodic_len)) || (is252 && next)) return MS_OK;
    const int pf = is252 ? MS_STARK252_FP : MS_GOLDILOCKS_FP;
    const size_t n = (size_t)1 << log_n;
    const mseval::Instr* prog = (const mseval::Instr*)h_prog;
    int pkind[16] = {0};                                     // 1: read as base-field elements, 3: as Fq3 elements
    if (!is252) MSCHK(canon_host(ctx, entry, "h_consts", MS_GOLDILOCKS_FP, h_consts, nconst_words));       // every word, P or Q constant alike
    for (unsigned k = 0; k < ninstr; k++) {
        const mseval::Instr I = prog[k];
        if ((I.op == mseval::OP_PERIODIC_P || I.op == mseval::OP_PERIODIC_Q) && I.a < nperiodic) pkind[I.a] = I.op == mseval::OP_PERIODIC_P ? 1 : 3;
        if (is252 && I.op == mseval::OP_CONST_P && (uint64_t)I.a + 4 <= nconst_words) {
            const uint64_t* w = (const uint64_t*)h_consts + I.a;
            if (mscanon::f252_bad(w[0], w[1], w[2], w[3])) return refuse(entry, "h_consts", 4, 0, I.a, 0);   // row = the constant's word index
        }
    }
    MSCHK(canon_host(ctx, entry, "h_domain_offset", pf, h_domain_offset, 1));
    MSCHK(canon_col(ctx, entry, "d_x_lde", pf, n, d_x_lde));
    MSCHK(canon_cols(ctx, entry, "d_base_cols", pf, n, d_base_cols, nbase));
    MSCHK(canon_cols(ctx, entry, "d_ext_cols", MS_GOLDILOCKS_FQ3, n, d_ext_cols, next));
    for (unsigned c = 0; c < nperiodic; c++) {
        if (!pkind[c] || !d_periodic[c] || !periodic_len[c]) continue;
        const void* tab[1] = {d_periodic[c]};
        ms_canon_report r;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            MSCHK(scan_locked(ctx, is252 ? 4 : (unsigned)pkind[c], periodic_len[c], tab, 1, &r));
        }
        if (r.count) return refuse(entry, "d_periodic", is252 ? 4 : (unsigned)pkind[c], c, r.first_row, r.first_word);
    }
    return MS_OK;
}
