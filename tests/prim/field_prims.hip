// TEST INFRASTRUCTURE ONLY -- the field primitives one at a time, for tests/test_field_primitives.py.
//
// One kernel per header (gl.h, gl_dev.h, gl_limb.h, the accumulators of eval_kernels.h, fp252.h); `op` picks the primitive and
// its template arguments.  The RPO-256 permutation (rpo_kernels.h, rpo_coin_kernels.h) has one lane-per-case kernel for its pieces,
// two kernels that hold a state across lanes as the wide forms do, and one entry that runs the whole permutation in every form.  Case i reads in[i * is ..] and writes every word of its result to out[i * os ..]: weak residues, raw
// limbs and raw accumulator columns as they are, so that the device build can be compared word for word with the host build.
//
// Built twice by tests/prim/prims.py: by hipcc for gfx950 (the inline assembly, builtins and constant-address-space loads of the
// device branches) and by g++ against the simulator of tests/emu (the #else branches).  The product headers are included unchanged.
//
// Blocks are one wave (64 lanes).  What the product reads through the constant address space at a wave-uniform index (w4_at,
// w4x4_at, ev_cword) is read here at an index derived from blockIdx.x only, so that the scalar-load path is the one that runs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gl.h"
#include "gl_dev.h"
#include "gl_limb.h"
#include "fp252.h"
#include "eval_kernels.h"
#include "ntt2_kernels.h"
#include "rpo_kernels.h"
#include "rpo_coin_kernels.h"
#include <string.h>
#include <vector>

typedef uint64_t u64;
static constexpr int BLOCK = 64;

#define KARGS int op, int aux, const u64* in, int is, u64* out, int os, int n, const u64* tab, int ntab
#define CASE_PTRS                                                  \
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);         \
    if (i >= n) return;                                            \
    const u64* a = in + (size_t)i * is;                            \
    u64* o = out + (size_t)i * os;

// ---- gl.h ---------------------------------------------------------------------------------------------------------------------
// op: 0 add, 1 sub, 2 neg, 3 add_lazy, 4 sub_lazy, 5 canon, 6 reduce128, 7 mul, 8 mont_mul, 9 to_mont, 10 from_mont, 11 mont_pow,
//     12 mont_inv, 13 Fq3 mont_mul, 14 Fq3 mont_inv
__global__ void __launch_bounds__(BLOCK) k_gl(KARGS) {
    CASE_PTRS
    switch (op) {
    case 0: o[0] = gl::add(a[0], a[1]); break;
    case 1: o[0] = gl::sub(a[0], a[1]); break;
    case 2: o[0] = gl::neg(a[0]); break;
    case 3: o[0] = gl::add_lazy(a[0], a[1]); break;
    case 4: o[0] = gl::sub_lazy(a[0], a[1]); break;
    case 5: o[0] = gl::canon(a[0]); break;
    case 6: o[0] = gl::reduce128(a[0], a[1]); break;
    case 7: o[0] = gl::mul(a[0], a[1]); break;
    case 8: o[0] = gl::mont_mul(a[0], a[1]); break;
    case 9: o[0] = gl::to_mont(a[0]); break;
    case 10: o[0] = gl::from_mont(a[0]); break;
    case 11: o[0] = gl::mont_pow(a[0], a[1]); break;
    case 12: o[0] = gl::mont_inv(a[0]); break;
    case 13: {
        const gl::Fq3 r = gl::mont_mul(gl::Fq3{a[0], a[1], a[2]}, gl::Fq3{a[3], a[4], a[5]});
        o[0] = r.c0; o[1] = r.c1; o[2] = r.c2;
        break;
    }
    case 14: {
        const gl::Fq3 r = gl::mont_inv(gl::Fq3{a[0], a[1], a[2]});
        o[0] = r.c0; o[1] = r.c1; o[2] = r.c2;
        break;
    }
    default: break;
    }
    (void)aux; (void)tab; (void)ntab;
}

// ---- gl_dev.h -----------------------------------------------------------------------------------------------------------------
template <bool INV, int E, bool VC>
__device__ __forceinline__ void gld_bfly(const u64* a, u64* o) {
    u64 u = a[0], v = a[1];
    gld::bfly<INV, E, VC>(u, v);
    o[0] = u; o[1] = v;
}
template <int N, bool INV>
__device__ __forceinline__ void gld_dft(const u64* a, u64* o) {
    u64 x[N];
    #pragma unroll
    for (int q = 0; q < N; q++) x[q] = a[q];
    gld::dft_lazy<N, INV>(x);
    #pragma unroll
    for (int q = 0; q < N; q++) o[q] = x[q];
}
template <int NA, bool INV>
__device__ __forceinline__ void gld_pruned(const u64* a, u64* o) {
    u64 x[16];
    #pragma unroll
    for (int q = 0; q < 16; q++) x[q] = q < NA ? a[q] : 0;
    gld::dft16_pruned<NA, INV>(x);
    #pragma unroll
    for (int q = 0; q < 16; q++) o[q] = x[q];
}

// op: 0 mmul, 1 add_lazy, 2 sub_lazy, 3 canon, 10 + k mul_pow2<12 (k + 1)>, 100 + 16 INV + 2 E + V_CANON bfly,
//     200 + 2 N + INV dft_lazy<N>, 300 + 2 NA + INV dft16_pruned<NA>
__global__ void __launch_bounds__(BLOCK) k_gld(KARGS) {
    CASE_PTRS
#define BF(I, E) case 100 + 16 * I + 2 * E: gld_bfly<I, E, false>(a, o); break; case 101 + 16 * I + 2 * E: gld_bfly<I, E, true>(a, o); break;
#define DF(N) case 200 + 2 * N: gld_dft<N, false>(a, o); break; case 201 + 2 * N: gld_dft<N, true>(a, o); break;
#define PR(NA) case 300 + 2 * NA: gld_pruned<NA, false>(a, o); break; case 301 + 2 * NA: gld_pruned<NA, true>(a, o); break;
    switch (op) {
    case 0: o[0] = gld::mmul(a[0], a[1]); break;
    case 1: o[0] = gld::add_lazy(a[0], a[1]); break;
    case 2: o[0] = gld::sub_lazy(a[0], a[1]); break;
    case 3: o[0] = gld::canon(a[0]); break;
    case 10: o[0] = gld::mul_pow2<12>(a[0]); break;
    case 11: o[0] = gld::mul_pow2<24>(a[0]); break;
    case 12: o[0] = gld::mul_pow2<36>(a[0]); break;
    case 13: o[0] = gld::mul_pow2<48>(a[0]); break;
    case 14: o[0] = gld::mul_pow2<60>(a[0]); break;
    case 15: o[0] = gld::mul_pow2<72>(a[0]); break;
    case 16: o[0] = gld::mul_pow2<84>(a[0]); break;
    BF(0, 0) BF(0, 1) BF(0, 2) BF(0, 3) BF(0, 4) BF(0, 5) BF(0, 6) BF(0, 7)
    BF(1, 0) BF(1, 1) BF(1, 2) BF(1, 3) BF(1, 4) BF(1, 5) BF(1, 6) BF(1, 7)
    DF(2) DF(4) DF(8) DF(16)
    PR(1) PR(2) PR(4)
    default: break;
    }
#undef BF
#undef DF
#undef PR
    (void)aux; (void)tab; (void)ntab;
}

// ---- gl_limb.h ----------------------------------------------------------------------------------------------------------------
// a limb travels as one 64-bit word holding its 32 bits (two's complement)
__device__ __forceinline__ glimb::L4 ld4(const u64* a) {
    glimb::L4 r;
    #pragma unroll
    for (int k = 0; k < 4; k++) r.l[k] = (uint32_t)a[k];
    return r;
}
__device__ __forceinline__ void st4(u64* o, const glimb::L4& x) {
    #pragma unroll
    for (int k = 0; k < 4; k++) o[k] = x.l[k];
}
template <int S>
__device__ __forceinline__ void limb_bfly(const u64* a, u64* o) {
    glimb::L4 u = ld4(a), v = ld4(a + 4);
    glimb::bfly<S>(u, v);
    st4(o, u); st4(o + 4, v);
}
template <int N, bool INV, bool BIAS>
__device__ __forceinline__ void limb_dft(const u64* a, u64* o) {
    glimb::L4 x[N];
    #pragma unroll
    for (int q = 0; q < N; q++) x[q] = ld4(a + 4 * q);
    glimb::dft<N, INV, BIAS>(x);
    #pragma unroll
    for (int q = 0; q < N; q++) st4(o + 4 * q, x[q]);
}
template <int NA, bool INV>
__device__ __forceinline__ void limb_pruned(const u64* a, u64* o) {
    glimb::L4 x[16];
    #pragma unroll
    for (int q = 0; q < 16; q++) x[q] = q < NA ? ld4(a + 4 * q) : glimb::L4{{0, 0, 0, 0}};
    glimb::dft16_pruned<NA, INV>(x);
    #pragma unroll
    for (int q = 0; q < 16; q++) st4(o + 4 * q, x[q]);
}

// op: 0 from_u64, 1 perm (SEL_345, SEL_234), 2 mul_to_limbs, 3 half_shift, 100 + k bfly<12 k>,
//     200 + 4 N + 2 INV + BIAS dft<N>, 300 + 2 NA + INV dft16_pruned<NA>, 400 / 401 fold_t<CANON>, 402 fold_h,
//     410 / 411 mul_fold<CANON>, 412 / 413 mul_fold_co<CANON> (twiddle copies: w4_at at slot blockIdx.x mod ntab / 4),
//     414 mul_fold_co<false> against the four copies of w4x4_at (slots 4 (blockIdx.x mod ntab / 16) ..), 420 mul3_to_limbs,
//     430 / 431 to_weak<CANON>, 432 to_canon
__global__ void __launch_bounds__(BLOCK) k_limb(KARGS) {
    CASE_PTRS
#define LB(K) case 100 + K: limb_bfly<12 * K>(a, o); break;
#define LD(N, I) case 200 + 4 * N + 2 * I: limb_dft<N, I, false>(a, o); break; case 201 + 4 * N + 2 * I: limb_dft<N, I, true>(a, o); break;
#define LP(NA) case 300 + 2 * NA: limb_pruned<NA, false>(a, o); break; case 301 + 2 * NA: limb_pruned<NA, true>(a, o); break;
    switch (op) {
    case 0: st4(o, glimb::from_u64(a[0])); break;
    case 1:
        o[0] = glimb::perm((uint32_t)a[0], (uint32_t)a[1], glimb::SEL_345);
        o[1] = glimb::perm((uint32_t)a[0], (uint32_t)a[1], glimb::SEL_234);
        break;
    case 2: st4(o, glimb::mul_to_limbs(a[0], a[1])); break;
    case 3: st4(o, glimb::half_shift(ld4(a))); break;
    LB(0) LB(1) LB(2) LB(3) LB(4) LB(5) LB(6) LB(7) LB(8) LB(9) LB(10) LB(11) LB(12) LB(13) LB(14) LB(15)
    LD(2, 0) LD(2, 1) LD(4, 0) LD(4, 1) LD(8, 0) LD(8, 1) LD(16, 0) LD(16, 1)
    LP(1) LP(2) LP(4)
    case 400: o[0] = glimb::fold_t<false>(a[0], a[1]); break;
    case 401: o[0] = glimb::fold_t<true>(a[0], a[1]); break;
    case 402: o[0] = glimb::fold_h((uint32_t)a[0], a[1]); break;
    case 410: o[0] = glimb::mul_fold<false>(ld4(a), msntt2::w4_at(tab, blockIdx.x % (unsigned)(ntab / 4))); break;
    case 411: o[0] = glimb::mul_fold<true>(ld4(a), msntt2::w4_at(tab, blockIdx.x % (unsigned)(ntab / 4))); break;
    case 412: o[0] = glimb::mul_fold_co<false>(ld4(a), msntt2::w4_at(tab, blockIdx.x % (unsigned)(ntab / 4))); break;
    case 413: o[0] = glimb::mul_fold_co<true>(ld4(a), msntt2::w4_at(tab, blockIdx.x % (unsigned)(ntab / 4))); break;
    case 414: {
        glimb::W4 w[4];
        msntt2::w4x4_at(tab, 4 * (blockIdx.x % (unsigned)(ntab / 16)), w);
        const glimb::L4 x = ld4(a);
        #pragma unroll
        for (int k = 0; k < 4; k++) o[k] = glimb::mul_fold_co<false>(x, w[k]);
        break;
    }
    case 420: st4(o, glimb::mul3_to_limbs(a[0], glimb::q3_from(a[1], a[2], a[3]))); break;
    case 430: o[0] = glimb::to_weak<false>(ld4(a)); break;
    case 431: o[0] = glimb::to_weak<true>(ld4(a)); break;
    case 432: o[0] = glimb::to_canon(ld4(a)); break;
    default: break;
    }
#undef LB
#undef LD
#undef LP
    (void)aux;
}

// ---- eval_kernels.h: unreduced sums of products -------------------------------------------------------------------------------
// aux = terms per case.  The constant pool is `tab`; term t of a case in block b uses pool entry (b + t) mod (pool size), a
// wave-uniform slot as in the evaluator.  Acc6 / AccQ cases write their raw columns, then the reduced words; Acc19 cases the 19
// raw columns, then the 4 reduced words.
//   0 acc_macp (v, b)        1 acc_macc (v; pool entries of 2 words)
//   2 accq_macc_p_cp (v; 2)  3 accq_macc_q_cp (Fq3 v; 2)  4 accq_macc_p_cq (v; 10)  5 accq_macc_q_cq (Fq3 v; 10)
//   6 accq_macp_p_p (v, b)   7 accq_macp_q_p (Fq3 v, b)
//   10 Acc19 acc_macp (v, b: 4 words each)   11 Acc19 acc_macc (v; pool entries of 5 words)
//   12 / 13 f252::reduce_columns<CANON> on the 19 columns of the case
__device__ __forceinline__ void st_acc6(u64* o, const mseval::Acc6& A) {
    #pragma unroll
    for (int k = 0; k < 6; k++) o[k] = A.s[k];
}
__global__ void __launch_bounds__(BLOCK) k_acc(KARGS) {
    CASE_PTRS
    const unsigned T = (unsigned)aux, b = blockIdx.x;
    auto slot = [&](unsigned t, unsigned words) { return words * ((b + t) % ((unsigned)ntab / words)); };
    auto q3 = [](const u64* p) { return gl::Fq3{p[0], p[1], p[2]}; };
    auto e4 = [](const u64* p) { return f252::E{{p[0], p[1], p[2], p[3]}}; };
    if (op <= 1) {
        mseval::Acc6 A;
        mseval::acc_zero(A);
        for (unsigned t = 0; t < T; t++) {
            if (op == 0) mseval::acc_macp(A, a[2 * t], a[2 * t + 1]);
            else mseval::acc_macc(A, a[t], tab, slot(t, 2));
        }
        st_acc6(o, A);
        o[6] = mseval::acc_reduce(A);
    } else if (op <= 7) {
        mseval::AccQ A;
        mseval::acc_zero(A);
        for (unsigned t = 0; t < T; t++) {
            switch (op) {
            case 2: mseval::accq_macc_p_cp(A, a[t], tab, slot(t, 2)); break;
            case 3: mseval::accq_macc_q_cp(A, q3(a + 3 * t), tab, slot(t, 2)); break;
            case 4: mseval::accq_macc_p_cq(A, a[t], tab, slot(t, 10)); break;
            case 5: mseval::accq_macc_q_cq(A, q3(a + 3 * t), tab, slot(t, 10)); break;
            case 6: mseval::accq_macp_p_p(A, a[2 * t], a[2 * t + 1]); break;
            default: mseval::accq_macp_q_p(A, q3(a + 4 * t), a[4 * t + 3]); break;
            }
        }
        for (int k = 0; k < 3; k++) st_acc6(o + 6 * k, A.c[k]);
        const gl::Fq3 r = mseval::accq_reduce(A);
        o[18] = r.c0; o[19] = r.c1; o[20] = r.c2;
    } else if (op <= 11) {
        mseval::Acc19 A;
        mseval::acc_zero(A);
        for (unsigned t = 0; t < T; t++) {
            if (op == 10) mseval::acc_macp(A, e4(a + 8 * t), e4(a + 8 * t + 4));
            else mseval::acc_macc(A, e4(a + 4 * t), tab, slot(t, 5));
        }
        #pragma unroll
        for (int k = 0; k < 19; k++) o[k] = A.c[k];
        const f252::E r = mseval::acc_reduce(A);
        #pragma unroll
        for (int k = 0; k < 4; k++) o[19 + k] = r.l[k];
    } else {
        u64 c[19];
        #pragma unroll
        for (int k = 0; k < 19; k++) c[k] = a[k];
        const f252::E r = op == 12 ? f252::reduce_columns<true>(c) : f252::reduce_columns<false>(c);
        #pragma unroll
        for (int k = 0; k < 4; k++) o[k] = r.l[k];
    }
}

// ---- fp252.h ------------------------------------------------------------------------------------------------------------------
// op: 0 add, 1 neg, 2 sub, 3 mul, 4 sqr, 5 inv, 6 to_mont, 7 from_mont, 8 mul_t<false>, 9 add_lazy, 10 kp_minus<2>, 11 kp_minus<4>,
//     12 reduce_lazy, 13 digits9 (nine words)
__global__ void __launch_bounds__(BLOCK) k_f252(KARGS) {
    CASE_PTRS
    const f252::E x{{a[0], a[1], a[2], a[3]}}, y{{a[4], a[5], a[6], a[7]}};
    f252::E r{{0, 0, 0, 0}};
    switch (op) {
    case 0: r = f252::add(x, y); break;
    case 1: r = f252::neg(x); break;
    case 2: r = f252::sub(x, y); break;
    case 3: r = f252::mul(x, y); break;
    case 4: r = f252::sqr(x); break;
    case 5: r = f252::inv(x); break;
    case 6: r = f252::to_mont(x); break;
    case 7: r = f252::from_mont(x); break;
    case 8: r = f252::mul_t<false>(x, y); break;
    case 9: r = f252::add_lazy(x, y); break;
    case 10: r = f252::kp_minus<2>(x); break;
    case 11: r = f252::kp_minus<4>(x); break;
    case 12: r = f252::reduce_lazy(x); break;
    case 13: {
        uint32_t d[9];
        f252::digits9(x, d);
        #pragma unroll
        for (int k = 0; k < 9; k++) o[k] = d[k];
        return;
    }
    default: break;
    }
    #pragma unroll
    for (int k = 0; k < 4; k++) o[k] = r.l[k];
    (void)aux; (void)tab; (void)ntab;
}

// ---- rpo_kernels.h, rpo_coin_kernels.h: the pieces of the RPO-256 permutation ---------------------------------------------------
// One lane per case.  op: 0 apply_mds (12 words), 1 pow7, 2 pow_inv7 (one word), 3 pow_inv7_all (12 words, then the twelve pow_inv7
//     of the same words), 4 pow7(gl::add(s[j], RC0[12 aux + j])), 5 pow_inv7(gl::add(s[j], RC1[12 aux + j])) for j < 12: the two
//     S-box layers of round aux as msrpo::permute and the wide forms write them
__global__ void __launch_bounds__(BLOCK) k_rpo(KARGS) {
    CASE_PTRS
    msrpo::State st;
    #pragma unroll
    for (int j = 0; j < 12; j++) st.s[j] = is >= 12 ? a[j] : 0;
    switch (op) {
    case 0:
        msrpo::apply_mds(st);
        #pragma unroll
        for (int j = 0; j < 12; j++) o[j] = st.s[j];
        break;
    case 1: o[0] = msrpo::pow7(a[0]); break;
    case 2: o[0] = msrpo::pow_inv7(a[0]); break;
    case 3:
        #pragma unroll
        for (int j = 0; j < 12; j++) o[12 + j] = msrpo::pow_inv7(st.s[j]);
        msrpo::pow_inv7_all(st.s);
        #pragma unroll
        for (int j = 0; j < 12; j++) o[j] = st.s[j];
        break;
    case 4:
        #pragma unroll
        for (int j = 0; j < 12; j++) o[j] = msrpo::pow7(gl::add(st.s[j], msrpo::RC0[aux * 12 + j]));
        break;
    case 5:
        #pragma unroll
        for (int j = 0; j < 12; j++) o[j] = msrpo::pow_inv7(gl::add(st.s[j], msrpo::RC1[aux * 12 + j]));
        break;
    default: break;
    }
    (void)tab; (void)ntab;
}
// op 100: msrpo::mds_wide as rpo256_merge_level_wide holds a state -- sixteen lanes per case, four cases per block of 64, lane j < 12
// of a group owns element j, the four spare lanes shadow elements 0..3.  Words 0..12 of a case: mds_wide; words 12..24: apply_mds
// on the same state, by the group's first lane.  Every lane reaches both barriers.
__global__ void __launch_bounds__(BLOCK) k_rpo_mds16(KARGS) {
    __shared__ u64 sh_all[BLOCK / 16][12];
    const unsigned g = threadIdx.x / 16, j16 = threadIdx.x % 16;
    const bool owner = j16 < 12;
    const unsigned j = owner ? j16 : j16 - 12;
    const size_t i = (size_t)blockIdx.x * (BLOCK / 16) + g;
    const bool live = i < (size_t)n;
    uint32_t row[12];
    #pragma unroll
    for (int q = 0; q < 12; q++) row[q] = msrpo::MDS_ROW[(q + 12 - j) % 12];
    u64 s = live ? in[i * is + j] : 0;
    s = msrpo::mds_wide(s, sh_all[g], j, owner, row);
    if (live && owner) out[i * os + j] = s;
    if (live && j16 == 0) {
        msrpo::State st;
        #pragma unroll
        for (int q = 0; q < 12; q++) st.s[q] = in[i * is + q];
        msrpo::apply_mds(st);
        #pragma unroll
        for (int q = 0; q < 12; q++) out[i * os + 12 + q] = st.s[q];
    }
    (void)op; (void)aux; (void)tab; (void)ntab;
}
// op 101: msrpo::mds_wide as the coin holds a state -- msrpocoin::Wide, one case (a 16-word state record) per block of 64, lanes
// 12..63 shadow; the record written back carries pos = 4 in word 12
__global__ void __launch_bounds__(BLOCK) k_rpo_mds_coin(KARGS) {
    __shared__ u64 sh[12];
    msrpocoin::Wide sp;
    sp.load((const msrpocoin::State*)(in + (size_t)blockIdx.x * is), sh);
    sp.s = msrpo::mds_wide(sp.s, sp.sh, sp.j, sp.owner, sp.row);
    sp.store((msrpocoin::State*)(out + (size_t)blockIdx.x * os), 4);
    (void)op; (void)aux; (void)n; (void)tab; (void)ntab;
}
// op 200, first part: msrpo::permute called directly, one lane per case; words 0..12
__global__ void __launch_bounds__(BLOCK) k_rpo_permute(KARGS) {
    CASE_PTRS
    msrpo::State st;
    #pragma unroll
    for (int j = 0; j < 12; j++) st.s[j] = a[j];
    msrpo::permute(st);
    #pragma unroll
    for (int j = 0; j < 12; j++) o[j] = st.s[j];
    (void)op; (void)aux; (void)tab; (void)ntab;
}

// ---- host entries: allocate, upload, launch, synchronise, download.  0 = success; a failing step returns its line, never aborts.
#define TRY(x) do { if (rc == 0 && (x) != hipSuccess) rc = __LINE__; } while (0)
template <class K>
static int run(K kern, int op, int aux, const u64* in, int is, u64* out, int os, int n, const u64* tab, int ntab, int per_block = BLOCK) {
    if (n <= 0 || is <= 0 || os <= 0 || ntab < 0) return -1;
    const size_t nin = (size_t)n * is, nout = (size_t)n * os, nt = ntab > 0 ? (size_t)ntab : 1;
    u64 *din = nullptr, *dout = nullptr, *dtab = nullptr;
    int rc = 0;
    TRY(hipMalloc((void**)&din, nin * 8));
    TRY(hipMalloc((void**)&dout, nout * 8));
    TRY(hipMalloc((void**)&dtab, nt * 8));
    TRY(hipMemcpy(din, in, nin * 8, hipMemcpyHostToDevice));
    TRY(hipMemset(dout, 0, nout * 8));
    TRY(hipMemset(dtab, 0, nt * 8));
    if (ntab > 0) TRY(hipMemcpy(dtab, tab, (size_t)ntab * 8, hipMemcpyHostToDevice));
    if (rc == 0) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(BLOCK), 0, 0, op, aux, din, is, dout, os, n, dtab, ntab);
        TRY(hipGetLastError());
    }
    TRY(hipDeviceSynchronize());
    TRY(hipMemcpy(out, dout, nout * 8, hipMemcpyDeviceToHost));
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (dtab) (void)hipFree(dtab);
    return rc;
}

// rpo op 200: the whole permutation in every device form, on the same n states of 12 words.  42 words per case:
//    0..12  msrpo::permute, called directly (k_rpo_permute)
//   12..24  the coin's Wide form: rpo_coin_step<Wide, OP_CREATE> launched as ms_rpo_coin.cpp launches it (one block of one wave) on a
//           state record that holds the state with nothing unread (pos = 12); word 40 = the record's pos afterwards (4)
//   24..36  the same with the coin's Narrow form; word 41 = pos
//   36..40  rpo256_merge_level_wide itself, launched as ms_rpo256_merkle launches it (64 threads, four nodes per workgroup), on the
//           rate words 4..12 of the state: its capacity is zero by construction
template <class SP>
static int run_coin_permute(const u64* in, u64* out, int os, int n, int at, int pos_at) {
    std::vector<msrpocoin::State> recs((size_t)n);
    memset(recs.data(), 0, recs.size() * sizeof(msrpocoin::State));
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < 12; j++) recs[i].s[j] = in[(size_t)i * 12 + j];
        recs[i].pos = 12;
    }
    msrpocoin::State* d = nullptr;
    int rc = 0;
    TRY(hipMalloc((void**)&d, recs.size() * sizeof(msrpocoin::State)));
    TRY(hipMemcpy(d, recs.data(), recs.size() * sizeof(msrpocoin::State), hipMemcpyHostToDevice));
    for (int i = 0; i < n && rc == 0; i++) {
        hipLaunchKernelGGL((msrpocoin::rpo_coin_step<SP, msrpocoin::OP_CREATE>), dim3(1), dim3(msrpocoin::WAVE), 0, 0, d + i, (const u64*)nullptr, (u64)0,
                           (size_t)0, (u64*)nullptr);
        TRY(hipGetLastError());
    }
    TRY(hipDeviceSynchronize());
    TRY(hipMemcpy(recs.data(), d, recs.size() * sizeof(msrpocoin::State), hipMemcpyDeviceToHost));
    if (d) (void)hipFree(d);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < 12; j++) out[(size_t)i * os + at + j] = recs[i].s[j];
        out[(size_t)i * os + pos_at] = recs[i].pos;
    }
    return 0;
}
static int run_permute_forms(const u64* in, int is, u64* out, int os, int n) {
    if (n <= 0 || is != 12 || os != 42) return -1;
    std::vector<u64> tmp((size_t)n * 12);
    int rc = run(k_rpo_permute, 200, 0, in, 12, tmp.data(), 12, n, nullptr, 0);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 12; j++) out[(size_t)i * os + j] = tmp[(size_t)i * 12 + j];
    if ((rc = run_coin_permute<msrpocoin::Wide>(in, out, os, n, 12, 40)) != 0) return rc;
    if ((rc = run_coin_permute<msrpocoin::Narrow>(in, out, os, n, 24, 41)) != 0) return rc;
    std::vector<u64> src((size_t)n * 8), dig((size_t)n * 4);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 8; j++) src[(size_t)i * 8 + j] = in[(size_t)i * 12 + 4 + j];
    u64 *dsrc = nullptr, *ddst = nullptr;
    TRY(hipMalloc((void**)&dsrc, src.size() * 8));
    TRY(hipMalloc((void**)&ddst, dig.size() * 8));
    TRY(hipMemcpy(dsrc, src.data(), src.size() * 8, hipMemcpyHostToDevice));
    TRY(hipMemset(ddst, 0, dig.size() * 8));
    if (rc == 0) {
        hipLaunchKernelGGL(msrpo::rpo256_merge_level_wide, dim3((unsigned)((n + 3) / 4)), dim3(msrpo::NTW), 0, 0, (const u64*)dsrc, ddst, (size_t)n);
        TRY(hipGetLastError());
    }
    TRY(hipDeviceSynchronize());
    TRY(hipMemcpy(dig.data(), ddst, dig.size() * 8, hipMemcpyDeviceToHost));
    if (dsrc) (void)hipFree(dsrc);
    if (ddst) (void)hipFree(ddst);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 4; j++) out[(size_t)i * os + 36 + j] = dig[(size_t)i * 4 + j];
    return 0;
}
extern "C" int fp_rpo(int op, int aux, const u64* in, int is, u64* out, int os, int n, const u64* tab, int ntab) {
    switch (op) {                                       // every kernel indexes a case by these widths: refuse any other
    case 0: return is == 12 && os == 12 ? run(k_rpo, op, aux, in, is, out, os, n, tab, ntab) : -1;
    case 1: case 2: return is == 1 && os == 1 ? run(k_rpo, op, aux, in, is, out, os, n, tab, ntab) : -1;
    case 3: return is == 12 && os == 24 ? run(k_rpo, op, aux, in, is, out, os, n, tab, ntab) : -1;
    case 4: case 5: return is == 12 && os == 12 && aux >= 0 && aux < 7 ? run(k_rpo, op, aux, in, is, out, os, n, tab, ntab) : -1;
    case 100: return is == 12 && os == 24 ? run(k_rpo_mds16, op, aux, in, is, out, os, n, tab, ntab, BLOCK / 16) : -1;
    case 101: return is == 16 && os == 16 ? run(k_rpo_mds_coin, op, aux, in, is, out, os, n, tab, ntab, 1) : -1;
    case 200: return run_permute_forms(in, is, out, os, n);
    default: return -1;
    }
}
#undef TRY

#define ENTRY(name, kern)                                                                                               \
    extern "C" int name(int op, int aux, const u64* in, int is, u64* out, int os, int n, const u64* tab, int ntab) {     \
        return run(kern, op, aux, in, is, out, os, n, tab, ntab);                                                       \
    }
ENTRY(fp_gl, k_gl)
ENTRY(fp_gld, k_gld)
ENTRY(fp_limb, k_limb)
ENTRY(fp_acc, k_acc)
ENTRY(fp_f252, k_f252)
