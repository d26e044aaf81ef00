// Constraint validation on the trace domain: `Stark::validate_constraints` (src/stark.rs:66-75), whose body
// `default_validate_constraints` (src/debug.rs:10-127) is a stub in the reference; its commented-out intent evaluates
// every constraint at every row with `Constraint::check` (src/constraints.rs:172-248), which gives None where a
// non-zero value is divided by zero.  Here: ONE launch for all the constraints of an AIR, a checked interpreter over the
// public opcodes of the constraint program (include/ministark_hip.h, enum ms_eval_op) run exactly as given -- none of
// the rewriting passes of eval_opt.h / eval_shift.h / eval_regroup.h and no specialised kernel: those rely on
// denominators that never vanish, and on the trace domain X^n - 1 vanishes at every row.
//
// Checked semantics (⊥ = None):
//   NEG(⊥) = ADD(⊥, .) = ADD(., ⊥) = POW(⊥, e) = EMBED(⊥) = ⊥   (every e, 0 included)
//   MUL(a, ⊥) = MUL(⊥, a) = 0 when a is defined and zero, else ⊥
//   INV(⊥) = INV(0) = ⊥, otherwise the inverse                 (an Fq3 element is zero when all three components are)
// Div(a, b) is MUL(a, INV(b)), which reproduces every arm of check's Div except one: the reference gives Div(⊥, 0) = 0
// (its arm reuses Mul's pattern), the program gives ⊥ -- it cannot tell that case from the others, and reporting the row
// is the conservative side.
//
// ⊥ is a non-canonical word, so it costs no register: every value the kernels see is canonical (include/ministark_hip.h)
// and the sentinel is all ones in the Fp word, in c0 of an Fq3 element, in the top limb of a 252-bit element.
//
// A constraint ends in its own STORE_P / STORE_Q whose `b` is its index; a ⊥ there counts toward that constraint's
// first failing row (a minimum) and number of failing rows (a sum).  The grid is fixed (grid-stride loop), so the partial
// results do not grow with n; a lane keeps its own per-constraint minimum and count, a workgroup reduces them in LDS and
// writes one partial per constraint with plain stores, and validate_finish folds the partials (a workgroup per constraint).
#pragma once
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#endif
#include "gl.h"
#include "gl_dev.h"
#include "fp252.h"
#include "stage_kernels.h"
#include "eval_kernels.h"

namespace msvalidate {

using mseval::EvalParams;
using mseval::Instr;
using mseval::NT;
static constexpr int VK = 64;              // constraints counted per launch (the host runs more in several launches)
static constexpr unsigned VGRID = 1024;    // workgroups of the grid-stride loop
static constexpr uint64_t BOT = ~0ull;     // ⊥: no canonical word is all ones
static constexpr uint64_t NONE = ~0ull;    // first failing row of a constraint that holds everywhere

// what the counting part of a launch needs besides the interpreter's parameters
struct ValParams {
    uint64_t* part_first;    // [gridDim.x][VK]
    uint64_t* part_count;    // [gridDim.x][VK]
    uint32_t k0, nk;         // this launch counts the constraints k0 .. k0 + nk - 1
};

__device__ __forceinline__ bool bot(uint64_t v) { return v == BOT; }
__device__ __forceinline__ bool bot(const gl::Fq3& v) { return v.c0 == BOT; }
__device__ __forceinline__ bool bot(const f252::E& v) { return v.l[3] == BOT; }
__device__ __forceinline__ gl::Fq3 bot_q() { return {BOT, 0, 0}; }
__device__ __forceinline__ f252::E bot_252() { return f252::E{{0, 0, 0, BOT}}; }
using mseval::ev_is_zero;

// MUL with one operand ⊥: 0 when the other one is a defined zero
template <class A, class B>
__device__ __forceinline__ bool mul_is_bot(const A& a, const B& b) {
    const bool ba = bot(a), bb = bot(b);
    return (ba && (bb || !ev_is_zero(b))) || (bb && !ev_is_zero(a));
}
template <class A, class B>
__device__ __forceinline__ bool mul_is_zero(const A& a, const B& b) { return bot(a) != bot(b); }   // (and not ⊥): one side ⊥, the other 0

// a store: count a ⊥ toward constraint b
__device__ __forceinline__ void count_store(const ValParams& V, uint32_t b, bool is_bot, size_t row, uint64_t* first, uint32_t* cnt) {
    const uint32_t c = b - V.k0;
    if (is_bot && c < V.nk) {
        if (first[c] == NONE) first[c] = row;
        cnt[c]++;
    }
}

// the lanes' per-constraint results -> one partial per workgroup and constraint (tree reductions in LDS; every lane
// reaches every barrier)
__device__ __forceinline__ void reduce_block(const ValParams& V, const uint64_t* first, const uint32_t* cnt) {
    __shared__ uint64_t s_first[NT];
    __shared__ uint64_t s_count[NT];
    const unsigned t = threadIdx.x;
    for (uint32_t c = 0; c < V.nk; c++) {
        s_first[t] = first[c];
        s_count[t] = cnt[c];
        __syncthreads();
        for (unsigned s = NT / 2; s > 0; s >>= 1) {
            if (t < s) {
                s_first[t] = s_first[t + s] < s_first[t] ? s_first[t + s] : s_first[t];
                s_count[t] += s_count[t + s];
            }
            __syncthreads();
        }
        if (t == 0) {
            V.part_first[(size_t)blockIdx.x * VK + c] = s_first[0];
            V.part_count[(size_t)blockIdx.x * VK + c] = s_count[0];
        }
        __syncthreads();
    }
}

// Goldilocks: P (Fp) and Q (Fq3) registers.  Cheap operations are computed and then selected; an inversion is skipped where its
// operand is ⊥ or zero (X^n - 1 on the trace domain: every lane of the wave).
template <int NP, int NQ>
__global__ void __launch_bounds__(NT) validate_program(EvalParams P, ValParams V) {
    using F3 = msstage::Fq3T;
    using F1 = msstage::FpT;
    uint64_t first[VK];
    uint32_t cnt[VK];
    for (uint32_t c = 0; c < V.nk; c++) { first[c] = NONE; cnt[c] = 0; }
    uint64_t rp[NP];
    gl::Fq3 rq[NQ];
    const size_t stride = (size_t)gridDim.x * NT;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += stride) {
        for (uint32_t pc = 0; pc < P.ninstr; pc++) {
            const Instr I = P.prog[pc];
            switch (I.op) {
            case mseval::OP_X_P: rp[I.dst] = mseval::ev_x(P, i); break;
            case mseval::OP_CONST_P: rp[I.dst] = P.consts[I.a]; break;
            case mseval::OP_CONST_Q: rq[I.dst] = mseval::ev_const_q(P, I.a); break;
            case mseval::OP_TRACE_P: rp[I.dst] = mseval::ev_trace_p(P, i, I.a, I.b); break;
            case mseval::OP_TRACE_Q: rq[I.dst] = mseval::ev_trace_q(P, i, I.a, I.b); break;
            case mseval::OP_PERIODIC_P: rp[I.dst] = mseval::ev_periodic_p(P, i, I.a); break;
            case mseval::OP_PERIODIC_Q: rq[I.dst] = mseval::ev_periodic_q(P, i, I.a); break;
            case mseval::OP_NEG_P: { const uint64_t a = rp[I.a]; rp[I.dst] = bot(a) ? BOT : gl::neg(a); } break;
            case mseval::OP_NEG_Q: { const gl::Fq3 a = rq[I.a]; rq[I.dst] = bot(a) ? bot_q() : gl::neg(a); } break;
            case mseval::OP_ADD_PP: { const uint64_t a = rp[I.a], b = rp[I.b]; rp[I.dst] = (bot(a) || bot(b)) ? BOT : gl::add(a, b); } break;
            case mseval::OP_ADD_QQ: { const gl::Fq3 a = rq[I.a], b = rq[I.b]; rq[I.dst] = (bot(a) || bot(b)) ? bot_q() : gl::add(a, b); } break;
            case mseval::OP_ADD_QP: {
                const gl::Fq3 a = rq[I.a]; const uint64_t b = rp[I.b];
                rq[I.dst] = (bot(a) || bot(b)) ? bot_q() : msstage::Mix<F3, F1>::add(a, b);
            } break;
            case mseval::OP_MUL_PP: {
                const uint64_t a = rp[I.a], b = rp[I.b];
                rp[I.dst] = mul_is_bot(a, b) ? BOT : mul_is_zero(a, b) ? 0 : gld::mmul(a, b);
            } break;
            case mseval::OP_MUL_QQ: {
                const gl::Fq3 a = rq[I.a], b = rq[I.b];
                rq[I.dst] = mul_is_bot(a, b) ? bot_q() : mul_is_zero(a, b) ? gl::Fq3{0, 0, 0} : F3::mul(a, b);
            } break;
            case mseval::OP_MUL_QP: {
                const gl::Fq3 a = rq[I.a]; const uint64_t b = rp[I.b];
                rq[I.dst] = mul_is_bot(a, b) ? bot_q() : mul_is_zero(a, b) ? gl::Fq3{0, 0, 0} : msstage::Mix<F3, F1>::mul(a, b);
            } break;
            case mseval::OP_INV_P: {
                const uint64_t a = rp[I.a];
                uint64_t r = BOT;
                if (!bot(a) && a != 0) r = F1::inv(a);
                rp[I.dst] = r;
            } break;
            case mseval::OP_INV_Q: {
                const gl::Fq3 a = rq[I.a];
                gl::Fq3 r = bot_q();
                if (!bot(a) && !ev_is_zero(a)) r = F3::inv(a);
                rq[I.dst] = r;
            } break;
            case mseval::OP_POW_P: { const uint64_t a = rp[I.a]; rp[I.dst] = bot(a) ? BOT : msstage::powu<F1>(a, I.b); } break;
            case mseval::OP_POW_Q: { const gl::Fq3 a = rq[I.a]; rq[I.dst] = bot(a) ? bot_q() : msstage::powu<F3>(a, I.b); } break;
            case mseval::OP_EMBED: { const uint64_t a = rp[I.a]; rq[I.dst] = bot(a) ? bot_q() : gl::Fq3{a, 0, 0}; } break;
            case mseval::OP_STORE_Q: count_store(V, I.b, bot(rq[I.a]), i, first, cnt); break;
            case mseval::OP_STORE_P: count_store(V, I.b, bot(rp[I.a]), i, first, cnt); break;
            default: break;
            }
        }
    }
    reduce_block(V, first, cnt);
}

// Fp252 (Fq = Fp): P registers only, 4-limb elements (`a` of CONST_P indexes u64 words); h_mont is the word index of the domain
// offset (one) in consts, as in eval_program252
template <int NP>
__global__ void __launch_bounds__(NT) validate_program252(EvalParams P, ValParams V) {
    using F = msstage::Fp252T;
    uint64_t first[VK];
    uint32_t cnt[VK];
    for (uint32_t c = 0; c < V.nk; c++) { first[c] = NONE; cnt[c] = 0; }
    f252::E rp[NP];
    const size_t stride = (size_t)gridDim.x * NT;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += stride) {
        for (uint32_t pc = 0; pc < P.ninstr; pc++) {
            const Instr I = P.prog[pc];
            switch (I.op) {
            case mseval::OP_X_P: rp[I.dst] = mseval::ev252_x(P, i); break;
            case mseval::OP_CONST_P: rp[I.dst] = mseval::ev252_const(P, I.a); break;
            case mseval::OP_TRACE_P: rp[I.dst] = mseval::ev252_trace(P, i, I.a, I.b); break;
            case mseval::OP_PERIODIC_P: rp[I.dst] = mseval::ev252_periodic(P, i, I.a); break;
            case mseval::OP_NEG_P: { const f252::E a = rp[I.a]; rp[I.dst] = bot(a) ? bot_252() : f252::neg(a); } break;
            case mseval::OP_ADD_PP: { const f252::E a = rp[I.a], b = rp[I.b]; rp[I.dst] = (bot(a) || bot(b)) ? bot_252() : f252::add(a, b); } break;
            case mseval::OP_MUL_PP: {
                const f252::E a = rp[I.a], b = rp[I.b];
                f252::E r = bot_252();
                if (!bot(a) && !bot(b)) r = f252::mul(a, b);
                else if (mul_is_zero(a, b) && !mul_is_bot(a, b)) r = f252::E{{0, 0, 0, 0}};
                rp[I.dst] = r;
            } break;
            case mseval::OP_INV_P: {
                const f252::E a = rp[I.a];
                f252::E r = bot_252();
                if (!bot(a) && !ev_is_zero(a)) r = f252::inv(a);
                rp[I.dst] = r;
            } break;
            case mseval::OP_POW_P: {
                const f252::E a = rp[I.a];
                f252::E r = bot_252();
                if (!bot(a)) r = msstage::powu<F>(a, I.b);
                rp[I.dst] = r;
            } break;
            case mseval::OP_STORE_P: count_store(V, I.b, bot(rp[I.a]), i, first, cnt); break;
            default: break;
            }
        }
    }
    reduce_block(V, first, cnt);
}

// the partials of `nblocks` workgroups -> out_first[c] = their minimum, out_count[c] = their sum: one workgroup per constraint c (blockIdx.x),
// each lane folds every NT-th partial, then a tree reduction in LDS
__global__ void __launch_bounds__(NT) validate_finish(const uint64_t* part_first, const uint64_t* part_count, unsigned nblocks,
                                                      uint64_t* out_first, uint64_t* out_count) {
    __shared__ uint64_t s_first[NT];
    __shared__ uint64_t s_count[NT];
    const unsigned t = threadIdx.x, c = blockIdx.x;
    uint64_t f = NONE, s = 0;
    for (unsigned b = t; b < nblocks; b += NT) {
        const uint64_t v = part_first[(size_t)b * VK + c];
        f = v < f ? v : f;
        s += part_count[(size_t)b * VK + c];
    }
    s_first[t] = f;
    s_count[t] = s;
    __syncthreads();
    for (unsigned h = NT / 2; h > 0; h >>= 1) {
        if (t < h) {
            s_first[t] = s_first[t + h] < s_first[t] ? s_first[t + h] : s_first[t];
            s_count[t] += s_count[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        out_first[c] = s_first[0];
        out_count[c] = s_count[0];
    }
}

}  // namespace msvalidate
