// torch.optim.SparseAdam's update of one table row (torch.optim._functional.sparse_adam written out), shared by
// mi_lazy_adam_rows_f32 (lazy_adam.hip) and the lazy backwards of the projector and its text columns (pinsage_proj.hip,
// pinsage_text.hip: the per-row operation of segsum::head_kernel).  For a referenced row with summed gradient g:
//     d  = g - m            m' = m + d * c1         c1 = (float)(1 - beta1)
//     s  = g*g - v          v' = v + s * c2         c2 = (float)(1 - beta2)
//     q  = m' / (sqrt(v') + (float)eps)
//     p' = p + q * ss       ss = (float)(-lr * sqrt(1 - beta2^t) / (1 - beta1^t)),  in double on the host, t = step
// Every operation is one rounding: equal bits wherever this is inlined, and tests/lazy_adam_emulation.py restates it in NumPy
// float32.  Device code is compiled with contraction on, and without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define
// __fadd_rn / __fmul_rn / __fsub_rn as the plain operators — which the compiler then contracts (a v_fma_f32 in the disassembly) —
// and __fsqrt_rn as the native v_sqrt_f32 (1 ulp).  So the chain is written with the operators under `#pragma clang fp
// contract(off)` (hipcc's -ffp-contract=fast-honor-pragmas honours it), and the square root and the division are sqrtf and /,
// which compile to the correctly rounded sequences (the default -fhip-fp32-correctly-rounded-divide-sqrt).  Rows nobody
// references are not read or written: their moments do not decay (which is what separates this from mi_adam_update4's dense
// Adam, beside the placement of the bias corrections).
#pragma once
#include "common.hpp"

struct MiLazyConsts {
    float c1, c2, eps, ss;
};

__host__ inline MiLazyConsts mi_lazy_consts(const mi_lazy_adam& a) {
    const double bc1 = 1.0 - pow(a.beta1, (double)a.step);
    const double bc2 = 1.0 - pow(a.beta2, (double)a.step);
    const double step_size = a.lr * sqrt(bc2) / bc1;
    MiLazyConsts c;
    c.c1 = (float)(1.0 - a.beta1);
    c.c2 = (float)(1.0 - a.beta2);
    c.eps = (float)a.eps;
    c.ss = (float)(-step_size);
    return c;
}

// 0, or the code to return: the hyper-parameters torch.optim.SparseAdam itself accepts, and a step that counts from 1
__host__ inline int mi_lazy_check(const mi_lazy_adam* a) {
    if (!a) return MI_ERR_BAD_ARG;
    if (!(a->lr >= 0.0) || !(a->eps >= 0.0) || !(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || a->step < 1)
        return MI_ERR_BAD_ARG;
    return 0;
}

__device__ __forceinline__ void mi_lazy_adam_update1(float& p, float g, float& m, float& v, const MiLazyConsts& c) {
#pragma clang fp contract(off)
    const float d = g - m;
    const float dm = d * c.c1;
    m = m + dm;
    const float gg = g * g;
    const float s = gg - v;
    const float dv = s * c.c2;
    v = v + dv;
    const float den = sqrtf(v) + c.eps;
    const float q = m / den;
    const float u = q * c.ss;
    p = p + u;
}

__device__ __forceinline__ void mi_lazy_adam_update4(float4& pp, const float4& gg, float4& mm, float4& vv, const MiLazyConsts& c) {
    mi_lazy_adam_update1(pp.x, gg.x, mm.x, vv.x, c);
    mi_lazy_adam_update1(pp.y, gg.y, mm.y, vv.y, c);
    mi_lazy_adam_update1(pp.z, gg.z, mm.z, vv.z, c);
    mi_lazy_adam_update1(pp.w, gg.w, mm.w, vv.w, c);
}

// The per-row operation of segsum::head_kernel: a slot with moments gets the update from its summed row, and the row reads zero
// afterwards (fused: the gradient buffer is all-zero again without a clear pass); a slot without is left to the dense optimizer.
// Ptrs4: one float4 pointer per slot with .at(slot) (segsum::Ptrs<float4, kSlots>).
template <typename Ptrs4>
struct MiLazyRowOp {
    Ptrs4 p, m, v;
    MiLazyConsts c;
    __device__ __forceinline__ void operator()(int slot, int64_t off, float4* cell) const {
        float4* mt = m.at(slot);
        if (!mt) return;
        float4 *pt = p.at(slot) + off, *vt = v.at(slot) + off;
        mt += off;
        float4 pp = *pt, mm = *mt, vv = *vt;
        mi_lazy_adam_update4(pp, *cell, mm, vv, c);
        *pt = pp;
        *mt = mm;
        *vt = vv;
        *cell = mi_f4_zero();
    }
};
