// obs_frame.hpp -- constants and device helpers of the register-form emission builders (pitch logits -> log observation
// probabilities), shared by observation_reg_kernel (emission.hip: rows to HBM) and fused_logits_kernel (fused.hip: rows into the
// LDS ring of the forward recursion).  The frame body itself is obs_frame_body.inc.
#pragma once
#include "device_common.hpp"

namespace vit {

constexpr float kTiny = 1.1754944e-38f;        // np.finfo(np.float32).tiny
constexpr float kLogTiny = -87.33654475f;      // float32 log(tiny) = -87.33655 (bits 0xC2AEAC50)

namespace {

// a lane's NPL consecutive floats as 16- / 8- / 4-byte pieces at 4-byte alignment (coalesced across the wave)
template <int NPL>
__device__ __forceinline__ void ob_load(const float* __restrict__ p, float (&v)[NPL]) {
    int k = 0;
#pragma unroll
    for (; k + 3 < NPL; k += 4) { const f32x4_u t = *reinterpret_cast<const f32x4_u*>(p + k); v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w; }
#pragma unroll
    for (; k + 1 < NPL; k += 2) { const f32x2_u t = *reinterpret_cast<const f32x2_u*>(p + k); v[k] = t.x; v[k + 1] = t.y; }
    if (k < NPL) v[k] = p[k];
}
template <int NPL>
__device__ __forceinline__ void ob_store(float* __restrict__ p, const float (&v)[NPL]) {
    int k = 0;
#pragma unroll
    for (; k + 3 < NPL; k += 4) { f32x4_u t; t.x = v[k]; t.y = v[k + 1]; t.z = v[k + 2]; t.w = v[k + 3]; *reinterpret_cast<f32x4_u*>(p + k) = t; }
#pragma unroll
    for (; k + 1 < NPL; k += 2) { f32x2_u t; t.x = v[k]; t.y = v[k + 1]; *reinterpret_cast<f32x2_u*>(p + k) = t; }
    if (k < NPL) p[k] = v[k];
}

__device__ __forceinline__ float ob_wave_sum(float x) {   // inclusive scan by rows, lane 63 holds the total
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(x));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
// e^x through v_exp_f32 (2^y, 1 ulp): log2(e) = hi + lo, the rounding error of x * hi is recovered with an fma and applied as
// the factor 2^lo ~ 1 + lo ln 2 -- ~2 ulp where a plain x * log2(e) would lose |x| * 1e-7
__device__ __forceinline__ float ob_exp(float x) {
    const float hi = x * 1.44269502f;
    const float lo = __builtin_fmaf(x, 1.44269502f, -hi);              // the product's rounding error, exactly
    const float e2 = __builtin_amdgcn_exp2f(hi);
    return __builtin_fmaf(e2, lo * 0.693147182f, e2);                   // (what float(log2 e) itself is off by adds |x| * 1.3e-8: < 1 ulp up to |x| = 8)
}
// e^x for any x: v_exp_f32 flushes results below 2^-126 (x < -87.34) to 0, where float32 has subnormals (down to e^-103.3) and the
// reference's np.exp keeps them.  There the exponent is raised by 64 before the instruction and the result scaled by 2^-64 after it:
// one rounding into the subnormal range, as a full expf does.  (e^-1000 is still 0.)
__device__ __forceinline__ float ob_exp_far(float x) {
    const float hi = x * 1.44269502f;
    const float lo = __builtin_fmaf(x, 1.44269502f, -hi);
    const bool sub = hi < -126.f;
    const float e2 = __builtin_amdgcn_exp2f(sub ? hi + 64.f : hi);    // (hi + 64 is exact)
    const float r = __builtin_fmaf(e2, lo * 0.693147182f, e2);
    return sub ? r * 5.42101086e-20f : r;                               // 2^-64
}
// ln y through v_log_f32 (log2, 1 ulp), ln 2 = hi + lo
__device__ __forceinline__ float ob_log(float y) {
    const float l2 = __builtin_amdgcn_logf(y);
    return __builtin_fmaf(l2, 0.693147182f, l2 * -1.90465421e-9f);
}

}  // namespace

}  // namespace vit
