// device_common.hpp -- device helpers shared by the gfx950 (MI355X) kernel files of the float32 log-domain Viterbi decoder.
//
// Semantics (reference: imm/tf_viterbi.py:91-107, tonet/for_paper.py:1855-1868):
//   delta_0[j]  = fl32(log_pi[j] + logE[0][j])
//   m_j         = max_i fl32(delta_{t-1}[i] + logA_T[j][i]);  psi_t[j] = LOWEST i attaining it
//   delta_t[j]  = fl32(m_j + logE[t][j])
//   s_{T-1}     = lowest argmax_j delta_{T-1}[j];  s_t = psi_{t+1}[s_{t+1}]
// Only add / compare / select (built with -ffp-contract=off): bit-identical to the reference's
// NumPy float32 loop.
//
// "Lazy back-pointers": gfx950 retires one wave64 VALU instruction per 4 cycles per SIMD, and
// tracking the argmax index of every (frame, state) costs more instructions than the max itself,
// while the back-trace consumes ONE back-pointer per frame.  So
//   * the forward kernels are value-only (packed adds + max3) and store the delta row of every
//     frame (the reference's T1, tonet/for_paper.py:1852) instead of the back-pointer rows (T2);
//   * the back-trace recomputes psi_{t+1}[s_{t+1}] exactly -- the same fl32 sums, first index
//     attaining the max -- only for the state on the path.
// No MFMA: the recurrence is max-plus, not an add-contract.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"

namespace vit {

inline constexpr int kBig = 0x7fffffff;           // index sentinel: "no state yet" (loses every first-max tie)
inline constexpr size_t kLdsBytes = 160 * 1024;   // LDS of one CU (gfx950): the most one workgroup can allocate

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// element-aligned vector views: a lane's columns start on a 4-byte (f32) / 2-byte (f16) boundary only
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2_u __attribute__((ext_vector_type(2), aligned(4)));
typedef int i32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef _Float16 f16x2_u __attribute__((ext_vector_type(2), aligned(2)));
typedef _Float16 f16x4_u __attribute__((ext_vector_type(4), aligned(2)));

// frames of song `song`: lengths[song] clamped to [1, T] (T when there is no lengths tensor)
__device__ __forceinline__ int song_length(const int64_t* lengths, int song, int T) {
    if (!lengths) return T;
    long long v = lengths[song];
    v = v < 1 ? 1 : v;
    return v > T ? T : (int)v;
}
// min(max(x, 0), hi): one v_med3_i32
__device__ __forceinline__ int clamp_med3(int x, int hi) {
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(x), "s"(hi));
    return r;
}

template <typename ET>
__device__ __forceinline__ float load_e(const ET* p);
template <>
__device__ __forceinline__ float load_e<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float load_e<__half>(const __half* p) { return __half2float(*p); }

// ---- value-only wave primitives
// Inclusive prefix max over lanes 0..lane: six v_max_f32 with a DPP source operand
// (row_shr:1/2/4/8, row_bcast:15 on rows 1,3, row_bcast:31 on rows 2,3).  A lane whose DPP source
// is invalid or whose row is masked is not written and keeps its own value.  The s_nop 1 pairs are
// the two wait states a DPP read of a just-written VGPR needs.
__device__ __forceinline__ float wave_scan_max(float x) {
    asm volatile(
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(x));
    return x;
}
// max over all 64 lanes, returned in every lane (wave-uniform)
__device__ __forceinline__ float wave_max_all(float x) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_scan_max(x)), 63));
}
// ---- the same on doubles (f64.hip): the two halves travel through DPP moves, the max is one v_max_f64 per step
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_max_step_f64(const double x) {
    const long long b = __double_as_longlong(x);
    const int lo = (int)(unsigned)(b & 0xffffffffll), hi = (int)(b >> 32);
    // a lane without a source (or in a masked row) keeps its own value: max(x, x) = x
    const int slo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int shi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const double s = __longlong_as_double(((long long)shi << 32) | (long long)(unsigned)slo);
    return fmax(x, s);
}
// inclusive prefix max over lanes 0 .. lane (the row_shr / row_bcast ladder of wave_scan_max): lane 63 holds the wave's maximum
__device__ __forceinline__ double wave_scan_max_f64(double x) {
    x = dpp_max_step_f64<0x111, 0xf>(x);
    x = dpp_max_step_f64<0x112, 0xf>(x);
    x = dpp_max_step_f64<0x114, 0xf>(x);
    x = dpp_max_step_f64<0x118, 0xf>(x);
    x = dpp_max_step_f64<0x142, 0xa>(x);
    x = dpp_max_step_f64<0x143, 0xc>(x);
    return x;
}
__device__ __forceinline__ double readlane_f64(const double x, const int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_max_all_f64(const double x) { return readlane_f64(wave_scan_max_f64(x), 63); }
// max(x[l], x[l ^ 32]) in every lane: v_permlane32_swap exchanges the upper 32 lanes of its first operand with the lower 32
// of its second; fed two copies of x it leaves {x.lo, x.lo} and {x.hi, x.hi}
__device__ __forceinline__ float max_other_half(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// max(x[l], x[l ^ 8]) in every lane: row_ror:8 turns each row of sixteen lanes by half a row, and the compiler folds the move into
// the maximum (one v_max_f32_dpp).  Every lane has a source, so the old value is never taken.
inline constexpr int kDppRowRor8 = 0x128;
__device__ __forceinline__ float max_lane_xor8(float x) {
    return fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kDppRowRor8, 0xf, 0xf, false)));
}
// ---- LDS stores without an address register (ds_write_addtid_b32): lane l stores its dword at byte M0[15:0] + BYTE_OFF + 4 * l.
// The instruction hands the LDS one register instead of two and takes half the issue time of ds_write_b32 (measured:
// scripts/ubench/lds_store_tail.hip).  M0 is set by lds_addtid_base, ONCE in front of a loop of stores -- as an input operand of the
// store the compiler re-issued the s_mov in every iteration.  The compiler does not know either asm as an LDS operation: the "memory"
// clobber keeps its own LDS accesses on their side of the store, but it counts no lgkmcnt for it, so whoever needs the store
// to have landed (a barrier) states s_waitcnt lgkmcnt(0) himself.  Nothing else between base and stores may write M0 (check the .s).
// `p` points into LDS; the base is its 32-bit LDS address (wave-uniform), which must fit 16 bits together with every BYTE_OFF used.
__device__ __forceinline__ void lds_addtid_base(const float* p) {
    const unsigned base = (unsigned)(unsigned long)(__attribute__((address_space(3))) const float*)p;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(base) : "memory");   // (one wait state between an M0 write and an add-tid store)
}
template <int BYTE_OFF>
__device__ __forceinline__ void lds_store_addtid(float v) {
    static_assert(BYTE_OFF >= 0 && BYTE_OFF < 65536 && BYTE_OFF % 4 == 0, "the instruction's 16-bit offset field");
    asm volatile("ds_write_addtid_b32 %0 offset:%1" ::"v"(v), "n"(BYTE_OFF) : "memory");
}
// Four add-tid stores of v (byte offsets O0 .. O3 from M0, as lds_store_addtid) and the maximum of v over the lane's quad (fm_publish's
// two DPP steps), one statement.  A DPP step may read a register two wait states behind the VALU instruction that wrote it, and every
// instruction issued in between is one: the first step stands behind the first two stores, the second behind the other two, and v
// itself may come from the instruction right in front of the statement.  Left to the compiler, whose hazard recognizer counts no
// instruction inside an asm statement, the same six instructions took an s_nop 1 in front of each step.
// KEEP TWO INSTRUCTIONS IN FRONT OF EACH STEP: the compiler knows nothing of the DPP reads in this string and pads nothing inside it.
// Whoever reorders it, drops a store or reuses it with another mix must leave at least two instructions (or an s_nop 1) between the
// start of the string and the first step -- the writer of v may be the instruction in front of the statement -- and between the two steps.
// Counts, waits and M0 as for lds_store_addtid: the compiler counts no lgkmcnt for these stores.
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ float lds_store_addtid4_quad_max(float v) {
    static_assert(O0 >= 0 && O1 >= 0 && O2 >= 0 && O3 >= 0 && O0 < 65536 && O1 < 65536 && O2 < 65536 && O3 < 65536 &&
                  (O0 | O1 | O2 | O3) % 4 == 0, "the instruction's 16-bit offset field");
    float q;
    asm volatile("ds_write_addtid_b32 %1 offset:%2\n\tds_write_addtid_b32 %1 offset:%3\n\t"
                 "v_max_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "ds_write_addtid_b32 %1 offset:%4\n\tds_write_addtid_b32 %1 offset:%5\n\t"
                 "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                 : "=&v"(q) : "v"(v), "n"(O0), "n"(O1), "n"(O2), "n"(O3) : "memory");
    return q;
}
// lane l <- x[l-1], lane 0 <- fill   (wave_shr:1)
__device__ __forceinline__ float wave_shift_up(float x, float fill) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x138, 0xf, 0xf, false));
}
// lane l <- x[l+1], lane 63 <- fill   (wave_shl:1)
__device__ __forceinline__ float wave_shift_down(float x, float fill) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x130, 0xf, 0xf, false));
}
// The same shifts with bound_ctrl: the lane without a source reads 0 and no fill value is moved in (one v_mov fewer per
// shift).  For callers to whom that lane's value does not matter.
__device__ __forceinline__ float dpp_shr1(float x) {   // lane l <- x[l-1]
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_shl1(float x) {   // lane l <- x[l+1]
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x130, 0xf, 0xf, true));
}

// ---- (value, index) first-max wave primitives
struct VI {
    float v;
    int i;
};

__device__ __forceinline__ VI vi_identity() { return VI{-INFINITY, kBig}; }
// first-max: `later` (higher index) replaces `earlier` only if strictly greater
__device__ __forceinline__ VI op_fwd(VI earlier, VI later) { return later.v > earlier.v ? later : earlier; }
// pieces visited in DESCENDING index order: the next (lower-index) piece wins ties
__device__ __forceinline__ VI op_rev(VI acc, VI next) { return next.v >= acc.v ? next : acc; }

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ VI dpp_fetch(VI x) {
    VI r;
    r.v = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(x.v), CTRL,
                                                     ROW_MASK, 0xf, false));
    r.i = __builtin_amdgcn_update_dpp(kBig, x.i, CTRL, ROW_MASK, 0xf, false);
    return r;
}

// Inclusive wave64 scan with the ordered first-max operator (value, index).
// DPP: row_shr:1/2/4/8 inside each row of 16, then row_bcast:15 (rows 1,3), row_bcast:31 (rows 2,3).
template <bool REV>
__device__ __forceinline__ VI wave_scan(VI x) {
#define VIT_SCAN_STEP(CTRL, MASK)                        \
    {                                                    \
        VI s = dpp_fetch<CTRL, MASK>(x);                 \
        x = REV ? op_rev(s, x) : op_fwd(s, x);           \
    }
    VIT_SCAN_STEP(0x111, 0xf)
    VIT_SCAN_STEP(0x112, 0xf)
    VIT_SCAN_STEP(0x114, 0xf)
    VIT_SCAN_STEP(0x118, 0xf)
    VIT_SCAN_STEP(0x142, 0xa)
    VIT_SCAN_STEP(0x143, 0xc)
#undef VIT_SCAN_STEP
    return x;
}

// Workgroup-wide lowest-index argmax of delta (terminal state); every thread of the workgroup calls.
__device__ __forceinline__ void terminal_argmax(float dj, int j, bool valid, VI* tot, int nw, int32_t* last_state,
                                                float* loglik, int song) {
    VI x{valid ? dj : -INFINITY, valid ? j : kBig};
    x = wave_scan<false>(x);
    if ((threadIdx.x & 63) == 63) tot[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        VI acc = vi_identity();
        for (int b = 0; b < nw; ++b) acc = op_fwd(acc, tot[b]);
        if (acc.i == kBig) acc.i = 0;
        last_state[song] = acc.i;
        if (loglik) loglik[song] = acc.v;
    }
}

// The same for callers that hold their wave index in a scalar register (`wave`, wave-uniform) and their lane: the slot of `tot` is
// scalar arithmetic, and no per-thread address has to stay in a vector register up to the call (kernels that call it once per
// song of a list with every register spoken for).
__device__ __forceinline__ void terminal_argmax_w(float dj, int j, bool valid, VI* tot, int nw, int wave, int lane, int32_t* last_state,
                                                  float* loglik, int song) {
    VI x{valid ? dj : -INFINITY, valid ? j : kBig};
    x = wave_scan<false>(x);
    if (lane == 63) tot[wave] = x;
    __syncthreads();
    if (wave == 0 && lane == 0) {
        VI acc = vi_identity();
        for (int b = 0; b < nw; ++b) acc = op_fwd(acc, tot[b]);
        if (acc.i == kBig) acc.i = 0;
        last_state[song] = acc.i;
        if (loglik) loglik[song] = acc.v;
    }
}

}  // namespace vit
