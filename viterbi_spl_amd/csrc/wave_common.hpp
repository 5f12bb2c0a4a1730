// wave_common.hpp -- what the wave-form forward kernels (wave.hip, and the consumer waves of fused.hip) share besides their frame
// arithmetic (wave_frame_body.inc) and terminal arg-max (wave_terminal.inc): the history mode as a type with its properties, the one
// function from FwdArgs to the mode, the table of what a mode instantiates, and the per-lane setup as inlined helpers.
#pragma once
#include "device_common.hpp"

namespace vit {

// What wave_forward_kernel keeps of the delta rows and whose rows a wave computes.  The values are part of the kernels' names.
enum class WaveHist : int {
    Full = 0,            // every row: row t of a song at hist + t * 64*NPL                                     (vit_decode)
    Half = 1,            // the rows of EVEN frames only, the scalars of the odd frame in front riding along   ("wave_history" 2)
    NoStores = 2,        // timing builds only (results wrong): Full without the history stores,
    NoLoads = 3,         //   without the emission loads,
    NoLoadsNoStores = 4, //   without either
    CkptPass = 5,        // checkpoint rows only, every other store to one scratch row per song       (vit_decode_checkpointed, pass 1)
    Segment = 6,         // frames t_begin .. t_end - 1 resumed from init_rows, row t at t - t_begin   (vit_decode_checkpointed, pass 2)
    Packed = 7,          // a wave is a SLOT that walks a list of songs; rows at the songs' offsets    (vit_decode_packed)
    PackedSegment = 8,   // a wave is a UNIT: Segment for segment unit_seg[u] of song unit_song[u]     (vit_decode_packed_checkpointed, pass 2)
    PackedCkptPass = 9,  // the slot walk of Packed with the stores of CkptPass                         (vit_decode_packed_checkpointed, pass 1)
};
enum class WaveRows { Every, Even, Checkpoints };     // which frames' rows are kept
enum class WaveBase { Song, Offset, Unit, Shared };   // where a song's rows start in hist: song * hist_rows | offsets[song] | wave * hist_rows | 0 (rows ckpt_base[song] ..)
struct WaveHistTraits {
    bool slot_walk;     // the wave walks the songs slot_songs[slot_begin[w] .. slot_begin[w + 1]) back to back
    bool unit;          // the wave's song and segment come from unit_song / unit_seg
    bool segment;       // one segment, resumed from a checkpoint row; the terminal state is the checkpoint pass's business
    bool offsets;       // a song's emission rows and its length come from offsets, not from T and lengths
    WaveRows rows;
    WaveBase base;
    bool aux3;          // every row kept: with one extra column and six idle slots row t also carries the scalars of frames t-1 and t-2
    bool loads, stores; // false in the timing-only modes
};
constexpr WaveHistTraits wave_hist_traits(WaveHist h) {
    switch (h) {
        case WaveHist::Full: return {false, false, false, false, WaveRows::Every, WaveBase::Song, true, true, true};
        case WaveHist::Half: return {false, false, false, false, WaveRows::Even, WaveBase::Song, false, true, true};
        case WaveHist::CkptPass: return {false, false, false, false, WaveRows::Checkpoints, WaveBase::Song, false, true, true};
        case WaveHist::Segment: return {false, false, true, false, WaveRows::Every, WaveBase::Song, true, true, true};
        case WaveHist::Packed: return {true, false, false, true, WaveRows::Every, WaveBase::Offset, true, true, true};
        case WaveHist::PackedSegment: return {false, true, true, true, WaveRows::Every, WaveBase::Unit, true, true, true};
        case WaveHist::PackedCkptPass: return {true, false, false, true, WaveRows::Checkpoints, WaveBase::Shared, false, true, true};
        default: return {false, false, false, false, WaveRows::Every, WaveBase::Song, false, h == WaveHist::NoStores, h == WaveHist::NoLoads};   // timing-only
    }
}

// The mode a launch runs, from what capi.hip sets in FwdArgs.  This order is the precedence, and it is written here only.
constexpr WaveHist wave_hist_of(const FwdArgs& a) {
#ifdef VIT_TIMING_HOOKS
    // result-breaking ablations (make TIMING=1 only): bits 0 / 1 of the timing mask drop the history stores / the emission loads
    if (a.debug & 3) return (a.debug & 3) == 1 ? WaveHist::NoStores : ((a.debug & 3) == 2 ? WaveHist::NoLoads : WaveHist::NoLoadsNoStores);
#endif
    if (a.ckpt_base) return a.unit_song ? WaveHist::PackedSegment : WaveHist::PackedCkptPass;
    if (a.offsets) return WaveHist::Packed;
    if (a.ckpt_every > 0) return WaveHist::CkptPass;
    if (a.t_begin > 0 || a.t_end < a.T) return WaveHist::Segment;
    return a.hist_half ? WaveHist::Half : WaveHist::Full;
}

// What a mode instantiates and how a launch chooses (launch_wave_mode, wave.hip).  Every mode has the 512-register form (one wave
// per SIMD, PF1 rows in flight; up to 1024 waves, with wave_flags bit 1 or two extra columns) and the general 256-register form
// (two waves per SIMD, PF2 rows, UV 0).  The UV forms are 256-register ones, for one extra column (UV 2 / 3: six states per lane).
struct WaveLaunch {
    bool uv1;        // the last-state form alone, FwdArgs::wave_u5 >= 1
    bool uv23;       // the uniform-lane forms, wave_u5 2 / 3
    bool by_slots;   // the waves of the launch: n_slots, else B (songs, or units)
    bool flag0;      // wave_flags bit 0 forces the 256-register form
};
constexpr WaveLaunch wave_launch_of(WaveHist h) {
    switch (h) {
        case WaveHist::Full:
        case WaveHist::Half: return {true, true, false, true};
        case WaveHist::Packed:
        case WaveHist::PackedCkptPass: return {true, true, true, false};    // (the packed launches never honoured bit 0)
        case WaveHist::PackedSegment: return {false, true, false, false};   // no UV 1: its fp16 instantiation takes 292 bytes of scratch, the general one none
        default: return {false, false, false, true};                        // CkptPass, Segment and the timing-only modes: no UV forms
    }
}

// ---- NPL consecutive columns as 16-, 8- and 4-byte pieces (float16 emissions: 8, 4, 2), element-aligned
template <typename ET> struct RowVec;
template <> struct RowVec<float> { typedef float E; typedef f32x4_u V4; typedef f32x2_u V2; };
template <> struct RowVec<__half> { typedef _Float16 E; typedef f16x4_u V4; typedef f16x2_u V2; };

template <int NPL, typename ET>
__device__ __forceinline__ void load_cols(const ET* __restrict__ pe, float (&e)[NPL]) {
    typedef RowVec<ET> R;
    const typename R::E* p = reinterpret_cast<const typename R::E*>(pe);
    int k = 0;
#pragma unroll
    for (; k + 3 < NPL; k += 4) { const typename R::V4 v = *reinterpret_cast<const typename R::V4*>(p + k); e[k] = (float)v.x; e[k + 1] = (float)v.y; e[k + 2] = (float)v.z; e[k + 3] = (float)v.w; }
#pragma unroll
    for (; k + 1 < NPL; k += 2) { const typename R::V2 v = *reinterpret_cast<const typename R::V2*>(p + k); e[k] = (float)v.x; e[k + 1] = (float)v.y; }
    if (k < NPL) e[k] = (float)p[k];
}

template <int NPL>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&d)[NPL]) {
    int k = 0;
#pragma unroll
    for (; k + 3 < NPL; k += 4) { f32x4_u v; v.x = d[k]; v.y = d[k + 1]; v.z = d[k + 2]; v.w = d[k + 3]; *reinterpret_cast<f32x4_u*>(p + k) = v; }
#pragma unroll
    for (; k + 1 < NPL; k += 2) { f32x2_u v; v.x = d[k]; v.y = d[k + 1]; *reinterpret_cast<f32x2_u*>(p + k) = v; }
    if (k < NPL) p[k] = d[k];
}

// ---- per-lane pieces (the weight loads and the history-row assembly are text: wave_lane_weights.inc, wave_hist_row.inc)
// maximum of delta over the wave, wave-uniform
template <int NPL>
__device__ __forceinline__ float wave_frame_max(const float (&v)[NPL]) {
    float loc = v[0];
#pragma unroll
    for (int k = 1; k < NPL; ++k) loc = fmaxf(loc, v[k]);
    return wave_max_all(loc);
}
// delta of the one extra column where it is the last state (UV >= 1): state S-1 = lane 63, last slot
template <int NPL>
__device__ __forceinline__ float wave_last_delta(const float (&v)[NPL]) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[NPL - 1]), 63));
}

}  // namespace vit
