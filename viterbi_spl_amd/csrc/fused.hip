// fused.hip -- pitch logits -> path in ONE forward launch (gfx950): the emission builder and the wave-form forward recursion
// in the same workgroup, the emission rows handed over through LDS instead of HBM.
//
// One workgroup = eight waves = four songs.  Waves 0-3 are CONSUMERS (the forward recursion of wave_forward_kernel: the rows of
// WaveHist::Full, its frame arithmetic included as text -- wave_frame_body.inc --, its per-lane setup from wave_common.hpp), waves 4-7 are PRODUCERS (the frame body of
// observation_reg_kernel -- obs_frame_body.inc), producer p building the emission rows of consumer p's song.  512 threads at 256
// registers are exactly one workgroup per CU: four songs per CU resident, larger batches run as further rounds of workgroups.
//
// Hand-off: per song two half-rings of FH rows in LDS.  In phase i the producers fill half i & 1 with frames [FH*i, FH*i + FH)
// while the consumers eat frames [FH*(i-1), FH*(i-1) + FH) from the other half; ONE workgroup barrier per phase separates them.
// No flags, no spinning: the trip count is ceil(Tmax / FH) + 1 with Tmax the longest of the workgroup's four songs, computed the
// same way by all eight waves before the loop, and no wave returns or skips a barrier -- waves of songs past B and waves whose
// song has ended keep walking the phases doing nothing.  The barrier waits for the wave's LDS operations only (lgkmcnt): the
// producers' logit rows in flight and the consumers' history stores stay in flight across it.
//
// A ring row is 384 floats with state i at float o + i, o = 384 - S (the unvoiced state last): the builder is left-aligned (lane l
// owns bins NPLP*l ..) and writes its values one by one, the recursion is right-aligned with six slots per lane (slot 6l + k =
// state 6l + k - o) and reads floats 6l .. 6l + 5 as three 8-byte pieces, one frame ahead of their use.  The o leading floats of a row
// feed idle slots whose delta is -inf + e: they are zeroed once before the first barrier (they must be finite).
#include "obs_frame.hpp"
#include "wave_common.hpp"

namespace vit {

#include "fused_wg.inc"

// NPLP bins per builder lane (5: 320 bins, 6: 360), SPW / MODE: the builder (emission.hip), UV: the recursion's uniform-lane form (wave.hip)
template <int NPLP, int SPW, int MODE, int UV>
__global__ void __launch_bounds__(512) fused_logits_kernel(FusedArgs fa) {
    __shared__ float ring[kFusedRing];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sl = wv & 3;                                 // this wave's song within the workgroup
    // lengths of the workgroup's four songs (0 past the batch): every wave computes the same phase count
    int Tl = 0, Tmax = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t sg = (int64_t)blockIdx.x * 4 + q;
        const int tq = sg < fa.f.B ? song_length(fa.f.lengths, (int)sg, fa.f.T) : 0;
        Tmax = tq > Tmax ? tq : Tmax;
        Tl = q == sl ? tq : Tl;
    }
    const int nph = (Tmax + kFusedFH - 1) / kFusedFH + 1;
    // the ring starts finite everywhere (the o leading floats of a row are never written again)
    for (int i = threadIdx.x; i < kFusedRing; i += 512) ring[i] = 0.f;
    ring_barrier();
    const int64_t song = (int64_t)blockIdx.x * 4 + sl;
    float* my = ring + sl * (2 * kFusedFH * kFusedRow);
    if (wv >= 4) fused_produce<NPLP, SPW, MODE>(fa, my, song, 0, Tl, nph, lane);
    else fused_consume<UV, FusedHist::Full>(fa.f, my, song, 0, Tl, nph, lane);
}

template <int NPLP, int SPW, int MODE>
static hipError_t launch_fused_u(const FusedArgs& fa, hipStream_t st) {
    const dim3 grid((unsigned)((fa.f.B + 3) / 4)), block(512);
    switch (fa.f.wave_u5) {
        case 1: hipLaunchKernelGGL((fused_logits_kernel<NPLP, SPW, MODE, 1>), grid, block, 0, st, fa); break;
        case 2:      // (the two-group form needs the idle slots to end at a lane boundary + 5: never with 320 bins)
            if (NPLP != 6) return hipErrorInvalidConfiguration;
            hipLaunchKernelGGL((fused_logits_kernel<6, SPW, MODE, 2>), grid, block, 0, st, fa);
            break;
        case 3: hipLaunchKernelGGL((fused_logits_kernel<NPLP, SPW, MODE, 3>), grid, block, 0, st, fa); break;
        default: return hipErrorInvalidConfiguration;
    }
    return hipGetLastError();
}

hipError_t launch_fused_logits(const FusedArgs& fa, hipStream_t st) {
    if (!fused_logits_applies(fa.f.S, fa.f.wave_ok, fa.f.wave_npl, fa.f.wave_dk, fa.f.n_extras, fa.f.wave_u5, fa.mode, fa.n_bins, fa.spw))
        return hipErrorInvalidConfiguration;
    if (fa.f.B <= 0) return hipSuccess;
    const bool b320 = fa.n_bins == 320;
    if (fa.mode == 0) return b320 ? launch_fused_u<5, 5, 0>(fa, st) : launch_fused_u<6, 5, 0>(fa, st);
    if (fa.mode == 1) return b320 ? launch_fused_u<5, 15, 1>(fa, st) : launch_fused_u<6, 15, 1>(fa, st);
    return b320 ? launch_fused_u<5, 5, 2>(fa, st) : launch_fused_u<6, 5, 2>(fa, st);
}

}  // namespace vit
