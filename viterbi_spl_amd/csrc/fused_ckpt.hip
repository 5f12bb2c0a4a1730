// fused_ckpt.hip -- the fused logits -> path workgroup of fused.hip under a workspace budget (gfx950): the two forward launches of
// vit_decode_logits_checkpointed.  The workgroup is fused.hip's (fused_wg.inc: eight waves, four songs, producers 4-7
// building for consumers 0-3 through two half-rings of LDS, one lgkmcnt-only barrier per phase, a trip count every wave computes the
// same way and no wave leaves early); what differs is which rows the consumer keeps (FusedHist) and, for a segment, where both start.
//
//   pass 1 (FusedHist::CkptPass)  frames 0 .. T_b - 1, the delta row in front of every segment of K frames kept, every other store to
//                                 the song's scratch row; the terminal state and the log-likelihood as in the full-history kernel
//   segment (FusedHist::Segment)  frames t_begin .. min(t_end, T_b) - 1: the producers rebuild the segment's emission rows from the logits
//                                 (the builders work per frame: the same bits as in pass 1), the consumer resumes from the checkpoint row
//
// The emission rows are built twice and never reach device memory.  A translation unit of its own so that fused.hip's instantiations
// compile to what they compiled to before, and beside them: wave.hip records what folding t_begin into a full-history kernel cost.
#include "obs_frame.hpp"
#include "wave_common.hpp"

namespace vit {

#include "fused_wg.inc"

template <int NPLP, int SPW, int MODE, int UV, bool SEG>
__global__ void __launch_bounds__(512) fused_logits_ckpt_kernel(FusedArgs fa) {
    __shared__ float ring[kFusedRing];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sl = wv & 3;                                 // this wave's song within the workgroup
    // first frame of this launch, and per song one past the last (0 past the batch): every wave computes the same phase count from the
    // longest part the four songs have left; a song that ended before t0 walks the phases doing nothing
    const int t0 = SEG ? fa.f.t_begin : 0;
    int Tl = 0, Tmax = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t sg = (int64_t)blockIdx.x * 4 + q;
        int tq = sg < fa.f.B ? song_length(fa.f.lengths, (int)sg, fa.f.T) : 0;
        if (SEG) tq = tq < fa.f.t_end ? tq : fa.f.t_end;
        const int left = tq - t0;
        Tmax = left > Tmax ? left : Tmax;
        Tl = q == sl ? tq : Tl;
    }
    const int nph = (Tmax + kFusedFH - 1) / kFusedFH + 1;
    // the ring starts finite everywhere (the o leading floats of a row are never written again)
    for (int i = threadIdx.x; i < kFusedRing; i += 512) ring[i] = 0.f;
    ring_barrier();
    const int64_t song = (int64_t)blockIdx.x * 4 + sl;
    float* my = ring + sl * (2 * kFusedFH * kFusedRow);
    if (SEG) {
        if (wv >= 4) fused_produce<NPLP, SPW, MODE>(fa, my, song, t0, Tl, nph, lane);
        else fused_consume<UV, FusedHist::Segment>(fa.f, my, song, t0, Tl, nph, lane);
    } else {
        if (wv >= 4) fused_produce<NPLP, SPW, MODE>(fa, my, song, 0, Tl, nph, lane);
        else fused_consume<UV, FusedHist::CkptPass>(fa.f, my, song, 0, Tl, nph, lane);
    }
}

template <int NPLP, int SPW, int MODE, bool SEG>
static hipError_t launch_fused_ckpt_u(const FusedArgs& fa, hipStream_t st) {
    const dim3 grid((unsigned)((fa.f.B + 3) / 4)), block(512);
    switch (fa.f.wave_u5) {
        case 1: hipLaunchKernelGGL((fused_logits_ckpt_kernel<NPLP, SPW, MODE, 1, SEG>), grid, block, 0, st, fa); break;
        case 2:      // (the two-group form needs the idle slots to end at a lane boundary + 5: never with 320 bins)
            if (NPLP != 6) return hipErrorInvalidConfiguration;
            hipLaunchKernelGGL((fused_logits_ckpt_kernel<6, SPW, MODE, 2, SEG>), grid, block, 0, st, fa);
            break;
        case 3: hipLaunchKernelGGL((fused_logits_ckpt_kernel<NPLP, SPW, MODE, 3, SEG>), grid, block, 0, st, fa); break;
        default: return hipErrorInvalidConfiguration;
    }
    return hipGetLastError();
}

template <bool SEG>
static hipError_t launch_fused_ckpt_m(const FusedArgs& fa, hipStream_t st) {
    const bool b320 = fa.n_bins == 320;
    if (fa.mode == 0) return b320 ? launch_fused_ckpt_u<5, 5, 0, SEG>(fa, st) : launch_fused_ckpt_u<6, 5, 0, SEG>(fa, st);
    if (fa.mode == 1) return b320 ? launch_fused_ckpt_u<5, 15, 1, SEG>(fa, st) : launch_fused_ckpt_u<6, 15, 1, SEG>(fa, st);
    return b320 ? launch_fused_ckpt_u<5, 5, 2, SEG>(fa, st) : launch_fused_ckpt_u<6, 5, 2, SEG>(fa, st);
}

hipError_t launch_fused_logits_ckpt(const FusedArgs& fa, bool segment, hipStream_t st) {
    if (!fused_logits_applies(fa.f.S, fa.f.wave_ok, fa.f.wave_npl, fa.f.wave_dk, fa.f.n_extras, fa.f.wave_u5, fa.mode, fa.n_bins, fa.spw))
        return hipErrorInvalidConfiguration;
    // what the two forms read of the arguments: pass 1 its segment length and at least the scratch row, a segment its frames inside
    // [0, T], rows for all of them and, where it resumes, the checkpoint rows
    if (segment ? (fa.f.t_begin < 0 || fa.f.t_end > fa.f.T || fa.f.t_end <= fa.f.t_begin || fa.f.hist_rows < fa.f.t_end - fa.f.t_begin ||
                   (fa.f.t_begin > 0 && !fa.f.init_rows))
                : (fa.f.ckpt_every < 1 || fa.f.hist_rows < 1))
        return hipErrorInvalidValue;
    if (fa.f.B <= 0) return hipSuccess;
    return segment ? launch_fused_ckpt_m<true>(fa, st) : launch_fused_ckpt_m<false>(fa, st);
}

}  // namespace vit
