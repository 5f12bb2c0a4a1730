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

namespace {

constexpr int kFusedFH = 4;            // frames per half-ring: 4 songs x 2 halves x 4 rows x 1536 B = 48 KB of LDS
constexpr int kFusedRow = 384;         // floats of a ring row = history row stride of the wave form with six states per lane
constexpr int kFusedRing = 4 * 2 * kFusedFH * kFusedRow;

// end of a phase: this wave's LDS reads and writes have completed, then the workgroup barrier.  Inline assembly on purpose: the
// compiler puts a full s_waitcnt vmcnt(0) lgkmcnt(0) in front of its own barrier, which would drain the logit loads and history stores.
__device__ __forceinline__ void ring_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- producer: the rows of song `song` (Tl frames; 0 = no song) into its two half-rings
template <int NPL, int SPW, int MODE>
__device__ __forceinline__ void fused_produce(const FusedArgs& fa, float* __restrict__ ring, const int64_t song, const int Tl, const int nph,
                                              const int lane) {
    constexpr int H = (SPW + NPL - 1) / NPL;          // lanes a lane looks at on either side
    constexpr int NA = NPL + 2 * SPW;                 // local neighbourhood: bins NPL*lane - SPW .. NPL*lane + NPL + SPW - 1
    constexpr int FH = kFusedFH;
    const int U = fa.n_bins, S = U + 1, o = kFusedRow - S;
    const double threshold = fa.threshold, offset = fa.offset, scale = fa.scale;
    const float* __restrict__ prior = fa.prior;
    const int in_stride = MODE == 1 ? U + 1 : U;
    const int in_off = MODE == 1 ? 1 : 0;
    // per-lane geometry: observation_reg_kernel's (emission.hip)
    bool real[NPL], never[NPL], first[NPL];
    float rprior[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int b = NPL * lane + k;
        real[k] = b < U;
        never[k] = b >= 1 && 2 * b <= SPW;
        first[k] = b == 0;
        rprior[k] = (MODE == 2 && prior && real[k]) ? 1.f / prior[b] : 1.f;
    }
    const float rprior_u = (MODE == 2 && prior) ? 1.f / prior[U] : 1.f;
    const int col0 = NPL * lane;
    const bool full = col0 + NPL <= U, partial = !full && col0 < U;
    const int64_t row0 = (Tl > 0 ? song : 0) * fa.f.T;                 // first row of the song in the logit and emission tensors
    const float* __restrict__ lg = fa.logits + row0 * in_stride;
    float* __restrict__ eo = fa.logE_out ? fa.logE_out + row0 * S : nullptr;
    // two logit rows in flight (two register sets); a row index past the song's end is clamped, so no branch surrounds a load
    float xq[2][NPL];
    float x0q[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < NPL; ++k) xq[q][k] = -INFINITY;
    auto fetch = [&](const int fr, float (&xn)[NPL], float& x0n) {
        const float* __restrict__ x = lg + (int64_t)fr * in_stride + in_off;
        if (full) ob_load<NPL>(x + col0, xn);
        if (partial) {
#pragma unroll
            for (int k = 0; k < NPL; ++k)
                if (real[k]) xn[k] = x[col0 + k];
        }
        if (MODE == 1) x0n = lg[(int64_t)fr * in_stride];
    };
    if (Tl > 0) {
        fetch(0, xq[0], x0q[0]);
        fetch(Tl > 1 ? 1 : 0, xq[1], x0q[1]);
    }
    auto process = [&](const int fr, float* __restrict__ row, float (&xn)[NPL], float& x0n) {
        float a[NA];
        const float x0f = x0n;
#pragma unroll
        for (int k = 0; k < NPL; ++k) a[SPW + k] = xn[k];
        fetch(fr + 2 < Tl ? fr + 2 : Tl - 1, xn, x0n);
#include "obs_frame_body.inc"
        // the row into the ring: state i at float o + i, the unvoiced state last
        float* __restrict__ r = row + o + col0;
#pragma unroll
        for (int k = 0; k < NPL; ++k)
            if (real[k]) r[k] = v[k];
        if (MODE == 2) last *= rprior_u;                 // (a peak-less frame: 1 / prior)
        const float ll = ob_log(last + kTiny);
        if (lane == 0) row[kFusedRow - 1] = ll;
        if (eo) {                                        // callers that want the emissions as well: the stand-alone builder's stores
            float* __restrict__ op = eo + (int64_t)fr * S;
            if (full) ob_store<NPL>(op + col0, v);
            if (partial) {
#pragma unroll
                for (int k = 0; k < NPL; ++k)
                    if (real[k]) op[col0 + k] = v[k];
            }
            if (lane == 0) op[U] = ll;
        }
    };
    for (int i = 0; i < nph; ++i) {
        float* __restrict__ half = ring + (i & 1) * (FH * kFusedRow);
        const int tb = FH * i;
        static_assert(FH % 2 == 0, "the register set of a frame is a compile-time property of its place in the phase");
#pragma unroll
        for (int q = 0; q < FH; ++q)
            if (tb + q < Tl) process(tb + q, half + q * kFusedRow, xq[q & 1], x0q[q & 1]);
        ring_barrier();
    }
}

// ---- consumer: the forward recursion of song `song` (Tl frames; 0 = no song) over the rows of its two half-rings
template <int UV>
__device__ __forceinline__ void fused_consume(const FwdArgs& a, const float* __restrict__ ring, const int64_t song, const int Tl, const int nph,
                                              const int lane) {
    constexpr int NPL = 6, D = 14, NX = 1, FH = kFusedFH;
    constexpr int H = wave_halo(NPL, D);
    constexpr int NG = 2 * H + 1;              // lane groups of the neighbourhood
    constexpr int NPM = wave_pairs(D);
    constexpr int SDW = 64 * NPL;              // history row stride of the wave form
    constexpr bool U5 = UV == 2, U3 = UV == 3;
    static_assert(SDW == kFusedRow && UV >= 1 && UV <= 3, "geometry");
    const int S = a.S;
    const int o = SDW - S;                                 // idle leading slots
    const int j0 = NPL * lane - o;                         // state of slot 0 of this lane (negative: idle)
    const bool l0a = lane == 0 && wave_aux_frames(NPL, S, NX) == 3;    // this lane's slots 2 .. 5 carry the scalars of frames t-1, t-2
    constexpr bool A3 = true;                  // WaveHist::Full's rows: the scalars of three frames in lane 0's leading slots
#include "wave_lane_weights.inc"
    float cj[NPL];
    float xa[1][NPL];
    float lp[NPL];
    {
        const float* __restrict__ rc = reinterpret_cast<const float*>(a.image + a.off_rowc);
        const float* __restrict__ xaT = reinterpret_cast<const float*>(a.image + a.off_extraA);
        const float* __restrict__ lpi = reinterpret_cast<const float*>(a.image + a.off_logpi);
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int j = j0 + k;
            cj[k] = j >= 0 ? rc[j] : -INFINITY;
            xa[0][k] = j >= 0 ? xaT[j] : -INFINITY;
            lp[k] = j >= 0 ? lpi[j] : -INFINITY;
        }
    }
    float* __restrict__ hist = a.hist + (size_t)(Tl > 0 ? song : 0) * a.hist_rows * SDW;
    auto store_hist = [&](const int t, const float (&d)[NPL], const float M, const float (&xd)[1], const float Mp, const float (&xp)[1], const float Mq,
                          const float xq) {
#include "wave_hist_row.inc"
        store_row<NPL>(hist + (size_t)t * SDW + NPL * lane, v);
    };
    // this lane's six values of a ring row: floats 6l .. 6l + 5, 8-byte aligned
    auto load_ring = [&](const float* __restrict__ row, float (&e)[NPL]) {
        const f32x2* __restrict__ p = reinterpret_cast<const f32x2*>(row + NPL * lane);
#pragma unroll
        for (int m = 0; m < NPL / 2; ++m) { const f32x2 v = p[m]; e[2 * m] = v.x; e[2 * m + 1] = v.y; }
    };
    float d[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) d[k] = -INFINITY;
    float M = 0.f, Mb = 0.f, xb = 0.f;
    float xd[1] = {0.f};
#pragma unroll
    for (int k = 0; k < NPL; ++k)
#pragma unroll
        for (int m = 0; m < NPM; ++m) asm volatile("" ::"v"(aw[k][m]));

    auto frame0 = [&](const float (&e)[NPL]) {             // delta_0 = log_pi + e_0
#pragma unroll
        for (int k = 0; k < NPL; ++k) d[k] = j0 + k >= 0 ? lp[k] + e[k] : -INFINITY;
        M = wave_frame_max<NPL>(d);
        xd[0] = wave_last_delta<NPL>(d);
        store_hist(0, d, M, xd, M, xd, M, xd[0]);
        Mb = M;
        xb = xd[0];
    };
    auto frame = [&](const int t, const float (&e)[NPL]) {
#include "wave_frame_body.inc"
        const float Mp = M, xp[1] = {xd[0]};   // the previous frame's scalars (wave-uniform: scalar registers)
        M = wave_frame_max<NPL>(d);
        xd[0] = wave_last_delta<NPL>(d);   // for the next frame's candidates, and for the history row
        store_hist(t, d, M, xd, Mp, xp, Mb, xb);
        Mb = Mp;
        xb = xp[0];
    };
    for (int i = 0; i < nph; ++i) {
        const int tb = FH * (i - 1);
        if (i >= 1 && tb < Tl) {               // wave-uniform; no barrier inside
            const float* __restrict__ half = ring + ((i - 1) & 1) * (FH * kFusedRow);
            float er[2][NPL];
            load_ring(half, er[0]);
#pragma unroll
            for (int q = 0; q < FH; ++q) {
                if (q + 1 < FH) load_ring(half + (q + 1) * kFusedRow, er[(q + 1) & 1]);    // one frame ahead of its use
                if (tb + q < Tl) {
                    if (q == 0 && i == 1) frame0(er[0]);
                    else frame(tb + q, er[q & 1]);
                }
            }
        }
        ring_barrier();
    }
    // ---------------- terminal state: lowest-index argmax of delta_{Tl-1}
    if (Tl > 0) {
#include "wave_terminal.inc"
        if (lane == 63) {
            a.last_state[song] = bi == kBig ? 0 : bi;
            if (a.loglik) a.loglik[song] = bv;
        }
    }
}

}  // namespace

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
    if (wv >= 4) fused_produce<NPLP, SPW, MODE>(fa, my, song, Tl, nph, lane);
    else fused_consume<UV>(fa.f, my, song, Tl, nph, lane);
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
