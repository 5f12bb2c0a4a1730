// fused_wg.inc -- the producer / consumer workgroup of the fused logits decode, included as TEXT inside namespace vit by fused.hip
// (fused_logits_kernel: the full history) and fused_ckpt.hip (fused_logits_ckpt_kernel: the checkpoint pass and the segment of
// vit_decode_logits_checkpointed), so that both translation units hold the same statements and compile side by side.  The scheme is
// described at the top of fused.hip.  Needs obs_frame.hpp and wave_common.hpp.
//
// FusedHist: which rows the consumer keeps -- the modes of the same names of wave.hip (WaveHist).  Full: every row, row t of a song at
// hist + t * 384, the scalars of three frames in lane 0's leading slots.  CkptPass: row (t + 1) / K - 1 for the frames t with
// (t + 1) % K == 0 (the row in front of every segment of K frames) as long as that is below hist_rows - 1, every other store to the
// song's scratch row hist_rows - 1: no branch surrounds a store.  Segment: producers and consumer start at frame t0 = t_begin, the
// consumer from init_rows[song] = delta_{t0 - 1} in slot order (a checkpoint row; idle slots and lane 0's scalar slots are reset to
// -inf), frames t0 .. min(t_end, T_b) - 1, row t at t - t0, no terminal state unless t_end >= T.  CkptPass and Segment rows carry each
// frame's own scalars only.  Phases count from t0, which need not be a multiple of the ring's FH frames: "the first frame of the
// launch" is a place in the phase (q == 0 of phase 1), and frame 0 is the log_pi path only where t0 == 0.  Full and CkptPass are
// called with a literal t0 = 0, which the compiler folds: the t0 arithmetic exists in the Segment instantiations only.
namespace {

enum class FusedHist { Full, CkptPass, Segment };

constexpr int kFusedFH = 4;            // frames per half-ring: 4 songs x 2 halves x 4 rows x 1536 B = 48 KB of LDS
constexpr int kFusedRow = 384;         // floats of a ring row = history row stride of the wave form with six states per lane
constexpr int kFusedRing = 4 * 2 * kFusedFH * kFusedRow;

// end of a phase: this wave's LDS reads and writes have completed, then the workgroup barrier.  Inline assembly on purpose: the
// compiler puts a full s_waitcnt vmcnt(0) lgkmcnt(0) in front of its own barrier, which would drain the logit loads and history stores.
__device__ __forceinline__ void ring_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- producer: the rows of frames t0 .. Tl - 1 of song `song` (Tl <= t0: no song, or none of its frames in this launch) into its two half-rings
template <int NPL, int SPW, int MODE>
__device__ __forceinline__ void fused_produce(const FusedArgs& fa, float* __restrict__ ring, const int64_t song, const int t0, const int Tl,
                                              const int nph, const int lane) {
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
    const int64_t row0 = (Tl > t0 ? song : 0) * fa.f.T;                // first row of the song in the logit and emission tensors
    const float* __restrict__ lg = fa.logits + row0 * in_stride;
    float* __restrict__ eo = fa.logE_out ? fa.logE_out + row0 * S : nullptr;
    // two logit rows in flight (two register sets); a row index past the last frame this launch builds is clamped, so no branch surrounds a load
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
    if (Tl > t0) {
        fetch(t0, xq[0], x0q[0]);
        fetch(Tl > t0 + 1 ? t0 + 1 : t0, xq[1], x0q[1]);
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
        const int tb = t0 + FH * i;
        static_assert(FH % 2 == 0, "the register set of a frame is a compile-time property of its place in the phase");
#pragma unroll
        for (int q = 0; q < FH; ++q)
            if (tb + q < Tl) process(tb + q, half + q * kFusedRow, xq[q & 1], x0q[q & 1]);
        ring_barrier();
    }
}

// ---- consumer: the forward recursion of frames t0 .. Tl - 1 of song `song` (Tl <= t0: nothing) over the rows of its two half-rings
template <int UV, FusedHist HM>
__device__ __forceinline__ void fused_consume(const FwdArgs& a, const float* __restrict__ ring, const int64_t song, const int t0, const int Tl,
                                              const int nph, const int lane) {
    constexpr int NPL = 6, D = 14, NX = 1, FH = kFusedFH;
    constexpr int H = wave_halo(NPL, D);
    constexpr int NG = 2 * H + 1;              // lane groups of the neighbourhood
    constexpr int NPM = wave_pairs(D);
    constexpr int SDW = 64 * NPL;              // history row stride of the wave form
    constexpr bool U5 = UV == 2, U3 = UV == 3;
    constexpr bool CK = HM == FusedHist::CkptPass, SG = HM == FusedHist::Segment;
    static_assert(SDW == kFusedRow && UV >= 1 && UV <= 3, "geometry");
    const int S = a.S;
    const int o = SDW - S;                                 // idle leading slots
    const int j0 = NPL * lane - o;                         // state of slot 0 of this lane (negative: idle)
    const bool l0a = lane == 0 && wave_aux_frames(NPL, S, NX) == 3;    // this lane's slots 2 .. 5 carry the scalars of frames t-1, t-2
    constexpr bool A3 = HM == FusedHist::Full; // WaveHist::Full's rows: the scalars of three frames in lane 0's leading slots
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
    float* __restrict__ hist = a.hist + (size_t)(Tl > t0 ? song : 0) * a.hist_rows * SDW;
    // (CkptPass) frames arrive in order from 0: the next checkpoint frame and its row as counters instead of a division per frame
    const int ck_scratch = (int)a.hist_rows - 1;
    int ck_next = a.ckpt_every, ck_row = 0;
    auto store_hist = [&](const int t, const float (&d)[NPL], const float M, const float (&xd)[1], const float Mp, const float (&xp)[1], const float Mq,
                          const float xq) {
#include "wave_hist_row.inc"
        int row = SG ? t - t0 : t;
        if (CK) {
            const bool hit = t + 1 == ck_next;
            row = hit && ck_row < ck_scratch ? ck_row : ck_scratch;    // checkpoint, else the scratch row
            ck_row += hit ? 1 : 0;
            ck_next += hit ? a.ckpt_every : 0;
        }
        store_row<NPL>(hist + (size_t)row * SDW + NPL * lane, v);
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
    if (SG && t0 > 0 && Tl > t0) {             // (wave-uniform) resumed: delta_{t0 - 1} and its scalars from the checkpoint row
        const float* __restrict__ ir = a.init_rows + (size_t)song * a.init_stride + NPL * lane;
#pragma unroll
        for (int k = 0; k < NPL; ++k) d[k] = j0 + k >= 0 ? ir[k] : -INFINITY;
        M = wave_frame_max<NPL>(d);
        xd[0] = wave_last_delta<NPL>(d);
    }
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
        const int tb = t0 + FH * (i - 1);
        if (i >= 1 && tb < Tl) {               // wave-uniform; no barrier inside
            const float* __restrict__ half = ring + ((i - 1) & 1) * (FH * kFusedRow);
            float er[2][NPL];
            load_ring(half, er[0]);
#pragma unroll
            for (int q = 0; q < FH; ++q) {
                if (q + 1 < FH) load_ring(half + (q + 1) * kFusedRow, er[(q + 1) & 1]);    // one frame ahead of its use
                if (tb + q < Tl) {
                    if (q == 0 && i == 1 && t0 == 0) frame0(er[0]);
                    else frame(tb + q, er[q & 1]);
                }
            }
        }
        ring_barrier();
    }
    // ---------------- terminal state: lowest-index argmax of delta_{Tl-1} (a segment: only the launch that reaches the songs' end)
    if (Tl > t0 && (!SG || a.t_end >= a.T)) {
#include "wave_terminal.inc"
        if (lane == 63) {
            a.last_state[song] = bi == kBig ? 0 : bi;
            if (a.loglik) a.loglik[song] = bv;
        }
    }
}

}  // namespace
