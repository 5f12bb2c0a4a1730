// f64.hip -- the float64-accumulating decode (vit_decode_f64): the reference's float64 Viterbi variant
// (dcnet/tf_viterbi_decoding.py:209-263), whose T1 is float64 while its parameters and emissions are float32.
//
//   d_0[j]  = f64( fl32(log_pi[j] + E_0[j]) )              (the reference adds two float32 arrays, then stores into T1)
//   m_j     = max_i fl64( d_{t-1}[i] + f64(A[j][i]) );      psi_t[j] = LOWEST i attaining m_j
//   d_t[j]  = fl64( m_j + f64(E_t[j]) )
//   s_{T-1} = lowest argmax_j d_{T-1}[j];  s_t = psi_{t+1}[s_{t+1}];  loglik = d_{T-1}[s_{T-1}]
//
// Forward (f64_floor_forward_kernel): the floor form of banded.hip in double.  Rounding to float64 is monotone as rounding to
// float32 is, so with M = max of d_{t-1} over the non-extra sources
//   m_j = max( window candidates, fl64(M + c_j), extra-column candidates )
// is the dense value for every plan whose floor form is proven (plan.floor_ok): the plan image is read as it is.  One song per
// workgroup, one target per lane, value-only; the history keeps every d row and M_t ([B, T, SD64] doubles, state i in column i,
// M_t in column S).
// Back-trace (f64_backtrace_kernel): lazy_backtrace_kernel's banded case in double under the chunk scheme of backtrace_common.hpp
// (bt_run_chunks: a speculative pass per (song, chunk), a verify / repair pass per song).
// Both kernels take one F64Variant (kernels.hpp), described at each.  Packed (vit_decode_f64_packed): a workgroup per forward slot
// that walks its songs back to back, back-trace waves over per-song chunk lists, rows at offsets[b] of the packed buffers.
// Ckpt (vit_decode_f64_checkpointed): the forward kernel as pass 1 (checkpoint rows only) or over one segment resumed from a
// checkpoint row, the back-trace over one segment's sub-problems.  PackedCkpt (vit_decode_f64_packed_checkpointed): the two combined --
// pass 1 as a slot walk that keeps checkpoint rows only, pass 2 over (song, segment) units.
// The wave primitives on doubles are device_common.hpp's (wave_scan_max_f64, wave_max_all_f64), the lowest-index argmax of a d row is
// the double overload of bt_row_argmax (backtrace_common.hpp).
#include "backtrace_common.hpp"

namespace vit {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------
// Forward kernel
// ---------------------------------------------------------------------------------------
// LDS, in doubles from the start of the dynamic segment.  d lives in two copies per buffer: copy c holds d[i] at index i + c, so a lane
// whose window starts at source lo reads it from copy lo & 1 at the even index lo + (lo & 1) -- 16-byte reads throughout.  The copy
// stride DC = 14 mod 32 puts the two copies 128 bytes (mod 256) apart: the eight lanes of a 16-lane read group that read copy 0 and the
// eight that read copy 1 (consecutive targets, consecutive window starts) cover all 64 banks once.
// W > 64 on twelve waves (three waves per SIMD: 168 registers) keeps its last W - WR window weights in LDS, float4-interleaved as the
// float32 kernel does (W = 128: 44 of them, which with the d buffers fills the 160 KB).
template <int W, int NWT>
struct F64Lds {
    static constexpr int NP = NWT * 64;
    static constexpr int DC = NP + 14;                   // doubles per copy
    static constexpr int BUF = 2 * DC;                   // doubles per d buffer
    static constexpr int WR = (W > 64 && NWT > 8) ? (W == 128 ? 84 : 64) : W;   // register-resident window weights (floats)
    static constexpr int dls = 0;                        // [2][2][DC] d buffers
    static constexpr int pm = dls + 2 * BUF;             // [2][16] per-wave partial maxima of M, one set per buffer
    static constexpr int awl = pm + 2 * 16;              // [(W - WR) / 4][NP] f32x4: window weights WR .. W - 1
    static constexpr size_t bytes() { return sizeof(double) * awl + sizeof(float) * (size_t)(W - WR) * NP; }
    static_assert(DC % 2 == 0 && BUF % 2 == 0 && pm % 2 == 0 && awl % 2 == 0, "16-byte aligned sections");
    static_assert(NWT <= 16 && bytes() <= kLdsBytes, "one workgroup's LDS");
};

constexpr int kF64Prefetch = 4;    // emission rows in flight (frames ahead)

// Packed: packed batch (vit_decode_f64_packed).  One workgroup per forward slot: it walks the songs slot_songs[slot_begin[sl] ..
// slot_begin[sl + 1]) back to back (the scheme of wg_cursor.inc's take_song()); the emission and history rows of song b start at row
// offsets[b] of the packed buffers (64-bit row offsets).  The per-lane plan constants are loaded once; frame 0, the emission
// prefetch (clamped to the song's own last row) and the terminal argmax are per song.  Between two songs stands one barrier of its
// own, behind the terminal read: wave 0 reads d_{Tb-1} out of buffer (Tb - 1) & 1 after the song's last barrier, and without it
// the other waves would already publish the next song's frame 0 into buffer 0 and its partial maxima into pm[0] -- the buffer
// being read when Tb is odd (a one-frame song included).  Behind that barrier nothing of the finished song is read any more (the
// frame loop's reads all sit before its last barrier), so one barrier is enough for every parity.
// Ckpt: checkpointed decode (vit_decode_f64_checkpointed), one workgroup per song, in one of two wave-uniform runtime modes.
//   pass 1 (ckpt_every = K > 0): every frame of the song.  Of the history only the d rows of frames mK - 1 are kept, at rows m - 1 of
//     the song's own rows of hist (m = 1 ..; the host provides ceil(T / K) rows, so the row of frame T - 1 has a place when K divides
//     T); every other frame skips its stores by a wave-uniform branch, M is not stored at all.  Terminal state and log-likelihood
//     as ever.
//   one segment (ckpt_every = 0): frames t_begin .. min(length, t_end) - 1; a song that ends before t_begin leaves at once.  With
//     t_begin > 0 the checkpoint row init_rows[song] = d_{t_begin - 1} stands where frame 0 stands: published into buffer 0 in both
//     copies, with the per-wave partial maxima taken the same way.  Frames are counted from that row: local frame n is frame
//     base + n, base = max(t_begin - 1, 0); the buffer parity, the emission prefetch (clamped to the last frame this launch
//     computes) and the unrolled loop all run on n.  Row t is stored at t - t_begin; M_{t-1} goes next to its row as ever, which
//     for the first frame of a resumed segment is the row in FRONT of hist (the checkpoint's place: written, never read).  M of
//     the segment's last row, which no frame of this launch takes, is formed behind the loop from the partial maxima of the last
//     buffer (where the song goes on: the back-trace of the segment decides that row's frame).  No terminal.
// Both modes share one store: the next frame to keep (`keep`) and its row (`hrow`) advance by K frames / one row in pass 1 and by
// one frame / one row in a segment.
// PackedCkpt: packed checkpointed decode (vit_decode_f64_packed_checkpointed), K = a.ckpt_every frames per segment, song b with
// n_b = ceil(T_b / K) of them; two wave-uniform runtime modes, as WgVariant::PackedCkpt of the float32 floor kernel.
//   pass 1 (a.unit_song null): Packed's slot walk (hand-over barrier and prefetch clamp included) storing as Ckpt's pass 1 does, but
//     per song: the d rows of frames mK - 1, m = 1 .. n_b - 1, at rows ckpt_base[b] + m - 1 of hist.  The area holds sum (n_b - 1)
//     rows: frame T_b - 1 of a song whose length K divides has NO row (the next song's rows, or the end of the area, stand there),
//     so the store is bounded by t < T_b - 1 -- exactly the frames mK - 1 with m <= n_b - 1.  Terminal state and log-likelihood per song.
//   pass 2 (a.unit_song set): workgroup u < a.B runs Ckpt's one segment for segment g = unit_seg[u] of song b = unit_song[u]: frames
//     gK .. min(T_b, gK + K) - 1 with emission rows at offsets[b], resumed from row ckpt_base[b] + g - 1 of init_rows where g > 0,
//     into the unit's own rows at hist + u * hist_song_stride (K + 1 rows per unit, hist at the second).
// Plain compiles to the code it was before the variants existed (PK / CK / PC below: the variant as flags).
template <int W, int NWT, typename ET, F64Variant V = F64Variant::Plain>
__global__ void __launch_bounds__(NWT * 64) f64_floor_forward_kernel(F64Args a) {
    constexpr bool PC = V == F64Variant::PackedCkpt, PK = V == F64Variant::Packed || PC, CK = V == F64Variant::Ckpt || PC;
    using L = F64Lds<W, NWT>;
    constexpr int NP = L::NP, DC = L::DC, BUF = L::BUF, WR = L::WR, PF = kF64Prefetch;
    constexpr int CH = (W > 64 && NWT > 8) ? 8 : 16;        // window sources in flight
    constexpr bool WD = W <= 32 || (W == 64 && NWT <= 8);   // the window weights live in registers as doubles (two waves per SIMD at W = 64)
    static_assert(W % 4 == 0 && WR % 4 == 0 && PF % 2 == 0, "whole quads; the unrolled frames cycle through both buffers");
    extern __shared__ __align__(16) unsigned char smem[];
    double* dls = reinterpret_cast<double*>(smem) + L::dls;
    double* pm = reinterpret_cast<double*>(smem) + L::pm;
    f32x4* awl = reinterpret_cast<f32x4*>(reinterpret_cast<double*>(smem) + L::awl);
    const int S = a.S, SP = a.SP, T = a.T, SD = a.SD64, nx = a.n_extras;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    int song = blockIdx.x;
    int Tb = PK ? 1 : song_length(a.lengths, song, T);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (PK ? (size_t)0 : (size_t)song * T * S);
    double* __restrict__ hist = a.hist + (PK ? (size_t)0 : CK ? (size_t)song * a.hist_song_stride : (size_t)song * T * SD);
    // (CK) wave-uniform: pass 1 or a segment, whether the song goes on behind this launch's last frame, the next frame whose row
    // is kept, the frames between two kept rows, and the kept row's place.  From here on Tb counts LOCAL frames and E starts at
    // local frame 0.
    // (PC) pass 1 or a unit's segment (wave-uniform); the unit's segment within its song
    [[maybe_unused]] const int ug = PC && a.unit_song ? a.unit_seg[blockIdx.x] : 0;
    [[maybe_unused]] const bool pass1 = PC ? a.unit_song == nullptr : CK && a.ckpt_every > 0;
    [[maybe_unused]] const bool resumed = PC ? ug > 0 : CK && a.t_begin > 0;
    [[maybe_unused]] bool goes_on = false;
    [[maybe_unused]] int keep = 0, keep_step = 1;
    [[maybe_unused]] double* hrow = hist;
    if constexpr (CK && !PC) {
        const int t_last = Tb < a.t_end ? Tb : a.t_end;   // one past the last frame this launch computes
        if (t_last <= a.t_begin) return;                  // the song ended before this segment
        goes_on = !pass1 && Tb > t_last;
        const int base = resumed ? a.t_begin - 1 : 0;
        Tb = t_last - base;
        E += (size_t)base * S;
        keep = pass1 ? a.ckpt_every - 1 : 1;
        keep_step = pass1 ? a.ckpt_every : 1;
        hrow = pass1 || resumed ? hist : hist + SD;       // (local frame 1 of a segment from the prior is row 1)
    }
    // (PK) position in slot_songs and the end of the slot's list; the song at si: its length, emission rows and history rows.
    // Wave-uniform: scalar loads.
    [[maybe_unused]] int si = 0, si_end = 1;
    [[maybe_unused]] auto take_song = [&]() {
        song = a.slot_songs[si];
        const long long r0 = a.offsets[song];
        Tb = (int)(a.offsets[song + 1] - r0);
        E = reinterpret_cast<const ET*>(a.logE) + (size_t)r0 * S;
        if constexpr (!PC) {
            hist = a.hist + (size_t)r0 * SD;
        } else {                                          // (pass 1) the song's first kept frame and its checkpoint row
            keep = a.ckpt_every - 1;
            hrow = a.hist + (size_t)a.ckpt_base[song] * SD;
        }
    };
    if constexpr (PK) {
        if (!PC || pass1) {                               // (PC: pass 1 is the slot walk)
            if ((int)blockIdx.x >= a.n_slots) return;
            si = a.slot_begin[blockIdx.x];
            si_end = a.slot_begin[blockIdx.x + 1];
            if (si >= si_end) return;                     // an empty slot (the host makes none)
            take_song();
        }
    }
    if constexpr (PC) {
        if (pass1) {
            keep_step = a.ckpt_every;
        } else {
            // the unit's segment, as Ckpt's one segment: Tb counts LOCAL frames from the checkpoint's frame (or from frame 0), E
            // starts at local frame 0, every local frame from 1 on is stored
            song = a.unit_song[blockIdx.x];
            const long long r0 = a.offsets[song];
            const int Tfull = (int)(a.offsets[song + 1] - r0);
            const int t_begin = ug * a.ckpt_every;
            const int t_last = Tfull - t_begin < a.ckpt_every ? Tfull : t_begin + a.ckpt_every;
            goes_on = Tfull > t_last;
            const int base = resumed ? t_begin - 1 : 0;
            Tb = t_last - base;
            E = reinterpret_cast<const ET*>(a.logE) + (size_t)(r0 + base) * S;
            hist = a.hist + (size_t)blockIdx.x * a.hist_song_stride;
            keep = 1;
            hrow = resumed ? hist : hist + SD;
        }
    }

    // ---------------- per-lane constants.  Idle lanes (j >= S) publish -inf.
    const int j = tid;
    const bool tvalid = j < S;
    const int jc = tvalid ? j : 0;
    const int lo = tvalid ? reinterpret_cast<const int32_t*>(a.image + a.off_lo)[jc] : 0;
    const double cj = tvalid ? (double)reinterpret_cast<const float*>(a.image + a.off_rowc)[jc] : -INFINITY;
    float aw[WR];
    float xa[kMaxExtras];
    int xcol[kMaxExtras];
    bool is_x = false;                                   // this lane's state is an extra column: not part of M
    {
        const float* __restrict__ tab = reinterpret_cast<const float*>(a.image + a.off_tabA);
        const float* __restrict__ xaT = reinterpret_cast<const float*>(a.image + a.off_extraA);
#pragma unroll
        for (int w = 0; w < WR; ++w) aw[w] = tvalid ? tab[(size_t)w * SP + jc] : -INFINITY;
#pragma unroll
        for (int q = 0; q < (W - WR) / 4; ++q) {
            f32x4 w4;
            w4.x = tvalid ? tab[(size_t)(WR + 4 * q + 0) * SP + jc] : -INFINITY;
            w4.y = tvalid ? tab[(size_t)(WR + 4 * q + 1) * SP + jc] : -INFINITY;
            w4.z = tvalid ? tab[(size_t)(WR + 4 * q + 2) * SP + jc] : -INFINITY;
            w4.w = tvalid ? tab[(size_t)(WR + 4 * q + 3) * SP + jc] : -INFINITY;
            awl[q * NP + j] = w4;
        }
#pragma unroll
        for (int k = 0; k < kMaxExtras; ++k) {
            xcol[k] = k < nx ? a.extras[k] : 0;
            xa[k] = (tvalid && k < nx) ? xaT[(size_t)k * SP + jc] : -INFINITY;
            is_x |= (k < nx && j == xcol[k]);
        }
    }
    const int cp = lo & 1;
    const double* rp = dls + cp * DC + lo + cp;           // window start in the copy that aligns it (an even index)
    double* wp = dls + j;                                 // own entry of copy 0 (copy 1: + DC + 1)

    // produce(): publish a new d value -- both copies of buffer WB -- and the wave's share of M
    auto produce = [&](const double dn, const int WB) {
        wp[WB * BUF] = dn;
        wp[WB * BUF + DC + 1] = dn;
        const double part = wave_scan_max_f64(is_x ? -INFINITY : dn);
        if (lane == 63) pm[WB * 16 + wv] = part;
    };

    // frame t = 1 + PF n + u reads buffer u & 1 and writes the other one; one barrier per frame
    auto frame = [&](const int t, float& e_slot, const int u) {
        const int RB = u & 1, WB = RB ^ 1;
        const f64x2* __restrict__ win = reinterpret_cast<const f64x2*>(rp + RB * BUF);
        double xd[kMaxExtras];
#pragma unroll
        for (int k = 0; k < kMaxExtras; ++k) xd[k] = dls[RB * BUF + xcol[k]];
        f64x2 pq[NWT / 2];
#pragma unroll
        for (int q = 0; q < NWT / 2; ++q) pq[q] = reinterpret_cast<const f64x2*>(pm + RB * 16)[q];
        // M = max of d_{t-1} over the non-extra sources
        double M = fmax(pq[0].x, pq[0].y);
#pragma unroll
        for (int q = 1; q < NWT / 2; ++q) M = fmax(fmax(M, pq[q].x), pq[q].y);
        double m0 = M + cj, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
        // the window in chunks of CH sources (CH / 2 reads): wide windows must not hold all their data at once
#pragma unroll
        for (int w0 = 0; w0 < W; w0 += CH) {
            f64x2 dw[CH / 2];
#pragma unroll
            for (int q = 0; q < CH / 2; ++q)
                if (w0 + 2 * q < W) dw[q] = win[w0 / 2 + q];
#pragma unroll
            for (int w = w0; w < W && w < w0 + CH; w += 4) {
                f32x4 wa;
                if (w < WR) {
                    // (wide windows: the weights stay float32 in registers and are widened at use -- exact; left alone the compiler
                    // hoists the conversions out of the frame loop and keeps W doubles)
                    if constexpr (!WD) asm volatile("" : "+v"(aw[w < WR ? w : 0]), "+v"(aw[w < WR ? w + 1 : 0]), "+v"(aw[w < WR ? w + 2 : 0]), "+v"(aw[w < WR ? w + 3 : 0]));
                    wa = f32x4{aw[w < WR ? w : 0], aw[w < WR ? w + 1 : 0], aw[w < WR ? w + 2 : 0], aw[w < WR ? w + 3 : 0]};
                } else {
                    wa = awl[((w - WR) / 4) * NP + j];
                }
                const f64x2 da = dw[(w - w0) / 2], db = dw[(w - w0) / 2 + 1];
                m0 = fmax(m0, da.x + (double)wa.x);
                m1 = fmax(m1, da.y + (double)wa.y);
                m2 = fmax(m2, db.x + (double)wa.z);
                m3 = fmax(m3, db.y + (double)wa.w);
            }
        }
#pragma unroll
        for (int k = 0; k < kMaxExtras; ++k) m1 = fmax(m1, xd[k] + (double)xa[k]);   // (-inf weights beyond the plan's extra columns)
        double dn = fmax(fmax(m0, m1), fmax(m2, m3)) + (double)e_slot;
        dn = tvalid ? dn : -INFINITY;
        produce(dn, WB);
        if constexpr (!CK) {
            if (tvalid) hist[(size_t)t * SD + j] = dn;
            if (wv == 0 && lane == 0) hist[(size_t)(t - 1) * SD + S] = M;   // M_{t-1}, next to the row it was taken over
        } else if (PC ? t == keep && (!pass1 || t + 1 < Tb) : t == keep) {   // (PC pass 1: a song's last frame has no checkpoint row)
            if (tvalid) hrow[j] = dn;
            if (wv == 0 && lane == 0 && !pass1) hrow[S - SD] = M;           // (a resumed segment's first frame: the row in front)
            hrow += SD;
            keep += keep_step;
        }
        const int tn = t + PF < Tb ? t + PF : Tb - 1;
        e_slot = load_e<ET>(E + (size_t)tn * S + jc);
        __syncthreads();
    };

    // one song per pass (PK: the slot's songs one after the other)
    for (;;) {
        // ---------------- frame 0: the reference forms log_pi + E_0 in float32 and stores it into the float64 T1
        {
            const float d0f = tvalid ? reinterpret_cast<const float*>(a.image + a.off_logpi)[jc] + load_e<ET>(E + jc) : -INFINITY;
            double d0 = (double)d0f;
            if constexpr (!CK) {
                if (tvalid) hist[j] = d0;
            } else {
                // the checkpoint row: d_{t_begin - 1} (PC: in front of segment ug of the song)
                if (resumed) d0 = tvalid ? a.init_rows[(PC ? (size_t)(a.ckpt_base[song] + ug - 1) * SD : (size_t)song * a.init_stride) + jc] : -INFINITY;
                else if (tvalid && !pass1) hist[j] = d0;
            }
            produce(d0, 0);
        }
        float er[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) er[k] = load_e<ET>(E + (size_t)(1 + k < Tb ? 1 + k : Tb - 1) * S + jc);
        __syncthreads();

        int t = 1;
        for (; t + PF - 1 < Tb; t += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) frame(t + k, er[k], k);
        }
#pragma unroll
        for (int k = 0; k < PF - 1; ++k)
            if (t + k < Tb) frame(t + k, er[k], k);

        if constexpr (CK) {
            if (!pass1) {
                // M of the segment's last row (buffer (Tb - 1) & 1, complete behind the last barrier), in frame()'s order
                if (goes_on && wv == 0 && lane == 0) {
                    const f64x2* __restrict__ pl = reinterpret_cast<const f64x2*>(pm + ((Tb - 1) & 1) * 16);
                    double M = fmax(pl[0].x, pl[0].y);
#pragma unroll
                    for (int q = 1; q < NWT / 2; ++q) M = fmax(fmax(M, pl[q].x), pl[q].y);
                    hrow[S - SD] = M;
                }
                return;
            }
        }
        // ---------------- the terminal state: lowest-index argmax of d_{Tb-1}, and its value
        if (wv == 0) {
            const int fb = (Tb - 1) & 1;                  // buffer holding d_{Tb-1}
            double best;
            int ln = lane;
            // (PK: left alone the compiler hoists the argmax's NWT row masks out of the song loop and keeps them in scalar registers
            // through the frames: twelve waves at W = 128 then spill)
            if constexpr (PK) asm volatile("" : "+v"(ln));
            const int s = bt_row_argmax<NWT>(dls + fb * BUF, S, ln, &best);
            if (lane == 0) {
                a.last_state[song] = s;
                if (a.loglik) a.loglik[song] = best;
            }
        }
        if constexpr (!PK) {
            break;
        } else {
            if (++si >= si_end) break;
            take_song();
            __syncthreads();                              // the hand-over: the terminal read above before the next song's frame 0
        }
    }
}

// ---------------------------------------------------------------------------------------
// Back-trace kernel
// ---------------------------------------------------------------------------------------
// One wave per (song, chunk) in MODE 0, per song in MODE 1; kF64BtWaves waves per workgroup.  A wave keeps the d row of the frame it
// decides in its own LDS row and the next row (one frame down) in flight in registers: the row a step reads does not depend on the
// path, only the columns do.  For the path state j at t + 1:
//   * candidate c = 64 k + lane: c < W window source lo_j + c, W <= c < W + n_extras an extra column; its weight is entry c of the
//     plan's per-target candidate row (tabX[j]: window, extra columns, row constant), read from the image (L2-resident);
//   * fl64(M_t + c_j) bounds every row-constant candidate: below the candidates' maximum, the lowest matching source wins;
//   * otherwise all S candidates are evaluated and the lowest index attaining the maximum wins (an all -inf frame: state 0).
// Packed: packed batch (vit_decode_f64_packed; lazy_backtrace_kernel's PK case).  MODE 0 runs one wave per entry of wave_song; song b owns
// the waves and the chunk entries chunk_base[b] .. chunk_base[b + 1] - 1, so its chunk count grows with its length; MODE 1 one wave
// per song over that song's own chunk count.  Its history rows and states sit at row offsets[b] of the packed buffers and there are
// no frames past its end to fill.
// Ckpt: one segment of a checkpointed decode (vit_decode_f64_checkpointed).  Song b is a sub-problem of seg_len[b] frames (0: the song
// ended before the segment; its waves leave) whose last frame already has its state, seg_last[b]; its rows start at
// hist_song_stride * b and its states at states + b * T, a.states being advanced to the segment's first frame.  Nothing is filled
// past a song's end: the host fills the whole buffer once.
// PackedCkpt: Ckpt's walk over the units of one launch of a packed checkpointed decode (vit_decode_f64_packed_checkpointed): unit u has
// seg_len[u] frames from state seg_last[u], rows at hist_song_stride * u, chunk entries at u * chunks and its states at states +
// unit_states[u] (offsets[song] + segment * K, 64-bit).  Nothing past a unit's end is filled: those frames are the next song's.
constexpr int kF64BtWaves = 4;
constexpr int kF64BtSlots = 3;     // candidate slots per lane: W + kMaxExtras <= 192

template <int NWT, int MODE, F64Variant V = F64Variant::Plain>
__global__ void __launch_bounds__(kF64BtWaves * 64) f64_backtrace_kernel(F64Args a) {
    constexpr bool PC = V == F64Variant::PackedCkpt, PK = V == F64Variant::Packed, CK = V == F64Variant::Ckpt || PC;
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int EPL = NWT, NP = NWT * 64, KC = kF64BtSlots;
    const int S = a.S, SD = a.SD64, T = a.T, W = a.W, nx = a.n_extras;
    const int WX1 = W + kMaxExtras + 1;                   // candidate-table row: window, extras, row constant
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* rowL = reinterpret_cast<double*>(smem) + (size_t)wv * NP;   // this wave's d row
    // which song and chunk this wave serves, the song's length and its rows (PK: from the tables)
    const int C0 = PK ? 1 : a.chunks;
    const long long gw = (long long)blockIdx.x * kF64BtWaves + wv;
    if (PK && MODE == 0 && gw >= a.n_waves) return;
    const long long song_l = PK ? (MODE == 0 ? (long long)a.wave_song[gw] : gw) : (MODE == 0 ? gw / C0 : gw);
    if (song_l >= a.B) return;
    const int song = (int)song_l;
    const int cbase = PK ? a.chunk_base[song] : 0;
    const int C = PK ? a.chunk_base[song + 1] - cbase : C0;
    const int chunk = MODE == 0 ? (PK ? (int)(gw - cbase) : (int)(gw % C)) : 0;
    const long long row0 = PK ? (long long)a.offsets[song] : 0;   // (PK) first history row / state of the song
    const int Tb = PK ? (int)(a.offsets[song + 1] - row0) : CK ? (int)a.seg_len[song] : song_length(a.lengths, song, T);
    if (CK && Tb < 1) return;
    int32_t* states = a.states + (PK ? (size_t)row0 : PC ? (size_t)a.unit_states[song] : (size_t)song * T);       // (no __restrict__: MODE 1 reads what chase() stored)
    int32_t* entry = a.entry + (PK ? (size_t)cbase : (size_t)song * C);
    const double* __restrict__ hist = a.hist + (PK ? (size_t)row0 * SD : CK ? (size_t)song * a.hist_song_stride : (size_t)song * T * SD);
    const float* __restrict__ tabX = reinterpret_cast<const float*>(a.image + a.off_tabX);
    const int32_t* __restrict__ loT = reinterpret_cast<const int32_t*>(a.image + a.off_lo);

    // per-lane constants of the candidate slots and of the strided sources
    bool isw[KC], cand[KC];
    int xs[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = 64 * k + lane;
        isw[k] = c < W;
        cand[k] = c < W + nx;
        xs[k] = (c >= W && c < W + nx) ? a.extras[(c - W) & (kMaxExtras - 1)] : 0;
    }
    int xk[EPL];                                          // strided source i = 64 e + lane: -1 ordinary, k = extra column k, -2 none
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int i = e * 64 + lane;
        int x = i < S ? -1 : -2;
#pragma unroll
        for (int k = 0; k < kMaxExtras; ++k) x = (k < nx && i == a.extras[k]) ? k : x;
        xk[e] = x;
    }

    auto fetch = [&](double (&stage)[EPL], double& Mrow, int& old, const int t) {
        const double* __restrict__ r = hist + (size_t)t * SD;
#pragma unroll
        for (int e = 0; e < EPL; ++e) stage[e] = e * 64 + lane < S ? r[e * 64 + lane] : -INFINITY;
        Mrow = r[S];
        old = MODE == 1 ? states[t] : -1;
    };

    // chase(top, bottom, cur, write): decide the states of frames top .. bottom (descending) from the d rows top .. bottom, starting
    // from state `cur` at frame top + 1; returns the state at frame `bottom`
    auto chase = [&](const int top, const int bottom, int cur, const bool write) -> int {
        if (top < bottom) return cur;
        double stage[EPL], Mn;
        int oldn;
        fetch(stage, Mn, oldn, top);
        for (int t = top; t >= bottom; --t) {
            cur = __builtin_amdgcn_readfirstlane(cur);
            // the weights of target cur: issued first, they are the step's only dependent global reads
            const int lo = __builtin_amdgcn_readfirstlane(loT[cur]);
            const float* __restrict__ tx = tabX + (size_t)cur * WX1;
            float av[KC];
#pragma unroll
            for (int k = 0; k < KC; ++k) av[k] = (64 * k < W + nx && cand[k]) ? tx[64 * k + lane] : -INFINITY;
            const double cj = (double)tx[W + kMaxExtras];
#pragma unroll
            for (int e = 0; e < EPL; ++e) rowL[e * 64 + lane] = stage[e];
            const double Mt = Mn;
            const int old = oldn;
            if (t > bottom) fetch(stage, Mn, oldn, t - 1);
            // the row is this wave's own: every lane's stores above before any lane's reads below (LDS runs a wave's accesses in
            // order; the fence and the wave barrier keep the compiler from moving the reads up, and cost no instruction)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            double v[KC];
            double m = -INFINITY;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                v[k] = -INFINITY;
                if (64 * k < W + nx) {
                    const double dv = cand[k] ? rowL[isw[k] ? lo + 64 * k + lane : xs[k]] : -INFINITY;
                    v[k] = cand[k] ? dv + (double)av[k] : -INFINITY;
                }
                m = fmax(m, v[k]);
            }
            m = wave_max_all_f64(m);
            const double bound = Mt + cj;                  // fl64(M_t + c_j): every row-constant candidate is at most this
            unsigned idx = 0x7fffffffu;
            double mm = m;
            if (!(bound < m)) {
                // full evaluation: a row-constant candidate may tie or win
                double vf[EPL];
                double m2 = -INFINITY;
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int i = e * 64 + lane;
                    const bool excl = xk[e] != -1 || (unsigned)(i - lo) < (unsigned)W;   // covered by v[] (or no source at all)
                    vf[e] = excl ? -INFINITY : rowL[i] + cj;
                    m2 = fmax(m2, vf[e]);
                }
                mm = fmax(m, wave_max_all_f64(m2));
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int i = e * 64 + lane;
                    const bool excl = xk[e] != -1 || (unsigned)(i - lo) < (unsigned)W;
                    const unsigned long long mk = __ballot(vf[e] == mm && !excl);
                    if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
                }
            }
            // lowest source among the window / extra-column candidates that attain the maximum
            bool have_w = false;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                if (64 * k >= W + nx) continue;
                const unsigned long long mk = __ballot(v[k] == mm && cand[k]);
                const unsigned long long mw = mk & __ballot(isw[k]);
                if (mw && !have_w) {                           // window candidates ascend with the source index
                    const unsigned c = lo + 64 * k + __builtin_ctzll(mw);
                    idx = c < idx ? c : idx;
                    have_w = true;
                }
                unsigned long long mx = mk & ~__ballot(isw[k]);   // extra columns: arbitrary indices
                while (mx) {
                    const unsigned c = (unsigned)__builtin_amdgcn_readlane(xs[k], __builtin_ctzll(mx));
                    idx = c < idx ? c : idx;
                    mx &= mx - 1;
                }
            }
            cur = idx == 0x7fffffffu ? 0 : (int)idx;       // (an all -inf frame resolves to state 0 like np.argmax)
            // MODE 1 re-chases a chunk whose assumed entry state was wrong: as soon as the new path meets the stored one the rest of
            // the chunk is already right (the step below a state depends on that state only)
            if (MODE == 1 && cur == __builtin_amdgcn_readfirstlane(old)) return __builtin_amdgcn_readfirstlane(states[bottom]);
            if (write && lane == 0) states[t] = cur;
        }
        return cur;
    };

    // (the variant only decides which pointers and limits the chunk scheme gets: Plain alone has frames past a song's end to fill)
    bt_run_chunks<MODE, EPL>(chase, [&](const int f) { return hist + (size_t)f * SD; }, states, entry,
                             MODE == 0 ? (CK ? a.seg_last[song] : a.last_state[song]) : 0, Tb, PK || CK ? Tb : T, chunk, C, a.warm, S, lane);
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
template <typename F>
static hipError_t f64_dispatch_width(int W, F&& f) {
    static_assert(sizeof(kBandedWidths) / sizeof(int) == 6, "one case per instantiated window width");
    switch (W) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 84: return f(std::integral_constant<int, 84>{});
        case 96: return f(std::integral_constant<int, 96>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidConfiguration;
    }
}
template <typename F>
static hipError_t f64_dispatch_waves(int S, F&& f) {
    switch (banded_waves_for(S)) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 12: return f(std::integral_constant<int, 12>{});
        default: return hipErrorInvalidConfiguration;
    }
}

// what a launch of variant v needs of F64Args (the sibling of wg_variant_args_ok); bt: the back-trace's launch
static bool f64_variant_args_ok(const F64Args& a, F64Variant v, bool bt) {
    if (a.B < 1) return false;
    if (bt ? a.chunks < 1 || a.chunks > kBtMaxChunks || a.W + kMaxExtras > 64 * kF64BtSlots : a.W > a.S) return false;
    switch (v) {
        case F64Variant::Plain: return bt || a.T >= 1;
        case F64Variant::Packed:
            if (!a.offsets) return false;
            return bt ? a.wave_song && a.chunk_base && a.n_waves >= 1 : a.slot_begin && a.slot_songs && a.n_slots >= 1;
        case F64Variant::Ckpt:
            if (a.offsets) return false;
            if (bt) return a.seg_len && a.seg_last;
            // pass 1 (a.ckpt_every > 0, from frame 0) or one segment (resumed from a.init_rows where a.t_begin > 0)
            return a.T >= 1 && a.t_begin >= 0 && a.t_end <= a.T && a.t_begin < a.t_end && (a.t_begin <= 0 || a.init_rows) &&
                   (a.ckpt_every <= 0 || a.t_begin <= 0) && a.ckpt_every >= 0;
        case F64Variant::PackedCkpt:
            if (!a.offsets || !a.ckpt_base || a.ckpt_every < 1) return false;
            if (bt) return a.seg_len && a.seg_last && a.unit_states;
            // pass 1 (a.unit_song null: the slot walk) or the units of one launch, each with K + 1 rows of its own
            return a.unit_song ? a.unit_seg && a.init_rows && a.hist_song_stride >= ((int64_t)a.ckpt_every + 1) * a.SD64
                               : a.slot_begin && a.slot_songs && a.n_slots >= 1;
    }
    return false;
}

// The forward instantiation of the plan for variant V: launched over one workgroup per song (Packed: per slot; PackedCkpt: per slot in
// pass 1, per unit in pass 2), or (per_cu set) asked how many of its workgroups one compute unit holds at once (the occupancy query at
// its LDS size)
template <F64Variant V>
static hipError_t f64_forward_v(const F64Args& a, bool f16, hipStream_t st, int* per_cu) {
    return f64_dispatch_width(a.W, [&](auto w) {
        return f64_dispatch_waves(a.S, [&](auto n) -> hipError_t {
            constexpr int W = decltype(w)::value, NWT = decltype(n)::value;
            constexpr size_t lds = F64Lds<W, NWT>::bytes();
            static_assert(f64_pckpt_units_per_cu(W, NWT) * lds <= kLdsBytes || f64_pckpt_units_per_cu(W, NWT) == 1, "the units of one CU fit its LDS");
            const bool slots = V == F64Variant::Packed || (V == F64Variant::PackedCkpt && !a.unit_song);
            auto go = [&](auto kern) -> hipError_t {
                if (per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, NWT * 64, lds);
                hipLaunchKernelGGL(kern, dim3((unsigned)(slots ? a.n_slots : a.B)), dim3(NWT * 64), lds, st, a);
                return hipGetLastError();
            };
            return f16 ? go(f64_floor_forward_kernel<W, NWT, __half, V>) : go(f64_floor_forward_kernel<W, NWT, float, V>);
        });
    });
}
static hipError_t f64_forward(const F64Args& a, F64Variant v, bool f16, hipStream_t st, int* per_cu) {
    switch (v) {
        case F64Variant::Plain: return f64_forward_v<F64Variant::Plain>(a, f16, st, per_cu);
        case F64Variant::Packed: return f64_forward_v<F64Variant::Packed>(a, f16, st, per_cu);
        case F64Variant::Ckpt: return f64_forward_v<F64Variant::Ckpt>(a, f16, st, per_cu);
        case F64Variant::PackedCkpt: return f64_forward_v<F64Variant::PackedCkpt>(a, f16, st, per_cu);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_f64_forward(const F64Args& a, F64Variant v, bool f16, hipStream_t st) {
    if (!f64_variant_args_ok(a, v, false)) return hipErrorInvalidValue;
    return f64_forward(a, v, f16, st, nullptr);
}

hipError_t f64_forward_resident(const F64Args& a, F64Variant v, bool f16, int* per_cu) {
    if ((v != F64Variant::Packed && v != F64Variant::PackedCkpt) || a.W > a.S) return hipErrorInvalidValue;   // (the variants whose slot launches are sized by it)
    return f64_forward(a, v, f16, nullptr, per_cu);
}

// The two passes (launch_two_pass): one wave per (song, chunk) -- Packed: per entry of wave_song, a.chunks the largest chunk count of
// any song; Ckpt, PackedCkpt: a.chunks chunks per sub-problem whatever its length, an empty chunk stands by itself -- then one wave
// per song.
template <F64Variant V>
static hipError_t f64_backtrace_v(const F64Args& a, hipStream_t st) {
    return f64_dispatch_waves(a.S, [&](auto n) -> hipError_t {
        constexpr int NWT = decltype(n)::value;
        const long long waves0 = V == F64Variant::Packed ? (long long)a.n_waves : (long long)a.B * a.chunks;
        return launch_two_pass(f64_backtrace_kernel<NWT, 0, V>, f64_backtrace_kernel<NWT, 1, V>, waves0, a.B, kF64BtWaves,
                               sizeof(double) * kF64BtWaves * NWT * 64, st, a);
    });
}
hipError_t launch_f64_backtrace(const F64Args& a, F64Variant v, hipStream_t st) {
    if (!f64_variant_args_ok(a, v, true)) return hipErrorInvalidValue;
    switch (v) {
        case F64Variant::Plain: return f64_backtrace_v<F64Variant::Plain>(a, st);
        case F64Variant::Packed: return f64_backtrace_v<F64Variant::Packed>(a, st);
        case F64Variant::Ckpt: return f64_backtrace_v<F64Variant::Ckpt>(a, st);
        case F64Variant::PackedCkpt: return f64_backtrace_v<F64Variant::PackedCkpt>(a, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace vit
