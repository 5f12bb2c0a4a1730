// wave.hip -- "wave" form of the banded forward pass: ONE SONG PER WAVEFRONT (gfx950).
//
// The workgroup kernels of banded.hip advance a song one frame per LDS round trip and barrier: ~830 cycles per
// frame whatever the arithmetic, which is what a small batch needs (latency) and what a large batch does not
// (throughput: four songs per CU still leave the VALU ~60 % idle).  Here a song never leaves one wavefront:
//
//   * lane l owns NPL = ceil(S/64) CONTIGUOUS states (right-aligned: slot NPL*l + k holds state NPL*l + k - (64*NPL - S));
//     delta lives in registers;
//   * the plan proved that every exception span lies within D sources of its target, so a lane needs delta only from
//     the H = ceil(D/NPL) lanes on either side: 2*H wave-wide DPP shifts of its NPL registers (wave_shr:1 / wave_shl:1; a
//     lane beyond the wave edge delivers 0, and the weights of sources that do not exist are -inf) -- no LDS, no
//     barrier, no other wave;
//   * own state k evaluates the 2*D+1 sources j-D .. j+D as D+1 even-aligned source pairs: one v_pk_add_f32 and one
//     v_max3_f32 per pair, weights register-resident (the true matrix entries: positions outside a row's exception span
//     carry the row constant, a candidate the dense recursion forms as well);
//   * everything else is the floor-max identity of banded_floor_forward_kernel with M taken over ALL sources
//     (plan.floor_all_ok: extra-column entries dominate the row constant too, so an extra column inside M only adds a
//     dominated candidate):  m_j = max( window candidates, fl(M + c_j), fl(delta_x + logA_T[j][x]) for extra columns x ).
//
// Every value compared is one the dense recursion forms, so delta is bit-identical (CPU replay: tests/plan_replay.py
// replay_wave).  Per frame and wave 253 VALU instructions (272 in all) and nothing to wait for but the emission prefetch;
// songs of different lengths simply finish at different times.  The history rows are written in slot order (row stride
// 64*NPL floats; layout at the kernel below) and vit_forward records that layout for the back-trace kernels.  Which rows a launch
// keeps is the history mode, a WaveHist; launch_wave takes it from the arguments (wave_hist_of) and picks the instantiation from the
// mode's row of the launch table (wave_launch_of), both in wave_common.hpp.
// Measured (S = 361, fp32, T = 30000): 19.9 ms for 1024 songs, 35.7 ms for 2048 -- HBM-bound at 4.5-5 TB/s of real
// traffic.
#include "wave_common.hpp"

namespace vit {

// NPL states per lane, D window half-width, NX extra columns, PF emission rows in flight, WPS minimum waves per SIMD the
// register budget must allow.
//
// Lane <-> state mapping, RIGHT-aligned: slot q = NPL*lane + k (k = 0 .. NPL-1) holds state q - o with o = 64*NPL - S,
// so lane 63 ends exactly at state S-1 and the o leading slots are idle (weights -inf: their delta stays -inf).  With
// that, a lane's NPL emission columns are one unconditional vector load at E_row + NPL*lane - o -- for the leading
// lanes that reaches back into the previous row of the SAME tensor (rows >= 1 only: row 0 is loaded element-wise), never
// out of bounds -- and the history row is stored in slot order: row stride 64*NPL floats, state i in column o + i, and
// M_t = max_i delta_t[i] in column 0, a copy of delta_t of extra column x in column 1 + x (idle slots) -- and, with one extra column and six idle
// slots (A3), the same two scalars of frames t-1 and t-2 in columns 2 3 | 4 5: they are still in scalar registers, four more selects per frame,
// and the back-trace kernels then find the scalars of three frames in ONE line (the carrier row t - t % 3 + 2; B = 2048: -8 % / -13 %).  No branch surrounds a memory instruction, so the in-order vmcnt
// of the emission prefetch is exact.  The back-trace is told the column offset and the column of M (BtArgs::col0, mcol).
//
// HM, the history mode (WaveHist, wave_common.hpp: its members, the properties the kernel reads -- WaveHistTraits --, the function
// from FwdArgs to the mode and the table of what each mode instantiates).  Full: every row.  Half: row t/2 of the EVEN frames; lane 0's
// idle slots carry, behind M_t and delta_t of the extra columns, the same scalars of the odd frame t-1 -- still in scalar registers
// when row t is stored, so the odd frames cost no store at all -- and the back-trace (backtrace_half.hip) rebuilds the 32 delta values
// of an odd frame that it needs with the very sums and maxima of this recursion: 768 instead of 1536 history bytes per frame.
// CkptPass: row (t + 1) / K - 1 for the frames t with (t + 1) % K == 0, the row in front of every segment of K frames; every other
// store goes to one scratch row per song (the same address over and over: it stays in L2), so that no branch surrounds a store.
// Segment: resumes from init_rows[song] = delta_{t_begin - 1} in slot order (a checkpoint row; lane 0's scalar slots are idle slots and
// are reset to -inf), computes frames t_begin .. min(t_end, T_b) - 1 and stores row t at t - t_begin.  A mode of its own so that the
// t_begin arithmetic stays out of Full: folded in, it cost the full-history kernel 25 % (19.9 -> 25.1 ms at B = 1024).
// PackedCkptPass / PackedSegment: the same two per slot / per unit (FwdArgs::ckpt_base, unit_song in kernels.hpp); a unit's song,
// segment and checkpoint row are loaded once per wave, in front of the frame loop.
//
// UV >= 1 (one extra column and it is the last state, S - 1 = slot 64*NPL - 1 whatever S): delta of the extra column is a plain
// v_readlane of lane 63's last slot instead of a select chain over the lane's slots (which the compiler turned into an LDS round
// trip per frame).  UV = 2 (plan-proven, FwdArgs::wave_u5; NPL = 6) in addition: the row constant and the extra-column weight are the
// same for a lane's slots 0..4 (the 360 voiced targets of the reference's matrices: log tiny, log(sw10 / n_bins); idle slots: -inf) and
// only slot 5 -- lane 63's unvoiced target, lane 3's first state at S = 361 -- has its own.  Then fl(M + c), fl(delta_x + a_x) and
// their maximum are formed ONCE per lane and once for slot 5 (4 adds + 2 max instead of 12 adds, and six two-operand maxima
// instead of six max3), and delta of the extra column is a plain v_readlane of lane 63's slot 5.  UV = 3: the same with three groups of
// slots, {0,1,2} {3,4} {5} -- S = 321 (msnet / dcnet / ftanet), whose idle slots end in the middle of lane 10 (6 adds + 3 max).
template <int NPL, int D, int NX, int PF, int WPS, WaveHist HM, typename ET, int UV = 0>
__global__ void __launch_bounds__(256, WPS) wave_forward_kernel(FwdArgs a) {
    constexpr int H = wave_halo(NPL, D);
    constexpr int NG = 2 * H + 1;              // lane groups of the neighbourhood
    constexpr int NPM = wave_pairs(D);
    constexpr int SDW = 64 * NPL;              // history row stride of this form
    static_assert(NPL <= 8 && NPL % 2 == 0 && NX <= kWaveMaxExtras && NX + 1 <= NPL && PF >= 1, "geometry (source pairs never straddle two lanes)");
    constexpr WaveHistTraits HT = wave_hist_traits(HM);
    constexpr bool HALF = HT.rows == WaveRows::Even, CKPT = HT.rows == WaveRows::Checkpoints;
    static_assert(!HALF || 2 * (NX + 1) <= NPL, "half history: lane 0 carries the scalars of two frames");
    static_assert(UV == 0 || NX == 1, "last-state / uniform-lane forms: one extra column");
    static_assert(UV < 2 || NPL == 6, "uniform-lane forms: six states per lane");
    constexpr bool U5 = UV == 2, U3 = UV == 3;
    constexpr bool PK = HT.slot_walk;          // packed batch: this wave is a SLOT that walks a list of songs back to back
    constexpr bool SG = HT.segment;            // one segment, resumed from a checkpoint row
    constexpr bool PO = HT.offsets;            // a song's rows come from the offsets
    constexpr bool A3 = HT.aux3 && NX == 1 && NPL >= 6;      // rows carry the scalars of three frames (and six idle slots: run time, l0a below; kernels.hpp wave_aux_row)
    const int S = a.S;
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wid >= (PK ? a.n_slots : a.B)) return; // whole waves only; there is no barrier in this kernel
    // ---------------- per-lane constants
    const int o = SDW - S;                                 // idle leading slots (>= 1)
    const int j0 = NPL * lane - o;                         // state of slot 0 of this lane (negative: idle)
    const bool l0a = A3 && lane == 0 && wave_aux_frames(NPL, S, NX) == 3 && !(a.wave_flags & 4);   // this lane's slots 2 .. 5 carry the scalars of frames t-1, t-2
#include "wave_lane_weights.inc"
    float cj[NPL];
    float xa[NX > 0 ? NX : 1][NPL];
    int xl[NX > 0 ? NX : 1];                               // lane that owns extra column x
    bool xs[NX > 0 ? NX : 1][NPL];                         // this lane's slot k holds extra column x
    {
        const float* __restrict__ rc = reinterpret_cast<const float*>(a.image + a.off_rowc);
        const float* __restrict__ xaT = reinterpret_cast<const float*>(a.image + a.off_extraA);
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int j = j0 + k;
            cj[k] = j >= 0 ? rc[j] : -INFINITY;
#pragma unroll
            for (int x = 0; x < NX; ++x) xa[x][k] = j >= 0 ? xaT[(size_t)x * a.SP + j] : -INFINITY;
        }
#pragma unroll
        for (int x = 0; x < NX; ++x) {
            xl[x] = (a.extras[x] + o) / NPL;
#pragma unroll
            for (int k = 0; k < NPL; ++k) xs[x][k] = j0 + k == a.extras[x];
        }
    }
    const int k_begin = PK ? a.slot_begin[wid] : 0, k_end = PK ? a.slot_begin[wid + 1] : 1;
    for (int kk = k_begin; kk < k_end; ++kk) {
    // ---------------- this song: emission rows, history rows, length
    const int song = PK ? a.slot_songs[kk] : (HT.unit ? a.unit_song[wid] : wid);
    const long long off = PO ? a.offsets[song] : (long long)song * a.T;           // first emission row of the song in the tensor
    const int T = PO ? (int)(a.offsets[song + 1] - off) : a.T;                     // rows the song owns (packed: its length)
    const int useg = HT.unit ? a.unit_seg[wid] : 0;                            // (units) the segment this wave recomputes
    const int t0 = !SG ? 0 : (HT.unit ? useg * a.ckpt_every : a.t_begin);      // first frame of this launch
    const int Tl = PO ? T : song_length(a.lengths, song, T);
    const int te = HT.unit ? t0 + a.ckpt_every : a.t_end;
    const int Tb = SG && te < Tl ? te : Tl;                                    // one past the last frame of this launch
    if (Tb <= t0) continue;                                                    // (segments: the song ended before this one)
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (size_t)off * S;
    // hist_rows = T (Full), (T + 1) / 2 (Half), segments (CkptPass), K + 1 (Segment, PackedSegment: per song / per unit), all checkpoint rows (PackedCkptPass)
    float* __restrict__ hist = a.hist + (HT.base == WaveBase::Shared ? (size_t)0 : (HT.base == WaveBase::Offset ? (size_t)off : (size_t)(HT.base == WaveBase::Unit ? wid : song) * a.hist_rows)) * SDW;
    const long long ck0 = HT.base == WaveBase::Shared ? a.ckpt_base[song] : 0; // (PackedCkptPass) the song's first checkpoint row
    // emission columns of this lane in rows >= 1 (see above): the leading lanes reach back into the row in front -- of the same song,
    // or (packed, row 0 is never loaded this way) of the song before it in the tensor; the first row of the tensor has none
    const long ecol = (T > 1 || off > 0) ? (long)j0 : (long)(j0 < 0 ? 0 : j0);
    const int row_min = T > 1 ? 1 : 0;
    auto load_row = [&](int row, float (&e)[NPL]) {
        row = row < row_min ? row_min : row;
        load_cols<NPL>(E + (size_t)row * S + ecol, e);
    };
    // history row t in slot order (Half: row t/2 of an even frame t; Mp / xp = the scalars of frame t-1, slots 1+NX .. 1+2*NX)
    auto store_hist = [&](const int t, const float (&d)[NPL], const float M, const float (&xd)[NX > 0 ? NX : 1], const float Mp,
                          const float (&xp)[NX > 0 ? NX : 1], const float Mq, const float xq) {
#include "wave_hist_row.inc"
        if (HALF) {
            v[1 + NX] = lane == 0 ? Mp : v[1 + NX];
#pragma unroll
            for (int x = 0; x < NX; ++x) v[2 + NX + x] = lane == 0 ? xp[x] : v[2 + NX + x];
        }
        size_t row = HALF ? t >> 1 : t - t0;
        if (CKPT && !PK) {
            const int q = (t + 1) / a.ckpt_every;
            row = (t + 1) - q * a.ckpt_every == 0 && q - 1 < a.hist_rows - 1 ? q - 1 : a.hist_rows - 1;     // checkpoint, else the scratch row
        }
        if (CKPT && PK) {
            const int q = (t + 1) / a.ckpt_every;
            row = (t + 1) - q * a.ckpt_every == 0 && t + 1 < T ? (size_t)(ck0 + q - 1) : (size_t)(a.hist_rows + wid);   // checkpoint, else this slot's scratch row
        }
        store_row<NPL>(hist + row * SDW + NPL * lane, v);
    };
    // delta of the extra columns, wave-uniform
    auto extra_deltas = [&](const float (&d)[NPL], float (&xd)[NX > 0 ? NX : 1]) {
        if (UV >= 1) { xd[0] = wave_last_delta<NPL>(d); return; }
#pragma unroll
        for (int x = 0; x < NX; ++x) {
            float v = d[0];
#pragma unroll
            for (int k = 1; k < NPL; ++k) v = xs[x][k] ? d[k] : v;   // per-lane masks: one v_cndmask each
            xd[x] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), xl[x]));
        }
    };

    // ---------------- frame 0, or the checkpoint row in front of this segment
    float d[NPL];
    if (t0 == 0) {
        const float* __restrict__ lpi = reinterpret_cast<const float*>(a.image + a.off_logpi);
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int j = j0 + k;
            d[k] = j >= 0 ? lpi[j] + load_e<ET>(E + j) : -INFINITY;
        }
    } else {
        const float* __restrict__ ir = a.init_rows + (HT.unit ? (size_t)(a.ckpt_base[song] + useg - 1) * SDW : (size_t)song * a.init_stride) + NPL * lane;
#pragma unroll
        for (int k = 0; k < NPL; ++k) d[k] = j0 + k >= 0 ? ir[k] : -INFINITY;
    }
    float M = wave_frame_max<NPL>(d);
    float xd[NX > 0 ? NX : 1] = {};
    extra_deltas(d, xd);
    if (t0 == 0) store_hist(0, d, M, xd, M, xd, M, xd[0]);
    float Mb = M, xb = xd[0];                  // (A3) the scalars of the frame before the previous one
    const int t1 = t0 == 0 ? 1 : t0;           // first frame the loop computes

    float er[PF][NPL];
#pragma unroll
    for (int q = 0; q < PF; ++q) load_row(t1 + q < Tb ? t1 + q : Tb - 1, er[q]);
#pragma unroll
    for (int k = 0; k < NPL; ++k)
#pragma unroll
        for (int m = 0; m < NPM; ++m) asm volatile("" ::"v"(aw[k][m]));

    auto frame = [&](const int t, float (&e)[NPL], auto stored) {
#include "wave_frame_body.inc"
        const float Mp = M;                // the previous frame's scalars (wave-uniform: scalar registers)
        float xp[NX > 0 ? NX : 1];
#pragma unroll
        for (int x = 0; x < (NX > 0 ? NX : 1); ++x) xp[x] = xd[x];
        M = wave_frame_max<NPL>(d);
        extra_deltas(d, xd);               // for the next frame's candidates, and for the history row
        if (decltype(stored)::value && HT.stores) store_hist(t, d, M, xd, Mp, xp, Mb, xb);
        if (A3) { Mb = Mp; xb = xp[0]; }
        if (HT.loads) load_row(t + PF < Tb ? t + PF : Tb - 1, e);                // (no stores / no loads: the timing-only modes)
    };
    // The loop body is a whole number of frame pairs when only even frames are stored: t is odd at its top, frame t + q is
    // even for odd q, and "store or not" is a compile-time property of each unrolled frame (no branch around a store).
    constexpr int UN = (HALF && (PF & 1)) ? 2 * PF : PF;
    int t = t1;
    for (; t + UN - 1 < Tb; t += UN) {
#pragma unroll
        for (int q = 0; q < UN; ++q) {
            if (!HALF || (q & 1)) frame(t + q, er[q % PF], std::true_type{});
            else frame(t + q, er[q % PF], std::false_type{});
        }
    }
#pragma unroll
    for (int q = 0; q < UN - 1; ++q)
        if (t + q < Tb) {
            if (!HALF || (q & 1)) frame(t + q, er[q % PF], std::true_type{});
            else frame(t + q, er[q % PF], std::false_type{});
        }

    // ---------------- terminal state: lowest-index argmax of delta_{Tb-1} (not in a segment launch)
    if (!HT.unit && (!SG || a.t_end >= T)) {
#include "wave_terminal.inc"
        if (lane == 63) {
            a.last_state[song] = bi == kBig ? 0 : bi;
            if (a.loglik) a.loglik[song] = bv;
        }
    }
    }   // songs of this slot
}

// One mode's launch: the register form and the UV form, chosen once from the mode's row of the table (wave_launch_of, wave_common.hpp).
// 512 registers (one wave per SIMD, PF1 emission rows in flight: full history, B = 1024, PF 2 / 3 / 4 / 6 / 8 -> 24.6 / 21.4 / 19.9 / 21.5 /
// 33.8 ms) against 256 registers (two waves per SIMD, PF2 rows).  With the half history the kernel no longer waits for memory and the
// 256-register code is the faster one even with a single wave on each SIMD (B = 1024, full / half history: 512-register form 19.9 /
// 21.3 ms, 256-register form 19.7 / 16.5 ms), so it runs at every batch size unless a second extra column pushes it into scratch.
template <int NPL, int D, int NX, WaveHist HM, typename ET>
static hipError_t launch_wave_mode(const FwdArgs& a, hipStream_t st) {
    constexpr WaveLaunch L = wave_launch_of(HM);
    constexpr int PF1 = NX == 2 ? 3 : 4, PF2 = NX == 2 ? 2 : 3;
    constexpr int U1 = L.uv1 && NX == 1 ? 1 : 0, U2 = L.uv23 && NX == 1 && NPL == 6 ? 2 : 0, U3 = U2 ? 3 : 0;   // 0: the mode or the geometry has no such form
    const int n = L.by_slots ? a.n_slots : (int)a.B;
    const dim3 grid((n + 3) / 4), block(256);
    if (n <= 1024 && !(L.flag0 && (a.wave_flags & 1)) && ((a.wave_flags & 2) || NX == 2))
        hipLaunchKernelGGL((wave_forward_kernel<NPL, D, NX, PF1, 1, HM, ET>), grid, block, 0, st, a);
    else if (U2 && a.wave_u5 == 2) hipLaunchKernelGGL((wave_forward_kernel<NPL, D, NX, PF2, 2, HM, ET, U2>), grid, block, 0, st, a);
    else if (U3 && a.wave_u5 == 3) hipLaunchKernelGGL((wave_forward_kernel<NPL, D, NX, PF2, 2, HM, ET, U3>), grid, block, 0, st, a);
    else if (U1 && a.wave_u5 >= 1) hipLaunchKernelGGL((wave_forward_kernel<NPL, D, NX, PF2, 2, HM, ET, U1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((wave_forward_kernel<NPL, D, NX, PF2, 2, HM, ET>), grid, block, 0, st, a);
    return hipGetLastError();
}

template <int NPL, int D, int NX, typename ET>
static hipError_t launch_wave_x(const FwdArgs& a, hipStream_t st) {
    switch (wave_hist_of(a)) {
#define VIT_WAVE_MODE(M) case WaveHist::M: return launch_wave_mode<NPL, D, NX, WaveHist::M, ET>(a, st);
        VIT_WAVE_MODE(Full) VIT_WAVE_MODE(Half) VIT_WAVE_MODE(CkptPass) VIT_WAVE_MODE(Segment)
        VIT_WAVE_MODE(Packed) VIT_WAVE_MODE(PackedSegment) VIT_WAVE_MODE(PackedCkptPass)
#ifdef VIT_TIMING_HOOKS
        VIT_WAVE_MODE(NoStores) VIT_WAVE_MODE(NoLoads) VIT_WAVE_MODE(NoLoadsNoStores)
#endif
#undef VIT_WAVE_MODE
        default: return hipErrorInvalidConfiguration;
    }
}

template <typename ET>
static hipError_t launch_wave_e(const FwdArgs& a, hipStream_t st) {
    if (a.wave_dk != 14 || a.wave_npl != 6) return hipErrorInvalidConfiguration;   // the one instantiated geometry
    switch (a.n_extras) {
        case 0: return launch_wave_x<6, 14, 0, ET>(a, st);
        case 1: return launch_wave_x<6, 14, 1, ET>(a, st);
        case 2: return launch_wave_x<6, 14, 2, ET>(a, st);
        default: return hipErrorInvalidConfiguration;
    }
}

__global__ void segment_prep_kernel(const int64_t* __restrict__ lengths, int64_t B, int T, int s0, int e0, const int32_t* __restrict__ states,
                                    const int32_t* __restrict__ last, int64_t* __restrict__ seg_len, int32_t* __restrict__ seg_last) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int Tb = song_length(lengths, (int)b, T);
    if (Tb > e0) {                    // the song goes on behind this segment: its state at frame e0 is decided already
        seg_len[b] = e0 - s0 + 1;
        seg_last[b] = states[(size_t)b * T + e0];
    } else if (Tb > s0) {             // the song ends inside this segment: pass 1 left its terminal state
        seg_len[b] = Tb - s0;
        seg_last[b] = last[b];
    } else {
        seg_len[b] = 0;
        seg_last[b] = 0;
    }
}

hipError_t launch_segment_prep(const int64_t* lengths, int64_t B, int T, int s0, int e0, const int32_t* states, const int32_t* last,
                               int64_t* seg_len, int32_t* seg_last, hipStream_t st) {
    hipLaunchKernelGGL(segment_prep_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, lengths, B, T, s0, e0, states, last, seg_len, seg_last);
    return hipGetLastError();
}

// segment_prep_kernel per unit of a packed checkpointed decode: the sub-problem of segment [s0, s0 + K) of a song of T_b frames holds
// its frames and, where the song goes on, frame s0 + K, whose state the unit of the segment behind it decided in an earlier launch
__global__ void packed_segment_prep_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ unit_song, const int32_t* __restrict__ unit_seg,
                                           int n_units, int K, const int32_t* __restrict__ states, const int32_t* __restrict__ last,
                                           int64_t* __restrict__ seg_len, int32_t* __restrict__ seg_last, int64_t* __restrict__ unit_states) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_units) return;
    const int b = unit_song[u];
    const int64_t off = offsets[b], Tb = offsets[b + 1] - off, s0 = (int64_t)unit_seg[u] * K, e0 = s0 + K;
    unit_states[u] = off + s0;
    if (Tb > e0) {
        seg_len[u] = K + 1;
        seg_last[u] = states[off + e0];
    } else {                          // the song's last segment: pass 1 left its terminal state
        seg_len[u] = Tb - s0;
        seg_last[u] = last[b];
    }
}

hipError_t launch_packed_segment_prep(const int64_t* offsets, const int32_t* unit_song, const int32_t* unit_seg, int n_units, int K,
                                      const int32_t* states, const int32_t* last, int64_t* seg_len, int32_t* seg_last, int64_t* unit_states,
                                      hipStream_t st) {
    hipLaunchKernelGGL(packed_segment_prep_kernel, dim3((unsigned)((n_units + 255) / 256)), dim3(256), 0, st, offsets, unit_song, unit_seg, n_units, K,
                       states, last, seg_len, seg_last, unit_states);
    return hipGetLastError();
}

hipError_t launch_wave(const FwdArgs& a, bool f16, hipStream_t st) {
    if (!a.wave_ok) return hipErrorInvalidConfiguration;
    return f16 ? launch_wave_e<__half>(a, st) : launch_wave_e<float>(a, st);
}

}  // namespace vit
