// kernels.hpp -- launch interface between the C ABI (capi.hip) and the kernel files (dense, step, banded, wave, emission, activations, fused, f64,
// backtrace_rows / _sparse / _half / _lane .hip; those four share backtrace_common.hpp: the chunk scheme, the pieces of a decision and
// the launch helpers).  The two workgroup forward kernels that have variants -- banded_floor_forward_kernel (banded.hip, banded_pc.hip)
// and step4s_forward_kernel (step.hip) -- take one WgVariant, share their song / segment bookkeeping as text (wg_cursor.inc) and are
// reached through one launch and one occupancy entry point per family (launch_*_variant, *_variant_resident).  The float64 family
// (f64.hip) is built the same way: both of its kernels take one F64Variant and are reached through launch_f64_forward,
// f64_forward_resident and launch_f64_backtrace; its back-trace runs under the chunk scheme and the two-pass launch of
// backtrace_common.hpp, and its wave maximum and row argmax on doubles stand next to the float32 ones (device_common.hpp,
// backtrace_common.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "plan.hpp"

namespace vit {

// Banded kernel geometry: NWT target waves (64*NWT >= S), NWT in {2,4,6,8,12}.  Which (W, NWT) combinations are
// instantiated is bounded by registers: W window entries stay register-resident per thread.
//   scan form  (banded_forward_kernel: + two scan waves)      W <= 32: NWT <= 12;  W == 64: NWT <= 6
//   floor form (banded_floor_forward_kernel, plan.floor_ok)   W <= 128: NWT <= 12 (W = 128 with twelve waves keeps 32 weights in LDS)
constexpr int banded_waves_for(int S) {
    const int need = (S + 63) / 64;
    const int opts[5] = {2, 4, 6, 8, 12};
    for (int k = 0; k < 5; ++k)
        if (opts[k] >= need) return opts[k];
    return 0;
}
constexpr bool scan_form_instantiated(int W, int nwt) { return nwt > 0 && ((W <= 32 && nwt <= 12) || (W == 64 && nwt <= 6)); }
constexpr bool floor_form_instantiated(int W, int nwt) { return nwt > 0 && W <= 128 && nwt <= 12; }
// target waves of the scan form for (S, W), or 0 when it is not instantiated
constexpr int banded_target_waves(int S, int W) {
    const int nwt = banded_waves_for(S);
    return scan_form_instantiated(W, nwt) ? nwt : 0;
}
// What a workgroup of banded_floor_forward_kernel / step4s_forward_kernel decodes (described at the kernels):
//   Plain       its own song, every row kept                                     (vit_decode)
//   Packed      the songs of its slot, back to back, rows at offsets[song]       (vit_decode_packed)
//   Ckpt        its own song: pass 1 (checkpoint rows only) or one segment       (vit_decode_checkpointed)
//   PackedCkpt  pass 1 over the songs of its slot, or one segment unit           (vit_decode_packed_bounded)
//   Stream      its own song of a session: the next frames, from a chunk of rows (vit_stream_append)
//   StreamRing  Stream over a ring of a.hist_rows rows per song: frame t in row t mod hist_rows (vit_stream_open_ring; floor kernel only)
enum class WgVariant { Plain, Packed, Ckpt, PackedCkpt, Stream, StreamRing };
// packed variant of the one-target floor kernel (banded_floor_forward_kernel<.., WgVariant::Packed>, vit_decode_packed for plans without
// the wave form): every instantiated (W, NWT) pair of the floor form; idle slot S stores the frame maximum, so S < 64 * NWT
constexpr bool floor_packed_applies(int S, int W, bool floor_ok, int n_dense) {
    const int nwt = banded_waves_for(S);
    return floor_ok && n_dense == 0 && nwt > 0 && S < nwt * 64 && banded_width_instantiated(W) && floor_form_instantiated(W, nwt);
}
// checkpoint / resume variant of the same kernel (banded_floor_forward_kernel<.., WgVariant::Ckpt>, vit_decode_checkpointed for plans without
// the wave form): the packed variant's pairs but the narrow windows on few waves (W <= 32, S <= 384) -- plans that narrow take the
// wave form, but for the odd one with three extra columns or S = 64 * npl, and banded.hip is the longest compile as it is
constexpr bool floor_ckpt_pair(int W, int nwt) { return W >= 64 || nwt >= 8; }
constexpr bool floor_ckpt_applies(int S, int W, bool floor_ok, int n_dense) {
    return floor_packed_applies(S, W, floor_ok, n_dense) && floor_ckpt_pair(W, banded_waves_for(S));
}
// packed-checkpoint variant of the same kernel (banded_floor_forward_kernel<.., WgVariant::PackedCkpt> in banded_pc.hip, vit_decode_packed_bounded
// for plans without the wave form): every pair of the checkpoint / resume variant -- each of them compiles free of scratch
constexpr bool floor_pckpt_applies(int S, int W, bool floor_ok, int n_dense) { return floor_ckpt_applies(S, W, floor_ok, n_dense); }
// stream variant of the same kernel (banded_floor_forward_kernel<.., WgVariant::Stream> in banded_stream.hip, vit_stream_append): every
// pair of the packed variant -- the narrow windows on six waves (S = 321 / 361), which floor_ckpt_pair leaves out, are the sessions
// it is for; a session runs the workgroup family whatever its batch
constexpr bool floor_stream_applies(int S, int W, bool floor_ok, int n_dense) { return floor_packed_applies(S, W, floor_ok, n_dense); }
// step-structured kernel (plan.step_ok): instantiated for the Durrieu geometry -- 20-bin bands, 9 near bands, 705..768 voiced states
constexpr bool step_kernel_instantiated(int S, int bw, int kb) { return bw == 20 && kb == 9 && S - 1 > 704 && S - 1 <= 768; }
// the dense kernel keeps NS running (best, arg) pairs per thread
constexpr int dense_max_threads(int NS) { return NS <= 2 ? 1024 : 512; }

struct FwdArgs {
    const uint8_t* image;   // device plan image
    const void* logE;       // [B,T,S] f32 or f16
    const int64_t* lengths; // [B] or null
    float* hist;            // [B,T,SD] delta history (the reference's T1), SD = ceil((S+2)/4)*4: columns [0,S) = delta_t,
                            // column S = max_i delta_t[i] over the non-extra sources (banded kernels), S+1.. = scratch
    float* fmax;            // [B,64] scratch for the timing experiments (phase stamps)
    int32_t* last_state;    // [B]
    float* loglik;          // [B] or null
    int64_t B;
    int T, S, SP, S4, SD, W;
    int n_extras, n_dense;
    int extras[kMaxExtras];
    float c0;
    int debug;              // timing-only ablation mask; always 0 unless built with -DVIT_TIMING_HOOKS
    int fwd_form;           // banded forward form: 0 by batch size | 1 one target per lane | 2 two targets per lane | 3 scan | 6 split windows (eight waves)
    int dense_kt1;          // dense kernel: one thread per target even where two fit
    int dense_form;         // dense kernel: 0 matrix-resident form where it applies | 1 always the streaming form
    int step_form;          // step kernel: 3 = four targets per lane in one wave (step4_forward_kernel)
    size_t off_logpi, off_A4, off_lo, off_kind, off_tabA, off_extraA, off_denseA, off_rowc, off_lo2, off_tabP;
    int pair_ok;            // the plan proved pair windows: use the two-targets-per-lane kernel
    int floor_ok;           // the plan proved the one-maximum form (banded_floor_forward_kernel)
    int step_ok, step_bw, step_kb;   // step structure (step.hip)
    float step_cn;          // logA_T[j][S-1] for every voiced target j
    size_t off_stepC, off_Arow;
    int win_shift2;         // the same for the pair windows of banded_floor_pair_forward_kernel
    size_t off_tabV;        // wave form (wave.hip)
    int wave_ok, wave_npl, wave_dk;
    int wave_u5;            // wave.hip UV: 1 = the one extra column is state S-1; 2 = also: row constant and extra-column weight uniform over a
                            // lane's slots 0..4; 3 = uniform over slots {0,1,2} and {3,4}
    int wave_flags;         // bit 0: force the 256-register (two waves per SIMD) instantiation, bit 1: the 512-register one up to 1024 songs
    int hist_half;          // wave form: 1 = only the delta rows of even frames are stored (wave.hip, WaveHist::Half)
    int64_t hist_rows;      // history rows per song: T, or (T + 1) / 2 with hist_half; checkpoint pass: segments + 1
    // vit_decode_checkpointed: ckpt_every > 0 = pass 1 (checkpoint rows only; wave.hip WaveHist::CkptPass, the Ckpt variants of the floor and step
    // kernels); t_begin > 0 / t_end < T = a segment resumed from init_rows (one row per song in the history layout of the form that
    // runs; row t stored at t - t_begin)
    int ckpt_every, t_begin, t_end;
    const float* init_rows;
    int64_t init_stride;    // floats from one song's init row to the next
    // packed batch (vit_decode_packed): emission rows of song b are rows offsets[b] .. offsets[b+1]-1 of logE, its history rows sit at
    // the same offsets; slot w < n_slots (a wave of the wave form, a workgroup of the packed floor / step kernels) decodes songs
    // slot_songs[slot_begin[w] .. slot_begin[w+1]) back to back
    const int64_t* offsets; // device [B+1], or null
    int n_slots;
    const int32_t* slot_begin;   // device [n_slots + 1]
    const int32_t* slot_songs;   // device [B]
    // packed checkpointed decode (vit_decode_packed_checkpointed, the wave form: described here; vit_decode_packed_bounded, the
    // workgroup kernels: the same fields with a workgroup for a wave, see banded_floor.inc / step.hip, WgVariant::PackedCkpt).  Segments are per song: song b has
    // ceil(T_b / ckpt_every) of them.  ckpt_base set, unit_song null = pass 1 (wave.hip WaveHist::PackedCkptPass): the slot walk of the packed batch, but
    // the only rows kept are the ones in front of segments 1 .. n_b - 1, at rows ckpt_base[b] .. of hist; every other store goes to
    // scratch row hist_rows + slot.  unit_song set = pass 2 (WaveHist::PackedSegment): wave u < B recomputes segment unit_seg[u] of song unit_song[u]
    // from checkpoint row ckpt_base[song] + segment - 1 of init_rows (segment 0: from the prior) into rows u * hist_rows .. of hist
    const int64_t* ckpt_base;    // device [songs]: checkpoint rows in front of song b's = sum of (n_b' - 1) over b' < b
    const int32_t* unit_song;    // device [B units of this launch]
    const int32_t* unit_seg;     // device [B units of this launch]
    // stream session (vit_stream_append; WgVariant::Stream of the workgroup kernels), in fields the other variants leave unused: song b
    // computes frames pos[b] .. pos[b] + cnt[b] - 1 (cnt 0: nothing) with pos = unit_song and cnt = unit_seg, device [B] tables of this
    // launch -- or, both null, pos = t_begin and cnt = t_end - t_begin for every song.  Frame t reads emission row t - pos[b] of the
    // chunk logE + b * init_stride (init_stride in elements) and is stored at row t of the song's T rows of hist (T = the session's
    // capacity) in the Plain layout; pos > 0 resumes from row pos - 1 of those rows.
    int win_shift;         // 0..3: delta is stored shifted by this many floats in LDS so that the window starts of a
                            // 16-lane group are 16-byte aligned in the SAME copy order (bank-conflict-free b128 reads)
    int floor_live;         // split floor kernel (host side only): window entries the full waves' targets [0, 64 * kSplitFullWaves) must evaluate
                            // (floor_live_width; W = no trim, also with vit_plan_set_option "floor_live_window" 1)
};

struct BtArgs {
    const uint8_t* image;
    const float* hist;      // [B,T,SD]
    const int32_t* last_state;
    const int64_t* lengths;
    int32_t* states;        // [B,T]
    int32_t* entry;         // [B,chunks] state each chunk assumed at its upper boundary
    int64_t B;
    int T, S, SP, SD, W, K;
    int col0, mcol;         // history row layout: state i in column col0 + i, the frame maximum in column mcol
    int xcol0;              // >= 0: column xcol0 + k holds a copy of delta of extra column k (next to the frame maximum); -1: none
    int aux_frames;         // 1, or 3 (wave form with every row stored and one extra column, wave_aux_frames): row t also carries the scalars of
                            // frames t-1 and t-2, at columns mcol + 2k / xcol0 + 2k -- the back-trace reads the scalars of frame t from the
                            // carrier row wave_aux_row(t, last row) and touches one scalar line per three frames instead of one per frame
    int chunks, warm;       // time-parallel back-trace: chunks per song, warm-up frames
    int banded;             // 1: row structure (window / c0 / extras / dense rows) proven by the plan
    int have_fmax;          // the forward pass was a banded kernel (it fills pad column S of the history rows)
    int bt_form;            // 0 auto (sparse fetch where it applies) | 1 generic (lazy) kernel | 2 whole-row kernels
    int lo_affine, lo_off;  // lo[j] == clamp(j - lo_off, 0, S - W)
    int dense_rows[kMaxDenseRows];
    int n_extras, n_dense;
    int extras[kMaxExtras];
    float c0;
    size_t off_lo, off_kind, off_tabA, off_extraA, off_denseA, off_Arow, off_rowc, off_tabX, off_stepC;
    int step_ok, step_kb, step_mult;   // step-structured dense matrix: band = min((dist * step_mult) >> 16, step_kb)
    float step_cn;
    // half history (wave form, WaveHist::Half): row r of a song holds frame 2r; its aux slots mcol / xcol0 + k carry the frame maximum and the
    // extra-column deltas of frame 2r, slots mcol_odd / xcol0_odd + k those of frame 2r - 1.  The back-trace reads the emissions again.
    int hist_half;
    int64_t hist_rows;
    int mcol_odd, xcol0_odd;
    const void* logE;       // [B,T,S] the tensor vit_forward decoded (f32 or f16)
    int e_f16;
    int64_t states_stride;  // states of song b start at states + b * states_stride (T; a segment of a checkpointed decode: the whole song's T)
    int block_waves;        // half back-trace: waves per workgroup (0 / 16 default | 8 | 4: small enough to start beside resident forward waves)
    int no_fast_rows;       // sparse / half back-trace: 1 = every row through the general code (vit_plan_set_option "bt_fast_rows" 1; tests)
    int skip_nonpositive;   // sparse, lane and lazy (launch_backtrace_rows_segment) kernels: a song whose lengths[] entry is < 1 is skipped
                            // (segments; vit_decode clamps to 1 instead)
    int32_t* counters;      // [B][kBtCounters] per-song event counts of the sparse / half / half-wave kernels (zeroed by vit_backtrace)
    // packed batch (vit_decode_packed): history rows / states of song b at offsets[b] (its length: offsets[b+1] - offsets[b]); the
    // speculative pass runs one wave per entry of wave_song (song b owns waves chunk_base[b] .. chunk_base[b+1]-1 = its chunks;
    // chunk entries are indexed the same way)
    // (lane form and, for plans that are not banded, the lazy kernel of backtrace_rows.hip: launch_backtrace_rows_packed)
    const int64_t* offsets; // device [B+1], or null
    const int32_t* wave_song;    // device [n_waves]
    const int32_t* chunk_base;   // device [B+1]
    int n_waves;
    uint32_t* mask;         // [B][kLaneMaskWords] lane form: bit c = chunk c assumed the wrong state at its upper boundary (zeroed by vit_backtrace)
    // sparse kernel and the lazy kernel's segment form over the segment units of a packed checkpointed decode: the states of sub-problem b start at states +
    // unit_states[b] (not b * states_stride), and nothing is written behind its lengths[b] frames -- those belong to the next song
    const int64_t* unit_states;  // device [B], or null
    // lane form over the committed ranges of a streaming session (vit_stream_commit): sub-problem b is rows / frames first_row[b] ..
    // first_row[b] + lengths[b] - 1 of song b (history by hist_rows, states by states_stride, both moved by first_row[b]); null: 0
    const int64_t* first_row;    // device [B], or null
    // the same over a ring session (vit_stream_open_ring): ring_rows = R > 0 -- row k of sub-problem b is row (first_row[b] + k) mod R of
    // song b's R rows (hist_rows = R; lengths[b] <= R); 0: rows as above.  states_rel = 1: the states of sub-problem b start at states +
    // b * states_stride, not moved by first_row[b] (vit_stream_commit_rel, vit_stream_tail); 0: as above
    int64_t ring_rows;
    int states_rel;
};

// fused.hip: emission builder + wave-form forward recursion in one workgroup (vit_decode_logits).  f: the forward pass's arguments
// (logE unused: the emission rows never leave the CU; hist_rows = T, full history in the wave layout); the rest: the builder's
// (emission.hip; mode 0 "shaun" | 1 softmax, logits [B, T, n_bins + 1] with the unvoiced column first | 2 scaled softmax).
struct FusedArgs {
    FwdArgs f;
    const float* logits;    // [B, T, n_bins] (mode 1: n_bins + 1) float32
    float* logE_out;        // [B, T, n_bins + 1] or null: the producers also write their rows here
    int mode, n_bins, spw;
    double threshold, offset, scale;   // mode 0: threshold logit, offset, scale; mode 2: threshold = the unvoiced logit
    const float* prior;     // mode 2: [n_bins + 1] or null
};
// what fused.hip is instantiated for: the wave form with six states per lane and ONE extra column that is the last state (wave_u5 =
// FwdArgs::wave_u5 after the plan's options, 1 .. 3), and the builders the reference ships for the 320- and 360-bin grids
constexpr bool fused_logits_applies(int S, int wave_ok, int wave_npl, int wave_dk, int n_extras, int wave_u5, int mode, int n_bins, int spw) {
    return wave_ok && wave_npl == 6 && wave_dk == 14 && n_extras == 1 && wave_u5 >= 1 && wave_u5 <= 3 && n_bins + 1 == S &&
           (n_bins == 360 || (n_bins == 320 && wave_u5 != 2)) && 64 * 6 - S >= 6 &&
           ((mode == 0 && spw == 5) || (mode == 1 && spw == 15) || (mode == 2 && spw == 5));
}
hipError_t launch_fused_logits(const FusedArgs& fa, hipStream_t st);
// fused_ckpt.hip: the same workgroup for vit_decode_logits_checkpointed, with FwdArgs' checkpoint fields as wave.hip reads them (WaveHist::CkptPass /
// Segment).  segment false = pass 1: f.ckpt_every = K, f.hist_rows = segments per song (the last row is the scratch row).  segment true:
// frames f.t_begin .. min(f.t_end, length) - 1 resumed from f.init_rows (t_begin > 0), row t at t - t_begin of the song's f.hist_rows
// rows; the emission rows are rebuilt from the logits.  logE_out is honoured by both but the decode passes none.
hipError_t launch_fused_logits_ckpt(const FusedArgs& fa, bool segment, hipStream_t st);

// f64.hip: the float64-accumulating decode (vit_decode_f64): float32 parameters and emissions, d (the reference's float64 T1) in double.
// The floor form in double, so what it serves is what the floor form is proven and instantiated for: banded plans with floor_ok, no
// dense rows, an instantiated window width and a target-wave count.  Unstructured, step and dense-row plans are refused.
constexpr bool f64_decode_applies(int S, int W, bool banded_ok, bool floor_ok, int n_dense) {
    return banded_ok && floor_ok && n_dense == 0 && banded_width_instantiated(W) && W <= S && banded_waves_for(S) > 0;
}
// history row stride in doubles: state i in column i, the frame maximum M_t (over the non-extra sources) in column S; rows 16-byte aligned
constexpr int f64_hist_stride(int S) { return (S + 3) / 2 * 2; }
struct F64Args {
    const uint8_t* image;   // device plan image, read as it is: tabA, lo, rowc, extraA, log_pi, tabX
    const void* logE;       // [B,T,S] f32 or f16
    const int64_t* lengths; // [B] or null
    double* hist;           // [B,T,SD64]
    int32_t* last_state;    // [B]
    double* loglik;         // [B] or null
    int32_t* states;        // [B,T]
    int32_t* entry;         // [B,chunks] state each chunk assumed at its upper boundary
    int64_t B;
    int T, S, SP, SD64, W;
    int n_extras;
    int extras[kMaxExtras];
    int chunks, warm;       // time-parallel back-trace: chunks per song (<= kBtMaxChunks), warm-up frames
    size_t off_logpi, off_lo, off_tabA, off_extraA, off_rowc, off_tabX;
    // packed batch (vit_decode_f64_packed; behind the fields above, whose places the plain kernels keep): logE, hist and states are
    // [sum T_b, ..], the rows of song b start at row offsets[b]; entry is [n_waves]
    const int64_t* offsets;     // [B+1] frame offsets
    int n_slots;                // forward slots: one workgroup each
    const int32_t* slot_begin;  // [n_slots+1]
    const int32_t* slot_songs;  // [B] song ids grouped by slot
    const int32_t* wave_song;   // [n_waves] song of each back-trace wave (speculative pass)
    const int32_t* chunk_base;  // [B+1] first wave / chunk entry of each song; chunks = the largest chunk count of any song
    int n_waves;
    // checkpointed decode (vit_decode_f64_checkpointed; the Ckpt variant of both kernels).  Forward: ckpt_every = K > 0 is pass 1 -- every
    // frame of the song, the d row of frame mK - 1 kept at row m - 1 of the song's rows of hist, nothing else stored but the terminal
    // state and log-likelihood; ckpt_every = 0 is one segment -- frames t_begin .. min(length, t_end) - 1, resumed from
    // init_rows[song] = d_{t_begin - 1} where t_begin > 0, row t stored at t - t_begin (and M of frame t_begin - 1 in the row in
    // front of hist).  A song's rows start hist_song_stride doubles after the one before.  Back-trace: song b is a sub-problem of
    // seg_len[b] frames (0: skipped) that starts from state seg_last[b]; states is advanced to the segment's first frame.
    int ckpt_every, t_begin, t_end;
    const double* init_rows;
    int64_t init_stride;        // doubles from one song's init row to the next
    int64_t hist_song_stride;
    const int64_t* seg_len;     // [B]
    const int32_t* seg_last;    // [B]
    // packed checkpointed decode (vit_decode_f64_packed_checkpointed; the PackedCkpt variant of both kernels; FwdArgs' fields of the same
    // names).  ckpt_every = K always; song b has n_b = ceil(T_b / K) segments.  unit_song null = pass 1: the slot walk of the packed
    // batch, the d rows of frames mK - 1 (m = 1 .. n_b - 1) kept at rows ckpt_base[b] + m - 1 of hist.  unit_song set = the B units of
    // one launch: workgroup u runs segment unit_seg[u] of song unit_song[u], resumed from row ckpt_base[song] + segment - 1 of init_rows
    // (segment 0: from the prior), into rows hist + u * hist_song_stride (the row in front of them takes M of the checkpoint frame).
    // Back-trace: unit u is the sub-problem seg_len[u] / seg_last[u] over those rows, its states start at states + unit_states[u].
    const int64_t* ckpt_base;   // [songs] checkpoint rows in front of song b's = sum of (n_b' - 1) over b' < b
    const int32_t* unit_song;   // [B units of this launch]
    const int32_t* unit_seg;    // [B units of this launch]
    const int64_t* unit_states; // [B units of this launch] offsets[song] + segment * K (launch_packed_segment_prep)
};
// What a workgroup of f64_floor_forward_kernel decodes and what the waves of f64_backtrace_kernel walk (described at the kernels):
//   Plain   a song each, every row kept; a.chunks chunks per song                                   (vit_decode_f64)
//   Packed  forward: the songs of a slot (a.n_slots workgroups); back-trace: one wave per entry of
//           a.wave_song, rows at offsets[song]                                                      (vit_decode_f64_packed)
//   Ckpt    forward: pass 1 (a.ckpt_every > 0) or one segment (a.t_begin / a.t_end, resumed from
//           a.init_rows); back-trace: the sub-problems a.seg_len / a.seg_last of one segment         (vit_decode_f64_checkpointed)
//   PackedCkpt  forward: pass 1 over the songs of a slot (a.unit_song null), or one (song, segment) unit per
//           workgroup (a.B units); back-trace: the units' sub-problems, states at a.unit_states      (vit_decode_f64_packed_checkpointed)
// f64_forward_resident: workgroups of the forward instantiation one compute unit holds at once (Packed and PackedCkpt, whose slot
// launches are sized by it; hipErrorInvalidValue for the others, as *_variant_resident).
enum class F64Variant { Plain, Packed, Ckpt, PackedCkpt };
// Units per compute unit and launch of the packed checkpointed decode's pass 2, per forward instantiation (W, target waves): 1 where the
// workgroup runs twelve waves (W >= 84 there also fills most of the LDS), elsewhere the workgroups whose waves fit one CU's registers
// -- four SIMDs x the waves per SIMD the kernel's register count allows (4 at W = 16, 3 at W = 32, 2 above:
// profiles/f64_packed_ckpt_resources.txt) over the workgroup's waves -- capped at 4; the LDS (at most 17 KB on eight waves) never binds.
// Every unit owns its rows: tuning, not correctness.  Measured at (32, 6), S = 361, 804 recordings: 2 beats 1 and 4 with disjoint
// ranges, also at equal bytes (profiles/f64_packed_ckpt_time.json).
constexpr int f64_pckpt_units_per_cu(int W, int nwt) {
    const int by_regs = 4 * (W <= 16 ? 4 : W <= 32 ? 3 : 2) / nwt;
    return nwt >= 12 || by_regs < 1 ? 1 : by_regs > 4 ? 4 : by_regs;
}
hipError_t launch_f64_forward(const F64Args& a, F64Variant v, bool f16, hipStream_t st);
hipError_t f64_forward_resident(const F64Args& a, F64Variant v, bool f16, int* per_cu);
hipError_t launch_f64_backtrace(const F64Args& a, F64Variant v, hipStream_t st);
hipError_t launch_dense(const FwdArgs& a, int songs_per_group, bool f16, hipStream_t st);
hipError_t launch_step(const FwdArgs& a, bool f16, hipStream_t st);
hipError_t launch_banded(const FwdArgs& a, bool f16, hipStream_t st);
hipError_t launch_wave(const FwdArgs& a, bool f16, hipStream_t st);   // wave.hip: one song per wavefront; the mode: wave_hist_of (wave_common.hpp)
// The variants of the workgroup kernels, for plans without the wave form (Plain is not one: launch_banded / launch_step; hipErrorInvalidValue here):
//   Packed      one workgroup per slot (a.n_slots, a.offsets, a.slot_begin, a.slot_songs)
//   Ckpt        one workgroup per song: pass 1 (a.ckpt_every > 0: checkpoint rows + terminal state) or one segment (a.t_begin / a.t_end,
//               resumed from a.init_rows; the banded kernel also writes one pad column of the row in front of a.hist, see banded_floor.inc)
//   PackedCkpt  a.ckpt_base set, a.ckpt_every = K.  a.unit_song null = pass 1: one workgroup per slot (a.n_slots) walks its songs, keeps
//               the rows in front of segments 1 .. n_b - 1 at rows ckpt_base[b] .. of a.hist and sends every other store to scratch row
//               a.hist_rows + slot.  a.unit_song set = one workgroup per unit (a.B of them): segment unit_seg[u] of song unit_song[u],
//               resumed from row ckpt_base[song] + segment - 1 of a.init_rows, into rows u * a.hist_rows .. of a.hist (the banded kernel
//               also writes one pad column of the row in front of them and runs one frame past the segment where the song goes on:
//               K + 2 rows per unit, a.hist at the second; the step kernel: K + 1).
//   Stream      one workgroup per song of a session (a.B): a.unit_song / a.unit_seg = this launch's positions and counts, or both null and
//               a.t_begin / a.t_end for every song; a.logE = the chunk, a.init_stride its elements per song; rows at their absolute
//               index of the song's a.T rows, resumed from the row in front of the first (see FwdArgs)
// *_variant_resident: workgroups of that instantiation one compute unit holds at once (the occupancy query at its LDS size; Packed and
// PackedCkpt, whose launches are sized by it).
hipError_t launch_banded_variant(const FwdArgs& a, WgVariant v, bool f16, hipStream_t st);
hipError_t banded_variant_resident(const FwdArgs& a, WgVariant v, bool f16, int* per_cu);
// banded.hip -> banded_pc.hip: the PackedCkpt instantiations of the floor kernel build in a translation unit of their own
hipError_t floor_pckpt(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu);
// banded.hip -> banded_stream.hip: the Stream instantiations, likewise
hipError_t floor_stream(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu);
// banded.hip -> banded_stream_ring.hip: the StreamRing instantiations, likewise
hipError_t floor_stream_ring(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu);
hipError_t launch_step_variant(const FwdArgs& a, WgVariant v, bool f16, hipStream_t st);
hipError_t step_variant_resident(const FwdArgs& a, WgVariant v, bool f16, int* per_cu);
// what a variant launch needs of FwdArgs; rows_in_front: extra rows the check demands of a unit's hist_rows beyond K (as before: banded 2, step 0)
inline bool wg_variant_args_ok(const FwdArgs& a, WgVariant v, int rows_in_front) {
    const bool slots = a.slot_begin && a.slot_songs && a.n_slots >= 1;
    switch (v) {
        case WgVariant::Packed: return a.offsets && slots;
        case WgVariant::Ckpt: return !a.offsets && a.hist_rows >= 1 && (a.t_begin <= 0 || a.init_rows) && (a.ckpt_every <= 0 || a.t_begin <= 0);
        case WgVariant::PackedCkpt:
            if (!a.offsets || !a.ckpt_base || a.ckpt_every < 1 || a.hist_rows < 0) return false;
            return a.unit_song ? (a.unit_seg && a.init_rows && a.B >= 1 && a.hist_rows >= (int64_t)a.ckpt_every + rows_in_front) : slots;
        case WgVariant::Stream:
            if (a.offsets || a.lengths || a.B < 1 || a.T < 1 || a.init_stride < 0 || !a.unit_song != !a.unit_seg) return false;
            return a.unit_song || (a.t_begin >= 0 && a.t_end >= a.t_begin && a.t_end <= a.T);
        case WgVariant::StreamRing:     // frames are absolute (a.T: their limit), rows live in a ring of a.hist_rows rows per song
            if (a.offsets || a.lengths || a.B < 1 || a.T < 1 || a.init_stride < 0 || !a.unit_song != !a.unit_seg || a.hist_rows < 2) return false;
            return a.unit_song || (a.t_begin >= 0 && a.t_end >= a.t_begin && a.t_end <= a.T && a.t_end - a.t_begin <= a.hist_rows);
        default: return false;   // (Plain has no variant launch)
    }
}
// per song, for the segment [s0, e0) of a checkpointed decode: the sub-problem's length (0: the song ends before s0) and the state
// its back-trace starts from (the state already decided at frame e0, or the song's terminal state)
hipError_t launch_segment_prep(const int64_t* lengths, int64_t B, int T, int s0, int e0, const int32_t* states, const int32_t* last,
                               int64_t* seg_len, int32_t* seg_last, hipStream_t st);
// the same per segment unit of a packed checkpointed decode (unit u = segment unit_seg[u] of K frames of song unit_song[u], whose
// frames sit at offsets[song]); also the unit's first entry in the packed states (BtArgs::unit_states)
hipError_t launch_packed_segment_prep(const int64_t* offsets, const int32_t* unit_song, const int32_t* unit_seg, int n_units, int K,
                                      const int32_t* states, const int32_t* last, int64_t* seg_len, int32_t* seg_last, int64_t* unit_states,
                                      hipStream_t st);
// history layout of the wave form: row stride 64*npl floats, state i in column 64*npl - S + i, the frame maximum in column 0,
// a copy of delta of extra column k in column 1 + k
constexpr int wave_hist_stride(int npl) { return 64 * npl; }
// frames whose scalars a full-history row of the wave form carries in lane 0's idle slots (the row's own and the two before it)
constexpr int wave_aux_frames(int npl, int S, int n_extras) { return n_extras == 1 && npl >= 6 && 64 * npl - S >= 6 ? 3 : 1; }   // (six idle slots)
// the row the back-trace takes the scalars of frame t from: the next row with t % 3 == 2, or the last row written
__host__ __device__ constexpr int wave_aux_row(int t, int last) { return t - t % 3 + 2 < last ? t - t % 3 + 2 : last; }
hipError_t launch_backtrace(BtArgs a, hipStream_t st);
// the lazy kernel over a packed batch: one wave per entry of wave_song, then one wave per song (a.chunks = the largest per-song count)
hipError_t launch_backtrace_rows_packed(BtArgs a, hipStream_t st);
// backtrace_sparse.hip: fetches only the span of each history row around the path (banded plans, candidates on one lane)
bool sparse_backtrace_applies(const BtArgs& a);
// phases: bit 0 the speculative pass (one wave per (song, chunk)), bit 1 the verify-and-repair pass (one wave per song)
hipError_t launch_backtrace_sparse(const BtArgs& a, hipStream_t st, int phases = 3);
// backtrace_half.hip: the same for a half history (wave form, even rows only): odd frames are rebuilt from the row before them
bool half_backtrace_applies(const BtArgs& a);
hipError_t launch_backtrace_half(const BtArgs& a, hipStream_t st, int phases = 3);
// the lazy kernel over one segment of a checkpointed decode (plans that are not banded): song bases from hist_rows / states_stride,
// songs with lengths[] < 1 skipped (skip_nonpositive), a.chunks from the segment length; with a.unit_states the sub-problems are the
// units of a packed checkpointed decode: states at states + unit_states[b], nothing written behind a unit's lengths[b] frames
hipError_t launch_backtrace_rows_segment(BtArgs a, hipStream_t st);
int sparse_backtrace_chunks(int64_t B, int T, int n_cus);
// backtrace_lane.hip: one (song, chunk) stream per LANE (banded plans, full history): ~130 wave instructions per 64 decisions
bool lane_backtrace_applies(const BtArgs& a);
hipError_t launch_backtrace_lane(const BtArgs& a, hipStream_t st, int phases = 3);
int lane_backtrace_chunks(int64_t B, int T, int n_cus, int warm);
// stream_commit.hip: the commit point of a streaming session (vit_stream_commit).  b: the plan's fields, the session's rows (hist,
// hist_rows, the workgroup row layout with aux_frames = 1) and the caller's states / states_stride; one workgroup per recording.
struct CommitArgs {
    BtArgs b;
    const int64_t* pos;       // device [B]: frames appended so far
    int64_t* frontier;        // device [B]: frames committed so far (the commit state; read unless `reset`, then written)
    int64_t* committed;       // device [B]: the caller's copy of the new frontier
    // the committed range [f, c] as a sub-problem of the lane back-trace (BtArgs::first_row / lengths / last_state), device [B] each
    int64_t* sub_first;       // f
    int64_t* sub_len;         // c - f + 1, or 0: nothing committed (skip_nonpositive)
    int32_t* sub_last;        // s_c
    int64_t max_lookback;     // the merge is looked for in frames [max(f, n - 1 - max_lookback), n - 2]
    int reset;                // 1: every frontier counts as 0 (first commit after vit_stream_commit_begin / vit_stream_reset)
    int64_t* first;           // device [B], or null: the caller's copy of f, the frontier before this commit (vit_stream_commit_rel)
};
// the frames behind the frontier as sub-problems of the lane back-trace (vit_stream_tail): sub_first[b] = first[b] = f_b (0 with `reset`),
// sub_len[b] = pos[b] - f_b, sub_last[b] = last_state[b]; the frontier is read only
hipError_t launch_stream_tail_prep(const CommitArgs& c, const int32_t* last_state, hipStream_t st);
bool stream_commit_applies(const BtArgs& a);
bool stream_commit_table_in_lds(const BtArgs& a);
hipError_t launch_stream_commit(const CommitArgs& c, hipStream_t st);
hipError_t launch_voicing_map(const int32_t* states, int64_t n, int32_t n_bins, uint8_t* voiced, int32_t* bins,
                              hipStream_t st);
hipError_t launch_scan_selftest(const float* vals, int n_waves, int mode, float* out_v, int32_t* out_i,
                                hipStream_t st);
hipError_t launch_obs_shaun(const float* logits, int64_t n_frames, int U, int spw, double thr, double off, double sc,
                            float* out, hipStream_t st);
hipError_t launch_obs_softmax(const float* logits, int64_t n_frames, int U, int spw, float* out, hipStream_t st);
hipError_t launch_obs_softmax_scaled(const float* logits, int64_t n_frames, int U, int spw, double unvoiced_logit,
                                     const float* prior, float* out, hipStream_t st);
// emission_half.hip: the same builders with float16 logits (l16) and / or float16 emissions (e16), at least one of the two; mode 0 / 1 / 2
// = shaun / softmax / softmax_scaled, thr = the threshold logit (0) or the unvoiced logit (2)
hipError_t launch_obs_half(int mode, const void* logits, bool l16, int64_t n_frames, int U, int spw, double thr, double off, double sc,
                           const float* prior, void* out, bool e16, hipStream_t st);
hipError_t launch_snippets_append_f16(const void* snips, int n, int C, int F, int mode, float* out, int64_t rows, hipStream_t st);
// activations.hip: imm's activation front-end (vit_obs_activations): hf0 [U, total] with row stride ld -> log(hf0 + t_b) transposed to
// [total, U + 1], statistics per recording into stats [B][4]
hipError_t launch_activations(const float* hf0, int64_t ld, int U, int B, const int64_t* offsets, int64_t total, uint32_t clamp_below_bits,
                              float clamp_to, float* stats, void* out, bool f16, hipStream_t st);
hipError_t launch_snippets_append(const float* snips, int n, int C, int F, int mode, float* out, int64_t rows, hipStream_t st);
hipError_t launch_voicing_notes(const int32_t* states, int64_t n, int32_t n_bins, const float* note_range, uint8_t* voiced,
                                int32_t* bins, float* notes, float* notes_v, hipStream_t st);
int backtrace_tile_rows(int SD);
constexpr int kBtWarm = 128;       // warm-up frames of a speculative chunk (survivor paths coalesce within tens of frames)
constexpr int kBtWarmSparse = 64;  // the sparse kernel runs many short chunks: a shorter warm-up (a wrong guess only costs a repair)
constexpr int kBtMaxChunks = 32;    // one stream per wavefront (sparse / half / whole-row kernels)
constexpr int kLaneMaxChunks = 256; // one stream per lane (backtrace_lane.hip); the workspace holds [B][kLaneMaxChunks] chunk entries
constexpr int kLaneMaskWords = kLaneMaxChunks / 32;
// per-song event counters (include/viterbi_hip.h vit_backtrace_counters): tiles fetched, span misses, whole-row evaluations
// (bound failures), of those: odd rows rebuilt in full, chunks repaired, frames rewritten by repairs
constexpr int kBtCounters = 16;
enum { kCtTiles = 0, kCtMisses = 1, kCtFullRows = 2, kCtRebuilt = 3, kCtRepairs = 4, kCtRepairFrames = 5 };
int backtrace_chunks(int64_t B, int T);

}  // namespace vit
