// plan.hpp -- host-side analysis of a log-domain transition matrix.
//
// Pure C++ (no HIP): compiled into libviterbi_hip.so by hipcc and into
// libviterbi_plan_host.so by g++ so that the analysis and the exactness of the
// banded decomposition can be tested on a machine without a GPU.
//
// The decomposition: the production matrices built by the
// reference's */viterbi_transition_post_processing.py are
//   band(+/- d_max) + one dense row + one dense column, every other entry the
//   single constant c = log(0 + tiny).
// For a target row j whose entries outside a window [lo_j, lo_j+W) and outside a
// few shared "extra" columns all equal one constant c_j, rounding is monotone, so
//   max_{i outside} fl(delta_i + c_j) = fl( max_{i outside} delta_i + c_j ):
// one prefix-max and one suffix-max scan over the raw delta vector, evaluated at
// the window edges, replace S - W candidates per target.  Every value compared
// is one the dense recursion also computes, so the result is bit-identical.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vit {

constexpr int kMaxExtras = 4;
constexpr int kMaxDenseRows = 4;
// Window widths the banded kernels are instantiated for (jdc: d_max 40 -> 82, imm: 56 -> 114), narrowest first: the plan picks
// from these, and launch_banded_e (banded.hip) and launch_backtrace_lane (backtrace_lane.hip) have one case per entry (a
// static_assert next to each counts them).
inline constexpr int kBandedWidths[] = {16, 32, 64, 84, 96, 128};
constexpr bool banded_width_instantiated(int W) {
    for (int w : kBandedWidths)
        if (w == W) return true;
    return false;
}

struct BandedPlan {
    bool ok = false;          // the decomposition was proven for this matrix
    int S = 0;
    int SP = 0;               // S rounded up to a multiple of 64 (threads per workgroup)
    float c0 = 0.f;           // the most common row constant (informational)
    std::vector<float> rowc;  // [SP] row constant c_j: every entry of row j outside its window and the extra columns
    int n_extras = 0;
    int extras[kMaxExtras] = {0, 0, 0, 0};
    int n_dense = 0;
    int dense_rows[kMaxDenseRows] = {0, 0, 0, 0};
    int max_window = 0;       // widest proven exception window among banded rows
    int W = 0;                // window width the kernel evaluates (16/32/64/96/128)
    std::vector<int32_t> lo;  // [SP] first source of the evaluated window (lo + W <= S)
    std::vector<int32_t> kind;// [SP] -1 banded row, d >= 0 dense row d, -2 padding
    bool lo_affine = false;   // lo[j] == clamp(j - lo_off, 0, S - W) for every banded row
    bool floor_ok = false;    // every non-extra window entry of every banded row is >= that row's constant, and no dense rows:
                              // then max_{i outside window} fl(delta_i + c_j) can be replaced by fl(max_{all non-extra i} delta_i + c_j)
    std::vector<int32_t> live_last;   // [S] floor_ok plans: the last window position of banded row j that is neither an extra column nor, in bits,
                              // the row constant (-1: none).  Behind it the window holds only candidates that fl(M + c_j) or the
                              // extra-column path already cover (floor_live_width)
    bool pair_ok = false;     // targets (2p, 2p+1) share one window [lo2[p], lo2[p]+W) that covers both exception spans
    std::vector<int32_t> lo2; // [SP/2]
    bool lo2_affine = false;  // lo2[p] == clamp(2p - lo2_off, 0, S - W)
    int lo2_off = 0;
    int lo_off = 0;

    // "Step" structure (the Durrieu matrix of imm's own decoder; analyze_step): with n = S-1 voiced states, for voiced
    // source i and voiced target j  logA_T[j][i] == stepC[min(|i-j| / step_bw, step_kb)][i]  -- column i is piecewise
    // constant in distance bands of step_bw bins, constant from distance step_kb*step_bw on --, no near band of a column
    // is below its far value, and the unvoiced source column is one value for every voiced target (step_cn).  Then
    // fl(delta_i + logA_T[j][i]) takes only step_kb+1 values per source and the far sources reduce to ONE maximum.
    bool step_ok = false;
    int step_bw = 0, step_kb = 0;
    std::vector<float> stepC;   // [(kMaxStepBands+1)][SP]; -inf in the rows > step_kb (unused), in the columns i >= n, and where no voiced
                                // target lies in band k of source i (n < 2 * step_kb * step_bw: a middle source has no far band)
    float step_cn = 0.f;

    // "Wave" form (wave_forward_kernel: one song per wavefront, no LDS, no barrier).  Lane l owns the wave_npl =
    // ceil(S/64) contiguous states wave_npl*l ..; every exception span lies within wave_d sources of its target
    // (|i - j| <= wave_d), so a lane needs delta only from the lanes within ceil(wave_d / wave_npl) of itself.
    bool floor_all_ok = false;  // floor_ok, and every extra-column entry of a banded row is >= that row's constant too:
                                // then the frame maximum M may be taken over ALL sources (a dominated candidate more)
    bool wave_ok = false;       // floor_all_ok, no dense rows, <= kWaveMaxExtras extra columns, an instantiated geometry
    int wave_npl = 0;
    int wave_d = 0;             // proven half-width
    int wave_dk = 0;            // half-width the kernel (and tabV) is instantiated for (>= wave_d)
};

constexpr int kWaveMaxExtras = 2;
// half-width the wave kernel is instantiated for, given the states per lane and the proven half-width (0: none)
constexpr int wave_table_d(int npl, int d) { return (npl == 6 && d <= 14) ? 14 : 0; }
constexpr int wave_pairs(int dk) { return dk + 1; }   // packed source pairs per target: 2*dk + 1 sources, even-aligned
constexpr int wave_halo(int npl, int dk) { return (dk + npl - 1) / npl; }   // lanes a lane looks at on each side
// A lane's neighbourhood is the npl * (2*halo + 1) sources of lanes l-halo .. l+halo, position p <-> source
// npl * (l - halo) + p.  Own state k evaluates the even-aligned positions p0e .. p0e + 2*(dk+1) - 1, which cover
// its sources j - dk .. j + dk; pair m, half h sits at p0e + 2m + h.
constexpr int wave_p0e(int npl, int dk, int k) { return (k + npl * wave_halo(npl, dk) - dk) & ~1; }

constexpr int kMaxStepBands = 15;
// Fills the step_* fields of bp (bp.SP must be set: call after analyze_banded).
void analyze_step(const float* logA_T, int S, BandedPlan& bp);

// Analyse logA_T ([S,S] row-major, row j = into target j).
BandedPlan analyze_banded(const float* logA_T, int S);
// Live window width of the targets [0, n_rows) under the floor-max form: 1 + the last window position any of them must still evaluate.
// A trailing position w of row j is droppable when source lo_j + w is an extra column (the extra-column path forms that candidate anyway)
// or A[j][lo_j + w] is, in bits, the row constant c_j: then fl(delta_i + c_j) <= fl(M + c_j), which the floor form carries (rounding is
// monotone; M is the maximum over every non-extra source).  Only the trailing run is trimmed.  W where the plan does not prove the floor
// form (floor_ok, no dense rows): nothing may be dropped there.
int floor_live_width(const BandedPlan& bp, int n_rows);
// The split floor kernel (banded.hip): its full-window waves own targets [0, kSplitFullRows) and are instantiated for the whole window and
// for the live widths of the reference's grids (25: the 321-state grids, 29: the 361-state grid); a proven live width takes the
// narrowest instantiated one that covers it, anything else the whole window.
constexpr int kSplitFullRows = 256;
inline constexpr int kSplitLiveWidths[] = {25, 29};
// Everything the choice depends on, for the launcher (launch_floor_t, banded.hip) and the host library alike: the split kernel exists
// for W = 32 on the six-wave grids (256 < S < 384), and its trimmed instantiations for one extra column and fp32 emissions.
constexpr int split_full_width(int live, int W, int S, int n_extras, bool f16) {
    if (W != 32 || S <= kSplitFullRows || S >= 384 || n_extras != 1 || f16) return W;
    for (int w : kSplitLiveWidths)
        if (live >= 1 && live <= w && w < W) return w;
    return W;
}
// Rounds of the split kernel's frame loop.  Frames 1 .. Tb - 1 of a song run in rounds of PF unrolled frames that start at
// t = 1, 1 + PF, ..., and a tail of up to PF - 1 frames behind the last full round; frame t + u of a round that starts at t requests the
// emission row of frame t + u + PF, held at the song's last row.  A round is
//   full      when all its PF frames exist (its last frame t + PF - 1 <= Tb - 1);
//   interior  when none of its requests is held back (its last request t + 2 PF - 1 <= Tb - 1): the row offset of frame t + u is the
//             constant u and the loop body has no clamp.  Every full round but the last is interior.
// split_prefetch_row is the row frame t + u requests: in an interior round the unclamped sum, which the two conditions above keep
// inside the song; anywhere else the clamped one.  The kernel's loops and the host library's replay (vph_split_rounds) are both
// written with these three.
constexpr bool split_round_full(int t, int PF, int Tb) { return t + PF - 1 <= Tb - 1; }
constexpr bool split_round_interior(int t, int PF, int Tb) { return t + 2 * PF - 1 <= Tb - 1; }
constexpr int split_prefetch_row(int t, int u, int PF, int Tb, bool interior) {
    const int r = t + u + PF;
    return interior || r < Tb - 1 ? r : Tb - 1;
}
// the prefetch depth the split kernel is instantiated with (floor_pf<32>(), banded_floor.inc)
inline constexpr int kSplitPrefetch = 12;
// Copy writes of the split kernel's full-window waves (waves 0 .. 3, target j = 64 wave + lane).  delta[j] of buffer b goes to copy c
// at float split_copy_pos(sh, j, b, c) of the LDS segment (sh = win_shift; the four copies lie kSplitCopyStride floats apart, each
// shifted one float down against the one before, two buffers of four copies: FloorSplitLds, banded_floor.inc).  The kernel stores it
// with ds_write_addtid_b32, whose byte address is M0 + immediate + 4 * lane:
//   M0        = split_addtid_base(sh, wave), set once per wave (plus the LDS address of the segment, which the kernel takes from the pointer)
//   immediate = split_addtid_imm(b, c), a constant of the unrolled frame and copy
// Both are 16-bit fields.  The kernel, floor_lds_check.hip and the host library (vph_split_addtid) are written with these.
inline constexpr int kSplitCopyStride = 384 + 16;
constexpr int split_copy_pos(int sh, int j, int b, int c) { return 4 + sh + j + b * 4 * kSplitCopyStride + c * kSplitCopyStride - c; }
constexpr int split_addtid_base(int sh, int wave) { return 4 * (4 + sh + 64 * wave); }
constexpr int split_addtid_imm(int b, int c) { return 4 * (b * 4 * kSplitCopyStride + c * kSplitCopyStride - c); }
// Copy, lane and slot maps of the floor kernels' publication (used by the kernels in banded_floor.inc / banded.hip, by
// floor_lds_check.hip and by the replay below).  Copy c of a delta buffer holds delta[i] floor_copy_off(DC, c) floats behind copy 0's
// entry; an upper lane of the split kernel's half waves writes copies 2 and 3, so its write pointer starts split_upper_off(DC) further on.
constexpr int floor_copy_off(int DC, int c) { return c * DC - c; }
constexpr int split_upper_off(int DC) { return floor_copy_off(DC, 2); }
inline constexpr int kSplitFullWaves = 4, kSplitHalfWaves = 4;
inline constexpr int kSplitStates = 64 * kSplitFullWaves + 32 * kSplitHalfWaves;   // 384 target slots
inline constexpr int kSplitSlotGroups = 2 * 4 * kSplitCopyStride;                  // float position of the frame-maximum slot groups
constexpr int split_half_of(int lane) { return (lane >> 3) & 1; }
constexpr int split_half_target(int lane) { return ((lane >> 4) << 3) | (lane & 7); }   // 0 .. 31 within the wave
inline constexpr int kSplitXSlot = 3;
constexpr int split_fm_slot(int lane, bool is_x) { return 4 * (lane & 3) + (is_x ? kSplitXSlot : (lane >> 2) % 3); }
// target slot of lane `lane` of wave `wave` (0 .. 3 full, 4 .. 7 half)
constexpr int split_lane_target(int wave, int lane) {
    return wave < kSplitFullWaves ? 64 * wave + lane : 64 * kSplitFullWaves + 32 * (wave - kSplitFullWaves) + split_half_target(lane);
}
// float position of the first window entry lane `lane` of wave `wave` reads from buffer rb (affine plans: lo_j = clamp(j - off, 0, S - 32);
// idle targets read the last window), and of copy `c` of its own target in buffer wb
constexpr int split_window_pos(int S, int off, int sh, int wave, int lane, int rb) {
    const int j = split_lane_target(wave, lane);
    const int lo = j - off < 0 ? 0 : (j - off > S - 32 ? S - 32 : j - off);
    const int lov = (j < S ? lo : S - 32) + sh;
    return 4 + (lov & 3) * kSplitCopyStride + (lov & ~3) + (wave >= kSplitFullWaves ? 16 * split_half_of(lane) : 0) + rb * 4 * kSplitCopyStride;
}
// Extra LDS cycles (what SQ_LDS_BANK_CONFLICT counts) of one wave-instruction: the lanes are served in `ngroups` groups, a group takes
// one cycle and one more for every further distinct address on its busiest bank; `width` dwords per lane, `banks` banks of 4 bytes.
// same_address_serialises: lanes with one address count like lanes with different ones (an LDS atomic applies them one by one).
inline int lds_extra_cycles(const int* pos, const int (*groups)[16], int ngroups, int per_group, int width, int banks, bool same_address_serialises) {
    int total = 0;
    for (int g = 0; g < ngroups; ++g) {
        int worst = 1;
        for (int bank = 0; bank < banks; ++bank) {
            int seen[64], n = 0, lanes = 0;
            for (int i = 0; i < per_group; ++i) {
                const int lane = groups ? groups[g][i] : g * per_group + i;
                for (int k = 0; k < width; ++k) {
                    const int a = pos[lane] + k;
                    if (a % banks != bank) continue;
                    ++lanes;
                    bool dup = false;
                    for (int q = 0; q < n; ++q) dup |= seen[q] == a;
                    if (!dup) seen[n++] = a;
                }
            }
            const int ways = same_address_serialises ? lanes : n;
            if (ways > worst) worst = ways;
        }
        total += worst - 1;
    }
    return total;
}
inline constexpr int kLdsReadB128Groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                                  {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                                  {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                                  {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
// Extra LDS cycles of every LDS instruction one wave of the split kernel issues in a frame that reads buffer rb and writes the other,
// by instruction kind: [0] the slot quad's ds_read_b128, [1] the window's ds_read_b128 (WF / 4 of a full wave, 4 of a half wave),
// [2] a trimmed full wave's ds_read_b32, [3] the copy writes (4 add-tid stores | 2 ds_write_b32), [4] ds_max_f32, [5] the last half
// wave's slot reset.  Bank rules: reads of 16 bytes in four 16-lane groups over 64 banks, everything else in two 32-lane groups over 32.
// copy_of(half, k): the copy a half-wave lane of window half `half` writes with its k-th store (today 2 * half + k).
template <typename CopyOf, typename SlotOf>
inline void split_lds_conflicts(int S, int off, int WF, int wave, int rb, bool atomics_serialise, CopyOf copy_of, SlotOf slot_of, int out[6]) {
    const int sh = off % 4, wb = rb ^ 1, x = S - 1;
    const bool hw = wave >= kSplitFullWaves;
    int pos[64];
    for (int k = 0; k < 6; ++k) out[k] = 0;
    for (int l = 0; l < 64; ++l) pos[l] = kSplitSlotGroups;
    out[0] = lds_extra_cycles(pos, kLdsReadB128Groups, 4, 16, 4, 64, false);
    for (int q = 0; q < (hw ? 4 : WF / 4); ++q) {
        for (int l = 0; l < 64; ++l) pos[l] = split_window_pos(S, off, sh, wave, l, rb) + 4 * q;
        out[1] += lds_extra_cycles(pos, kLdsReadB128Groups, 4, 16, 4, 64, false);
    }
    if (!hw && WF % 4) {
        for (int l = 0; l < 64; ++l) pos[l] = split_window_pos(S, off, sh, wave, l, rb) + WF - 1;
        out[2] = lds_extra_cycles(pos, nullptr, 2, 32, 1, 32, false);
    }
    for (int k = 0; k < (hw ? 2 : 4); ++k) {
        for (int l = 0; l < 64; ++l) pos[l] = split_copy_pos(sh, split_lane_target(wave, l), wb, hw ? copy_of(split_half_of(l), k) : k);
        out[3] += lds_extra_cycles(pos, nullptr, 2, 32, 1, 32, false);
    }
    for (int l = 0; l < 64; ++l) pos[l] = kSplitSlotGroups + slot_of(l, split_lane_target(wave, l) == x);
    out[4] = lds_extra_cycles(pos, nullptr, 2, 32, 1, 32, atomics_serialise);
    if (wave == kSplitFullWaves + kSplitHalfWaves - 1) {
        for (int l = 0; l < 64; ++l) pos[l] = kSplitSlotGroups + 64 + l;
        out[5] = lds_extra_cycles(pos, nullptr, 2, 32, 1, 32, false);
    }
}

// Byte layout of the device image (all offsets in bytes from the image base,
// every section 256-byte aligned).
struct ImageLayout {
    int S = 0, SP = 0, S4 = 0, W = 0, n_extras = 0, n_dense = 0;
    size_t off_logpi = 0;    // float [SP]          (-inf padded)
    size_t off_A4 = 0;       // float [S4][SP][4]   A4[q][j][r] = logA_T[j][4q+r] (-inf padded)
    size_t off_lo = 0;       // int32 [SP]
    size_t off_kind = 0;     // int32 [SP]
    size_t off_tabA = 0;     // float [W][SP]       tabA[w][j] = logA_T[j][lo_j + w]
    size_t off_extraA = 0;   // float [4][SP]       extraA[k][j] = logA_T[j][extras[k]]
    size_t off_denseA = 0;   // float [4][SP]       denseA[d][i] = logA_T[dense_rows[d]][i]
    size_t off_Arow = 0;     // float [S][SP]       row-major copy (row j = into target j) for the back-trace
    size_t off_rowc = 0;     // float [SP]          row constants c_j
    size_t off_lo2 = 0;      // int32 [SP/2]        pair windows (pair_ok)
    size_t off_tabP = 0;     // float [W][SP]       tabP[w][j] = logA_T[j][lo2[j/2] + w]
    size_t off_tabX = 0;     // float [SP][W+5]     per target: W window entries, 4 extra-column entries, row constant (back-trace)
    size_t off_stepC = 0;    // float [16][SP]      step-structure band values per source (step_ok)
    size_t off_tabV = 0;     // float [npl][dk+1][2][64]  wave form: weights of lane l, own state k, source pair m, half h
    size_t bytes = 0;
};

// Launch schedule of pass 2 of the packed checkpointed decode (vit_decode_packed_checkpointed).  Song b (frames offsets[b] ..
// offsets[b+1]-1) has n_b = ceil(T_b / K) segments; a unit is a (song, segment) pair.  The units of a song run from its last segment
// to its first, one per launch at most (the back-trace of segment s starts from the state segment s + 1 decided); every launch
// takes the songs with the most segments left first (ties: lowest song), up to max_units of them, so that the launch count is
// about max(longest n_b, total units / max_units).  Units in launch order: launch l holds units launch_begin[l] ..
// launch_begin[l+1]-1.  ckpt_base[b] = sum of (n_b' - 1) over b' < b: the first of song b's checkpoint rows ([B + 1]).
struct PackedCkptSchedule {
    std::vector<int32_t> unit_song, unit_seg;
    std::vector<int64_t> launch_begin, ckpt_base;
};
// total units, or -1 when offsets are not strictly increasing from 0 or a song is longer than 2^30 frames
int64_t packed_ckpt_units(const int64_t* offsets, int64_t B, int64_t K);
void packed_ckpt_schedule(const int64_t* offsets, int64_t B, int64_t K, int64_t max_units, PackedCkptSchedule& out);

// Per-song chunk table of a packed back-trace (vit_decode_packed, vit_decode_f64_packed): song b is walked in
//   clamp(T_b / cf rounded down, or to nearest with round_nearest, 1, max_chunks)
// chunks of about cf = max(ceil(total frames / streams), min_frames, ceil(longest song / max_chunks)) frames -- `streams` (song, chunk)
// streams wanted at once, no chunk much shorter than min_frames, no song with more than max_chunks.  chunk_base[B + 1]: the first
// stream / chunk entry of each song; wave_song[chunk_base[b] .. chunk_base[b + 1]) = b; *largest: the largest per-song count.
// false, with nothing written at or past wave_song[capacity], when the table needs more than `capacity` entries.
bool packed_chunk_table(const int64_t* offsets, int64_t B, int64_t streams, int64_t max_chunks, int64_t min_frames, bool round_nearest,
                        int64_t capacity, int32_t* chunk_base, int32_t* wave_song, int64_t* largest);

ImageLayout make_layout(int S, const BandedPlan& bp);
void fill_image(const float* logA_T, const float* log_pi, const BandedPlan& bp,
                const ImageLayout& L, uint8_t* image);

}  // namespace vit
