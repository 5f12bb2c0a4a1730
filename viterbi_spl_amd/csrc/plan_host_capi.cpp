// plan_host_capi.cpp -- C entry points over plan.cpp for CPU-only tests (no HIP).
// Exposes the analysis result and the packed device image so that tests can replay
// the banded decomposition on the host and compare it with the dense oracle.
#include <cstring>
#include <vector>

#include "plan.hpp"

extern "C" {

struct vph_plan {
    vit::BandedPlan bp;
    vit::ImageLayout L;
    std::vector<uint8_t> image;
};

vph_plan* vph_create(const float* logA_T, const float* log_pi, int S) {
    vph_plan* p = new vph_plan();
    p->bp = vit::analyze_banded(logA_T, S);
    if (!p->bp.ok) vit::analyze_step(logA_T, S, p->bp);
    p->L = vit::make_layout(S, p->bp);
    p->image.resize(p->L.bytes);
    vit::fill_image(logA_T, log_pi, p->bp, p->L, p->image.data());
    return p;
}
void vph_destroy(vph_plan* p) { delete p; }

// info[0..15]: ok, S, SP, W, n_extras, n_dense, max_window, extras[4], dense_rows[4], S4
void vph_info(const vph_plan* p, int* info, float* c0) {
    info[0] = p->bp.ok; info[1] = p->bp.S; info[2] = p->bp.SP; info[3] = p->bp.W;
    info[4] = p->bp.n_extras; info[5] = p->bp.n_dense; info[6] = p->bp.max_window;
    for (int k = 0; k < 4; ++k) { info[7 + k] = p->bp.extras[k]; info[11 + k] = p->bp.dense_rows[k]; }
    info[15] = p->L.S4 | (p->bp.pair_ok ? 0x10000 : 0) | (p->bp.floor_ok ? 0x20000 : 0) | (p->bp.step_ok ? 0x40000 : 0) |
               ((p->bp.step_ok ? p->bp.step_kb : 0) << 20) | ((p->bp.step_ok ? p->bp.step_bw : 0) << 24);
    *c0 = p->bp.c0;
}
// offsets[0..11]: logpi, A4, lo, kind, tabA, extraA, denseA, total bytes, Arow, rowc, lo2, tabP
void vph_offsets(const vph_plan* p, long long* off) {
    off[0] = p->L.off_logpi; off[1] = p->L.off_A4; off[2] = p->L.off_lo; off[3] = p->L.off_kind;
    off[4] = p->L.off_tabA; off[5] = p->L.off_extraA; off[6] = p->L.off_denseA; off[7] = p->L.bytes;
    off[8] = p->L.off_Arow; off[9] = p->L.off_rowc; off[10] = p->L.off_lo2; off[11] = p->L.off_tabP;
}
// wave form: w[0..5] = wave_ok, npl, proven half-width, instantiated half-width, floor_all_ok, offset of tabV
void vph_wave(const vph_plan* p, long long* w) {
    w[0] = p->bp.wave_ok; w[1] = p->bp.wave_npl; w[2] = p->bp.wave_d; w[3] = p->bp.wave_dk;
    w[4] = p->bp.floor_all_ok; w[5] = (long long)p->L.off_tabV;
}
// step structure: s[0..3] = step_ok, band width, near bands, offset of the band table stepC [kMaxStepBands + 1][SP]; *cn = the
// unvoiced source's one value
void vph_step(const vph_plan* p, long long* s, float* cn) {
    s[0] = p->bp.step_ok; s[1] = p->bp.step_ok ? p->bp.step_bw : 0; s[2] = p->bp.step_ok ? p->bp.step_kb : 0;
    s[3] = (long long)p->L.off_stepC;
    *cn = p->bp.step_ok ? p->bp.step_cn : 0.f;
}
// live window width of targets [0, n_rows) under the floor-max form (vit::floor_live_width): what the split kernel's full waves evaluate
int vph_live_width(const vph_plan* p, int n_rows) { return vit::floor_live_width(p->bp, n_rows); }
// ... and the width the kernel then runs them at for fp32 (f16 = 0) or fp16 emissions: the launcher's own choice (vit::split_full_width)
int vph_split_full_width(const vph_plan* p, int f16) {
    return vit::split_full_width(vit::floor_live_width(p->bp, vit::kSplitFullRows), p->bp.W, p->bp.S, p->bp.ok ? p->bp.n_extras : 0, f16 != 0);
}
// The split kernel's frame loop for a song of Tb frames at prefetch depth pf (pf = 0: the depth it is instantiated with), replayed with
// the kernel's own predicates (vit::split_round_interior / split_round_full / split_prefetch_row): the interior rounds, the remaining
// full rounds, the tail.  Per frame, in loop order: its index, the emission row it requests and its round's class (2 interior round,
// 1 clamped full round, 0 tail).  Returns the number of frames, or -1 when they exceed cap or pf is no whole number of buffer rounds.
int vph_split_rounds(int Tb, int pf, int* frame, int* row, int* cls, int cap) {
    const int PF = pf > 0 ? pf : vit::kSplitPrefetch;
    if (Tb < 1 || PF % 2 != 0) return -1;
    int n = 0;
    auto emit = [&](int t, int u, int c) {
        if (n < cap) { frame[n] = t + u; row[n] = vit::split_prefetch_row(t, u, PF, Tb, c == 2); cls[n] = c; }
        ++n;
    };
    int t = 1;
    for (; vit::split_round_interior(t, PF, Tb); t += PF)
        for (int u = 0; u < PF; ++u) emit(t, u, 2);
    for (; vit::split_round_full(t, PF, Tb); t += PF)
        for (int u = 0; u < PF; ++u) emit(t, u, 1);
    for (int u = 0; u < PF - 1; ++u)
        if (t + u < Tb) emit(t, u, 0);
    return n <= cap ? n : -1;
}
int vph_split_prefetch(void) { return vit::kSplitPrefetch; }
// The copy write of lane `lane` of full wave `wave` (0 .. 3) into copy c of buffer b at win_shift sh, in both forms: out[0] = the
// ds_write_addtid_b32 base (M0, from the start of the LDS segment), out[1] = its immediate, out[2] = the float position the ds_write_b32
// form writes (wp[b * BUF + floor_copy_off(DC, c)], wp = dls + 4 + sh + j).  Returns 0, or -1 for an argument out of range.
int vph_split_addtid(int sh, int wave, int lane, int b, int c, int* out) {
    if (sh < 0 || sh > 3 || wave < 0 || wave >= vit::kSplitFullRows / 64 || lane < 0 || lane > 63 || b < 0 || b > 1 || c < 0 || c > 3) return -1;
    out[0] = vit::split_addtid_base(sh, wave);
    out[1] = vit::split_addtid_imm(b, c);
    out[2] = vit::split_copy_pos(sh, 64 * wave + lane, b, c);
    return 0;
}
// Extra LDS cycles per instruction kind of wave `wave` in a frame that reads buffer rb (vit::split_lds_conflicts; out[6]).  assignment:
// which copies the two lanes of a half-wave target write, first and second store -- 0 lower (0, 1) upper (2, 3), the kernel's;
// 1 lower (2, 3) upper (0, 1); 2 lower (0, 2) upper (1, 3); 3 lower (1, 3) upper (0, 2).  Returns -1 for arguments outside the split kernel.
int vph_split_lds_conflicts(int S, int off, int WF, int wave, int rb, int atomics_serialise, int assignment, int* out) {
    if (S <= vit::kSplitFullRows || S >= vit::kSplitStates || off < 0 || off > 31 || (WF != 25 && WF != 29 && WF != 32) || wave < 0 ||
        wave >= vit::kSplitFullWaves + vit::kSplitHalfWaves || rb < 0 || rb > 1 || assignment < 0 || assignment > 3)
        return -1;
    static const int pairs[4][2][2] = {{{0, 1}, {2, 3}}, {{2, 3}, {0, 1}}, {{0, 2}, {1, 3}}, {{1, 3}, {0, 2}}};
    vit::split_lds_conflicts(S, off, WF, wave, rb, atomics_serialise != 0, [&](int half, int k) { return pairs[assignment][half][k]; },
                             [](int lane, bool is_x) { return vit::split_fm_slot(lane, is_x); }, out);
    return 0;
}
// where the kernel's maps put things, for the host tests: out[0] target slot of (wave, lane), out[1] window half, out[2] frame-maximum
// slot of the lane when its target is not / out[3] is the extra column, out[4 + k] float position of the lane's k-th copy write into buffer b
// (4 for a full wave, 2 for a half wave; the rest -1), out[8] float position of the lane's first window entry in buffer b
int vph_split_maps(int S, int off, int wave, int lane, int b, int* out) {
    if (S <= vit::kSplitFullRows || S >= vit::kSplitStates || off < 0 || off > 31 || wave < 0 || wave >= 8 || lane < 0 || lane > 63 || b < 0 || b > 1) return -1;
    const bool hw = wave >= vit::kSplitFullWaves;
    const int sh = off % 4, j = vit::split_lane_target(wave, lane), hh = hw ? vit::split_half_of(lane) : 0;
    out[0] = j; out[1] = hh; out[2] = vit::split_fm_slot(lane, false); out[3] = vit::split_fm_slot(lane, true);
    for (int k = 0; k < 4; ++k) {
        out[4 + k] = -1;
        if (!hw) out[4 + k] = vit::split_copy_pos(sh, j, b, k);
        else if (k < 2) out[4 + k] = 4 + sh + j + hh * vit::split_upper_off(vit::kSplitCopyStride) + b * 4 * vit::kSplitCopyStride + vit::floor_copy_off(vit::kSplitCopyStride, k);
    }
    out[8] = vit::split_window_pos(S, off, sh, wave, lane, b);
    return 0;
}
void vph_image(const vph_plan* p, unsigned char* out) { std::memcpy(out, p->image.data(), p->image.size()); }

// Launch schedule of the packed checkpointed decode (vit::packed_ckpt_schedule), for the CPU tests.  Returns the number of launches,
// or -1 for bad offsets / more than cap_units units / more than cap_launches launches.  unit_song / unit_seg: [cap_units], units in
// launch order; launch_begin: [cap_launches + 1]; ckpt_base: [B + 1].
long long vph_packed_ckpt_schedule(const long long* offsets, long long B, long long K, long long max_units, int* unit_song, int* unit_seg,
                                   long long cap_units, long long* launch_begin, long long cap_launches, long long* ckpt_base) {
    std::vector<int64_t> off(offsets, offsets + B + 1);
    const int64_t units = vit::packed_ckpt_units(off.data(), B, K);
    if (units < 0 || units > cap_units) return -1;
    vit::PackedCkptSchedule sc;
    vit::packed_ckpt_schedule(off.data(), B, K, max_units, sc);
    const long long nl = (long long)sc.launch_begin.size() - 1;
    if (nl > cap_launches) return -1;
    for (size_t u = 0; u < sc.unit_song.size(); ++u) { unit_song[u] = sc.unit_song[u]; unit_seg[u] = sc.unit_seg[u]; }
    for (size_t l = 0; l < sc.launch_begin.size(); ++l) launch_begin[l] = sc.launch_begin[l];
    for (size_t b = 0; b < sc.ckpt_base.size(); ++b) ckpt_base[b] = sc.ckpt_base[b];
    return nl;
}

// Chunk table of a packed back-trace (vit::packed_chunk_table), for the CPU tests: 1 and *largest, or 0 when `capacity` is exceeded.
int vph_packed_chunk_table(const long long* offsets, long long B, long long streams, long long max_chunks, long long min_frames, int round_nearest,
                           long long capacity, int* chunk_base, int* wave_song, long long* largest) {
    std::vector<int64_t> off(offsets, offsets + B + 1);
    int64_t big = 0;
    const bool ok = vit::packed_chunk_table(off.data(), B, streams, max_chunks, min_frames, round_nearest != 0, capacity, chunk_base, wave_song, &big);
    *largest = big;
    return ok ? 1 : 0;
}

}  // extern "C"
