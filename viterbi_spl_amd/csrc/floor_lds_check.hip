// floor_lds_check.hip -- host replay of the LDS offset arithmetic of the floor forward kernels (FloorLds, banded_floor.inc), for
// every (W, NWT) the launchers can instantiate, every variant, the split kernel's lane map, every win_shift and every window start
// the plan can hand out.  A stand-alone program (tests/test_floor_lds_layout_host.py builds it for the host only, with the address
// and undefined-behaviour sanitizers, and runs it; no GPU):
//   * the four shifted delta copies of a buffer, the two buffers, the slot groups and the tail of the segment do not overlap;
//   * every lane's window read is 16-byte aligned and stays inside the copy it reads, and reads the delta values it means to;
//   * every lane's four (split kernel, half waves: two) copy writes land inside their copies;
//   * the half waves' lane map (split_half_of, split_half_target): partner lanes l and l ^ 8, 32 targets in ascending lane order, and
//     the LDS cycles of a half wave's four ds_read_b128 under the hardware's lane groups, against the map with the halves 32 lanes apart;
//   * the split kernel's frame-maximum slots with the extra column in M's quad (split_fm_slot);
//   * the conflict cycles of every LDS instruction of a split-kernel frame per role (split_lds_conflicts, plan.hpp), for the present copy
//     assignment of the half waves and the three alternatives: counted and printed, and none may beat the present one;
//   * which pairs of copy writes one ds_write2_b32 / ds_write2st64_b32 could encode (two 8-bit offsets in units of 1 / 64 dwords
//     from one address): printed per layout, and checked against the argument in DESIGN.md 7 for why none exists from NP = 256 on.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "device_common.hpp"

namespace vit {
#include "banded_floor.inc"
}
using namespace vit;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++failures <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                    \
    } while (0)

// one ds_write2_b32 reaches dword offsets o0, o1 <= 255 from the lane's address, one ds_write2st64_b32 offsets 64 * o, o <= 255
static bool write2_encodable(int stride) { return stride >= 0 && stride <= 255; }
static bool write2st64_encodable(int stride) { return stride >= 0 && stride % 64 == 0 && stride / 64 <= 255; }

// owner[] of every float of the segment: -1 free, else a tag; claims must not collide
struct Segment {
    std::vector<int> owner;
    explicit Segment(int n) : owner((size_t)n, -1) {}
    void claim(int pos, int tag, const char* what, int W, int NWT) {
        CHECK(pos >= 0 && pos < (int)owner.size(), "%s at %d outside the segment of %zu floats (W %d, NWT %d)", what, pos, owner.size(), W, NWT);
        if (pos < 0 || pos >= (int)owner.size()) return;
        CHECK(owner[(size_t)pos] == -1 || owner[(size_t)pos] == tag, "%s at %d: tag %d collides with %d (W %d, NWT %d)", what, pos, tag, owner[(size_t)pos], W, NWT);
        owner[(size_t)pos] = tag;
    }
};

// L: the layout; split: the split kernel's half waves read W / 2 sources per lane, the upper half 16 floats further on
template <typename L, int W>
static void replay(const char* name, int NWT, bool split) {
    constexpr int NP = L::NP, DC = L::DC, BUF = L::BUF;
    static_assert(DC % 4 == 0, "a copy starts on a 16-byte boundary");
    CHECK(L::fmg == 2 * BUF && L::reset == L::fmg + kFmGroups * kFmGroupFloats && L::end >= L::awl, "%s: carving order", name);
    for (int sh = 0; sh < 4; ++sh) {
        Segment seg(L::end);
        // ---- writes: delta[j] of buffer b goes to copy c at 4 + sh + j - c (kernel: wp[b * BUF + c * DC - c], wp = dls + 4 + sh + j)
        for (int b = 0; b < 2; ++b)
            for (int c = 0; c < 4; ++c)
                for (int j = 0; j < NP; ++j) {
                    const int pos = L::dls + 4 + sh + j + b * BUF + floor_copy_off(DC, c);
                    CHECK(pos >= L::dls + b * BUF + c * DC && pos < L::dls + b * BUF + (c + 1) * DC, "%s: write of delta[%d] leaves copy %d (sh %d)", name, j, c, sh);
                    seg.claim(pos, 16 * b + c, "delta copy", W, NWT);
                }
        for (int g = 0; g < kFmGroups; ++g)
            for (int l = 0; l < kFmGroupFloats; ++l) seg.claim(L::fmg + g * kFmGroupFloats + l, 64 + g, "slot group", W, NWT);
        for (int k = L::tot; k < L::end; ++k) seg.claim(k, 128, "terminal scratch / LDS-resident weights", W, NWT);
        // ---- reads: S < NP states (the idle slot S), lo in [0, max(0, S - W)] (plan.cpp), lov = lo + sh, copy r = lov & 3
        for (int S = 1; S < NP; ++S) {
            const int lo_max = S - W > 0 ? S - W : 0;
            for (int lo = 0; lo <= lo_max; ++lo) {
                const int lov = lo + sh, r = lov & 3;
                for (int hh = 0; hh < (split ? 2 : 1); ++hh) {
                    const int WL = split ? W / 2 : W;                     // window sources per lane
                    const int rp = L::dls + 4 + r * DC + (lov & ~3) + (split ? 16 * hh : 0);
                    for (int b = 0; b < 2; ++b) {
                        const int first = rp + b * BUF, last = first + WL - 1;
                        CHECK(first % 4 == 0, "%s: window read at %d not 16-byte aligned (lo %d, sh %d)", name, first, lo, sh);
                        CHECK(first >= L::dls + b * BUF + r * DC && last < L::dls + b * BUF + (r + 1) * DC,
                              "%s: window [%d, %d] leaves copy %d of buffer %d (S %d, lo %d, sh %d)", name, first, last, r, b, S, lo, sh);
                        // the float at `first + w` is delta[lo + 16 hh + w] of copy r: position 4 + sh + i - r of that copy
                        const int i0 = first - (L::dls + b * BUF + r * DC) - 4 - sh + r;
                        CHECK(i0 == lo + (split ? 16 * hh : 0), "%s: window starts at delta[%d], not delta[%d] (sh %d)", name, i0, lo + 16 * hh, sh);
                    }
                }
            }
        }
    }
    // ---- the split kernel's writers: a lower lane writes copies 0 and 1, an upper lane copies 2 and 3, through the kernel's own offset
    // helpers; each write must land where a reader of that copy looks for delta[j] (copy r holds delta[i] at r * DC + 4 + sh + i - r:
    // the window-start check above)
    if (split) {
        for (int sh = 0; sh < 4; ++sh)
            for (int wv = kSplitFullWaves; wv < kSplitFullWaves + kSplitHalfWaves; ++wv)
                for (int lane = 0; lane < 64; ++lane) {
                    const int hh = split_half_of(lane), j = 64 * kSplitFullWaves + 32 * (wv - kSplitFullWaves) + split_half_target(lane);
                    CHECK(j >= 64 * kSplitFullWaves && j < kSplitStates, "split target %d", j);
                    const int wp = L::dls + 4 + sh + j + hh * split_upper_off(DC);
                    for (int c = 0; c < 2; ++c) {
                        const int r = 2 * hh + c, pos = wp + floor_copy_off(DC, c);
                        CHECK(pos == L::dls + r * DC + 4 + sh + j - r, "split lane %d of wave %d: copy %d written at %d (sh %d)", lane, wv, r, pos, sh);
                    }
                }
    }
    // ---- the split kernel's full waves store by ds_write_addtid_b32: byte address = base (M0) + immediate + 4 * lane, from the start
    // of the segment (plan.hpp).  For every wave, lane, buffer, copy and shift that must be the byte address of the float the
    // ds_write_b32 form writes (the position claimed above, wp = dls + 4 + sh + j with j = 64 wave + lane), and base and immediate
    // must each fit the instruction's 16-bit field -- as must their sum with the lane term, the address the LDS sees.
    if (split) {
        static_assert(!std::is_same_v<L, FloorSplitLds> || (kSplitCopyStride == DC && L::dls == 0 && BUF == 4 * DC), "plan.hpp's address rule speaks of this layout");
        CHECK((std::is_same_v<L, FloorSplitLds>), "%s: the split kernel runs in FloorSplitLds", name);
        for (int sh = 0; sh < 4; ++sh)
            for (int wv = 0; wv < kSplitFullWaves; ++wv)
                for (int b = 0; b < 2; ++b)
                    for (int c = 0; c < 4; ++c) {
                        const int base = split_addtid_base(sh, wv), imm = split_addtid_imm(b, c);
                        CHECK(base >= 0 && base < 65536 && imm >= 0 && imm < 65536, "add-tid base %d / immediate %d outside 16 bits", base, imm);
                        for (int lane = 0; lane < 64; ++lane) {
                            const int j = 64 * wv + lane, pos = L::dls + 4 + sh + j + b * BUF + floor_copy_off(DC, c);
                            CHECK(pos == split_copy_pos(sh, j, b, c), "split_copy_pos(%d, %d, %d, %d) = %d, the kernel's offsets give %d", sh, j, b, c, split_copy_pos(sh, j, b, c), pos);
                            CHECK(base + imm + 4 * lane == 4 * pos, "add-tid store of wave %d lane %d, buffer %d copy %d, sh %d: byte %d, not %d", wv, lane, b, c, sh, base + imm + 4 * lane, 4 * pos);
                            CHECK(base + imm + 4 * lane + 4 <= 65536 && 4 * pos + 4 <= (int)L::bytes(), "add-tid store at byte %d leaves the segment", base + imm + 4 * lane);
                        }
                    }
        std::printf("split full waves: ds_write_addtid_b32 base + immediate + 4 * lane is the ds_write_b32 address for every wave, lane, buffer, copy and shift: ok\n");
    }
    // ---- paired writes.  The lane's four writes are `stride` = DC - 1 dwords apart.  The copies must sit at four different residues
    // mod 4 (each lane reads the one that aligns its window), so the distance between any two copies is not a multiple of 4, let alone
    // of 64: the st64 form can never pair two copies; the plain form needs a whole copy (> NP floats) within 255 dwords.
    const int stride = DC - 1;
    bool residues[4] = {false, false, false, false};
    for (int c = 0; c < 4; ++c) residues[(c * stride) & 3] = true;
    CHECK(residues[0] && residues[1] && residues[2] && residues[3], "%s: the four copies must cover the four alignments", name);
    bool any64 = false;
    for (int c0 = 0; c0 < 4; ++c0)
        for (int c1 = c0 + 1; c1 < 4; ++c1) any64 |= write2st64_encodable((c1 - c0) * stride);
    CHECK(!any64, "%s: an st64 pair would mean two copies with the same alignment", name);
    const bool plain = write2_encodable(stride);
    CHECK(plain == (NP + 15 <= 255), "%s: plain pair iff a copy fits 255 dwords", name);
    std::printf("%-28s NP %4d DC %4d bytes %6zu  copy stride %4d dwords: ds_write2_b32 %s, ds_write2st64_b32 no\n", name, NP, DC, L::bytes(),
                stride, plain ? "pairs (0,1) and (2,3)" : "no");
}

// ---- the half waves' lane map
// the map this one replaced: lane l and lane l + 32 share target l & 31
static int old_half_of(int lane) { return lane >> 5; }
static int old_half_target(int lane) { return lane & 31; }
static void replay_lane_map() {
    int next = 0;                                                         // lower lanes, in lane order, take targets 0, 1, 2, ...
    for (int lane = 0; lane < 64; ++lane) {
        const int hh = split_half_of(lane), k = split_half_target(lane), p = lane ^ 8;
        CHECK(hh == 0 || hh == 1, "lane %d: half %d", lane, hh);
        CHECK(k >= 0 && k < 32, "lane %d: target %d", lane, k);
        CHECK(split_half_target(p) == k && split_half_of(p) == 1 - hh, "lane %d: partner %d holds target %d half %d", lane, p, split_half_target(p), split_half_of(p));
        CHECK((lane >> 4) == (p >> 4), "lane %d: partner %d in another DPP row", lane, p);
        CHECK((k & 3) == (lane & 3), "lane %d: target %d sits elsewhere in its quad", lane, k);
        if (hh == 0) { CHECK(k == next, "lower lane %d takes target %d, not %d", lane, k, next); ++next; }
    }
    CHECK(next == 32, "%d lower lanes", next);
    std::printf("split lane map: partner l ^ 8 (row_ror:8), 32 lower lanes in ascending target order: ok\n");
}

// LDS cycles of one ds_read_b128 of a wave: the hardware serves it in four groups of sixteen lanes; a group takes one cycle, and one more
// for every further distinct address on its busiest bank (64 banks of 4 bytes, a lane covers four of them).
static int read_b128_cycles(const int* addr /* float positions, 64 lanes */) {
    static const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    int cycles = 0;
    for (int g = 0; g < 4; ++g) {
        int worst = 1;
        for (int bank = 0; bank < 64; bank += 4) {                        // aligned 16-byte reads: whole 4-bank groups
            int seen[16], n = 0;
            for (int i = 0; i < 16; ++i) {
                const int a = addr[groups[g][i]];
                if (a % 64 != bank) continue;
                bool dup = false;
                for (int q = 0; q < n; ++q) dup |= seen[q] == a;
                if (!dup) seen[n++] = a;
            }
            if (n > worst) worst = n;
        }
        cycles += worst;
    }
    return cycles;
}
// The four window reads of half wave hw at S states, window starts lo_j = clamp(j - off, 0, S - W) (the affine plans; idle targets
// read the last window, S - W, as the kernel has them do)
template <typename HF, typename TF>
static int half_wave_read_cycles(int S, int off, int sh, int hw, HF half_of, TF target_of) {
    using L = FloorSplitLds;
    constexpr int W = 32;
    int cycles = 0;
    for (int q = 0; q < W / 2 / 4; ++q) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int j = 64 * kSplitFullWaves + 32 * hw + target_of(lane);
            int lo = j - off;
            lo = lo < 0 ? 0 : (lo > S - W ? S - W : lo);
            const int lov = (j < S ? lo : S - W) + sh;
            addr[lane] = L::dls + 4 + (lov & 3) * L::DC + (lov & ~3) + 16 * half_of(lane) + 4 * q;
        }
        cycles += read_b128_cycles(addr);
    }
    return cycles;
}
static void replay_read_cycles(int S, int off) {
    for (int sh = 0; sh < 4; ++sh) {
        int was[kSplitHalfWaves], now[kSplitHalfWaves];
        for (int hw = 0; hw < kSplitHalfWaves; ++hw) {
            was[hw] = half_wave_read_cycles(S, off, sh, hw, old_half_of, old_half_target);
            now[hw] = half_wave_read_cycles(S, off, sh, hw, split_half_of, split_half_target);
            // (only the plan's own shift, off mod 4, ever runs: the others are printed for the record)
            if (sh == off % 4) CHECK(now[hw] <= was[hw], "S %d sh %d half wave %d: %d LDS cycles for its window reads, %d with the halves 32 lanes apart", S, sh, hw, now[hw], was[hw]);
        }
        std::printf("split window reads S %d off %d sh %d%s: ds_read_b128 cycles per half wave, halves 32 lanes apart %d / %d / %d / %d, partner l ^ 8 %d / %d / %d / %d\n",
                    S, off, sh, sh == off % 4 ? " (the plan's)" : "", was[0], was[1], was[2], was[3], now[0], now[1], now[2], now[3]);
    }
}

// ---- frame-maximum slots of the split kernel with the extra column in M's quad: one extra column x = S - 1, x % 4 == 0 (the launcher's test)
static void replay_slot_map() {
    int cases = 0;
    for (int S = 64 * kSplitFullWaves + 1; S < kSplitStates; S += 4) {
        const int x = S - 1;
        CHECK(x % 4 == 0, "x %d", x);
        bool x_reached = false;
        for (int wv = 0; wv < kSplitFullWaves + kSplitHalfWaves; ++wv) {
            bool quad_in_m[16] = {};
            for (int lane = 0; lane < 64; ++lane) {
                const bool half = wv >= kSplitFullWaves;
                const int j = half ? 64 * kSplitFullWaves + 32 * (wv - kSplitFullWaves) + split_half_target(lane) : 64 * wv + lane;
                const int slot = split_fm_slot(lane, j == x);
                CHECK(slot >= 0 && slot < 16, "slot %d", slot);
                // the quad of this lane holds x after the quad maximum iff one of its lanes is x's
                bool quad_has_x = false;
                for (int m = 0; m < 4; ++m) {
                    const int lm = (lane & ~3) | m;
                    const int jm = half ? 64 * kSplitFullWaves + 32 * (wv - kSplitFullWaves) + split_half_target(lm) : 64 * wv + lm;
                    quad_has_x |= jm == x;
                    if (quad_has_x && jm != x) CHECK(jm >= S, "S %d: state %d shares a quad with x and is live", S, jm);
                }
                if (slot < kSplitXSlot) {
                    CHECK(!quad_has_x, "S %d wave %d lane %d: a quad that holds x adds into M slot %d", S, wv, lane, slot);
                    quad_in_m[lane >> 2] = true;
                }
                if (slot == kSplitXSlot) {
                    CHECK(j == x, "S %d wave %d lane %d (state %d) adds into the extra column's slot", S, wv, lane, j);
                    x_reached = true;
                }
            }
            for (int q = 0; q < 16; ++q) {
                bool has_x = false;
                for (int m = 0; m < 4; ++m) {
                    const int lm = 4 * q + m;
                    has_x |= (wv >= kSplitFullWaves ? 64 * kSplitFullWaves + 32 * (wv - kSplitFullWaves) + split_half_target(lm) : 64 * wv + lm) == x;
                }
                CHECK(quad_in_m[q] != has_x, "S %d wave %d quad %d: %s", S, wv, q, has_x ? "holds x and reaches M" : "reaches none of slots 0 .. 2");
            }
        }
        CHECK(x_reached, "S %d: no lane adds x into slot %d", S, kSplitXSlot);
        ++cases;
    }
    std::printf("split slot map: every quad without x reaches one of slots 0 .. 2, x reaches slot %d alone: ok (%d state counts)\n", kSplitXSlot, cases);
}

// ---- LDS conflict cycles of a frame of the split kernel, per instruction kind and role (split_lds_conflicts, plan.hpp): the present
// copy assignment of the half waves against the three others a lane pair can take without another instruction (the two stores of a
// lane share one address register, so its copies lie one fixed distance apart: (0, 1) / (2, 3) or (0, 2) / (1, 3), either way round),
// and the slot map with same-address lanes of the ds_max_f32 counted once (they combine) or one by one (they serialise).
static void replay_conflicts(int S, int off, int WF) {
    static const int pairs[4][2][2] = {{{0, 1}, {2, 3}}, {{2, 3}, {0, 1}}, {{0, 2}, {1, 3}}, {{1, 3}, {0, 2}}};
    static const char* kind[6] = {"slot quad read", "window b128", "window b32", "copy writes", "ds_max_f32", "slot reset"};
    const auto slot = [](int lane, bool is_x) { return split_fm_slot(lane, is_x); };
    int frame_total[4][2] = {};
    for (int as = 0; as < 4; ++as)
        for (int ser = 0; ser < 2; ++ser)
            for (int rb = 0; rb < 2; ++rb)
                for (int wv = 0; wv < kSplitFullWaves + kSplitHalfWaves; ++wv) {
                    int c[6];
                    split_lds_conflicts(S, off, WF, wv, rb, ser != 0, [&](int half, int k) { return pairs[as][half][k]; }, slot, c);
                    for (int k = 0; k < 6; ++k) frame_total[as][ser] += c[k];
                    if (as == 0 && ser == 1 && (rb == 0 || wv == 0))
                        std::printf("split conflicts S %d WF %d buffer %d wave %d (%s):", S, WF, rb, wv, wv < kSplitFullWaves ? "full" : wv == 7 ? "half, resets" : "half");
                    if (as == 0 && ser == 1 && (rb == 0 || wv == 0)) {
                        for (int k = 0; k < 6; ++k) std::printf(" %s %d", kind[k], c[k]);
                        std::printf("\n");
                    }
                    CHECK(c[0] == 0 && c[5] == 0, "S %d wave %d: the broadcast slot read and the linear reset must be conflict-free", S, wv);
                    if (wv < kSplitFullWaves) CHECK(c[3] == 0, "S %d wave %d: the add-tid stores are linear in the lane", S, wv);
                }
    for (int as = 0; as < 4; ++as) {
        // per wave-frame: two buffers, eight waves
        std::printf("split conflicts S %d WF %d, half-wave copies lower (%d, %d) upper (%d, %d)%s: %.3f extra LDS cycles per wave-frame, %.3f with the ds_max_f32 lanes of one address serialised\n",
                    S, WF, pairs[as][0][0], pairs[as][0][1], pairs[as][1][0], pairs[as][1][1], as == 0 ? " (the kernel's)" : "", frame_total[as][0] / 16.0, frame_total[as][1] / 16.0);
        CHECK(frame_total[as][0] >= frame_total[0][0] && frame_total[as][1] >= frame_total[0][1], "S %d: copy assignment %d has fewer conflict cycles than the kernel's", S, as);
    }
}

template <int W, int NWT>
static void replay_pair() {
    char name[64];
    std::snprintf(name, sizeof name, "FloorLds<%d, %d>", W, NWT);
    replay<FloorLds<W, NWT, WgVariant::Plain>, W>(name, NWT, false);
    if constexpr (W == 128 && NWT > 8) {   // the variants differ in the LDS-resident weights only
        std::snprintf(name, sizeof name, "FloorLds<%d, %d, Packed>", W, NWT);
        replay<FloorLds<W, NWT, WgVariant::Packed>, W>(name, NWT, false);
    }
}
template <int W>
static void replay_width() {
    replay_pair<W, 2>();
    replay_pair<W, 4>();
    replay_pair<W, 6>();
    replay_pair<W, 8>();
    replay_pair<W, 12>();
}

int main() {
    static_assert(sizeof(kBandedWidths) / sizeof(int) == 6, "one call per instantiated window width");
    replay_width<16>();
    replay_width<32>();
    replay_width<64>();
    replay_width<84>();
    replay_width<96>();
    replay_width<128>();
    replay<FloorSplitLds, 32>("FloorSplitLds (split kernel)", kSplitStates / 64, true);
    replay_lane_map();
    replay_slot_map();
    replay_read_cycles(361, 15);                                          // the reference's 361-state grid: rows 344 .. 359 are clamped to S - W
    replay_read_cycles(321, 13);
    replay_conflicts(361, 15, 29);                                        // the two trimmed grids and the whole window
    replay_conflicts(321, 13, 25);
    replay_conflicts(361, 15, 32);
    // two workgroups per CU up to B = 512 at the production shape
    static_assert(2 * FloorSplitLds::bytes() <= kLdsBytes && 2 * FloorLds<32, 6>::bytes() <= kLdsBytes, "two workgroups share a CU's LDS");
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("floor LDS layouts: all checks passed\n");
    return 0;
}
