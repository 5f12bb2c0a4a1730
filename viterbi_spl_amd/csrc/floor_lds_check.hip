// floor_lds_check.hip -- host replay of the LDS offset arithmetic of the floor forward kernels (FloorLds, banded_floor.inc), for
// every (W, NWT) the launchers can instantiate, every variant, the split kernel's lane map, every win_shift and every window start
// the plan can hand out.  A stand-alone program (tests/test_floor_lds_layout_host.py builds it for the host only, with the address
// and undefined-behaviour sanitizers, and runs it; no GPU):
//   * the four shifted delta copies of a buffer, the two buffers, the slot groups and the tail of the segment do not overlap;
//   * every lane's window read is 16-byte aligned and stays inside the copy it reads, and reads the delta values it means to;
//   * every lane's four (split kernel, half waves: two) copy writes land inside their copies;
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
                    const int hh = lane >> 5, j = 64 * kSplitFullWaves + 32 * (wv - kSplitFullWaves) + (lane & 31);
                    CHECK(j >= 64 * kSplitFullWaves && j < kSplitStates, "split target %d", j);
                    const int wp = L::dls + 4 + sh + j + hh * split_upper_off(DC);
                    for (int c = 0; c < 2; ++c) {
                        const int r = 2 * hh + c, pos = wp + floor_copy_off(DC, c);
                        CHECK(pos == L::dls + r * DC + 4 + sh + j - r, "split lane %d of wave %d: copy %d written at %d (sh %d)", lane, wv, r, pos, sh);
                    }
                }
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
    // two workgroups per CU up to B = 512 at the production shape
    static_assert(2 * FloorSplitLds::bytes() <= kLdsBytes && 2 * FloorLds<32, 6>::bytes() <= kLdsBytes, "two workgroups share a CU's LDS");
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("floor LDS layouts: all checks passed\n");
    return 0;
}
