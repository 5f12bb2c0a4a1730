// banded.hip -- banded forward kernels (plan.ok): the scan form, the floor-max form and its two-targets-per-lane variant,
// and the DPP self-test of the wave primitives they are built from.
#include "device_common.hpp"

namespace vit {

// ---------------------------------------------------------------------------------------
// Banded forward kernel: one song per workgroup, value-only.
//
// For a banded target j (window [lo_j, lo_j+W), row constant c_j, extra columns X):
//   m_j = max( max_w fl(delta_{lo_j+w} + logA_T[j][lo_j+w]),   W register-resident window entries
//              fl( max(Pv[lo_j], Sv[lo_j+W]) + c_j ),          Pv/Sv: prefix / suffix max of the RAW delta
//              fl(delta_x + logA_T[j][x]), x in X )             (extra columns are excluded from the scans)
// Rounding is monotone, so max_i fl(delta_i + c_j) = fl(max_i delta_i + c_j): the value equals the max
// of the fl32 sums the dense recursion forms, and delta is bit-identical.  Dense rows (none for the
// reference's matrices) are a full max over all sources.
//
// Wave roles (NWT target waves, 64*NWT >= S):
//   waves 0..NWT-1  one thread per target: window max, merge, delta_t, history row
//   wave  NWT       prefix-max scan over all sources (NWT per lane)
//   wave  NWT+1     suffix-max scan (lanes hold the sources in descending blocks)
//   wave  NWT+2     dense rows
// A SIMD retires one wave64 VALU instruction per 4 cycles, shared by the waves resident on it, so
// the frame time is set by the VALU instruction count of the busiest SIMD plus the two barriers.
// Two workgroup barriers per frame; emission rows are fetched two frames ahead.
// ---------------------------------------------------------------------------------------
// DBG = true adds the timing-experiment hooks (ablation mask, cycle stamps); the production instantiation has none.
// NXT >= 0 specialises for exactly NXT extra columns and no dense rows (the reference's matrices: NXT = 1);
// NXT < 0 is the generic form (run-time counts).  Every untaken branch costs an issue slot per frame.
template <int W, int NWT, bool DW, bool DBG, int NXT, typename ET>
__global__ void __launch_bounds__((NWT + (DW ? 3 : 2)) * 64) banded_forward_kernel(FwdArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NP = NWT * 64;
    constexpr int EPL = NWT;
    const int S = a.S, SP = a.SP, T = a.T, SD = a.SD;
    // delta_{t-1} is kept as four copies shifted by 0..3 entries (entry m of copy c = delta[m + c], copy c
    // at dls + c*DC + 4): every lane reads its window with aligned 16-byte LDS reads (256 B/clk instead of
    // the 128 B/clk of 4-/8-byte reads, which bound the window phase) from the copy that makes its window
    // start 16-byte aligned.  Each copy has 4 pad entries in front, so the four writes of a new delta value
    // (entry j - c of copy c) need no bounds test.  Entries >= S stay -inf.
    constexpr int DC = NP + 16;                   // copy stride = 16 banks mod 64: a 16-lane read group covers all 64 banks
    float* dls = reinterpret_cast<float*>(smem);  // [4][DC]
    float* dl = dls + 4;                          // copy 0 (unshifted)
    float* Pv = dls + 4 * DC;                     // [NP+1]  Pv[q] = max_{i<q}  raw delta (extras excluded)
    float* Sv = Pv + NP + 1;                      // [NP+1]  Sv[q] = max_{i>=q} raw delta
    float* Dv = Sv + NP + 1;                      // [4]     dense-row maxima
    VI* tot = reinterpret_cast<VI*>(Dv + kMaxDenseRows);  // [16] terminal argmax scratch (4*DC + 2*NP + 6 floats before: 8-byte aligned)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform for the compiler
    const int song = blockIdx.x;
    const int Tb = song_length(a.lengths, song, T);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (size_t)song * T * S;
    float* __restrict__ hist = a.hist + (size_t)song * T * SD;
    constexpr bool GEN = NXT < 0;
    constexpr int NXL = GEN ? kMaxExtras : NXT;            // extra columns the loops are unrolled for
    const int nx = GEN ? a.n_extras : NXT, nd = GEN ? a.n_dense : 0;
#ifdef VIT_TIMING_HOOKS
    const int dbg = DBG ? a.debug : 0;
#else
    constexpr int dbg = 0;          // the ablation / probe hooks exist only in VIT_TIMING_HOOKS builds (scripts/)
#endif

    // ---------------- per-role setup
    const bool is_target = wv < NWT;
    const int j = tid;
    const bool tvalid = is_target && j < S;
    const int jst = j < S ? j : S + 1;                     // idle lanes store into pad column S+1 of the history row (SD >= S+2 always)
    const int jld = j < S ? j : S - 1;
    const int jc = j < SP ? j : 0;
    int lo = 0, kind = -2;
    float cj = 0.f;
    float aw[W];
    float xa[kMaxExtras];
    int xcol[kMaxExtras];
#pragma unroll
    for (int k = 0; k < kMaxExtras; ++k) { xa[k] = -INFINITY; xcol[k] = a.extras[k]; }
#pragma unroll
    for (int w = 0; w < W; ++w) aw[w] = 0.f;
    if (is_target) {
        cj = reinterpret_cast<const float*>(a.image + a.off_rowc)[jc];
        lo = reinterpret_cast<const int32_t*>(a.image + a.off_lo)[jc];
        kind = j < SP ? reinterpret_cast<const int32_t*>(a.image + a.off_kind)[jc] : -2;
        const float* __restrict__ tab = reinterpret_cast<const float*>(a.image + a.off_tabA);
        const float* __restrict__ xaT = reinterpret_cast<const float*>(a.image + a.off_extraA);
#pragma unroll
        for (int w = 0; w < W; ++w) aw[w] = tab[(size_t)w * SP + jc];
#pragma unroll
        for (int k = 0; k < kMaxExtras; ++k) xa[k] = xaT[(size_t)k * SP + jc];
    }
    const int role = wv - NWT;                 // 0 prefix, 1 suffix, 2 dense rows (DW) -- else the suffix wave reduces them
    constexpr int kDenseRole = DW ? 2 : 1;
    const int blk = role == 1 ? 63 - lane : lane;
    const int i0 = blk * EPL;
    bool smask[EPL];
    float dA[kMaxDenseRows][EPL];
    {
        const float* __restrict__ daT = reinterpret_cast<const float*>(a.image + a.off_denseA);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int i = i0 + e;
            bool m = i >= S;
#pragma unroll
            for (int k = 0; k < kMaxExtras; ++k) m |= (k < nx && i == xcol[k]);
            smask[e] = m;
#pragma unroll
            for (int d = 0; d < kMaxDenseRows; ++d)
                dA[d][e] = (role == kDenseRole && i < S && d < nd) ? daT[(size_t)d * SP + i] : -INFINITY;
        }
    }

    // ---------------- frame 0
    for (int k = tid; k < 4 * DC; k += blockDim.x) dls[k] = -INFINITY;
    __syncthreads();
    if (is_target) {
        if (tvalid) {
            const float d = reinterpret_cast<const float*>(a.image + a.off_logpi)[j] + load_e<ET>(E + j);
            hist[j] = d;
#pragma unroll
            for (int c = 0; c < 4; ++c) dl[c * DC + j - c] = d;
        }
    } else if (lane == 0) {
        if (role == 0) Pv[0] = -INFINITY;
        if (role == 1) Sv[NP] = -INFINITY;
    }
    // Emission rows are fetched two frames ahead and consumed only at the end of a frame: vmcnt
    // retires in order, so a wait on a younger load would also wait for the previous frame's store.
    float e_a = (tvalid && Tb > 1) ? load_e<ET>(E + S + j) : 0.f;
    float e_b = (tvalid && Tb > 2) ? load_e<ET>(E + 2 * (size_t)S + j) : 0.f;
    // Retire every set-up load here so the frame loop only sees the two memory ops it issues.
#pragma unroll
    for (int w = 0; w < W; ++w) asm volatile("" ::"v"(aw[w]));
#pragma unroll
    for (int k = 0; k < kMaxExtras; ++k) asm volatile("" ::"v"(xa[k]));
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
#pragma unroll
        for (int d = 0; d < kMaxDenseRows; ++d) asm volatile("" ::"v"(dA[d][e]));
    }
    asm volatile("" ::"v"(lo), "v"(kind), "v"(cj), "v"(e_a), "v"(e_b));
    __syncthreads();

    unsigned long long ph0 = 0, ph1 = 0, ph2 = 0, ph3 = 0;   // timing experiments only (dbg & 256)
    auto stamp = [&]() -> unsigned long long {
        unsigned long long v;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");
        return v;
    };
    auto frame = [&](const int t, float& e_slot) {
        float m = -INFINITY;
        const bool prof = (dbg & 256) != 0;
        const unsigned long long s0 = prof ? stamp() : 0ull;
        if (is_target) {
            // ---- window max (reads delta_{t-1}); four independent max3 chains
            float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
            float xd[NXL > 0 ? NXL : 1];
#pragma unroll
            for (int k = 0; k < NXL; ++k) xd[k] = (!GEN || k < nx) ? dl[xcol[k]] : -INFINITY;
            if (!(dbg & 1)) {
                // copy (lo & 3), entry (lo & ~3): delta[lo .. lo+W) as W/4 aligned 16-byte reads
                const f32x4* __restrict__ win = reinterpret_cast<const f32x4*>(dl + (lo & 3) * DC + (lo & ~3));
#pragma unroll
                for (int w = 0; w + 7 < W; w += 8) {
                    const f32x4 da = win[w / 4], db = win[w / 4 + 1];
                    // v_pk_add_f32: two fl32 adds per instruction (each lane still rounds separately)
                    const f32x2 c0_ = f32x2{da.x, da.y} + f32x2{aw[w + 0], aw[w + 1]};
                    const f32x2 c1_ = f32x2{da.z, da.w} + f32x2{aw[w + 2], aw[w + 3]};
                    const f32x2 c2_ = f32x2{db.x, db.y} + f32x2{aw[w + 4], aw[w + 5]};
                    const f32x2 c3_ = f32x2{db.z, db.w} + f32x2{aw[w + 6], aw[w + 7]};
                    m0 = fmaxf(fmaxf(m0, c0_.x), c0_.y);
                    m1 = fmaxf(fmaxf(m1, c1_.x), c1_.y);
                    m2 = fmaxf(fmaxf(m2, c2_.x), c2_.y);
                    m3 = fmaxf(fmaxf(m3, c3_.x), c3_.y);
                }
            }
            // extra columns are consumed after the window so that their LDS read shares the window's wait
#pragma unroll
            for (int k = 0; k < NXL; ++k) m1 = fmaxf(m1, xd[k] + xa[k]);
            m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
        } else if (!(dbg & 2)) {
            float d[EPL];
#pragma unroll
            for (int e = 0; e < EPL; ++e) d[e] = dl[i0 + e];
            if (role == 0) {
                float p[EPL];
                float run = -INFINITY;
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    run = fmaxf(run, smask[e] ? -INFINITY : d[e]);
                    p[e] = run;
                }
                const float inc = wave_scan_max(run);
                const float ex = wave_shift_up(inc, -INFINITY);                 // sources of all lower lanes
#pragma unroll
                for (int e = 0; e < EPL; ++e) Pv[i0 + e + 1] = fmaxf(ex, p[e]);
                // max of delta_{t-1} over the non-extra sources: bounds every row-constant candidate in the back-trace
                if (lane == 63 && !(dbg & 8)) hist[(size_t)(t - 1) * SD + S] = inc;   // pad column S of row t-1
            } else {
                if (role == 1) {
                    float p[EPL];
                    float run = -INFINITY;
#pragma unroll
                    for (int e = EPL - 1; e >= 0; --e) {
                        run = fmaxf(run, smask[e] ? -INFINITY : d[e]);
                        p[e] = run;
                    }
                    const float ex = wave_shift_up(wave_scan_max(run), -INFINITY);  // sources of all higher blocks
#pragma unroll
                    for (int e = 0; e < EPL; ++e) Sv[i0 + e] = fmaxf(ex, p[e]);
                }
                if (GEN && role == kDenseRole) {
#pragma unroll
                    for (int dr = 0; dr < kMaxDenseRows; ++dr) {
                        if (dr < nd) {
                            float dm = -INFINITY;
#pragma unroll
                            for (int e = 0; e < EPL; ++e) dm = fmaxf(dm, d[e] + dA[dr][e]);
                            dm = wave_max_all(dm);
                            if (lane == 0) Dv[dr] = dm;
                        }
                    }
                }
            }
        }
        const unsigned long long s1 = prof ? stamp() : 0ull;
        __syncthreads();
        const unsigned long long s2 = prof ? stamp() : 0ull;

        if (is_target && !(dbg & 4)) {
            m = fmaxf(m, fmaxf(Pv[lo], Sv[lo + W]) + cj);
            if (GEN) {
                const float dres = Dv[kind >= 0 ? kind : 0];
                if (kind >= 0) m = dres;
            }
            {
                // Every target lane stores and prefetches unconditionally (idle lanes: a pad column of the
                // history row / the last valid emission) so that the in-order vmcnt of the next use is exact
                // -- a conditional would make the compiler wait for the previous frame's store as well.
                const float dn = tvalid ? m + e_slot : -INFINITY;
#pragma unroll
                for (int c = 0; c < 4; ++c) dl[c * DC + j - c] = dn;
                if (!(dbg & 8)) {
                    float* __restrict__ hrow = hist + (size_t)t * SD;          // wave-uniform row bases:
                    const int tn = t + 2 < Tb ? t + 2 : Tb - 1;                 // scalar base + lane offset
                    const ET* __restrict__ erow = E + (size_t)tn * S;
                    hrow[jst] = dn;
                    e_slot = load_e<ET>(erow + jld);
                }
            }
        }
        const unsigned long long s3 = prof ? stamp() : 0ull;
        __syncthreads();
        if (prof) {
            const unsigned long long s4 = stamp();
            ph0 += s1 - s0; ph1 += s2 - s1; ph2 += s3 - s2; ph3 += s4 - s3;
        }
    };
    const unsigned long long clk0 = (dbg & 48) ? __builtin_amdgcn_s_memtime() : 0ull;
    const unsigned long long rt0 = (dbg & 48) ? __builtin_amdgcn_s_memrealtime() : 0ull;
    int t = 1;
    for (; t + 1 < Tb; t += 2) {
        frame(t, e_a);
        frame(t + 1, e_b);
    }
    if (t < Tb) frame(t, e_a);

    terminal_argmax(is_target ? dl[j] : -INFINITY, j, tvalid, tot, NWT + (DW ? 3 : 2), a.last_state, a.loglik, song);
    if ((dbg & 256) && lane == 0 && Tb > 1) {   // per-wave phase averages -> fmax[song][4*wave .. 4*wave+3]
        float* o = a.fmax + (size_t)song * 64 + 4 * wv;
        const float n = (float)(Tb - 1);
        o[0] = (float)ph0 / n; o[1] = (float)ph1 / n; o[2] = (float)ph2 / n; o[3] = (float)ph3 / n;
    }
    if ((dbg & 48) && tid == 0) {  // timing experiments only: cycles (16) or 100 MHz ticks (32) per frame -> scratch slot 63
        const unsigned long long d = (dbg & 16) ? __builtin_amdgcn_s_memtime() - clk0 : __builtin_amdgcn_s_memrealtime() - rt0;
        a.fmax[(size_t)song * 64 + 63] = (float)d / (float)(Tb > 1 ? Tb - 1 : 1);
    }
}

// ---------------------------------------------------------------------------------------
// Banded forward kernel, "floor-max" form (plan.floor_ok): one song per workgroup, value-only, ONE barrier
// and no scan waves per frame.
//
// The plan proved that no in-window entry of a banded row is below the row constant c_j.  Let M be the max of
// the RAW delta_{t-1} over all non-extra sources, attained at i*.  If i* is outside the window of target j,
// fl(M + c_j) IS the out-of-window term.  If i* is inside, fl(M + c_j) <= fl(delta_i* + logA_T[j][i*]) (rounding
// is monotone and logA_T[j][i*] >= c_j), which the window max already contains, and every out-of-window term is
// <= fl(M + c_j) -- so in both cases
//   m_j = max( window max, fl(M + c_j), extra-column terms )
// is the value the dense recursion computes, bit for bit.  M is one number per frame, formed by LDS float atomics:
// every lane (after a max over its quad, two DPP steps) sends its new delta value with a no-return ds_max_f32 into one
// of four slots of the frame's slot group, in the same burst as its four delta copy writes; after the frame's only
// barrier every lane reads the four slots back (one ds_read_b128).  Four slot groups rotate: frame t adds into
// group t % 4, reads group (t - 1) % 4 and resets group (t + 1) % 4 to -inf (last read in frame t - 2; frame t + 1 is
// the first to add into it).  Four, not three, so that both emission prefetch depths (PF = 12 and 4) unroll into whole
// rounds.  delta is double-buffered in LDS (four shifted copies each, see banded_forward_kernel), so nothing a wave
// reads in frame t is written before the barrier that ends frame t.  M (= the back-trace's bound on every
// row-constant candidate) is stored in pad column S of the history row.
// ---------------------------------------------------------------------------------------
#include "banded_floor.inc"

// ---------------------------------------------------------------------------------------
// Floor-max banded forward kernel with split windows: eight waves for the grids that take six (256 < S < 384, W = 32).
//
// Six waves on four SIMDs put two waves on SIMD 0 and 1 and one on SIMD 2 and 3, and the frame waits for the full ones.
// Here every SIMD carries one FULL wave (waves 0-3: one target per lane, the whole window, exactly the frame body of
// banded_floor_forward_kernel) and one HALF-WINDOW wave (waves 4-7): the lanes l and l ^ 8 of wave w share target
// 256 + 32 (w - 4) + split_half_target(l); the one with bit 3 clear evaluates its sources 0-15, the other its sources 16-31 (4 reads,
// 8 packed adds, 8 max3 each).  The lower half also carries the floor candidate fl(M + c_j), the upper half the extra columns; the other half holds -inf for them, so one
// instruction stream serves both.  The two partial maxima are joined in registers (one v_max_f32_dpp: the partner lanes
// are half a DPP row apart, row_ror:8) and only then is the emission added: max is exact and order-free, every candidate still gets exactly one rounded add, so the
// result is the float the one-target kernel forms.  After the join both lanes of a target hold its new delta; the lower
// lane writes copies 0 and 1 of it, the upper lane copies 2 and 3 (two ds_write each, nothing dead), and both add it into
// the frame-maximum slots (a duplicate changes no maximum).  Both lanes store the history column (the same bits to the
// same address), and the two lanes of idle slot S play the one-target kernel's "lane S" (M into pad column S of the previous
// row); the other idle slots hit pad column S + 1 with -inf as they do there.  LDS layout (copy stride from the 384 state slots), barrier, read order, pinning, prefetch depth
// and the history rows, pad columns included, are those of banded_floor_forward_kernel<32, 6, ...>, byte for byte.
// The wave role is a scalar test outside the frame loop: three loop bodies with the same barriers (full wave, half wave, and the
// last half wave, which also resets the slot group of the frame after next -- a role, not a wave test per frame).  The history and
// emission rows of a round of twelve frames hang off one buffer descriptor each; a frame's row is the instruction's scalar offset.
// ---------------------------------------------------------------------------------------
// (kSplitFullWaves, kSplitHalfWaves, kSplitStates and FloorSplitLds: banded_floor.inc, next to FloorLds)
// s_waitcnt immediate of gfx9: vmcnt in bits 3:0 and 15:14, expcnt (left open) in 6:4, lgkmcnt in 11:8
constexpr int split_waitcnt(int vm, int lgkm) { return (vm & 15) | ((vm >> 4) << 14) | (7 << 4) | (lgkm << 8); }
constexpr int kNoVmWait = 63;
// A trimmed full-wave window is read as NQ quads, in order, and one float behind them, the last LDS reads of the frame's burst: the
// reads still behind quad pair g (quads 2g, 2g + 1), i.e. the lgkmcnt that waits for that pair and everything in front of it
constexpr int split_reads_behind(int NQ, int g) { return (NQ + 1) - 2 * (g + 1); }
// f(std::integral_constant<int, K>) for K = 0, 1, ...: the unrolled frames and window groups need their index as a constant
// (the s_waitcnt immediate is derived from it)
template <int... K, typename F>
__device__ __forceinline__ void split_frames(std::integer_sequence<int, K...>, F&& f) { (f(std::integral_constant<int, K>{}), ...); }
// WF: the window entries a full wave evaluates (FwdArgs::floor_live, proven by the plan: floor_live_width).  WF = W is the whole window.
// WF = 4 n + 1 < W reads n quads and position WF - 1 as one float, loads no weight beyond it, and reduces its WF + 2 candidates
// (window, floor, extra column) in (WF + 1) / 2 v_max3_f32 (15 at WF = 29): two chains seeded with fl(M + c_j) and with the extra-column
// sum, one pair of sums per step, and the single entry joins the two chains in the last one.  M takes one v_max3_f32 more (XQ: three
// slots; else four slots and a v_max_f32 on top): 16 per frame at WF = 29, 36 VALU in all.  The half waves always take W / 2 each.
template <int NXT, int PF, typename ET, bool WPR = false, bool XQ = false, int WF = 32>
__global__ void __launch_bounds__(64 * (kSplitFullWaves + kSplitHalfWaves)) banded_floor_split_forward_kernel(FwdArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int W = 32;
    static_assert(WF == W || (WF % 4 == 1 && WF >= 9 && WF < W && NXT == 1), "a trimmed window: whole quads and one float, one extra column");
    constexpr int NWF = kSplitFullWaves, NW = kSplitFullWaves + kSplitHalfWaves;
    using L = FloorSplitLds;                      // the copy stride comes from the state slots, not from the thread count
    constexpr int DC = L::DC, BUF = L::BUF;
    float* dls = reinterpret_cast<float*>(smem) + L::dls;
    float* fmg = dls + L::fmg;
    VI* tot = reinterpret_cast<VI*>(dls + L::tot);
    const int S = a.S, SP = a.SP, T = a.T, SD = a.SD;
    constexpr bool GEN = NXT < 0;
    constexpr int NXL = GEN ? kMaxExtras : NXT;
    const int nx = GEN ? a.n_extras : NXT;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool half = wv >= NWF;                                          // wave-uniform role
    const int hh = half ? split_half_of(lane) : 0;                        // which half of the window (half waves: lanes l and l ^ 8 share a target)
    const int song = blockIdx.x;
    const int Tb = song_length(a.lengths, song, T);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (size_t)song * T * S;
    float* __restrict__ hist = a.hist + (size_t)song * T * SD;

    // ---------------- per-lane constants.  Idle targets (j >= S) carry -inf tables: their delta stays -inf.
    const int j = half ? 64 * NWF + 32 * (wv - NWF) + split_half_target(lane) : tid;
    const bool tvalid = j < S;
    const bool own = tvalid && hh == 0;                                   // the lane that answers for its target (frame 0, terminal state)
    const int jc = tvalid ? j : 0;
    const int jld = tvalid ? j : S - 1;
    // history store of frame t, relative to row t-1, by target slot exactly as in the one-target kernel: own column of row t |
    // slot S: M into pad column S of row t-1 | the other idle slots: pad column S+1 of row t (never read).  Both lanes of a
    // split target store the same bits to the same address (S >= 256: slot S lies in the half waves).
    const bool is_fm = j == S;
    const unsigned hoff = tvalid ? (unsigned)(SD + j) : (is_fm ? (unsigned)S : (unsigned)(SD + S + 1));
    const unsigned hoffb = 4u * hoff, eoffb = (unsigned)(sizeof(ET) * jld);
    const int lo = reinterpret_cast<const int32_t*>(a.image + a.off_lo)[jc];
    int xcol[NXL > 0 ? NXL : 1];
    bool is_x = false;
#pragma unroll
    for (int k = 0; k < NXL; ++k) {
        xcol[k] = k < nx ? a.extras[k] : 0;
        is_x |= (k < nx && j == xcol[k]);
    }
    const int sh = a.win_shift;                                           // (see banded_floor_forward_kernel)
    // (an idle target reads the last window, where the clamped rows next to it read: one address for all of them, no bank shared with
    // a live partner lane -- from window 0 the lanes of target S - 1 and the idle lanes of its read group met on one bank, floor_lds_check.hip)
    const int lov = (tvalid ? lo : S - W) + sh;
    const float* rp = dls + 4 + (lov & 3) * DC + (lov & ~3) + 16 * hh;    // (half of the) window in the copy that aligns it
    // XQ: M lives in slots 0 .. 2 and both lanes of the extra column add into slot 3 of the same quad of floats (split_fm_slot), so the
    // frame's one 16-byte read of the group brings M's three slots and delta[x]; every other plan keeps the four slots and its own read of x
    constexpr bool XS = XQ;                                               // the extra column in M's slot quad
    float* fmp = fmg + (XS ? split_fm_slot(lane, is_x) : fm_slot(lane));
    static_assert(!XQ || NXT == 1, "the extra column leaves M by address only where the launcher proved its quad idle");

    for (int k = tid; k < L::reset; k += NW * 64) dls[k] = -INFINITY;
    __syncthreads();

#ifdef VIT_TIMING_HOOKS
    const bool probe = (a.debug & 48) != 0;
    constexpr bool wprobe = WPR;   // per-wave probe (see WaveProbe): an instantiation of its own, the loop without it is the release loop
    WaveProbe wp_;
#else
    constexpr bool probe = false;
#endif
    unsigned long long clk0 = 0ull, rt0 = 0ull;

    // one role's share of the song: HALF = false the full-window waves, true the half-window waves
    // (resets: the last half wave, which also sends the slot group of the frame after next back to -inf)
    auto body = [&](auto role, auto resets) {
        constexpr bool HALF = decltype(role)::value, RESETS = decltype(resets)::value;
        constexpr int WL = HALF ? W / 2 : WF;                             // window sources per lane
        constexpr bool TRIM = WL % 4 != 0;                                // (full waves with WF < W: WL / 4 quads and one float)
        const float cj = own ? reinterpret_cast<const float*>(a.image + a.off_rowc)[jc] : -INFINITY;   // (upper half: -inf)
        float aw[WL];
        float xa[NXL > 0 ? NXL : 1];
        {
            const float* __restrict__ tab = reinterpret_cast<const float*>(a.image + a.off_tabA);
            const float* __restrict__ xaT = reinterpret_cast<const float*>(a.image + a.off_extraA);
#pragma unroll
            for (int w = 0; w < WL; ++w) aw[w] = tvalid ? tab[(size_t)(w + (HALF ? 16 * hh : 0)) * SP + jc] : -INFINITY;
#pragma unroll
            for (int k = 0; k < NXL; ++k)
                xa[k] = (tvalid && k < nx && (!HALF || hh == 1)) ? xaT[(size_t)k * SP + jc] : -INFINITY;   // (lower half: -inf)
        }
        // Half waves: own entry of copy 0 (copy c: + c*DC - c); an upper lane starts at copy 2.
        // Full waves: no address register.  Lane l of wave wv writes float 4 + sh + 64 wv + l of copy 0 and the same entry of the other
        // copies a constant further on, so the store is ds_write_addtid_b32 (lds_store_addtid): M0 holds the wave's part, set here once
        // for the whole song (frame 0 included; nothing in this role writes M0 again -- checked in the .s), the instruction's immediate
        // the buffer's and the copy's, and the hardware adds 4 * lane.  Half the issue time of ds_write_b32 for the sixteen stores per
        // CU that end every frame (scripts/ubench/lds_store_tail.hip: 64 -> 32 cycles).  The half waves' targets are not
        // linear in the lane (split_half_target) and their stores do not close the frame: they keep ds_write_b32.
        [[maybe_unused]] float* wp = nullptr;
        if constexpr (HALF) wp = dls + 4 + sh + j + hh * split_upper_off(DC);
        else {
            static_assert(L::dls == 0 && DC == kSplitCopyStride && BUF == 4 * DC, "split_addtid_base / split_addtid_imm (plan.hpp) speak of this layout");
            static_assert(split_addtid_imm(1, 3) + split_addtid_base(3, NWF - 1) + 4 * 64 <= (int)L::bytes() && L::bytes() < 65536,
                          "the largest immediate, the largest base and their sum with the lane term: inside the segment, hence 16 bits each");
            lds_addtid_base(reinterpret_cast<const float*>(smem + split_addtid_base(sh, wv)));
        }
        // the extra columns' positions in copy 0, kept in a vector register: they are wave-uniform, and from a scalar register every
        // frame's ds_read_b32 needed a v_mov first  (XS: delta[x] comes with the M slots, no read and no register)
        [[maybe_unused]] int xo[NXL > 0 ? NXL : 1];
        if constexpr (!XS) {
#pragma unroll
            for (int k = 0; k < NXL; ++k) {
                xo[k] = 4 + sh + xcol[k];
                asm volatile("" : "+v"(xo[k]));
            }
        }

        // Full waves without the extra column's select (XQ, or no extra column at all): the four copy stores and the quad maximum are one
        // asm statement (lds_store_addtid4_quad_max) -- each DPP step has its two wait states in two of the stores, where the compiler,
        // which counts no instruction inside an asm statement, put an s_nop 1 in front of either step.  These waves close the frame.
        constexpr bool QUADASM = !HALF && (XQ || NXL == 0);
        auto produce = [&](const float dn, auto wbc, const int G, const int Z) {
            constexpr int WB = decltype(wbc)::value;                      // (a constant: the add-tid stores carry it in their immediate)
            if constexpr (QUADASM) {
                const float q = lds_store_addtid4_quad_max<split_addtid_imm(WB, 0), split_addtid_imm(WB, 1), split_addtid_imm(WB, 2),
                                                           split_addtid_imm(WB, 3)>(dn);
                __hip_atomic_fetch_max(fmp + G * kFmGroupFloats, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                return;
            }
            if constexpr (HALF) {
#pragma unroll
                for (int c = 0; c < 2; ++c) wp[WB * BUF + floor_copy_off(DC, c)] = dn;
            } else {
                split_frames(std::make_integer_sequence<int, 4>{}, [&](auto cc) {
                    static_assert(split_addtid_imm(WB, decltype(cc)::value) == 4 * (WB * BUF + floor_copy_off(DC, decltype(cc)::value)), "the ds_write_b32 form's offset");
                    lds_store_addtid<split_addtid_imm(WB, decltype(cc)::value)>(dn);
                });
            }
            // XQ: the extra column's lanes publish into a slot nobody reads (fmp above), every other plan keeps the select
            fm_publish(fmp + G * kFmGroupFloats, (!XQ && NXL > 0 && is_x) ? -INFINITY : dn);
            // (the resetting wave is a role of its own: no wave test per frame, the one-target kernel's costs three SALU slots)
            if constexpr (RESETS) fmg[Z * kFmGroupFloats + lane] = -INFINITY;
        };

        // ---------------- frame 0 (both lanes of a split target hold it)
        {
            const float d0 = tvalid ? reinterpret_cast<const float*>(a.image + a.off_logpi)[j] + load_e<ET>(E + j) : -INFINITY;
            if (own) hist[j] = d0;
            produce(d0, std::integral_constant<int, 0>{}, 0, 1);
        }
        // The full waves' copy writes are inline asm the compiler counts no lgkmcnt for: in front of EVERY barrier of this role the wait
        // for them is stated, not left to the one the compiler derives from the ds_max_f32.  A missing one is a silent race, not a fault.
        auto frame_barrier = [&] {
            if constexpr (!HALF) __builtin_amdgcn_s_waitcnt(split_waitcnt(kNoVmWait, 0));
            __syncthreads();
        };
        float er[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) er[k] = load_e<ET>(E + (size_t)(1 + k < Tb ? 1 + k : Tb - 1) * S + jld);
#pragma unroll
        for (int w = 0; w < WL; ++w) asm volatile("" ::"v"(aw[w]));
#pragma unroll
        for (int k = 0; k < NXL; ++k) asm volatile("" ::"v"(xa[k]));
        asm volatile("" ::"v"(cj));
        frame_barrier();

        // Row bases of a round of up to PF frames that starts at frame t: history row t - 1 and emission row min(t + PF, Tb - 1), one
        // descriptor each for the whole round.  Frame t + u reaches its rows through the buffer instructions' scalar offset: u history
        // rows on (u * rowH, a constant per unrolled frame), and min(u, Tb - 1 - (t + PF)) emission rows on, i.e. row
        // min(t + u + PF, Tb - 1) as ever (elim: that bound in bytes, at most PF rows; 0 once the round's base row is the last row).
        // Per frame that is one s_min_u32 where the row bases took two 64-bit multiply-adds, a clamp and two descriptor rebuilds -- and
        // only in the last full round and the tail: the rounds in front of them (interior_bases) cannot reach the bound and go without it.
        const unsigned rowH = 4u * (unsigned)SD, rowE = (unsigned)sizeof(ET) * (unsigned)S;
        float* hb = hist;
        const ET* eb = E;
        unsigned elim = 0;
        auto round_bases = [&](const int t) {
            const int r = split_prefetch_row(t, 0, PF, Tb, false);
            const int ahead = Tb - 1 - r < PF ? Tb - 1 - r : PF;
            hb = hist + (size_t)(t - 1) * SD;
            eb = E + (size_t)r * S;
            elim = (unsigned)ahead * rowE;
        };
        // An interior round (split_round_interior, plan.hpp): every request t + u + PF, u < PF, lies inside the song, so frame t + u
        // takes the constant offset u * rowE and the round needs no bound
        auto interior_bases = [&](const int t) {
            hb = hist + (size_t)(t - 1) * SD;
            eb = E + (size_t)split_prefetch_row(t, 0, PF, Tb, true) * S;
        };
        auto frame = [&](float& e_slot, auto uc, auto ic) {
            constexpr int u = decltype(uc)::value;
            constexpr bool INTERIOR = decltype(ic)::value;
            constexpr int RB = u & 1, WB = RB ^ 1;
            const int GR = u % kFmGroups, GW = (u + 1) % kFmGroups, GZ = (u + 2) % kFmGroups;
            const f32x4* __restrict__ win = reinterpret_cast<const f32x4*>(rp + RB * BUF);
            float xd[NXL > 0 ? NXL : 1];
            f32x4 fq;
            [[maybe_unused]] float m0, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
            // The small reads first (extra columns -- none of their own under XS --, then the M slots), the window quads right behind them and nothing after: the window
            // quads are the LAST LDS operations of the frame's read burst (the two quads of a pair in either order).  The paired waits below count on that
            // (lgkmcnt(2) = "all but the last two quads"); a read moved behind the window would turn them into waits for less than they
            // name, and the compiler would add its own wait again.  Every stated lgkmcnt counts the reads BEHIND the one it waits for
            // (split_reads_behind), so the extra column's read, the first of the burst, does not appear in any of them: with or without
            // it (XS) the immediates are the same, and the first wait covers the M slots, hence delta[x], either way.
            if constexpr (!XS) {
#pragma unroll
                for (int k = 0; k < NXL; ++k) xd[k] = dls[xo[k] + RB * BUF];
            }
            fq = reinterpret_cast<const f32x4*>(fmg + GR * kFmGroupFloats)[0];
            asm volatile("" ::: "memory");
            f32x4 dw[WL / 4];
#pragma unroll
            for (int q = 0; q < WL / 4; ++q) dw[q] = win[q];
            [[maybe_unused]] float ds = 0.f;                              // (TRIM) position WL - 1: the last LDS read of the burst
            if constexpr (TRIM) ds = (rp + RB * BUF)[WL - 1];
            __builtin_amdgcn_sched_barrier(0);
#ifdef VIT_TIMING_HOOKS
            if constexpr (wprobe && !TRIM) wp_.first_data(fq);
#endif
            if constexpr (TRIM) {
                // one wait for M and the first pair of quads: everything but the WL / 4 - 2 quads and the float behind them
                static_assert(split_reads_behind(WL / 4, 0) == WL / 4 + 1 - 2, "behind the first pair: every other window read of the burst");
                __builtin_amdgcn_s_waitcnt(split_waitcnt(kNoVmWait, split_reads_behind(WL / 4, 0)));
                asm volatile("" : "+v"(fq), "+v"(dw[0]), "+v"(dw[1]));
#ifdef VIT_TIMING_HOOKS
                if constexpr (wprobe) wp_.first_data(fq);
#endif
            }
            const float M = XS ? fmaxf(fmaxf(fq.x, fq.y), fq.z) : fmaxf(fmaxf(fq.x, fq.y), fmaxf(fq.z, fq.w));
            if constexpr (XS) xd[0] = fq.w;                               // delta[x] of this frame, bit for bit (split_fm_slot)
            m0 = M + cj;
            asm volatile("" ::"v"(m0));   // M + c_j stays in front of the window sums (with the explicit waits below the add otherwise sinks behind them)
            __builtin_amdgcn_sched_barrier(0);
            float mx;
            // The emission of this frame was requested PF frames ago: behind it stand the PF - 1 younger prefetch loads and one row
            // store per frame since (u in the first round, where the prologue issued the loads back to back; 2 (PF - 1) >= PF - 1 + u
            // operations in every later round and in the tails), and vmcnt retires in order.  Stating that bound together with the
            // frame's last window wait saves the s_waitcnt vmcnt the compiler otherwise puts in front of "+ e".
            // Counted on this kernel's frame: ONE store (row_store_f32) and ONE load (row_load_e) per frame and role.  More VMEM per
            // frame (the probe instantiations) only makes the bound wait longer than needed; fewer would make it too weak.
            constexpr int vmw = PF - 1 + u;
            static_assert(vmw <= 2 * (PF - 1) && 2 * (PF - 1) < kNoVmWait, "vmcnt bound: one store and one load per frame, 6-bit field");
            if constexpr (TRIM) {
                // NQ quads and the single float behind them.  The tail -- the last quad of an odd count, the last two of an even one, and
                // the float -- is waited for at once, together with the emission (lgkmcnt(0), the frame's last wait); every pair of quads
                // in front of it waits once, for all but the reads behind it (the first pair together with M, above).
                constexpr int NQ = WL / 4, TQ = NQ % 2 ? 1 : 2, NPB = (NQ - TQ) / 2;
                static_assert(NXL == 1 && NQ >= 3 && 2 * NPB + TQ == NQ && 4 * NQ + 1 == WL, "pairs of quads, then the tail: one or two quads and one float");
                static_assert(split_reads_behind(NQ, 0) <= 15, "lgkmcnt is a four-bit field");
                static_assert(split_reads_behind(NQ, NPB - 1) == TQ + 1, "behind the last pair stand the tail's reads -- TQ quads and the float -- and nothing else");
                static_assert(split_reads_behind(NQ, NPB) + 2 == TQ + 1 && TQ <= 2, "the tail's wait, lgkmcnt(0), leaves no window read out");
                // The hazard recognizer takes an asm statement with register outputs for a writer whose result the next instruction must
                // not read, and a packed add for one whose result the next instruction (an asm statement included) must not read: a fence
                // of the form "+v" right behind the last packed add of its group, or right in front of the first maximum that reads one of
                // its outputs, costs an s_nop 0.  Hence the seed of the second chain below and the shape of the tail's fence.
                float mb;                                                 // the second chain starts from the extra-column sum (the burst's first read)
                split_frames(std::make_integer_sequence<int, NPB>{}, [&](auto gc) {
                    constexpr int w = 8 * decltype(gc)::value;
                    f32x4 da = dw[w / 4], db = dw[w / 4 + 1];
                    if constexpr (decltype(gc)::value >= 1) {
                        constexpr int behind = split_reads_behind(NQ, decltype(gc)::value);   // the quads and the float behind this pair
                        static_assert(behind >= TQ + 1 && behind + 2 == split_reads_behind(NQ, decltype(gc)::value - 1), "two reads fewer than the pair before");
                        __builtin_amdgcn_s_waitcnt(split_waitcnt(kNoVmWait, behind));
                        asm volatile("" : "+v"(da), "+v"(db));
                    }
                    f32x2 c0_ = f32x2{da.x, da.y} + f32x2{aw[w + 0], aw[w + 1]};
                    f32x2 c1_ = f32x2{da.z, da.w} + f32x2{aw[w + 2], aw[w + 3]};
                    f32x2 c2_ = f32x2{db.x, db.y} + f32x2{aw[w + 4], aw[w + 5]};
                    f32x2 c3_ = f32x2{db.z, db.w} + f32x2{aw[w + 6], aw[w + 7]};
                    if constexpr (decltype(gc)::value == 0) {
                        // the seed add stands between the first group's last packed add and its fence (later groups have the maxima of
                        // the group before there)
                        mb = xd[0] + xa[0];
                        asm volatile("" : "+v"(c0_), "+v"(c1_), "+v"(c2_), "+v"(c3_) : "v"(mb));
                    } else
                    asm volatile("" : "+v"(c0_), "+v"(c1_), "+v"(c2_), "+v"(c3_));   // a group's sums before its maxima: no hazard s_nop
                    m0 = fmaxf(fmaxf(m0, c0_.x), c0_.y);
                    mb = fmaxf(fmaxf(mb, c1_.x), c1_.y);
                    m0 = fmaxf(fmaxf(m0, c2_.x), c2_.y);
                    mb = fmaxf(fmaxf(mb, c3_.x), c3_.y);
                });
                {
                    constexpr int w = 8 * NPB;
                    f32x4 da = dw[w / 4], db = dw[NQ - 1];                // (TQ == 1: db is da again and unused)
                    __builtin_amdgcn_s_waitcnt(split_waitcnt(vmw, 0));
                    if constexpr (TQ == 2) asm volatile("" : "+v"(da), "+v"(db), "+v"(ds)); else asm volatile("" : "+v"(da), "+v"(ds));
                    f32x2 c0_ = f32x2{da.x, da.y} + f32x2{aw[w + 0], aw[w + 1]};
                    f32x2 c1_ = f32x2{da.z, da.w} + f32x2{aw[w + 2], aw[w + 3]};
                    float cs = ds + aw[WL - 1];
                    if constexpr (TQ == 2) {
                        f32x2 c2_ = f32x2{db.x, db.y} + f32x2{aw[w + 4], aw[w + 5]};
                        f32x2 c3_ = f32x2{db.z, db.w} + f32x2{aw[w + 6], aw[w + 7]};
                        asm volatile("" : "+v"(c1_), "+v"(c2_), "+v"(c3_), "+v"(cs) : "v"(c0_));   // (c0_: see below)
                        m0 = fmaxf(fmaxf(m0, c0_.x), c0_.y);
                        mb = fmaxf(fmaxf(mb, c1_.x), c1_.y);
                        m0 = fmaxf(fmaxf(m0, c2_.x), c2_.y);
                        mb = fmaxf(fmaxf(mb, c3_.x), c3_.y);
                    } else {
                        // c0_ is an input only: it is formed in front of the fence like the others, and the first maximum behind the fence,
                        // which reads it, reads no output of the fence
                        asm volatile("" : "+v"(c1_), "+v"(cs) : "v"(c0_));
                        m0 = fmaxf(fmaxf(m0, c0_.x), c0_.y);
                        mb = fmaxf(fmaxf(mb, c1_.x), c1_.y);
                    }
                    mx = fmaxf(fmaxf(m0, mb), cs);                        // the single entry joins the two chains
                }
            } else {
                split_frames(std::make_integer_sequence<int, WL / 8>{}, [&](auto gc) {
                    constexpr int w = 8 * decltype(gc)::value;
                    constexpr bool last = w + 8 == WL;
                    // The late window quads are waited for in pairs: the last four of the full waves' eight, the last two of the half waves'
                    // four.  M and the first quads keep the compiler's stepped waits, which buy the early first max3.
                    constexpr bool pairw = w + 16 >= WL && w >= 8;
                    f32x4 da = dw[w / 4], db = dw[w / 4 + 1];
                    if constexpr (pairw) {
                        __builtin_amdgcn_s_waitcnt(split_waitcnt(last ? vmw : kNoVmWait, last ? 0 : 2));
                        asm volatile("" : "+v"(da), "+v"(db));
                    }
                    f32x2 c0_ = f32x2{da.x, da.y} + f32x2{aw[w + 0], aw[w + 1]};
                    f32x2 c1_ = f32x2{da.z, da.w} + f32x2{aw[w + 2], aw[w + 3]};
                    f32x2 c2_ = f32x2{db.x, db.y} + f32x2{aw[w + 4], aw[w + 5]};
                    f32x2 c3_ = f32x2{db.z, db.w} + f32x2{aw[w + 6], aw[w + 7]};
                    asm volatile("" : "+v"(c0_), "+v"(c1_), "+v"(c2_), "+v"(c3_));   // a group's sums before its maxima: no hazard s_nop
                    m0 = fmaxf(fmaxf(m0, c0_.x), c0_.y);
                    m1 = fmaxf(fmaxf(m1, c1_.x), c1_.y);
                    m2 = fmaxf(fmaxf(m2, c2_.x), c2_.y);
                    m3 = fmaxf(fmaxf(m3, c3_.x), c3_.y);
                });
#pragma unroll
                for (int k = 0; k < NXL; ++k) m1 = fmaxf(m1, xd[k] + xa[k]);
                mx = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
            }
            if constexpr (HALF) mx = max_lane_xor8(mx);                   // join the two halves of the window (partner lanes, one DPP maximum)
            const float dn = mx + e_slot;
#ifdef VIT_TIMING_HOOKS
            if constexpr (wprobe) wp_.before_publish(dn);
#endif
            // (the stored value and the emission offset are formed in front of the publication: the order the measured builds have)
            const float sv = (HALF && is_fm) ? M : dn;                    // (full waves hold live targets only)
            const unsigned eso = INTERIOR ? (unsigned)u * rowE : ((unsigned)u * rowE < elim ? (unsigned)u * rowE : elim);
            produce(dn, std::integral_constant<int, WB>{}, GW, GZ);
            asm volatile("" ::: "memory");   // the global store / prefetch fill the wait for the LDS write acknowledgement
            // KEEP THIS STORE SINGLE-DWORD: with a register soffset a store wider than 64 bits needs wait states in front of the next write
            // of its data registers that the compiler does not insert -- wrong rows, not reproducibly
            row_store_f32(hb, hoffb, sv, (unsigned)u * rowH);
            e_slot = row_load_e<ET>(eb, eoffb, eso);
#ifdef VIT_TIMING_HOOKS
            if constexpr (wprobe) wp_.barrier(); else   // (the probe's barrier states the same wait)
#endif
            frame_barrier();
        };
#ifdef VIT_TIMING_HOOKS
        if constexpr (wprobe) wp_.start();
#endif
        clk0 = probe ? __builtin_amdgcn_s_memtime() : 0ull;
        rt0 = probe ? __builtin_amdgcn_s_memrealtime() : 0ull;
        // The half waves are the younger wave of each SIMD and lost the arbitration to the full wave in every frame; with static priority 1
        // they publish first and the full waves, which have fewer instructions left per frame than the half waves' lag cost, close the frame.
        // Once per song, in the half-wave roles only (the role is a scalar branch, see below); nothing in the loop.
        // (per frame it was tried and lost: priority 0 for the half waves' read burst, so that the full waves' reads go first, gets the full
        // waves their first data ~105 cycles earlier and makes the frame 50 cycles LONGER -- DESIGN.md 7)
        if constexpr (HALF) __builtin_amdgcn_s_setprio(1);
        // Interior rounds (no request is held at the song's last row: constant row offsets, no clamp), then the last full round and the
        // tail with the clamp.  At T = 30000 that is 2498 rounds without it and one with.
        int t = 1;
        for (; split_round_interior(t, PF, Tb); t += PF) {
            interior_bases(t);
            split_frames(std::make_integer_sequence<int, PF>{}, [&](auto k) { frame(er[k], k, std::true_type{}); });
        }
        for (; split_round_full(t, PF, Tb); t += PF) {
            round_bases(t);
            split_frames(std::make_integer_sequence<int, PF>{}, [&](auto k) { frame(er[k], k, std::false_type{}); });
        }
        round_bases(t);
        split_frames(std::make_integer_sequence<int, PF - 1>{}, [&](auto k) {
            if (t + k < Tb) frame(er[k], k, std::false_type{});
        });
    };
    static_assert(PF % 2 == 0 && PF % kFmGroups == 0, "the unrolled frames must cycle through whole buffer and slot-group rounds");
    if (!half) body(std::false_type{}, std::false_type{});
    else if (wv == NW - 1) body(std::true_type{}, std::true_type{});
    else body(std::true_type{}, std::false_type{});

    const int fb = (Tb - 1) & 1;                                          // buffer holding delta_{Tb-1}
    terminal_argmax(own ? dls[4 + sh + fb * BUF + j] : -INFINITY, j, own, tot, NW, a.last_state, a.loglik, song);
    if (probe && tid == 0) {  // timing experiments only: cycles (16) or 100 MHz ticks (32) per frame -> scratch slot 63
        const unsigned long long d = (a.debug & 16) ? __builtin_amdgcn_s_memtime() - clk0 : __builtin_amdgcn_s_memrealtime() - rt0;
        a.fmax[(size_t)song * 64 + 63] = (float)d / (float)(Tb > 1 ? Tb - 1 : 1);
    }
#ifdef VIT_TIMING_HOOKS
    if constexpr (wprobe) wp_.finish(a.fmax + (size_t)song * 64, wv, lane, Tb - 1);
#endif
}

// ---------------------------------------------------------------------------------------
// Floor-max banded forward kernel, two targets per lane (plan.pair_ok && plan.floor_ok; what the bench runs).
//
// What bounds a frame of banded_floor_forward_kernel is the LDS return path: every target pulls its own W floats
// into registers (46 KB per frame at S = 361) and ds_read_b128 delivers ~128 B/clk per CU, ~380 of the ~870 cycles.
// The plan proves that the exception spans of targets 2p and 2p+1 together fit one window [lo2_p, lo2_p + W); entries
// of that window outside a row's own span are that row's constant (or an extra column), i.e. still >= c_j, so the
// floor-max identity holds for the common window.  One lane therefore evaluates BOTH targets from one set of W/4
// window reads: half the LDS traffic and half the waves (three at S = 361, one per SIMD), the same packed adds and
// max3 per target.  Everything else is as in banded_floor_forward_kernel, except that M is still published through the
// six-step wave scan and the history / emission rows are addressed with 64-bit per-lane pointers.
// ---------------------------------------------------------------------------------------
// LDS of the pair kernel, in floats: what the kernel carves and what its launcher asks for
template <int NPW>
struct FloorPairLds {
    static constexpr int NP = NPW * 128;                 // padded state count
    static constexpr int DC = NP + 16;                   // copy stride (see banded_forward_kernel)
    static constexpr int BUF = 4 * DC;                   // floats per delta buffer
    static constexpr int NWM = (NPW + 3) / 4 * 4;        // wave maxima per buffer, whole float4s (slots >= NPW hold -inf)
    static constexpr int dls = 0;                        // [2][4][DC]
    static constexpr int wm = dls + 2 * BUF;             // [2][NWM]
    static constexpr int reset = wm + 2 * NWM;           // floats that go to -inf before the song: everything up to here
    static constexpr int dump = reset;                   // [64 + NWM]
    static constexpr int tot = dump + 64 + NWM;          // [16] VI
    static constexpr int end = tot + 16 * (int)(sizeof(VI) / sizeof(float));
    static_assert(sizeof(float) * end <= kLdsBytes, "one workgroup's LDS");
    static constexpr size_t bytes() { return sizeof(float) * end; }
};

template <int W, int NPW, int NXT, int PF, typename ET>
__global__ void __launch_bounds__(NPW * 64) banded_floor_pair_forward_kernel(FwdArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    using L = FloorPairLds<NPW>;
    constexpr int DC = L::DC, BUF = L::BUF, NWM = L::NWM;
    float* dls = reinterpret_cast<float*>(smem) + L::dls;
    float* wm = dls + L::wm;
    float* dump = dls + L::dump;
    VI* tot = reinterpret_cast<VI*>(dls + L::tot);
    const int S = a.S, SP = a.SP, T = a.T, SD = a.SD;
    constexpr bool GEN = NXT < 0;
    constexpr int NXL = GEN ? kMaxExtras : NXT;
    const int nx = GEN ? a.n_extras : NXT;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int song = blockIdx.x;
    const int Tb = song_length(a.lengths, song, T);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (size_t)song * T * S;
    float* __restrict__ hist = a.hist + (size_t)song * T * SD;

    // ---------------- per-lane constants.  Slots past S carry -inf tables: their delta stays -inf.
    const int j0 = 2 * tid, j1 = 2 * tid + 1;
    const bool v0 = j0 < S, v1 = j1 < S;
    const int jc0 = v0 ? j0 : 0, jc1 = v1 ? j1 : jc0;
    const int jl0 = v0 ? j0 : S - 1, jl1 = v1 ? j1 : S - 1;               // emission columns (idle slots load a valid one)
    // history stores of frame t, relative to row t-1: own column of row t | slot S: M into pad column S of row t-1
    // | other idle slots: pad column S+1 of row t (never read)
    const unsigned hoff0 = v0 ? (unsigned)(SD + j0) : (j0 == S ? (unsigned)S : (unsigned)(SD + S + 1));
    const unsigned hoff1 = v1 ? (unsigned)(SD + j1) : (j1 == S ? (unsigned)S : (unsigned)(SD + S + 1));
    const bool fm0 = j0 == S, fm1 = j1 == S;
    const int lo2 = v0 ? reinterpret_cast<const int32_t*>(a.image + a.off_lo2)[jc0 >> 1] : 0;
    const float* __restrict__ rc = reinterpret_cast<const float*>(a.image + a.off_rowc);
    f32x2 cj = f32x2{v0 ? rc[jc0] : -INFINITY, v1 ? rc[jc1] : -INFINITY};
    float aw0[W], aw1[W];
    f32x2 xa[NXL > 0 ? NXL : 1];
    int xcol[NXL > 0 ? NXL : 1];
    bool x0 = false, x1 = false;                                          // slot is an extra column: not part of M
    {
        const float* __restrict__ tab = reinterpret_cast<const float*>(a.image + a.off_tabP);
        const float* __restrict__ xaT = reinterpret_cast<const float*>(a.image + a.off_extraA);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            aw0[w] = v0 ? tab[(size_t)w * SP + jc0] : -INFINITY;
            aw1[w] = v1 ? tab[(size_t)w * SP + jc1] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            xcol[k] = k < nx ? a.extras[k] : 0;
            xa[k] = f32x2{(v0 && k < nx) ? xaT[(size_t)k * SP + jc0] : -INFINITY, (v1 && k < nx) ? xaT[(size_t)k * SP + jc1] : -INFINITY};
            x0 |= (k < nx && j0 == xcol[k]);
            x1 |= (k < nx && j1 == xcol[k]);
        }
    }
    // delta[i] lives at float position 4 + sh + i - c of copy c; the lane reads the common window from the copy that
    // makes delta[lo2] 16-byte aligned (sh: see banded_floor_forward_kernel)
    const int sh = a.win_shift2;
    const int lov = lo2 + sh;
    const float* rp = dls + 4 + (lov & 3) * DC + (lov & ~3);
    float* wp = dls + 4 + sh + j0;                                        // slot 0 of copy 0 (copy c: + c*DC - c), slot 1 follows
    float* wmp = lane == 63 ? wm + wv : dump + lane;

    for (int k = tid; k < L::reset; k += NPW * 64) dls[k] = -INFINITY;
    __syncthreads();

    auto produce = [&](const f32x2 dn, const int WB) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wp[WB * BUF + c * DC - c] = dn.x;
            wp[WB * BUF + c * DC - c + 1] = dn.y;
        }
        const float inc = wave_scan_max(fmaxf((NXL > 0 && x0) ? -INFINITY : dn.x, (NXL > 0 && x1) ? -INFINITY : dn.y));
        wmp[WB * NWM] = inc;
    };

    // ---------------- frame 0
    {
        const float* __restrict__ lpi = reinterpret_cast<const float*>(a.image + a.off_logpi);
        f32x2 d0 = f32x2{-INFINITY, -INFINITY};
        if (v0) { d0.x = lpi[j0] + load_e<ET>(E + j0); hist[j0] = d0.x; }
        if (v1) { d0.y = lpi[j1] + load_e<ET>(E + j1); hist[j1] = d0.y; }
        produce(d0, 0);
    }
    f32x2 er[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const ET* __restrict__ row = E + (size_t)(1 + k < Tb ? 1 + k : Tb - 1) * S;
        er[k] = f32x2{load_e<ET>(row + jl0), load_e<ET>(row + jl1)};
    }
#pragma unroll
    for (int w = 0; w < W; ++w) asm volatile("" ::"v"(aw0[w]), "v"(aw1[w]));
#pragma unroll
    for (int k = 0; k < NXL; ++k) asm volatile("" ::"v"(xa[k]));
    asm volatile("" ::"v"(cj));
    __syncthreads();

    auto frame = [&](const int t, f32x2& e_slot, const int RB) {
        const int WB = RB ^ 1;
        const f32x4* __restrict__ win = reinterpret_cast<const f32x4*>(rp + RB * BUF);
        float xd[NXL > 0 ? NXL : 1];
#pragma unroll
        for (int k = 0; k < NXL; ++k) xd[k] = dls[4 + sh + RB * BUF + xcol[k]];
        f32x4 wq[NWM / 4];
#pragma unroll
        for (int q = 0; q < NWM / 4; ++q) wq[q] = reinterpret_cast<const f32x4*>(wm + RB * NWM)[q];
        f32x4 dw[W / 4];
#pragma unroll
        for (int q = 0; q < W / 4; ++q) dw[q] = win[q];
        float m0 = -INFINITY, m1 = -INFINITY, n0 = -INFINITY, n1 = -INFINITY;   // two max3 chains per target
#pragma unroll
        for (int w = 0; w + 3 < W; w += 4) {
            const f32x4 d = dw[w / 4];
            const f32x2 a0 = f32x2{d.x, d.y} + f32x2{aw0[w + 0], aw0[w + 1]};
            const f32x2 a1 = f32x2{d.z, d.w} + f32x2{aw0[w + 2], aw0[w + 3]};
            const f32x2 b0 = f32x2{d.x, d.y} + f32x2{aw1[w + 0], aw1[w + 1]};
            const f32x2 b1 = f32x2{d.z, d.w} + f32x2{aw1[w + 2], aw1[w + 3]};
            m0 = fmaxf(fmaxf(m0, a0.x), a0.y);
            n0 = fmaxf(fmaxf(n0, a1.x), a1.y);
            m1 = fmaxf(fmaxf(m1, b0.x), b0.y);
            n1 = fmaxf(fmaxf(n1, b1.x), b1.y);
        }
        // M = max of delta_{t-1} over the non-extra sources; slots >= NPW of wq hold -inf
        float M = fmaxf(fmaxf(wq[0].x, wq[0].y), fmaxf(wq[0].z, wq[0].w));
#pragma unroll
        for (int q = 1; q < NWM / 4; ++q) M = fmaxf(fmaxf(fmaxf(M, wq[q].x), wq[q].y), fmaxf(wq[q].z, wq[q].w));
        const f32x2 fl = f32x2{M, M} + cj;
        m0 = fmaxf(m0, fl.x);
        m1 = fmaxf(m1, fl.y);
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            const f32x2 xv = f32x2{xd[k], xd[k]} + xa[k];
            n0 = fmaxf(n0, xv.x);
            n1 = fmaxf(n1, xv.y);
        }
        const f32x2 dn = f32x2{fmaxf(m0, n0), fmaxf(m1, n1)} + e_slot;
        produce(dn, WB);
        asm volatile("" ::: "memory");   // history stores / prefetch behind the wave-max publication
        const int tn = t + PF < Tb ? t + PF : Tb - 1;
        float* __restrict__ hb = hist + (size_t)(t - 1) * SD;
        const ET* __restrict__ erow = E + (size_t)tn * S;
        hb[hoff0] = fm0 ? M : dn.x;
        hb[hoff1] = fm1 ? M : dn.y;
        e_slot = f32x2{load_e<ET>(erow + jl0), load_e<ET>(erow + jl1)};
        __syncthreads();
    };
#ifdef VIT_TIMING_HOOKS
    const bool probe = (a.debug & 48) != 0;
#else
    constexpr bool probe = false;   // cycle probe: VIT_TIMING_HOOKS builds only; it writes the per-song scratch, never an output
#endif
    const unsigned long long clk0 = probe ? __builtin_amdgcn_s_memtime() : 0ull;
    const unsigned long long rt0 = probe ? __builtin_amdgcn_s_memrealtime() : 0ull;
    int t = 1;
    for (; t + PF - 1 < Tb; t += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) frame(t + k, er[k], k & 1);
    }
#pragma unroll
    for (int k = 0; k < PF - 1; ++k)
        if (t + k < Tb) frame(t + k, er[k], k & 1);

    // terminal state: lowest-index argmax of delta_{T-1}; a lane holds two adjacent states
    {
        const int fb = (Tb - 1) & 1;
        const float* fin = dls + 4 + sh + fb * BUF;
        VI x = vi_identity();
        if (v0) x = VI{fin[j0], j0};
        if (v1) x = op_fwd(x, VI{fin[j1], j1});
        x = wave_scan<false>(x);
        if (lane == 63) tot[wv] = x;
        __syncthreads();
        if (tid == 0) {
            VI acc = vi_identity();
            for (int b = 0; b < NPW; ++b) acc = op_fwd(acc, tot[b]);
            if (acc.i == kBig) acc.i = 0;
            a.last_state[song] = acc.i;
            if (a.loglik) a.loglik[song] = acc.v;
        }
    }
    if (probe && tid == 0) {  // timing experiments only: cycles (16) or 100 MHz ticks (32) per frame -> scratch slot 63
        const unsigned long long d = (a.debug & 16) ? __builtin_amdgcn_s_memtime() - clk0 : __builtin_amdgcn_s_memrealtime() - rt0;
        a.fmax[(size_t)song * 64 + 63] = (float)d / (float)(Tb > 1 ? Tb - 1 : 1);
    }
}

// DPP self-test: mode 0/1 = (value, index) first-max scan fwd/rev; mode 2 = value-only prefix max;
// mode 3 = wave_shift_up of the prefix max; mode 4 = wave_max_all.
__global__ void scan_selftest_kernel(const float* __restrict__ vals, int mode, float* __restrict__ out_v,
                                     int32_t* __restrict__ out_i) {
    const int j = threadIdx.x + blockIdx.x * blockDim.x;
    VI x{vals[j], (int)threadIdx.x};
    if (mode == 0) x = wave_scan<false>(x);
    else if (mode == 1) x = wave_scan<true>(x);
    else if (mode == 2) x.v = wave_scan_max(x.v);
    else if (mode == 3) x.v = wave_shift_up(wave_scan_max(x.v), -INFINITY);
    else x.v = wave_max_all(x.v);
    out_v[j] = x.v;
    out_i[j] = x.i;
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
// floor-max forms (plan.floor_ok; idle slot S stores the frame maximum: needs S < 64 * NWT)
template <int W, int NWT, typename ET>
static hipError_t launch_floor_t(const FwdArgs& a, hipStream_t st) {
    constexpr int PF = floor_pf<W>();      // emission rows in flight: a row is requested PF frames (0.34 us each) before its use; under the overlapped
                                            // back-trace 4 left ~2 % on the table (B = 128: 4 -> 10.35, 8 -> 10.20, 12 -> 10.12, 16 -> 10.14 ms per forward pass)
    // Up to two songs per CU the one-target-per-lane kernel is (slightly) faster; beyond that the two-targets-per-lane
    // kernel wins because it moves half the window bytes through LDS (B = 512: 14.5 vs 15.5 ms).
    // FwdArgs::fwd_form 1 / 2 force one or the other.
    // Split windows over eight waves (fwd_form 6 forces it): the six-wave grids at W = 32, up to one song per CU, fp32
    // emissions.  Forward pass at [B, 30000, S], one-target -> split: S = 361 fp32 9.48 -> 8.98 ms (B = 128), 9.50 -> 9.03
    // (B = 256); S = 321 fp32 9.46 -> 8.97, 9.52 -> 9.05.  With fp16 emissions the split kernel is 50 % SLOWER
    // (S = 361: 10.28 -> 15.67 ms, S = 321: 10.27 -> 15.51 ms: its loops convert the 16-bit emission right behind the
    // prefetch load and wait for it every frame), so the default leaves those to the one-target kernel (profiles/r06_logs/floor_split_ab.log).
    if constexpr (W == 32 && NWT == 6) {
        static_assert(kSplitStates == NWT * 64, "the split kernel keeps the six-wave kernel's LDS and history layout");
        static_assert(kSplitFullRows == 64 * kSplitFullWaves, "FwdArgs::floor_live speaks for the full waves' targets");
        static_assert(PF == kSplitPrefetch, "the host library replays the split kernel's rounds at this depth");
        if (a.fwd_form == 6 || (a.fwd_form == 0 && a.B <= 256 && std::is_same_v<ET, float>)) {
            constexpr size_t ldss = FloorSplitLds::bytes();
            constexpr int NWS = kSplitFullWaves + kSplitHalfWaves;
            // The extra column leaves M by address only where its whole quad is otherwise idle: the quad maximum is formed before the
            // slot is chosen, so the column can only be dropped together with its quad.  One extra column x = S - 1 with x % 4 == 0 is
            // the publishing lane of its quad and states x + 1 .. x + 3 are idle slots (-inf for the whole song); any other plan
            // (generic extras, an extra column elsewhere, x % 4 != 0 with live states in the quad) keeps the select.
            const bool xq = a.n_extras == 1 && a.extras[0] == a.S - 1 && (a.S - 1) % 4 == 0;
            // The full waves evaluate the window entries the plan proves live for their targets (a.floor_live, floor_live_width): the
            // smallest instantiated width that covers them -- 29 for the reference's 361-state grid, 25 for its 321-state grids.  Generic
            // extras, fp16 emissions (forward form 6 only) and a plan whose first rows are clamped to the end of the grid take the whole window.
            const int wf = split_full_width(a.floor_live, W, a.S, a.n_extras, !std::is_same_v<ET, float>);
            auto go = [&](auto xqc, auto wfc) {
                constexpr bool XQ = decltype(xqc)::value;
                constexpr int WF = decltype(wfc)::value;
#ifdef VIT_TIMING_HOOKS
                if (a.debug & 64)
                    hipLaunchKernelGGL((banded_floor_split_forward_kernel<1, PF, ET, true, XQ, WF>), dim3((int)a.B), dim3(NWS * 64), ldss, st, a);
                else
#endif
                hipLaunchKernelGGL((banded_floor_split_forward_kernel<1, PF, ET, false, XQ, WF>), dim3((int)a.B), dim3(NWS * 64), ldss, st, a);
            };
            auto go_w = [&](auto xqc) {
                if constexpr (std::is_same_v<ET, float>) {
                    static_assert(sizeof(kSplitLiveWidths) / sizeof(int) == 2, "one case per instantiated live width");
                    if (wf == 25) return go(xqc, std::integral_constant<int, 25>{});
                    if (wf == 29) return go(xqc, std::integral_constant<int, 29>{});
                }
                return go(xqc, std::integral_constant<int, W>{});
            };
            if (xq) go_w(std::true_type{});
            else if (a.n_extras == 1) go_w(std::false_type{});
            else
                hipLaunchKernelGGL((banded_floor_split_forward_kernel<-1, PF, ET>), dim3((int)a.B), dim3(NWS * 64), ldss, st, a);
            return hipGetLastError();
        }
    }
    if constexpr (W <= 32 && NWT <= 8) {   // (at twelve waves, S = 722, the one-target kernel measured faster at every batch size)
        // (fwd_form 6 where the split kernel does not exist: the one-target kernel, as fwd_form 2 without pair_ok)
        const bool pair = a.pair_ok && ((a.B > 256 && a.fwd_form != 1 && a.fwd_form != 6) || a.fwd_form == 2);
        if (pair) {
            constexpr int NPW = (NWT + 1) / 2;
            constexpr int PFP = 4;             // (two workgroups share a CU here and cover each other's waits: 12 rows in flight measured 9 % slower)
            constexpr size_t ldsp = FloorPairLds<NPW>::bytes();
            if (W == 32 && a.n_extras == 1)
                hipLaunchKernelGGL((banded_floor_pair_forward_kernel<W, NPW, (W == 32 ? 1 : -1), PFP, ET>), dim3((int)a.B), dim3(NPW * 64), ldsp, st, a);
            else
                hipLaunchKernelGGL((banded_floor_pair_forward_kernel<W, NPW, -1, PFP, ET>), dim3((int)a.B), dim3(NPW * 64), ldsp, st, a);
            return hipGetLastError();
        }
    }
    constexpr size_t ldsf = FloorLds<W, NWT>::bytes();
#ifdef VIT_TIMING_HOOKS
    if constexpr (W == 32 && NWT == 6) {
        if ((a.debug & 64) && a.n_extras == 1) {
            hipLaunchKernelGGL((banded_floor_forward_kernel<W, NWT, 1, PF, ET, WgVariant::Plain, true>), dim3((int)a.B), dim3(NWT * 64), ldsf, st, a);
            return hipGetLastError();
        }
    }
#endif
    return with_nxt<W>(a.n_extras, [&](auto nxt) {
        hipLaunchKernelGGL((banded_floor_forward_kernel<W, NWT, decltype(nxt)::value, PF, ET>), dim3((int)a.B), dim3(NWT * 64), ldsf, st, a);
        return hipGetLastError();
    });
}

// general (scan) form
template <int W, int NWT, typename ET>
static hipError_t launch_scan_t(const FwdArgs& a, hipStream_t st) {
    constexpr int NP = NWT * 64;
    const size_t lds = sizeof(float) * (4 * (NP + 16) + 2 * (NP + 1) + kMaxDenseRows) + sizeof(VI) * 16;
    // NWT + 2 waves put exactly two on each SIMD at S = 361 and let two workgroups share a CU.  Only a
    // plan with dense rows, run at one workgroup per CU, gets a separate wave for them (it would
    // otherwise lengthen the suffix wave, the critical one).
    if (a.n_dense > 0 && a.B <= 256)
        hipLaunchKernelGGL((banded_forward_kernel<W, NWT, true, false, -1, ET>), dim3((int)a.B), dim3((NWT + 3) * 64), lds, st, a);
#ifdef VIT_TIMING_HOOKS
    else if (a.debug)
        hipLaunchKernelGGL((banded_forward_kernel<W, NWT, false, true, -1, ET>), dim3((int)a.B), dim3((NWT + 2) * 64), lds, st, a);
#endif
    else if (W == 32 && a.n_dense == 0 && a.n_extras == 1)   // the reference's matrices: band + unvoiced column
        hipLaunchKernelGGL((banded_forward_kernel<W, NWT, false, false, (W == 32 ? 1 : -1), ET>), dim3((int)a.B), dim3((NWT + 2) * 64), lds, st, a);
    else if (W == 32 && a.n_dense == 0 && a.n_extras == 0)
        hipLaunchKernelGGL((banded_forward_kernel<W, NWT, false, false, (W == 32 ? 0 : -1), ET>), dim3((int)a.B), dim3((NWT + 2) * 64), lds, st, a);
    else
        hipLaunchKernelGGL((banded_forward_kernel<W, NWT, false, false, -1, ET>), dim3((int)a.B), dim3((NWT + 2) * 64), lds, st, a);
    return hipGetLastError();
}

template <int W, int NWT, typename ET>
static hipError_t launch_banded_t(const FwdArgs& a, hipStream_t st) {
    // fwd_form 3 forces the general (scan) kernel; so do the ablation bits of a VIT_TIMING_HOOKS build (48 = cycle probes,
    // 64 = per-wave probe: they exist in the floor kernels as well)
    const bool floor_ok = a.floor_ok && a.S < NWT * 64 && a.fwd_form != 3 && !(a.debug & ~112);
    if constexpr (floor_form_instantiated(W, NWT)) {
        if (floor_ok) return launch_floor_t<W, NWT, ET>(a, st);
    }
    if constexpr (scan_form_instantiated(W, NWT)) return launch_scan_t<W, NWT, ET>(a, st);
    return hipErrorInvalidConfiguration;
}

hipError_t launch_banded(const FwdArgs& a, bool f16, hipStream_t st) {
    auto go = [&](auto et) {
        using ET = decltype(et);
        return dispatch_width(a.W, [&](auto w) {
            return dispatch_waves(a.S, [&](auto n) { return launch_banded_t<decltype(w)::value, decltype(n)::value, ET>(a, st); });
        });
    };
    return f16 ? go(__half{}) : go(float{});
}

// the variants of the one-target floor kernel
static hipError_t floor_variant(const FwdArgs& a, WgVariant v, bool f16, hipStream_t st, int* per_cu) {
    switch (v) {
        case WgVariant::Packed: return f16 ? floor_variant_e<__half, WgVariant::Packed>(a, st, per_cu) : floor_variant_e<float, WgVariant::Packed>(a, st, per_cu);
        case WgVariant::Ckpt: return f16 ? floor_variant_e<__half, WgVariant::Ckpt>(a, st, per_cu) : floor_variant_e<float, WgVariant::Ckpt>(a, st, per_cu);
        case WgVariant::PackedCkpt: return floor_pckpt(a, f16, st, per_cu);
        case WgVariant::Stream: return floor_stream(a, f16, st, per_cu);
        case WgVariant::StreamRing: return floor_stream_ring(a, f16, st, per_cu);
        default: return hipErrorInvalidValue;   // (Plain is launch_banded's)
    }
}

hipError_t launch_banded_variant(const FwdArgs& a, WgVariant v, bool f16, hipStream_t st) {
    if (!wg_variant_args_ok(a, v, 2)) return hipErrorInvalidValue;
    return floor_variant(a, v, f16, st, nullptr);
}

hipError_t banded_variant_resident(const FwdArgs& a, WgVariant v, bool f16, int* per_cu) { return floor_variant(a, v, f16, nullptr, per_cu); }

hipError_t launch_scan_selftest(const float* vals, int n_waves, int mode, float* out_v, int32_t* out_i,
                                hipStream_t st) {
    hipLaunchKernelGGL(scan_selftest_kernel, dim3(n_waves), dim3(64), 0, st, vals, mode, out_v, out_i);
    return hipGetLastError();
}

}  // namespace vit
