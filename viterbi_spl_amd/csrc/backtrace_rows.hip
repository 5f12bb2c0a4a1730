// backtrace_rows.hip -- back-trace kernels that stage whole history rows through LDS: the lean banded form and the
// generic (lazy) form for any matrix.
#include "device_common.hpp"

namespace vit {

// ---------------------------------------------------------------------------------------
// Banded back-trace, lean form: banded plan without dense rows whose forward pass left the frame maximum in
// pad column S of every history row.  Same decisions as lazy_backtrace_kernel (below), organised for the
// dependent chain of one step -- state -> two LDS reads -> add -> wave max -> compare -> lowest matching lane:
//   * lane l < W holds window candidate l, lanes W.. hold the extra-column candidates, and lane 63 forms
//     fl(max_i delta_t[i] + c_j) with the same two reads (pad column S of the row, the row-constant table), so the
//     bound that admits the fast path costs no extra instructions;
//   * the candidate table is stored per target (tabX[j][.] contiguous: conflict-free), every index is
//     wave-uniform scalar arithmetic, decided states are collected in a register and written once per tile;
//   * the full evaluation (a row-constant candidate may tie or win) is a separate, rarely taken block.
// One wave per (song, chunk) in MODE 0 / per song in MODE 1, blockDim/64 waves per workgroup share the tables.
// ---------------------------------------------------------------------------------------
constexpr int kBtVec = 12;  // float4 per lane per tile: K * SD <= 12 * 256 floats

__device__ __forceinline__ void bt_fetch(f32x4 (&stage)[kBtVec], const f32x4* __restrict__ rows, int nvec, int lane) {
#pragma unroll
    for (int v = 0; v < kBtVec; ++v) {
        const int idx = lane + v * 64;
        stage[v] = rows[idx < nvec ? idx : nvec - 1];  // clamped: always inside the tile
    }
}

// KC: candidate slots per lane (slot k of lane l holds candidate c = 64k + l; candidates: W window entries, then the
// kMaxExtras extra-column entries, then the bound fl(M_t + c_j) formed from pad column S and the row constant).
// GT: the per-target candidate table [SP][W+5] is read from the plan image in global memory (L2-resident) instead of
// LDS -- at S = 722, W = 96 it is 310 KB and does not fit; a step then waits for one L2 access (~1 us) instead of an
// LDS access, still far cheaper than evaluating whole matrix rows.
template <int NWT, bool AFF, int MODE, int KC, bool GT>
__global__ void __launch_bounds__(512) banded_backtrace_kernel(BtArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int EPL = NWT;               // sources per lane in the full evaluation, strided: i = e*64 + lane
    constexpr int TF = kBtVec * 256;       // floats per wave tile
    const int S = a.S, SP = a.SP, SD = a.SD, T = a.T, W = a.W, K = a.K;
    const int nx = a.n_extras;
    const int WX1 = W + kMaxExtras + 1;    // candidate-table row: window, extras, row constant
    const int CB = W + kMaxExtras;         // candidate index of the bound
    const int nwaves = blockDim.x >> 6;
    const float* L = reinterpret_cast<const float*>(smem);          // all LDS indices below are float indices into L
    float* tiles = reinterpret_cast<float*>(smem);                  // [nwaves][TF]
    int32_t* loL = reinterpret_cast<int32_t*>(tiles + nwaves * TF); // [SP]
    float* tabX = reinterpret_cast<float*>(loL + SP);               // [SP][WX1] (LDS form only)
    const float* __restrict__ gtab = reinterpret_cast<const float*>(a.image + a.off_tabX);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const int32_t* gl = reinterpret_cast<const int32_t*>(a.image + a.off_lo);
        const int nthr = blockDim.x;
        for (int k = tid; k < SP; k += nthr) loL[k] = gl[k];
        if (!GT)
            for (int k = tid; k < SP * WX1; k += nthr) tabX[k] = gtab[k];
    }
    __syncthreads();

    const int C = a.chunks;
    const int gw = blockIdx.x * nwaves + wv;            // global wave index
    const int song = MODE == 0 ? gw / C : gw;
    const int chunk = MODE == 0 ? gw % C : 0;
    if (song >= a.B) return;
    const int Tb = song_length(a.lengths, song, T);
    int32_t* __restrict__ states = a.states + (size_t)song * T;
    const float* __restrict__ hist = a.hist + (size_t)song * T * SD;
    float* tile = tiles + wv * TF;
    const int tile_off = wv * TF;

    // ---- per-lane constants, per candidate slot
    bool isw[KC], cand[KC];
    int pb[KC], tb[KC];
    unsigned long long wmask[KC];                                           // lanes of slot k that hold window candidates
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = 64 * k + lane;
        isw[k] = c < W;
        cand[k] = c < W + nx;
        const int xs = (c >= W && c < W + nx) ? a.extras[(c - W) & (kMaxExtras - 1)] : 0;
        pb[k] = c == CB ? a.mcol : a.col0 + (isw[k] ? c : xs);               // row entry read (window candidates: + lo)
        tb[k] = c < WX1 ? c : WX1 - 1;                                       // entry of the target's table row
        const int nwin = W - 64 * k;
        wmask[k] = nwin >= 64 ? ~0ull : (nwin <= 0 ? 0ull : ((1ull << nwin) - 1ull));
    }
    const int kb = CB >> 6, lb = CB & 63;                                    // slot / lane of the bound candidate
    const int tabX_off = (int)(tabX - tiles);
    int ic[EPL];
    bool isx[EPL], inS[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int i = e * 64 + lane;
        ic[e] = i < S ? a.col0 + i : a.col0;
        inS[e] = i < S;
        bool x = i >= S;
#pragma unroll
        for (int k = 0; k < kMaxExtras; ++k) x |= (k < nx && i == a.extras[k]);
        isx[e] = x;
    }
    const int rv = SD / 4;  // float4 per row

    // chase(top, bottom, cur, write): decide the states of frames top .. bottom (descending) from the delta rows
    // top .. bottom, starting from state `cur` at frame top+1; a tile holds rows [first, top].
    auto chase = [&](int top, const int bottom, int cur, const bool write) -> int {
        f32x4 stage[kBtVec];
        if (top >= bottom) {
            const int first = top - K + 1 > bottom ? top - K + 1 : bottom;
            bt_fetch(stage, reinterpret_cast<const f32x4*>(hist + (size_t)first * SD), (top - first + 1) * rv, lane);
        }
        while (top >= bottom) {
            const int first = top - K + 1 > bottom ? top - K + 1 : bottom;
            const int rows = top - first + 1;
#pragma unroll
            for (int v = 0; v < kBtVec; ++v) reinterpret_cast<f32x4*>(tile)[lane + v * 64] = stage[v];
            const int ntop = first - 1;
            if (ntop >= bottom) {
                const int nfirst = ntop - K + 1 > bottom ? ntop - K + 1 : bottom;
                bt_fetch(stage, reinterpret_cast<const f32x4*>(hist + (size_t)nfirst * SD), (ntop - nfirst + 1) * rv, lane);
            }
            int outv = 0;
            // MODE 1 re-chases a chunk whose assumed entry state was wrong: as soon as the new path meets the stored one the
            // rest of the chunk is already right (the step below a state depends on that state only)
            const int oldv = (MODE == 1 && lane < rows) ? states[first + lane] : -1;
            int rstop = -1;
            int row_off = __builtin_amdgcn_readfirstlane(tile_off + (rows - 1) * SD);
            for (int r = __builtin_amdgcn_readfirstlane(rows - 1); r >= 0; --r, row_off -= SD) {
                // row r of the tile = delta_t, t = first + r: decides the state at frame t from the state `cur` at t+1
                cur = __builtin_amdgcn_readfirstlane(cur);
                int lo;
                if (AFF) {
                    lo = cur - a.lo_off;
                    lo = lo < 0 ? 0 : (lo > S - W ? S - W : lo);
                } else {
                    lo = __builtin_amdgcn_readfirstlane(loL[cur]);
                }
                float v[KC], av[KC];
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const float dv = L[row_off + pb[k] + (isw[k] ? lo : 0)];
                    av[k] = GT ? gtab[(size_t)cur * WX1 + tb[k]] : L[tabX_off + (int)__umul24((unsigned)cur, (unsigned)WX1) + tb[k]];
                    v[k] = dv + av[k];
                }
                // the bound candidate: fl(max_i delta_t[i] + c_cur), on every row-constant candidate
                float mf = 0.f, cj = 0.f;
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (KC == 1 || k == kb) {
                        mf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), lb));
                        cj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(av[k]), lb));
                    }
                float mloc = -INFINITY;
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    v[k] = cand[k] ? v[k] : -INFINITY;
                    mloc = fmaxf(mloc, v[k]);
                }
                const float m = wave_max_all(mloc);
                // lowest source index among the window / extra-column candidates equal to `mm`
                auto lowest_candidate = [&](const float mm) -> unsigned {
                    unsigned best = 0x7fffffffu;
                    bool have_w = false;
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
                        const unsigned long long mk = __ballot(v[k] == mm && cand[k]);
                        const unsigned long long mw = mk & wmask[k];
                        if (mw && !have_w) {                                 // window candidates ascend with the source index
                            const unsigned c = lo + 64 * k + __builtin_ctzll(mw);
                            best = c < best ? c : best;
                            have_w = true;
                        }
                        unsigned long long mx = mk & ~wmask[k];              // extra-column candidates: arbitrary indices
                        while (mx) {
                            const unsigned c = __builtin_amdgcn_readlane(pb[k], __builtin_ctzll(mx)) - a.col0;   // column -> state
                            best = c < best ? c : best;
                            mx &= mx - 1;
                        }
                    }
                    return best;
                };
                unsigned idx = 0x7fffffffu;
                if (mf < m) {
                    // ---- common case: no row-constant candidate can tie or win
                    idx = lowest_candidate(m);
                } else {
                    // ---- full evaluation: every source outside the window / extras contributes fl(delta_t[i] + c_cur)
                    float vf[EPL];
                    float m2 = -INFINITY;
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        const int i = e * 64 + lane;
                        const float d = L[row_off + ic[e]];
                        const bool excl = isx[e] || (unsigned)(i - lo) < (unsigned)W;
                        vf[e] = excl ? -INFINITY : d + cj;
                        m2 = fmaxf(m2, vf[e]);
                    }
                    const float mm = fmaxf(m, wave_max_all(m2));
                    // lowest index among the candidates equal to the max (an all -inf frame resolves to index 0
                    // like np.argmax: every in-range source then matches)
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        const unsigned long long mk = __ballot(vf[e] == mm && inS[e]);
                        if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
                    }
                    const unsigned c = lowest_candidate(mm);
                    idx = c < idx ? c : idx;
                    if (idx == 0x7fffffffu) idx = 0;
                }
                cur = (int)idx;
                outv = lane == r ? cur : outv;
                if (MODE == 1 && cur == __builtin_amdgcn_readlane(oldv, r)) { rstop = r; break; }
            }
            if (write && lane < rows && lane > rstop) states[first + lane] = outv;
            if (MODE == 1 && rstop >= 0) return __builtin_amdgcn_readfirstlane(states[bottom]);   // the stored path continues unchanged
            top = ntop;
        }
        return cur;
    };

    // Chunking, speculative warm-up and verification exactly as in lazy_backtrace_kernel.
    const int Lf = Tb - 1;
    if (MODE == 0) {
        const int lo_c = (int)((long long)Lf * chunk / C), hi_c = (int)((long long)Lf * (chunk + 1) / C);
        if (chunk == C - 1) {
            for (int t = Tb + lane; t < T; t += 64) states[t] = -1;
            if (lane == 0) states[Tb - 1] = a.last_state[song];
        }
        int top = hi_c - 1 + a.warm;
        int cur;
        if (chunk == C - 1 || top >= Lf - 1) {
            top = Lf - 1;
            cur = __builtin_amdgcn_readfirstlane(a.last_state[song]);
        } else {
            // guess: lowest-index argmax of delta row top+1
            const float* g = hist + (size_t)(top + 1) * SD + a.col0;
            float d[EPL];
            float m = -INFINITY;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                d[e] = inS[e] ? g[e * 64 + lane] : -INFINITY;
                m = fmaxf(m, d[e]);
            }
            m = wave_max_all(m);
            unsigned idx = 0x7fffffffu;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const unsigned long long mk = __ballot(d[e] == m && inS[e]);
                if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
            }
            cur = idx == 0x7fffffffu ? 0 : (int)idx;
        }
        if (hi_c <= lo_c) {                       // empty chunk (very short song)
            if (lane == 0) a.entry[(size_t)song * C + chunk] = cur;
            return;
        }
        cur = chase(top, hi_c, cur, false);       // warm-up: frames top .. hi_c, nothing written
        if (lane == 0) a.entry[(size_t)song * C + chunk] = cur;   // state this chunk assumed at frame hi_c
        chase(hi_c - 1, lo_c, cur, true);
    } else {
        int truth = -1;                           // verified state at frame hi_c of the chunk being checked
        for (int c = C - 2; c >= 0; --c) {
            const int lo_c = (int)((long long)Lf * c / C), hi_c = (int)((long long)Lf * (c + 1) / C);
            if (truth < 0) truth = __builtin_amdgcn_readfirstlane(states[hi_c]);
            const int assumed = __builtin_amdgcn_readfirstlane(a.entry[(size_t)song * C + c]);
            if (hi_c > lo_c && assumed != truth) {
                truth = chase(hi_c - 1, lo_c, truth, true);   // re-chase from the true state; ends at frame lo_c
            } else {
                truth = -1;                       // chunk c stands: its frame lo_c is already in `states`
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Lazy back-trace: one wave per song (kBtWaves songs per workgroup share the LDS tables).
// For frame t (descending) and the path state j at t+1 it rebuilds the candidates of target j
//   fl(delta_t[i] + logA_T[j][i])   for every source i
// from the stored delta row (window / c0 floor / extra columns / dense row, or the full matrix
// row for unstructured matrices), takes the max over the wave and picks the LOWEST index
// attaining it (v_cmp_eq lane masks + s_ff1).  Delta rows are staged through LDS in tiles of K
// frames; the next tile is in flight in registers while the current one is chased.
// ---------------------------------------------------------------------------------------
constexpr int kBtWaves = 4;

// MODE 0: speculative pass, one wave per (song, chunk).  MODE 1: verify pass, one wave per song.
// PK: packed batch (vit_decode_packed for plans the lane form does not serve).  MODE 0 runs one wave per entry of wave_song; song b
// owns the waves and the chunk entries chunk_base[b] .. chunk_base[b+1]-1, so its chunk count grows with its length; its history
// rows and states sit at row offsets[b] of the packed buffers and there are no frames past its end to fill.
// SG: one segment of a checkpointed decode (vit_decode_checkpointed for step plans), in both passes what the sparse and lane kernels
// do: the song's history rows start at row song * hist_rows (the segment buffer), its states at song * states_stride (the segment's
// first frame within the whole song's row), and a song whose lengths[] entry is < 1 (skip_nonpositive: the segment does not reach it)
// is skipped, not clamped to one frame.  With a.unit_states the sub-problems are the segment units of a packed checkpointed decode
// (vit_decode_packed_bounded): the states of sub-problem b start at states + unit_states[b], and nothing is written behind its
// lengths[b] frames -- those entries belong to the next song.  PK = SG = false compiles to the code it was before the parameters existed.
template <int NWT, int MODE, bool PK = false, bool SG = false>
__global__ void __launch_bounds__(kBtWaves * 64) lazy_backtrace_kernel(BtArgs a) {
    static_assert(!(PK && SG), "a segment is a segment of a padded batch");
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int EPL = NWT;               // sources per lane, strided: i = e*64 + lane
    const int S = a.S, SP = a.SP, SD = a.SD, T = a.T, W = a.W, K = a.K;
    const bool banded = a.banded != 0;
    const int nx = a.n_extras, nd = a.n_dense;
    const int WX = W + nx;                  // window candidates + extra-column candidates, one per lane
    const bool fast_ok = banded && a.have_fmax && WX <= 64;
    // LDS: [tile per wave: kBtVec*64 float4][out per wave: 64 ints]
    //      [tables: lo, kind, rowc, tabX[j][.] = the W window entries then the extra-column entries of target j]
    f32x4* tiles = reinterpret_cast<f32x4*>(smem);
    int32_t* outs = reinterpret_cast<int32_t*>(tiles + kBtWaves * kBtVec * 64);
    int32_t* loL = outs + kBtWaves * 64;
    int32_t* kindL = loL + SP;
    float* rowcL = reinterpret_cast<float*>(kindL + SP);  // [SP] row constants
    float* tabX = rowcL + SP;                             // [SP][WXS]: one target's candidates are contiguous (lane l reads entry l: no bank conflicts)
    const int WXS = W + kMaxExtras;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform for the compiler
    // step-structured dense matrix (plan.step_ok): the (step_kb+1) x SP band table replaces the matrix rows in LDS
    float* stepL = reinterpret_cast<float*>(loL);
    const bool step = !banded && a.step_ok != 0;
    if (step) {
        const float* gs = reinterpret_cast<const float*>(a.image + a.off_stepC);
        for (int k = tid; k < (a.step_kb + 1) * SP; k += kBtWaves * 64) stepL[k] = gs[k];
    }
    if (banded) {
        const int32_t* gl = reinterpret_cast<const int32_t*>(a.image + a.off_lo);
        const int32_t* gk = reinterpret_cast<const int32_t*>(a.image + a.off_kind);
        const float* gx = reinterpret_cast<const float*>(a.image + a.off_extraA);
        const float* gt = reinterpret_cast<const float*>(a.image + a.off_tabA);
        const float* gc = reinterpret_cast<const float*>(a.image + a.off_rowc);
        for (int k = tid; k < SP; k += kBtWaves * 64) { loL[k] = gl[k]; kindL[k] = gk[k]; rowcL[k] = gc[k]; }
        for (int k = tid; k < W * SP; k += kBtWaves * 64) tabX[(k % SP) * WXS + k / SP] = gt[k];
        for (int k = tid; k < kMaxExtras * SP; k += kBtWaves * 64) tabX[(k % SP) * WXS + W + k / SP] = gx[k];
    }
    __syncthreads();

    const int gw = blockIdx.x * kBtWaves + wv;          // global wave index
    if (PK && MODE == 0 && gw >= a.n_waves) return;
    const int song = PK ? (MODE == 0 ? a.wave_song[gw] : gw) : (MODE == 0 ? gw / a.chunks : gw);
    if (song >= a.B) return;
    const int cbase = PK ? a.chunk_base[song] : 0;
    const int C = PK ? a.chunk_base[song + 1] - cbase : a.chunks;
    const int chunk = MODE == 0 ? (PK ? gw - cbase : gw % C) : 0;
    if constexpr (SG) {
        if (a.skip_nonpositive && a.lengths[song] < 1) return;          // segment of a checkpointed decode this song does not reach
    }
    const long long row0 = PK ? a.offsets[song] : (long long)song * T;  // first history row / state of the song
    const int Tb = PK ? (int)(a.offsets[song + 1] - row0) : song_length(a.lengths, song, T);
    const int Tpad = PK || (SG && a.unit_states) ? Tb : T;   // frames past the song's end are filled with -1 up to here
    int32_t* __restrict__ states = a.states + (SG ? (a.unit_states ? (size_t)a.unit_states[song] : (size_t)song * (size_t)a.states_stride) : (size_t)row0);
    const float* __restrict__ hist = a.hist + (SG ? (size_t)song * (size_t)a.hist_rows : (size_t)row0) * SD;
    int32_t* __restrict__ entry = a.entry + (PK ? (size_t)cbase : (size_t)song * C);   // [C] of this song
    const float* __restrict__ Arow = reinterpret_cast<const float*>(a.image + a.off_Arow);
    float* tile = reinterpret_cast<float*>(tiles + wv * kBtVec * 64);
    int32_t* out = outs + wv * 64;


    // loop invariants
    float dA[kMaxDenseRows][EPL];
    bool isx[EPL];                          // source excluded from the c0 floor: extra column or padding
    {
        const float* __restrict__ daT = reinterpret_cast<const float*>(a.image + a.off_denseA);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int i = e * 64 + lane;
            bool x = i >= S;
#pragma unroll
            for (int k = 0; k < kMaxExtras; ++k) x |= (k < nx && i == a.extras[k]);
            isx[e] = x;
#pragma unroll
            for (int d = 0; d < kMaxDenseRows; ++d)
                dA[d][e] = (banded && d < nd && i < S) ? daT[(size_t)d * SP + i] : -INFINITY;
        }
    }
    // fast path: lane l < W evaluates window source lo + l, lane W + k evaluates extra column k
    const int xsrc = (lane >= W && lane < WX) ? a.extras[(lane - W) & (kMaxExtras - 1)] : 0;
    const unsigned long long wmask = W >= 64 ? ~0ull : ((1ull << W) - 1ull);

    // chase(top, bottom, cur, write): decide the states of frames top .. bottom (descending) from the
    // delta rows top .. bottom, starting from state `cur` at frame top+1; a tile holds rows [first, top].
    const int rv = SD / 4;  // float4 per row
    auto chase = [&](int top, const int bottom, int cur, const bool write) -> int {
    f32x4 stage[kBtVec];
    if (top >= bottom) {
        const int first = top - K + 1 > bottom ? top - K + 1 : bottom;
        bt_fetch(stage, reinterpret_cast<const f32x4*>(hist + (size_t)first * SD), (top - first + 1) * rv, lane);
    }
    while (top >= bottom) {
        const int first = top - K + 1 > bottom ? top - K + 1 : bottom;
        const int rows = top - first + 1;
#pragma unroll
        for (int v = 0; v < kBtVec; ++v) reinterpret_cast<f32x4*>(tile)[lane + v * 64] = stage[v];
        const int ntop = first - 1;
        if (ntop >= bottom) {
            const int nfirst = ntop - K + 1 > bottom ? ntop - K + 1 : bottom;
            bt_fetch(stage, reinterpret_cast<const f32x4*>(hist + (size_t)nfirst * SD), (ntop - nfirst + 1) * rv, lane);
        }
        const int oldv = (MODE == 1 && lane < rows) ? states[first + lane] : -1;   // see banded_backtrace_kernel
        int rstop = -1;
        for (int r = rows - 1; r >= 0; --r) {
            const float* row = tile + r * SD + a.col0;   // delta_t, t = first + r; decides the state at frame t
            const int jj = __builtin_amdgcn_readfirstlane(cur);  // path state at frame t+1 (wave-uniform)
            int lo = 0;
            int kd = -3;                         // -3 unstructured plan, -1 banded row, >= 0 dense row
            if (banded) {
                if (a.lo_affine) {
                    lo = jj - a.lo_off;
                    lo = lo < 0 ? 0 : (lo > S - W ? S - W : lo);
                    kd = -1;
#pragma unroll
                    for (int d = 0; d < kMaxDenseRows; ++d) kd = (d < nd && jj == a.dense_rows[d]) ? d : kd;
                } else {
                    kd = __builtin_amdgcn_readfirstlane(kindL[jj]);
                    lo = __builtin_amdgcn_readfirstlane(loL[jj]);
                }
            }
            bool done = false;
            if (fast_ok && kd == -1) {
                // ---- common case: only the window + extra-column candidates of target jj
                const int src = lane < W ? lo + lane : xsrc;
                float v = -INFINITY;
                if (lane < WX) v = row[src] + tabX[jj * WXS + lane];
                const float m = wave_max_all(v);
                const float mf = tile[r * SD + a.mcol] + rowcL[jj];  // column mcol >= max_i delta_t[i] over the row-constant sources: fl(. + c_jj) bounds every row-constant candidate
                if (mf < m) {                    // no row-constant candidate can tie or win
                    const unsigned long long mk = __ballot(v == m);
                    unsigned idx = 0x7fffffffu;
                    if (mk & wmask) idx = lo + __builtin_ctzll(mk & wmask);   // window lanes ascend with the source index
                    unsigned long long mx = W >= 64 ? 0ull : (mk >> W);       // extra-column lanes: arbitrary indices
                    while (mx) {
                        const unsigned c = a.extras[__builtin_ctzll(mx) & (kMaxExtras - 1)];
                        idx = c < idx ? c : idx;
                        mx &= mx - 1;
                    }
                    cur = (int)idx;
                    done = true;
                }
            }
            if (!done) {
                // ---- full evaluation: every source (c0 floor / window / extras / dense row / matrix row)
                float d[EPL], vf[EPL];
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int i = e * 64 + lane;
                    d[e] = i < S ? row[i] : -INFINITY;
                }
                float vw = -INFINITY;
                if (kd == -1) {
                    const float cjj = rowcL[jj];
                    const int src = lane < W ? lo + lane : xsrc;
                    if (lane < WX) vw = row[src] + tabX[jj * WXS + lane];
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        const int i = e * 64 + lane;
                        // window sources lo .. lo+63 are the lanes of vw; a wider window (W = 96, 128) continues here with
                        // its table entries; everything else outside the extra columns carries the row constant
                        const unsigned wi = (unsigned)(i - lo);
                        const bool in_vw = wi < (unsigned)(W < 64 ? W : 64);
                        const float wgt = (wi < (unsigned)W && !in_vw) ? tabX[jj * WXS + (int)wi] : cjj;
                        vf[e] = (isx[e] || in_vw) ? -INFINITY : d[e] + wgt;
                    }
                    if (WX > 64) {  // extras did not fit beside the window: fold them into the strided part
#pragma unroll
                        for (int e = 0; e < EPL; ++e) {
                            const int i = e * 64 + lane;
#pragma unroll
                            for (int k = 0; k < kMaxExtras; ++k)
                                if (k < nx && i == a.extras[k]) vf[e] = d[e] + tabX[jj * WXS + W + k];
                        }
                    }
                } else if (kd >= 0) {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        float av = dA[0][e];
#pragma unroll
                        for (int q = 1; q < kMaxDenseRows; ++q) av = kd == q ? dA[q][e] : av;
                        vf[e] = d[e] + av;
                    }
                } else if (step && jj < S - 1) {
                    // voiced target of a step matrix: logA_T[jj][i] = stepC[min(|i-jj| / bw, kb)][i], unvoiced source: step_cn
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        const int i = e * 64 + lane;
                        const unsigned dist = (unsigned)(i > jj ? i - jj : jj - i);
                        unsigned band = (dist * (unsigned)a.step_mult) >> 16;          // dist / step_bw (host-checked for dist < 1024)
                        band = band < (unsigned)a.step_kb ? band : (unsigned)a.step_kb;
                        const float wgt = i < S - 1 ? stepL[band * SP + i] : (i == S - 1 ? a.step_cn : -INFINITY);
                        vf[e] = i < S ? d[e] + wgt : -INFINITY;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        const int i = e * 64 + lane;
                        vf[e] = i < S ? d[e] + Arow[(size_t)jj * SP + i] : -INFINITY;
                    }
                }
                float m = vw;
#pragma unroll
                for (int e = 0; e < EPL; ++e) m = fmaxf(m, vf[e]);
                m = wave_max_all(m);
                // lowest index among the candidates equal to the max (an all -inf frame resolves to
                // index 0 like np.argmax: every in-range source then matches)
                unsigned idx = 0x7fffffffu;
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const unsigned long long mk = __ballot(vf[e] == m && e * 64 + lane < S);
                    if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
                }
                if (kd == -1) {
                    const unsigned long long mk = __ballot(vw == m && lane < WX);
                    if (mk & wmask) { const unsigned c = lo + __builtin_ctzll(mk & wmask); idx = c < idx ? c : idx; }
                    unsigned long long mx = (W >= 64 || WX > 64) ? 0ull : (mk >> W);
                    while (mx) {
                        const unsigned c = a.extras[__builtin_ctzll(mx) & (kMaxExtras - 1)];
                        idx = c < idx ? c : idx;
                        mx &= mx - 1;
                    }
                }
                cur = idx == 0x7fffffffu ? 0 : (int)idx;
            }
            if (lane == 0) out[r] = cur;
            if (MODE == 1 && cur == __builtin_amdgcn_readlane(oldv, __builtin_amdgcn_readfirstlane(r))) { rstop = r; break; }
        }
        if (write)
            for (int r = lane; r < rows; r += 64)
                if (r > rstop) states[first + r] = out[r];
        if (MODE == 1 && rstop >= 0) return __builtin_amdgcn_readfirstlane(states[bottom]);
        top = ntop;
    }
    return cur;
    };

    // Frames 0 .. Tb-2 are decided (frame Tb-1 is the terminal state).  They are split into C chunks
    // [lo_c, hi_c); chunk c is chased from a warm-up point `a.warm` frames above hi_c, starting from
    // the best state of that frame (a guess); survivor paths coalesce, and MODE 1 verifies that the
    // state chunk c reached at frame hi_c equals what chunk c+1 (already verified) decided there --
    // if not, the chunk is chased again from the true state.  The result is exact either way.
    const int L = Tb - 1;
    if (MODE == 0) {
        const int lo_c = (int)((long long)L * chunk / C), hi_c = (int)((long long)L * (chunk + 1) / C);
        if (chunk == C - 1) {
            for (int t = Tb + lane; t < Tpad; t += 64) states[t] = -1;
            if (lane == 0) states[Tb - 1] = a.last_state[song];
        }
        int top = hi_c - 1 + a.warm;
        int cur;
        if (chunk == C - 1 || top >= L - 1) {
            top = L - 1;
            cur = __builtin_amdgcn_readfirstlane(a.last_state[song]);
        } else {
            // guess: lowest-index argmax of delta row top+1
            const float* g = hist + (size_t)(top + 1) * SD + a.col0;
            float d[EPL];
            float m = -INFINITY;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int i = e * 64 + lane;
                d[e] = i < S ? g[i] : -INFINITY;
                m = fmaxf(m, d[e]);
            }
            m = wave_max_all(m);
            unsigned idx = 0x7fffffffu;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const unsigned long long mk = __ballot(d[e] == m && e * 64 + lane < S);
                if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
            }
            cur = idx == 0x7fffffffu ? 0 : (int)idx;
        }
        if (hi_c <= lo_c) {                       // empty chunk (very short song)
            if (lane == 0) entry[chunk] = cur;
            return;
        }
        cur = chase(top, hi_c, cur, false);       // warm-up: frames top .. hi_c, nothing written
        if (lane == 0) entry[chunk] = cur;   // state this chunk assumed at frame hi_c
        chase(hi_c - 1, lo_c, cur, true);
    } else {
        int truth = -1;                           // verified state at frame hi_c of the chunk being checked
        for (int c = C - 2; c >= 0; --c) {
            const int lo_c = (int)((long long)L * c / C), hi_c = (int)((long long)L * (c + 1) / C);
            if (truth < 0) truth = __builtin_amdgcn_readfirstlane(states[hi_c]);
            const int assumed = __builtin_amdgcn_readfirstlane(entry[c]);
            if (hi_c > lo_c && assumed != truth) {
                truth = chase(hi_c - 1, lo_c, truth, true);   // re-chase from the true state; ends at frame lo_c
            } else {
                truth = -1;                       // chunk c stands: its frame lo_c is already in `states`
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
int backtrace_tile_rows(int SD) {
    int k = (kBtVec * 256) / SD;
    return k > 64 ? 64 : (k < 1 ? 1 : k);
}
template <int NWT, bool AFF, int KC, bool GT>
static hipError_t launch_bt_lean(const BtArgs& a, int nwaves, size_t lds, hipStream_t st) {
    const long long waves0 = (long long)a.B * a.chunks;
    hipLaunchKernelGGL((banded_backtrace_kernel<NWT, AFF, 0, KC, GT>), dim3((int)((waves0 + nwaves - 1) / nwaves)), dim3(nwaves * 64), lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.chunks <= 1) return e;
    hipLaunchKernelGGL((banded_backtrace_kernel<NWT, AFF, 1, KC, GT>), dim3((int)((a.B + nwaves - 1) / nwaves)), dim3(nwaves * 64), lds, st, a);
    return hipGetLastError();
}

template <int NWT, int KC, bool GT>
static hipError_t launch_bt_lean_a(const BtArgs& a, int nwaves, size_t lds, hipStream_t st) {
    return a.lo_affine ? launch_bt_lean<NWT, true, KC, GT>(a, nwaves, lds, st) : launch_bt_lean<NWT, false, KC, GT>(a, nwaves, lds, st);
}

template <int NWT>
static hipError_t launch_bt_t(BtArgs a, hipStream_t st) {
    // lean kernel: banded plan, no dense rows, frame maxima stored by the forward pass
    if constexpr (NWT <= 12) {
        if (a.banded && a.have_fmax && a.n_dense == 0 && a.W <= 128 && a.bt_form != 1) {
            const int kc = (a.W + kMaxExtras + 1 + 63) / 64;
            const size_t tile = sizeof(f32x4) * kBtVec * 64, lo_tab = sizeof(int32_t) * a.SP;
            const size_t table = sizeof(float) * (size_t)a.SP * (a.W + kMaxExtras + 1);
            // candidate table in LDS when it leaves room for at least four waves, else read from the image (L2)
            if (kc == 1 && 4 * tile + lo_tab + table + 1024 <= kLdsBytes) {
                const int nw = 8 * tile + lo_tab + table + 1024 <= kLdsBytes ? 8 : 4;
                return launch_bt_lean_a<NWT, 1, false>(a, nw, nw * tile + lo_tab + table, st);
            }
            const size_t lds = 8 * tile + lo_tab;
            if (kc == 1) return launch_bt_lean_a<NWT, 1, true>(a, 8, lds, st);
            if (kc == 2) return launch_bt_lean_a<NWT, 2, true>(a, 8, lds, st);
            if (kc == 3) return launch_bt_lean_a<NWT, 3, true>(a, 8, lds, st);
        }
    }
    size_t lds = sizeof(f32x4) * kBtWaves * kBtVec * 64 + sizeof(int32_t) * kBtWaves * 64;
    if (!a.banded && a.step_ok) lds += sizeof(float) * (a.step_kb + 1) * a.SP;
    if (a.banded) {
        const size_t tables = sizeof(int32_t) * 2 * a.SP + sizeof(float) * (1 + kMaxExtras + a.W) * a.SP;
        if (lds + tables + 1024 > kLdsBytes) {   // tables do not fit: evaluate full matrix rows instead (exact, slower)
            a.banded = 0;
            a.have_fmax = 0;
        } else {
            lds += tables;
        }
    }
    const long long waves0 = (long long)a.B * a.chunks;
    hipLaunchKernelGGL((lazy_backtrace_kernel<NWT, 0>), dim3((int)((waves0 + kBtWaves - 1) / kBtWaves)), dim3(kBtWaves * 64),
                       lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.chunks <= 1) return e;
    hipLaunchKernelGGL((lazy_backtrace_kernel<NWT, 1>), dim3((int)((a.B + kBtWaves - 1) / kBtWaves)), dim3(kBtWaves * 64),
                       lds, st, a);
    return hipGetLastError();
}

hipError_t launch_backtrace_rows_packed(BtArgs a, hipStream_t st) {
    if (!a.offsets || !a.wave_song || !a.chunk_base || a.n_waves < 1 || a.chunks < 1 || a.chunks > kBtMaxChunks) return hipErrorInvalidValue;
    if (a.banded) return hipErrorInvalidConfiguration;         // (banded plans take the lane form)
    a.K = backtrace_tile_rows(a.SD);
    a.have_fmax = 0;
    size_t lds = sizeof(f32x4) * kBtWaves * kBtVec * 64 + sizeof(int32_t) * kBtWaves * 64;
    if (a.step_ok) lds += sizeof(float) * (a.step_kb + 1) * a.SP;
    const int nwt = (a.S + 63) / 64;
    const dim3 g0((unsigned)((a.n_waves + kBtWaves - 1) / kBtWaves)), g1((unsigned)((a.B + kBtWaves - 1) / kBtWaves)), blk(kBtWaves * 64);
    if (nwt > 16) return hipErrorInvalidConfiguration;
    if (nwt <= 12) hipLaunchKernelGGL((lazy_backtrace_kernel<12, 0, true>), g0, blk, lds, st, a);
    else hipLaunchKernelGGL((lazy_backtrace_kernel<16, 0, true>), g0, blk, lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.chunks <= 1) return e;
    if (nwt <= 12) hipLaunchKernelGGL((lazy_backtrace_kernel<12, 1, true>), g1, blk, lds, st, a);
    else hipLaunchKernelGGL((lazy_backtrace_kernel<16, 1, true>), g1, blk, lds, st, a);
    return hipGetLastError();
}

hipError_t launch_backtrace_rows_segment(BtArgs a, hipStream_t st) {
    if (!a.lengths || a.offsets || a.hist_rows < a.T || a.chunks < 1 || a.chunks > kBtMaxChunks) return hipErrorInvalidValue;
    if (a.banded) return hipErrorInvalidConfiguration;         // (banded plans take the sparse or the lane form)
    a.K = backtrace_tile_rows(a.SD);
    a.have_fmax = 0;
    size_t lds = sizeof(f32x4) * kBtWaves * kBtVec * 64 + sizeof(int32_t) * kBtWaves * 64;
    if (a.step_ok) lds += sizeof(float) * (a.step_kb + 1) * a.SP;
    const int nwt = (a.S + 63) / 64;
    const long long waves0 = (long long)a.B * a.chunks;
    const dim3 g0((unsigned)((waves0 + kBtWaves - 1) / kBtWaves)), g1((unsigned)((a.B + kBtWaves - 1) / kBtWaves)), blk(kBtWaves * 64);
    if (nwt > 16) return hipErrorInvalidConfiguration;
    if (nwt <= 12) hipLaunchKernelGGL((lazy_backtrace_kernel<12, 0, false, true>), g0, blk, lds, st, a);
    else hipLaunchKernelGGL((lazy_backtrace_kernel<16, 0, false, true>), g0, blk, lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.chunks <= 1) return e;
    if (nwt <= 12) hipLaunchKernelGGL((lazy_backtrace_kernel<12, 1, false, true>), g1, blk, lds, st, a);
    else hipLaunchKernelGGL((lazy_backtrace_kernel<16, 1, false, true>), g1, blk, lds, st, a);
    return hipGetLastError();
}

int backtrace_chunks(int64_t B, int T) {
    // enough (song, chunk) waves to cover the chip twice over, chunks no shorter than ~8 warm-ups
    long long c = (2 * 1024 + B - 1) / (B > 0 ? B : 1);
    const long long cmax = T / (8 * kBtWarm) > 1 ? T / (8 * kBtWarm) : 1;
    c = c > cmax ? cmax : c;
    c = c > kBtMaxChunks ? kBtMaxChunks : c;
    return c < 1 ? 1 : (int)c;
}

hipError_t launch_backtrace(BtArgs a, hipStream_t st) {
    if (a.bt_form == 0 && sparse_backtrace_applies(a)) return launch_backtrace_sparse(a, st);
    a.K = backtrace_tile_rows(a.SD);
    const int nwt = (a.S + 63) / 64;
    if (nwt <= 2) return launch_bt_t<2>(a, st);
    if (nwt <= 4) return launch_bt_t<4>(a, st);
    if (nwt <= 6) return launch_bt_t<6>(a, st);
    if (nwt <= 8) return launch_bt_t<8>(a, st);
    if (nwt <= 12) return launch_bt_t<12>(a, st);
    return launch_bt_t<16>(a, st);
}

}  // namespace vit
