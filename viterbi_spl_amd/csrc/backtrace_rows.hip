// backtrace_rows.hip -- back-trace kernels that stage whole history rows through LDS: the lean banded form and the
// generic (lazy) form for any matrix.  Each kernel is its chase() over LDS tiles; the chunk scheme around it is the shared
// bt_run_chunks (backtrace_common.hpp), and the lean kernel takes its candidate slots, lowest_candidate and full evaluation
// from there too (the lazy kernel's full evaluation -- dense rows, step and unstructured matrices -- is its own).
#include "backtrace_common.hpp"

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
    const BtSlots<KC> sl(a, lane);
    const auto& isw = sl.isw;
    const auto& cand = sl.cand;
    const auto& tb = sl.tb;
    int pb[KC];                                                              // row entry read (window candidates: + lo)
#pragma unroll
    for (int k = 0; k < KC; ++k) pb[k] = 64 * k + lane == CB ? a.mcol : a.col0 + (isw[k] ? 64 * k + lane : sl.xs[k]);
    const int kb = CB >> 6, lb = CB & 63;                                    // slot / lane of the bound candidate
    const int tabX_off = (int)(tabX - tiles);
    const BtSourceFlags<EPL> src(a, lane);
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
                // common case: no row-constant candidate can tie or win; else the full evaluation
                // (pb, col0: the extra-column lanes of the row entries are col0 + the candidate's state)
                auto row = [&](const int e) { return src.inS[e] ? L[row_off + a.col0 + e * 64 + lane] : -INFINITY; };
                const unsigned idx = mf < m ? bt_lowest_candidate<KC>(sl, v, m, lo, 0.f, 0ull, pb, a.col0)
                                            : bt_full_row<EPL, KC>(src, sl, v, row, cj, m, lo, W, lane, 0ull, pb, a.col0);
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

    bt_run_chunks<MODE, EPL>(chase, [&](const int f) { return hist + (size_t)f * SD + a.col0; }, states, a.entry + (size_t)song * C,
                             MODE == 0 ? a.last_state[song] : 0, Tb, T, chunk, C, a.warm, S, lane);
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

    // (PK / SG only decide which pointers and limits the chunk scheme gets)
    bt_run_chunks<MODE, EPL>(chase, [&](const int f) { return hist + (size_t)f * SD + a.col0; }, states, entry,
                             MODE == 0 ? a.last_state[song] : 0, Tb, Tpad, chunk, C, a.warm, S, lane);
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
int backtrace_tile_rows(int SD) {
    int k = (kBtVec * 256) / SD;
    return k > 64 ? 64 : (k < 1 ? 1 : k);
}
template <int NWT, int KC, bool GT>
static hipError_t launch_bt_lean_a(const BtArgs& a, int nwaves, size_t lds, hipStream_t st) {
    return bt_dispatch_bool(a.lo_affine != 0, [&](auto aff) {
        return launch_two_pass(banded_backtrace_kernel<NWT, decltype(aff)::value, 0, KC, GT>, banded_backtrace_kernel<NWT, decltype(aff)::value, 1, KC, GT>,
                               (long long)a.B * a.chunks, a.B, nwaves, lds, st, a);
    });
}

// LDS bytes of the lazy kernel: tiles and decided states of its waves, the step table of a step plan, and (tables) the row
// tables of a banded plan
static size_t lazy_lds_bytes(const BtArgs& a, bool tables) {
    size_t lds = sizeof(f32x4) * kBtWaves * kBtVec * 64 + sizeof(int32_t) * kBtWaves * 64;
    if (!a.banded && a.step_ok) lds += sizeof(float) * (a.step_kb + 1) * a.SP;
    if (tables) lds += sizeof(int32_t) * 2 * a.SP + sizeof(float) * (1 + kMaxExtras + a.W) * a.SP;
    return lds;
}

template <int NWT>
static hipError_t launch_bt_t(BtArgs a, hipStream_t st) {
    // lean kernel: banded plan, no dense rows, frame maxima stored by the forward pass, at most three candidates per lane
    // (W <= 128 gives kc <= 3 with today's kMaxExtras; anything wider falls through to the lazy kernel)
    if constexpr (NWT <= 12) {
        const int kc = (a.W + kMaxExtras + 1 + 63) / 64;
        if (a.banded && a.have_fmax && a.n_dense == 0 && a.W <= 128 && kc <= 3 && a.bt_form != 1) {
            const size_t tile = sizeof(f32x4) * kBtVec * 64, lo_tab = sizeof(int32_t) * a.SP;
            const size_t table = sizeof(float) * (size_t)a.SP * (a.W + kMaxExtras + 1);
            // candidate table in LDS when it leaves room for at least four waves, else read from the image (L2)
            if (kc == 1 && 4 * tile + lo_tab + table + 1024 <= kLdsBytes) {
                const int nw = 8 * tile + lo_tab + table + 1024 <= kLdsBytes ? 8 : 4;
                return launch_bt_lean_a<NWT, 1, false>(a, nw, nw * tile + lo_tab + table, st);
            }
            return bt_dispatch_upto<1, 2, 3>(kc, [&](auto k) { return launch_bt_lean_a<NWT, decltype(k)::value, true>(a, 8, 8 * tile + lo_tab, st); });
        }
    }
    size_t lds = lazy_lds_bytes(a, false);
    if (a.banded) {
        if (lazy_lds_bytes(a, true) + 1024 > kLdsBytes) {   // tables do not fit: evaluate full matrix rows instead (exact, slower)
            a.banded = 0;
            a.have_fmax = 0;
        } else {
            lds = lazy_lds_bytes(a, true);
        }
    }
    return launch_two_pass(lazy_backtrace_kernel<NWT, 0>, lazy_backtrace_kernel<NWT, 1>, (long long)a.B * a.chunks, a.B, kBtWaves, lds, st, a);
}

// the lazy kernel over a packed batch (PK) or over one segment of a checkpointed decode (!PK): plans that are not banded
template <bool PK>
static hipError_t launch_rows_lazy(BtArgs a, hipStream_t st) {
    a.K = backtrace_tile_rows(a.SD);
    a.have_fmax = 0;
    const size_t lds = lazy_lds_bytes(a, false);
    const int nwt = (a.S + 63) / 64;
    if (nwt > 16) return hipErrorInvalidConfiguration;
    const long long waves0 = PK ? (long long)a.n_waves : (long long)a.B * a.chunks;
    return bt_dispatch_upto<12, 16>(nwt, [&](auto n) {
        return launch_two_pass(lazy_backtrace_kernel<decltype(n)::value, 0, PK, !PK>, lazy_backtrace_kernel<decltype(n)::value, 1, PK, !PK>, waves0, a.B,
                               kBtWaves, lds, st, a);
    });
}

hipError_t launch_backtrace_rows_packed(BtArgs a, hipStream_t st) {
    if (!a.offsets || !a.wave_song || !a.chunk_base || a.n_waves < 1 || a.chunks < 1 || a.chunks > kBtMaxChunks) return hipErrorInvalidValue;
    if (a.banded) return hipErrorInvalidConfiguration;         // (banded plans take the lane form)
    return launch_rows_lazy<true>(a, st);
}

hipError_t launch_backtrace_rows_segment(BtArgs a, hipStream_t st) {
    if (!a.lengths || a.offsets || a.hist_rows < a.T || a.chunks < 1 || a.chunks > kBtMaxChunks) return hipErrorInvalidValue;
    if (a.banded) return hipErrorInvalidConfiguration;         // (banded plans take the sparse or the lane form)
    return launch_rows_lazy<false>(a, st);
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
    return bt_dispatch_upto<2, 4, 6, 8, 12, 16>((a.S + 63) / 64, [&](auto nwt) { return launch_bt_t<decltype(nwt)::value>(a, st); });
}

}  // namespace vit
