// backtrace_common.hpp -- what the back-trace kernel files (backtrace_sparse / _half / _rows / _lane .hip, f64.hip) share: the ONE copy of
// the time-parallel chunk scheme of the wave-per-chunk kernels, the pieces of a frame's decision that the sparse and the lean
// whole-row kernel have in common, the counter flush, and the host-side launch helpers.
//
// The scheme.  Frames 0 .. Tb-2 of a song are decided (frame Tb-1 is the terminal state).  They are split into C chunks
// [lo_c, hi_c) = [Lf c / C, Lf (c + 1) / C), Lf = Tb - 1.  MODE 0 (one wave per (song, chunk)) chases chunk c from a warm-up
// point `warm` frames above hi_c, starting from the best state of that frame (a guess): survivor paths coalesce, so the state
// it reaches at hi_c is most likely the true one.  It stores that state as the chunk's `entry` and writes the chunk.  MODE 1
// (one wave per song) walks c = C-2 .. 0 and compares what chunk c assumed at hi_c with what the chunk above it (already
// verified) decided there; where they differ the chunk is chased again from the true state.  Exact whatever the guesses were.
//
// Everything here is __forceinline__ and takes the kernel's own lambdas as template parameters: no calls, no pointers to
// functions, nothing passed through memory.  profiles/bt_refactor_resources_*.txt: the kernels' registers, scratch and
// occupancy with the scheme written out in each of them and with this header.
#pragma once
#include <type_traits>

#include "device_common.hpp"

namespace vit {

// chunk c of C over the Lf decided frames of a song
__host__ __device__ __forceinline__ void bt_chunk_bounds(int Lf, int c, int C, int& lo_c, int& hi_c) {
    lo_c = (int)((long long)Lf * c / C);
    hi_c = (int)((long long)Lf * (c + 1) / C);
}

// Lowest-index argmax of one delta row (row[i] = delta of state i), sources strided: lane l holds i = 64 e + l.  An all -inf
// row resolves to index 0 like np.argmax.  Wave-uniform.
template <int EPL>
__device__ __forceinline__ int bt_row_argmax(const float* __restrict__ row, const int S, const int lane) {
    float d[EPL];
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        d[e] = e * 64 + lane < S ? row[e * 64 + lane] : -INFINITY;
        m = fmaxf(m, d[e]);
    }
    m = wave_max_all(m);
    unsigned idx = 0x7fffffffu;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const unsigned long long mk = __ballot(d[e] == m && e * 64 + lane < S);
        if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
    }
    return idx == 0x7fffffffu ? 0 : (int)idx;
}
// The same of a row of doubles (f64.hip: the d rows of its history, or of LDS); *mout = the maximum.  An overload, declared in
// front of bt_run_chunks: the call in there is resolved where the template is defined (a pointer to double has no namespace of its own).
template <int EPL>
__device__ __forceinline__ int bt_row_argmax(const double* row, const int S, const int lane, double* mout = nullptr) {
    double d[EPL];
    double m = -INFINITY;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        d[e] = e * 64 + lane < S ? row[e * 64 + lane] : -INFINITY;
        m = fmax(m, d[e]);
    }
    m = wave_max_all_f64(m);
    unsigned idx = 0x7fffffffu;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const unsigned long long mk = __ballot(d[e] == m && e * 64 + lane < S);
        if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
    }
    if (mout) *mout = m;
    return idx == 0x7fffffffu ? 0 : (int)idx;
}

// The chunk scheme of one wave.
//   chase(top, bottom, cur, write) -> int: decide frames top .. bottom (descending) starting from state `cur` at frame top + 1,
//       store them if `write`; returns the state at frame `bottom`
//   guess_row(f) -> const float* (f64.hip: const double*): the stored delta row of frame f, at the column of state 0
//   states, entry: the song's (states is the array chase() writes: no __restrict__ here, MODE 1 reads what chase() stored);
//       last: its terminal state; Tb: its frames; Tpad: -1 is written to states[Tb .. Tpad)
//   EVEN_GUESS: only even frames have a stored row (half history): the warm-up point is moved up to an odd frame
// MODE 0 uses chunk, warm, last, Tpad and the guess; MODE 1 walks every chunk.  Returns the chunks MODE 1 chased again.
template <int MODE, int EPL, bool EVEN_GUESS = false, typename Chase, typename GuessRow>
__device__ __forceinline__ int bt_run_chunks(Chase&& chase, GuessRow&& guess_row, int32_t* states, int32_t* entry,
                                             const int last, const int Tb, const int Tpad, const int chunk, const int C, const int warm,
                                             const int S, const int lane) {
    const int Lf = Tb - 1;
    int n_rep = 0;
    if (MODE == 0) {
        int lo_c, hi_c;
        bt_chunk_bounds(Lf, chunk, C, lo_c, hi_c);
        if (chunk == C - 1) {
            for (int t = Tb + lane; t < Tpad; t += 64) states[t] = -1;
            if (lane == 0) states[Tb - 1] = last;
        }
        int top = hi_c - 1 + warm;
        if (EVEN_GUESS) top += top & 1 ? 0 : 1;                   // the guess row top + 1 must be a stored (even) frame
        int cur;
        if (chunk == C - 1 || top >= Lf - 1) {
            top = Lf - 1;
            cur = __builtin_amdgcn_readfirstlane(last);
        } else {
            cur = bt_row_argmax<EPL>(guess_row(top + 1), S, lane);   // guess: lowest-index argmax of delta row top + 1
        }
        if (hi_c <= lo_c) {                       // empty chunk (very short song)
            if (lane == 0) entry[chunk] = cur;
            return 0;
        }
        cur = chase(top, hi_c, cur, false);       // warm-up: frames top .. hi_c, nothing written
        if (lane == 0) entry[chunk] = cur;        // state this chunk assumed at frame hi_c
        chase(hi_c - 1, lo_c, cur, true);
    } else {
        int truth = -1;                           // verified state at frame hi_c of the chunk being checked
        for (int c = C - 2; c >= 0; --c) {
            int lo_c, hi_c;
            bt_chunk_bounds(Lf, c, C, lo_c, hi_c);
            if (truth < 0) truth = __builtin_amdgcn_readfirstlane(states[hi_c]);
            const int assumed = __builtin_amdgcn_readfirstlane(entry[c]);
            if (hi_c > lo_c && assumed != truth) {
                ++n_rep;
                truth = chase(hi_c - 1, lo_c, truth, true);   // re-chase from the true state; ends at frame lo_c
            } else {
                truth = -1;                       // chunk c stands: its frame lo_c is already in `states`
            }
        }
    }
    return n_rep;
}

// Per-lane flags of the strided sources i = 64 e + lane of a full-row evaluation: inS = the source exists, xcol = it is an extra
// column or padding (its candidate is not a row-constant one).
template <int EPL>
struct BtSourceFlags {
    bool inS[EPL], xcol[EPL];
    __device__ __forceinline__ BtSourceFlags(const BtArgs& a, const int lane) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int i = e * 64 + lane;
            inS[e] = i < a.S;
            bool x = i >= a.S;
#pragma unroll
            for (int k = 0; k < kMaxExtras; ++k) x |= (k < a.n_extras && i == a.extras[k]);
            xcol[e] = x;
        }
    }
};

// Per-lane constants of the candidate slots of the sparse and the lean whole-row kernel: slot k of lane l holds candidate
// c = 64 k + l -- candidates 0 .. W-1 the window, W .. W+nx-1 the extra columns, W + kMaxExtras the bound fl(M_t + c_j).
template <int KC>
struct BtSlots {
    bool isw[KC], cand[KC];            // window candidate | window or extra-column candidate
    int xs[KC];                        // state of an extra-column candidate
    int tb[KC];                        // entry of the target's candidate-table row
    unsigned long long wmask[KC];      // lanes of slot k that hold window candidates
    __device__ __forceinline__ BtSlots(const BtArgs& a, const int lane) {
        const int W = a.W, nx = a.n_extras, WX1 = W + kMaxExtras + 1;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int c = 64 * k + lane;
            isw[k] = c < W;
            cand[k] = c < W + nx;
            xs[k] = (c >= W && c < W + nx) ? a.extras[(c - W) & (kMaxExtras - 1)] : 0;
            tb[k] = c < WX1 ? c : WX1 - 1;
            const int nwin = W - 64 * k;
            wmask[k] = nwin >= 64 ? ~0ull : (nwin <= 0 ? 0ull : ((1ull << nwin) - 1ull));
        }
    }
};

// Lowest source index among the window / extra-column candidates whose value v[k] equals `mm` (0x7fffffff: none); lo = the
// window's first source.  PRE: `pre` already holds the candidate lanes that attain `m` (KC == 1: the caller's one compare for
// the maximum and the bound), used when mm == m.  xsrc / xbase: a kernel that already keeps, per slot, a register whose
// extra-column lanes hold xbase + the candidate's state (the lean kernel's row entries) passes it instead of s.xs, which then
// costs it no registers.
template <int KC, bool PRE = false>
__device__ __forceinline__ unsigned bt_lowest_candidate(const BtSlots<KC>& s, const float (&v)[KC], const float mm, const int lo,
                                                        const float m = 0.f, const unsigned long long pre = 0ull, const int* xsrc = nullptr, const int xbase = 0) {
    unsigned best = 0x7fffffffu;
    bool have_w = false;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const unsigned long long mk = (PRE && mm == m) ? pre : __ballot(v[k] == mm && s.cand[k]);
        const unsigned long long mw = mk & s.wmask[k];
        if (mw && !have_w) {                                 // window candidates ascend with the source index
            const unsigned c = lo + 64 * k + __builtin_ctzll(mw);
            best = c < best ? c : best;
            have_w = true;
        }
        unsigned long long mx = mk & ~s.wmask[k];            // extra columns: arbitrary indices
        while (mx) {
            const unsigned c = __builtin_amdgcn_readlane(xsrc ? xsrc[k] : s.xs[k], __builtin_ctzll(mx)) - xbase;
            best = c < best ? c : best;
            mx &= mx - 1;
        }
    }
    return best;
}

// Full evaluation of a row (a row-constant candidate may tie or win): every source outside the window / extra columns
// contributes fl(delta_t[i] + cj); read(e) = delta_t[64 e + lane] from wherever the kernel keeps the row (any value where the
// source does not exist).  m = the maximum over the window / extra-column candidates v.  Returns the lowest index attaining the
// maximum over all of them; an all -inf frame resolves to index 0 like np.argmax.
template <int EPL, int KC, bool PRE = false, typename Read>
__device__ __forceinline__ unsigned bt_full_row(const BtSourceFlags<EPL>& f, const BtSlots<KC>& s, const float (&v)[KC], Read&& read,
                                                const float cj, const float m, const int lo, const int W, const int lane,
                                                const unsigned long long pre = 0ull, const int* xsrc = nullptr, const int xbase = 0) {
    float vf[EPL];
    float m2 = -INFINITY;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int i = e * 64 + lane;
        const float d = read(e);
        const bool excl = f.xcol[e] || (unsigned)(i - lo) < (unsigned)W;
        vf[e] = excl ? -INFINITY : d + cj;
        m2 = fmaxf(m2, vf[e]);
    }
    const float mm = fmaxf(m, wave_max_all(m2));
    unsigned idx = 0x7fffffffu;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const unsigned long long mk = __ballot(vf[e] == mm && f.inS[e]);
        if (mk) { const unsigned c = e * 64 + __builtin_ctzll(mk); idx = c < idx ? c : idx; }
    }
    const unsigned c = bt_lowest_candidate<KC, PRE>(s, v, mm, lo, m, pre, xsrc, xbase);
    idx = c < idx ? c : idx;
    return idx == 0x7fffffffu ? 0 : idx;
}

// One thread adds its event counts to the song's counters (vit_backtrace_counters); a count of zero costs nothing.
__device__ __forceinline__ void bt_flush_counters(int32_t* counters, const int song, const bool writer, const int n_tiles, const int n_miss,
                                                  const int n_full, const int n_reb, const int n_rep, const int n_repf) {
    if (!writer || !counters) return;
    int32_t* ct = counters + (size_t)song * kBtCounters;
    if (n_tiles) atomicAdd(ct + kCtTiles, n_tiles);
    if (n_miss) atomicAdd(ct + kCtMisses, n_miss);
    if (n_full) atomicAdd(ct + kCtFullRows, n_full);
    if (n_reb) atomicAdd(ct + kCtRebuilt, n_reb);
    if (n_rep) atomicAdd(ct + kCtRepairs, n_rep);
    if (n_repf) atomicAdd(ct + kCtRepairFrames, n_repf);
}

// ---------------------------------------------------------------------------------------
// host: launch helpers
// ---------------------------------------------------------------------------------------
// The two passes of a wave-per-chunk back-trace, nw waves per workgroup: kern0 (MODE 0) over waves0 waves if phases & 1, then --
// unless that failed, there is one chunk per song, or !(phases & 2) -- kern1 (MODE 1) over one wave per song.
// (Args: BtArgs, or F64Args of f64.hip -- a.chunks is all that is read of it)
template <typename Kern, typename Args>
static inline hipError_t launch_two_pass(Kern kern0, Kern kern1, const long long waves0, const long long songs, const int nw, const size_t lds,
                                         hipStream_t st, const Args& a, const int phases = 3) {
    hipError_t e = hipSuccess;
    if (phases & 1) {
        hipLaunchKernelGGL(kern0, dim3((unsigned)((waves0 + nw - 1) / nw)), dim3(nw * 64), lds, st, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess || a.chunks <= 1 || !(phases & 2)) return e;
    hipLaunchKernelGGL(kern1, dim3((unsigned)((songs + nw - 1) / nw)), dim3(nw * 64), lds, st, a);
    return hipGetLastError();
}

// f(std::integral_constant<int, N>) for the first N of the list with n <= N; the last N takes everything above it
template <int N, int... REST, typename F>
static inline hipError_t bt_dispatch_upto(const int n, F&& f) {
    if constexpr (sizeof...(REST) == 0) return f(std::integral_constant<int, N>{});
    else return n <= N ? f(std::integral_constant<int, N>{}) : bt_dispatch_upto<REST...>(n, f);
}
// f(std::true_type) or f(std::false_type)
template <typename F>
static inline hipError_t bt_dispatch_bool(const bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace vit
