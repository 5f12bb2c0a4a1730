// stream_commit.hip -- the commit point of a streaming session (vit_stream_commit): the survivor merge kernel that
// finds the path prefix no later frame can change.
//
// Back-pointers are lazy here: psi_{t+1}[j] is a function of delta row t and the plan, and a history row never changes once the
// forward pass has written it.  So the survivors of ALL S states of the newest frame n-1 can be traced backwards over the rows as
// they stand: U_{n-1} = every state, U_t = psi_{t+1}[U_{t+1}].  The first frame c at which U_c is one state s_c is a frame every
// path through frame n-1 -- hence every path of any longer recording -- passes in s_c: frames [f, c] are final (f = the frontier of
// the commit before).  The kernel writes (f, c - f + 1, s_c) as a sub-problem of the lane back-trace (backtrace_lane.hip:
// BtArgs::first_row / lengths / last_state), which vit_stream_commit launches behind it over the same rows: the committed range is
// walked in parallel chunks, however long it is.
//
// One workgroup per recording, one lane per surviving state, ceil(S / 64) waves:
//   * every thread copies its share of delta row t (and the frame maximum in pad column S) to LDS; the row's address does not
//     depend on any decision, so row t-1 is already in flight while frame t is decided;
//   * every live lane decides psi_{t+1}[its state] the way the lane back-trace does (backtrace_lane.hip LaneDecider::step): the
//     window and the extra columns in ascending order with the strict compare, then the bound fl(M_t + c_j) < m.  Where the
//     bound does not hold a row-constant candidate may tie or win, and the lane scans sources 0 .. S-1 outside its window and
//     the extra columns from the LDS row itself (every lane of a wave reads the same address: a broadcast).  Started from all S
//     states most lanes take this path in the first one or two frames -- a state far from the path takes the floor candidate --
//     which is why it is a per-lane scan here and not the lane kernel's whole-wave evaluation of two lanes per call;
//   * the survivors are deduplicated through an S-bit set in LDS: lane k takes the k-th set bit, a count of 1 ends the walk.
//     All lanes stand at the same frame at all times, so the merge test needs no catching up.
// The kernel writes the frontier, committed[b], the sub-problem and (vit_stream_commit_rel) first[b] = f, nothing else.
// Rows are addressed as t mod hist_rows: on a ring session (vit_stream_open_ring) the walk runs backwards across slot 0 -> R - 1; the
// rows [f, n) it may read are resident by the session's residency rule.  stream_tail_prep_kernel forms vit_stream_tail's sub-problems.
#include "backtrace_common.hpp"

namespace vit {

namespace {

constexpr int kScMaxThreads = 768;       // twelve waves: the largest state count a session serves (S < 64 * 12)

__device__ __forceinline__ int sc_row_floats(const int S) { return (S + 4) & ~3; }        // S states + the frame maximum

// psi_{t+1}[j]: rowL = delta row t in LDS (state i at rowL[i], the frame maximum at rowL[S]), wt = row j of the candidate table
// (W window weights, kMaxExtras extra-column weights, c_j).  The lowest index attaining the maximum; an all -inf frame resolves to 0.
__device__ __forceinline__ int sc_decide(const BtArgs& a, const float* rowL, const float* __restrict__ wt, const int lo) {
    const int S = a.S, W = a.W, nx = a.n_extras;
    float m = -INFINITY;
    int arg = kBig;
    for (int w = 0; w < W; w += 4) {              // (every instantiated window width is a multiple of 4: four reads in flight)
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = rowL[lo + w + r] + wt[w + r];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool gt = v[r] > m;
            m = gt ? v[r] : m;
            arg = gt ? lo + w + r : arg;
        }
    }
#pragma unroll
    for (int k = 0; k < kMaxExtras; ++k)
        if (k < nx) {
            const int xk = a.extras[k];
            const float v = rowL[xk] + wt[W + k];
            const bool take = v > m || (v == m && xk < arg);
            m = take ? v : m;
            arg = take ? xk : arg;
        }
    const float cj = wt[W + kMaxExtras];
    if (rowL[S] + cj < m) return arg;             // no row-constant candidate can tie or win
    float m2 = -INFINITY;
    int arg2 = kBig;
    for (int i = 0; i < S; ++i) {
        bool excl = (unsigned)(i - lo) < (unsigned)W;
#pragma unroll
        for (int k = 0; k < kMaxExtras; ++k) excl |= k < nx && i == a.extras[k];
        const float v = rowL[i] + cj;
        const bool gt = !excl && v > m2;
        m2 = gt ? v : m2;
        arg2 = gt ? i : arg2;
    }
    const float mm = fmaxf(m, m2);
    int r = m == mm ? arg : kBig;
    r = (m2 == mm && arg2 < r) ? arg2 : r;
    return (mm == -INFINITY || r == kBig) ? 0 : r;
}

// GT: the candidate table stays in global memory (it does not fit beside the rows in 64 KB of LDS: the wide windows of the 722-state grids)
template <bool GT>
__global__ void __launch_bounds__(kScMaxThreads) stream_commit_kernel(CommitArgs c) {
    extern __shared__ __align__(16) unsigned char smem[];
    const BtArgs& a = c.b;
    const int S = a.S, SD = a.SD, W = a.W, WX1 = W + kMaxExtras + 1;
    const int tid = threadIdx.x, NT = blockDim.x, song = blockIdx.x;
    const int SDL = sc_row_floats(S), BW = (S + 31) >> 5;
    float* rowbuf = reinterpret_cast<float*>(smem);                       // two rows
    uint32_t* bitbuf = reinterpret_cast<uint32_t*>(rowbuf + 2 * SDL);     // two survivor sets
    int32_t* loL = reinterpret_cast<int32_t*>(bitbuf + 2 * BW);
    float* tabL = reinterpret_cast<float*>(loL + a.SP);

    const long long n = c.pos[song];
    const long long f = c.reset ? 0 : c.frontier[song];
    const long long t_stop = f > n - 1 - c.max_lookback ? f : n - 1 - c.max_lookback;     // the lowest frame the merge may be found at
    if (n < 2 || t_stop > n - 2) {          // nothing to walk: the frontier stands (uniform in the workgroup)
        __syncthreads();
        if (tid == 0) {
            c.frontier[song] = f; c.committed[song] = f; c.sub_first[song] = f; c.sub_len[song] = 0; c.sub_last[song] = 0;
            if (c.first) c.first[song] = f;
        }
        return;
    }
    {
        const int32_t* gl = reinterpret_cast<const int32_t*>(a.image + a.off_lo);
        for (int k = tid; k < a.SP; k += NT) loL[k] = gl[k];
        if (!GT) {
            const float* __restrict__ gtab = reinterpret_cast<const float*>(a.image + a.off_tabX);
            for (int k = tid; k < a.SP * WX1; k += NT) tabL[k] = gtab[k];
        }
    }
    const float* __restrict__ hist = a.hist + (size_t)song * (size_t)a.hist_rows * SD;
    const float* tab = GT ? reinterpret_cast<const float*>(a.image + a.off_tabX) : tabL;

    float pre0 = 0.f, pre1 = 0.f;           // this thread's share of the row in flight: columns tid and tid + NT (S + 1 <= 2 NT)
    // frame t lives in row t mod hist_rows (a linear session: hist_rows = its capacity, the cursor never wraps); slot = the row in flight
    const long long R = a.hist_rows;
    long long slot = (n - 2) % R;
    auto fetch = [&]() {
        const float* __restrict__ r = hist + (size_t)slot * SD;
        if (tid <= S) pre0 = r[tid];
        if (tid + NT <= S) pre1 = r[tid + NT];
    };
    int cur = tid;                          // lane k < count: the k-th survivor at frame t + 1
    int count = S;
    long long t = n - 2;
    fetch();
    for (;; --t) {
        float* rowL = rowbuf + (t & 1) * SDL;
        uint32_t* bits = bitbuf + (t & 1) * BW;
        if (tid <= S) rowL[tid] = pre0;
        if (tid + NT <= S) rowL[tid + NT] = pre1;
        if (tid < BW) bits[tid] = 0u;
        if (t > t_stop) { slot = slot == 0 ? R - 1 : slot - 1; fetch(); }
        __syncthreads();
        if (tid < count) {
            int lo;
            if (a.lo_affine) { lo = cur - a.lo_off; lo = lo < 0 ? 0 : (lo > S - W ? S - W : lo); }
            else lo = loL[cur];
            const int nxt = sc_decide(a, rowL, tab + (size_t)cur * WX1, lo);
            atomicOr(&bits[nxt >> 5], 1u << (nxt & 31));
        }
        __syncthreads();
        int acc = 0, mine = 0;
        for (int w = 0; w < BW; ++w) {
            uint32_t v = bits[w];
            const int pc = __popc(v);
            if (tid >= acc && tid < acc + pc) {
                for (int r = tid - acc; r > 0; --r) v &= v - 1u;
                mine = 32 * w + __ffs(v) - 1;
            }
            acc += pc;
        }
        count = acc;
        cur = mine;
        if (count == 1 || t == t_stop) break;
    }
    if (tid == 0) {
        const bool merged = count == 1;     // at frame c = t in state cur
        const long long f2 = merged ? t + 1 : f;
        c.frontier[song] = f2;
        c.committed[song] = f2;
        c.sub_first[song] = f;
        c.sub_len[song] = f2 - f;
        c.sub_last[song] = cur;
        if (c.first) c.first[song] = f;
    }
}

// vit_stream_tail: the frames behind the frontier as one sub-problem per recording, formed from the frontier and the uploaded lengths
__global__ void stream_tail_prep_kernel(CommitArgs c, const int32_t* __restrict__ last_state) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.b.B) return;
    const long long n = c.pos[b];
    long long f = c.reset ? 0 : c.frontier[b];
    f = f > n ? n : f;
    c.sub_first[b] = f;
    c.sub_len[b] = n - f;
    c.sub_last[b] = last_state[b];
    c.first[b] = f;
}

size_t sc_lds_bytes(const BtArgs& a, const bool table_in_lds) {
    const size_t S = (size_t)a.S;
    return sizeof(float) * 2 * ((S + 4) & ~(size_t)3) + sizeof(uint32_t) * 2 * ((S + 31) >> 5) + sizeof(int32_t) * a.SP +
           (table_in_lds ? sizeof(float) * (size_t)a.SP * (a.W + kMaxExtras + 1) : 0);
}

}  // namespace

// Banded plans without dense rows over workgroup rows that carry the frame maximum: what the lane back-trace serves, on at most twelve waves.
bool stream_commit_applies(const BtArgs& a) {
    return a.banded && a.have_fmax && a.n_dense == 0 && !a.hist_half && a.aux_frames == 1 && a.col0 == 0 && a.mcol == a.S && a.xcol0 < 0 &&
           banded_width_instantiated(a.W) && a.W % 4 == 0 && a.W <= a.S && a.S + 1 <= a.SD && (a.S + 63) / 64 * 64 <= kScMaxThreads;
}
bool stream_commit_table_in_lds(const BtArgs& a) { return sc_lds_bytes(a, true) <= 64 * 1024; }

hipError_t launch_stream_commit(const CommitArgs& c, hipStream_t st) {
    const BtArgs& a = c.b;
    if (!stream_commit_applies(a) || a.B < 1) return hipErrorInvalidConfiguration;
    const bool in_lds = stream_commit_table_in_lds(a);
    const dim3 grid((unsigned)a.B), block((unsigned)((a.S + 63) / 64 * 64));
    if (in_lds) hipLaunchKernelGGL(stream_commit_kernel<false>, grid, block, sc_lds_bytes(a, true), st, c);
    else hipLaunchKernelGGL(stream_commit_kernel<true>, grid, block, sc_lds_bytes(a, false), st, c);
    return hipGetLastError();
}

hipError_t launch_stream_tail_prep(const CommitArgs& c, const int32_t* last_state, hipStream_t st) {
    if (c.b.B < 1 || !c.first || !last_state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_tail_prep_kernel, dim3((unsigned)((c.b.B + 255) / 256)), dim3(256), 0, st, c, last_state);
    return hipGetLastError();
}

}  // namespace vit
