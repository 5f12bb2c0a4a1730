// obs_kernels.inc -- the two emission-builder kernels with their launch table and the snippet hand-off kernel, included as TEXT inside namespace vit by emission.hip
// (float32 logits -> float32 emissions: the instantiations every release has had) and emission_half.hip (float16 logits and / or
// float16 emissions), so that both translation units hold the same statements and compile side by side (DESIGN.md 4.4c).  Needs
// obs_frame.hpp.
//
// LT: the logits' storage type, ET: the emissions' storage type, each float or __half.  The storage type exists at the loads and the
// stores only: a float16 logit is widened (exactly) where it is loaded, the frame is worked on in float32 whatever the types are, and
// the float32 result is rounded to nearest even (float16 subnormals kept: the compiler's v_cvt_f16_f32 under the default mode) where
// it is stored.  So with LT = __half the rows are the float32 builder's rows on the widened logits, and with ET = __half they are
// the float32 builder's rows after torch's .half(), bit for bit.  A float16 row is 2 * S bytes: with an odd S every other row starts
// off a 4-byte boundary, so the vector views of a lane's columns are declared with the ELEMENT's alignment (f16x8_u like f32x4_u)
// and the compiler picks accesses that are legal there.
namespace {

constexpr int kObsWaves = 4;

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ float wave_max_f(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
    return x;
}

typedef _Float16 f16x8_u __attribute__((ext_vector_type(8), aligned(2)));

// float32 -> float16, nearest even, of a FINISHED float32 value.  The empty asm hides where the value came from: ob_log ends in an fma,
// and the compiler folds fma + conversion into v_fma_mixlo_f16, which rounds the exact fma once, to float16 -- not the float32
// builder's value rounded again (seen: one row in 41 000 off by one float16 ulp).
__device__ __forceinline__ _Float16 ob_half(float v) {
    asm("" : "+v"(v));
    return (_Float16)v;
}

// one element: float as it is, float16 widened at the load / rounded to nearest even at the store
__device__ __forceinline__ float ob_ld(const float* p) { return *p; }
__device__ __forceinline__ float ob_ld(const __half* p) { return (float)*reinterpret_cast<const _Float16*>(p); }
// (value first: an assignment evaluates its right side before its left, and the float32 code is to stay the code it was)
__device__ __forceinline__ void ob_st(const float v, float* p) { *p = v; }
__device__ __forceinline__ void ob_st(const float v, __half* p) { *reinterpret_cast<_Float16*>(p) = ob_half(v); }

// a lane's NPL consecutive halves as 16- / 8- / 4- / 2-byte pieces at 2-byte alignment (the float forms are in obs_frame.hpp)
template <int NPL>
__device__ __forceinline__ void ob_load(const __half* __restrict__ ph, float (&v)[NPL]) {
    const _Float16* __restrict__ p = reinterpret_cast<const _Float16*>(ph);
    int k = 0;
#pragma unroll
    for (; k + 7 < NPL; k += 8) {
        const f16x8_u t = *reinterpret_cast<const f16x8_u*>(p + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k + j] = (float)t[j];
    }
#pragma unroll
    for (; k + 3 < NPL; k += 4) {
        const f16x4_u t = *reinterpret_cast<const f16x4_u*>(p + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k + j] = (float)t[j];
    }
#pragma unroll
    for (; k + 1 < NPL; k += 2) { const f16x2_u t = *reinterpret_cast<const f16x2_u*>(p + k); v[k] = (float)t.x; v[k + 1] = (float)t.y; }
    if (k < NPL) v[k] = (float)p[k];
}
template <int NPL>
__device__ __forceinline__ void ob_store(__half* __restrict__ ph, const float (&v)[NPL]) {
    _Float16* __restrict__ p = reinterpret_cast<_Float16*>(ph);
    int k = 0;
#pragma unroll
    for (; k + 7 < NPL; k += 8) {
        f16x8_u t;
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = ob_half(v[k + j]);
        *reinterpret_cast<f16x8_u*>(p + k) = t;
    }
#pragma unroll
    for (; k + 3 < NPL; k += 4) {
        f16x4_u t;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = ob_half(v[k + j]);
        *reinterpret_cast<f16x4_u*>(p + k) = t;
    }
#pragma unroll
    for (; k + 1 < NPL; k += 2) { f16x2_u t; t.x = ob_half(v[k]); t.y = ob_half(v[k + 1]); *reinterpret_cast<f16x2_u*>(p + k) = t; }
    if (k < NPL) p[k] = ob_half(v[k]);
}

}  // namespace

// MODE 0: "shaun" (soft voicing on the strongest peak); MODE 1: softmax over the peak set; MODE 2: softmax over the
// peak set with a constant unvoiced logit (`threshold`), every probability divided by its state prior.
// logits: MODE 0, 2 [n_frames, U]; MODE 1 [n_frames, U+1] with column 0 = unvoiced.  out: [n_frames, U+1].
// prior (MODE 2): [U+1] in state order (unvoiced last), or null for no scaling.
//
// One wave per frame, lane l owns bins l, l+64, ... (coalesced loads and stores, conflict-free LDS).  A bin is a peak when
// it is the FIRST maximum of its window: c > max(row[b-spw .. b-1]) and c >= max(row[b+1 .. b+spw]).  The two window maxima
// come from a doubling table in LDS, R_p[i] = max(row[i .. i+p-1]) with p the largest power of two <= spw (two overlapping
// p-windows cover a window of spw): 3 LDS operations per element and level + 5 reads per bin instead of 2*spw + 1 reads
// per bin (spw = 15: ~90 instead of ~190 per lane and frame, and no 2-way bank conflicts).
template <int EPL, int MODE, typename LT, typename ET>
__global__ void __launch_bounds__(kObsWaves * 64) observation_kernel(const LT* __restrict__ logits, int64_t n_frames,
                                                                     int U, int spw, double threshold, double offset,
                                                                     double scale, const float* __restrict__ prior,
                                                                     ET* __restrict__ out) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int PW = U + 2 * spw;                       // reflect-padded row
    const int PWS = PW + 1;
    float* row = smem + (size_t)wv * 4 * PWS;          // [4][PWS]: the row, two doubling buffers, per-bin results
    float* bufA = row + PWS;
    float* bufB = bufA + PWS;
    float* aux = bufB + PWS;
    const int in_stride = MODE == 1 ? U + 1 : U;
    const int in_off = MODE == 1 ? 1 : 0;
    const int S = U + 1;
    int p = 1, levels = 0;
    while (2 * p <= spw) { p *= 2; ++levels; }

    const int64_t fstep = (int64_t)gridDim.x * kObsWaves;
    int64_t f = (int64_t)blockIdx.x * kObsWaves + wv;
    // the next frame's row is in flight while this one is worked on (a wave handles its frames one after another: without
    // the prefetch every frame starts with a full HBM round trip)
    float xn[EPL];
    float x0n = 0.f;
    auto fetch = [&](const int64_t fr) {
        const LT* __restrict__ x = logits + fr * in_stride + in_off;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int b = lane + 64 * e;
            xn[e] = b < U ? ob_ld(&x[b]) : -INFINITY;
        }
        if (MODE == 1) x0n = ob_ld(&logits[fr * in_stride]);
    };
    if (f < n_frames) fetch(f);
    for (; f < n_frames; f += fstep) {
        ET* __restrict__ o = out + f * S;
        // stage the row, then the reflect padding: row[spw + i] = x[i]
        float xv[EPL];
        const float x0f = x0n;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int b = lane + 64 * e;
            xv[e] = xn[e];
            if (b < U) row[spw + b] = xv[e];
        }
        if (f + fstep < n_frames) fetch(f + fstep);
        asm volatile("" ::: "memory");
        if (lane < spw) {
            row[spw - 1 - lane] = row[spw + lane + 1];         // x[-k] = x[k]
            row[spw + U + lane] = row[spw + U - 2 - lane];     // x[U-1+k] = x[U-1-k]
        }
        // doubling: after the loop `src` holds R_p (valid for i <= PW - p).  One wave: its LDS operations execute in program
        // order, so a level reads what the level before wrote without a barrier (the fences only pin the compiler's order).
        asm volatile("" ::: "memory");
        const float* src = row;
        int w = 1;
        for (int lv = 0; lv < levels; ++lv) {
            float* dst = (lv & 1) ? bufB : bufA;
#pragma unroll
            for (int e = 0; e < EPL + 2; ++e) {                   // PW = U + 2*spw <= 64 * (EPL + 2): no loop-carried index arithmetic
                const int i = lane + 64 * e;
                if (i + 2 * w <= PW) dst[i] = fmaxf(src[i], src[i + w]);
            }
            asm volatile("" ::: "memory");
            src = dst;
            w *= 2;
        }
        bool pk[EPL];
        float lmax = -INFINITY;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int b = lane + 64 * e;
            pk[e] = false;
            if (b < U) {
                const int c0 = spw + b;                                       // position of the bin in the padded row
                const float mr = fmaxf(src[c0 + 1], src[c0 + spw - p + 1]);     // max(row[c0+1 .. c0+spw])
                const float ml = fmaxf(src[c0 - spw], src[c0 - p]);             // max(row[c0-spw .. c0-1])
                pk[e] = xv[e] > ml && xv[e] >= mr;
                if (pk[e]) lmax = fmaxf(lmax, xv[e]);
            }
        }
        // ---- the peaks, compacted: only they need exp / divide / log (a dozen or two per frame), so peak k moves to lane k
        //      (rank by ballot + popcount, bin index through LDS) and every lane does that arithmetic once per 64 peaks
        //      instead of once per owned bin
        asm volatile("" ::: "memory");
        float* list = bufA;                           // bin index of peak k (as float bits); R_p is no longer needed
        float* exb = bufB;                            // exp(x - g) of peak k
        float* res = aux;                             // log-probability by bin (peaks only)
        int npk = 0;
        const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const unsigned long long m = __ballot(pk[e]);
            if (pk[e]) list[npk + __popcll(m & lt)] = __int_as_float(lane + 64 * e);
            npk += __popcll(m);
        }
        asm volatile("" ::: "memory");
        // unvoiced logit: always in the peak set (MODE 2: the padded voicing-threshold logit, rounded to float32 like np.pad)
        const float x0 = MODE == 1 ? x0f : (MODE == 2 ? (float)threshold : -INFINITY);
        float g = wave_max_f(lmax);
        const bool any_peak = g > -INFINITY;
        if (MODE >= 1) g = fmaxf(g, x0);
        float lsum = 0.f;
        for (int k0 = 0; k0 < npk; k0 += 64) {
            const int k = k0 + lane;
            if (k < npk) {
                const int b = __float_as_int(list[k]);
                const float exv = expf(row[spw + b] - g);
                exb[k] = exv;
                lsum += exv;
            }
        }
        float tot = wave_sum(lsum);
        float last;                                                       // probability of the unvoiced state
        double t;                                                         // scale applied to exp(x - g)
        if (MODE == 0) {
            double pv = 0.0;
            if (any_peak) {
                const double gd = (double)g;
                const double s_ = gd >= threshold ? scale * (gd - threshold) + offset : scale * (gd - threshold) - offset;
                if (s_ > 0) pv = 1.0 / (1.0 + exp(-s_));
                else { const double q = exp(s_); pv = q / (1.0 + q); }
            }
            t = any_peak ? pv / (double)tot : 0.0;
            last = any_peak ? (float)(1.0 - pv) : 1.f;
        } else {
            const float e0 = expf(x0 - g);
            tot += e0;
            t = 1.0;
            last = any_peak ? e0 / tot : 1.f;
        }
        asm volatile("" ::: "memory");
        for (int k0 = 0; k0 < npk; k0 += 64) {
            const int k = k0 + lane;
            if (k < npk) {
                const int b = __float_as_int(list[k]);
                float pr;
                if (MODE == 0) pr = (float)((double)exb[k] * t);
                else pr = exb[k] / tot;
                if (MODE == 2 && prior) pr = pr / prior[b];      // two float32 divisions, like the reference
                res[b] = logf(pr + kTiny);
            }
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int b = lane + 64 * e;
            if (b < U) ob_st(pk[e] ? res[b] : kLogTiny, &o[b]);
        }
        if (MODE == 2 && prior) last = last / prior[U];          // a peak-less frame: 1 / prior
        if (lane == 0) ob_st(logf(last + kTiny), &o[U]);
        asm volatile("" ::: "memory");                        // (the next frame's staging must not overtake these reads)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// observation_reg_kernel: the same builders with the frame in REGISTERS (round 4).  The LDS form above spends 393 vector +
// 213 scalar + 100 LDS instructions per frame (profiles/r02_pmc_extras.txt) -- more vector work than the 233-instruction
// forward recursion it feeds -- on staging the row, a doubling table and ballot / popcount ranks for the peak compaction.  Here
// lane l owns NPL CONTIGUOUS bins (one coalesced vector load and store per lane), the SPW neighbours on either side arrive by
// wave-wide DPP shifts of whole registers (wave_shr:1 / wave_shl:1, chained for SPW > NPL; -inf beyond the row's ends), every
// window maximum is a chain of v_max3_f32 over registers with compile-time indices, and the reflect padding is never built: what
// it adds to the windows reduces to two rules at the left end (at the kernel).  exp / log run densely on the owner lanes with the
// hardware's v_exp_f32 / v_log_f32 and a compensated argument split (a few ulp) instead of through a compacted peak list;
// v_exp_f32 returns no subnormals, so a frame with a peak or unvoiced logit more than 80 nats below its top takes a scaled exp
// (ob_exp_far) and true divisions (a ballot per frame, a wave-uniform branch) and keeps the subnormal probabilities the
// reference's float32 np.exp and division give.  The wave reductions are DPP; the soft-voicing sigmoid stays in float64 like the
// reference's.  No LDS, no barrier.
// Instantiated for the reference's half-widths 5 ("shaun", dcnet's scaled likelihood) and 15 (softmax) and 5 / 6 / 8 / 12 bins per
// lane (U <= 64 NPL: the 320-, 360- and 721-bin grids and what lies between); other geometries keep the LDS form.
template <int NPL, int SPW, int MODE, typename LT, typename ET>
__global__ void __launch_bounds__(256) observation_reg_kernel(const LT* __restrict__ logits, int64_t n_frames, int U, double threshold,
                                                             double offset, double scale, const float* __restrict__ prior,
                                                             ET* __restrict__ out) {
    constexpr int H = (SPW + NPL - 1) / NPL;          // lanes a lane looks at on either side
    constexpr int NA = NPL + 2 * SPW;                 // local neighbourhood: bins NPL*lane - SPW .. NPL*lane + NPL + SPW - 1
    const int lane = threadIdx.x & 63;
    const int in_stride = MODE == 1 ? U + 1 : U;
    const int in_off = MODE == 1 ? 1 : 0;
    const int S = U + 1;
    // ---- per-lane geometry: slot k of lane l is bin NPL*l + k.  The reflect padding of the reference (np.pad 'reflect': x[-k] = x[k],
    //      x[U-1+k] = x[U-1-k]) never has to exist: beyond the row's ends the neighbourhood holds -inf, and what the mirrored values
    //      add to a window is already in it -- except at the left end, where the LEFT window is compared strictly:
    //        bin 0:              its left window is the mirror of its right one  ->  peak iff c > max(right window)
    //        bins 1 .. SPW / 2:  their left window contains their own mirror image ->  never a peak (c > c)
    //        every other bin:    the mirrored values are bins the window holds anyway (left end), or add c >= x for bins that the
    //                            strict left comparison covers (right end; the last bin's right window is all mirror: c >= -inf)
    bool real[NPL], never[NPL], first[NPL];
    float rprior[NPL];                                // MODE 2: 1 / prior of the bin
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int b = NPL * lane + k;
        real[k] = b < U;
        never[k] = b >= 1 && 2 * b <= SPW;
        first[k] = b == 0;
        rprior[k] = (MODE == 2 && prior && real[k]) ? 1.f / prior[b] : 1.f;
    }
    const float rprior_u = (MODE == 2 && prior) ? 1.f / prior[U] : 1.f;
    // a full lane's NPL columns are one contiguous, coalesced vector access; the one partial lane of a row whose length is not a
    // multiple of NPL goes column by column; lanes beyond the row hold -inf and store nothing
    const int col0 = NPL * lane;
    const bool full = col0 + NPL <= U, partial = !full && col0 < U;
    const int64_t fstep = (int64_t)gridDim.x * (blockDim.x >> 6);
    int64_t f = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // wave-uniform: row bases in scalar registers
    // two frames in flight per wave (two register sets, the loop unrolled by two): with eight waves per SIMD one row ahead left the
    // kernel waiting on HBM latency at 4.2 TB/s
    float xq[2][NPL];
    float x0q[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < NPL; ++k) xq[q][k] = -INFINITY;
    auto fetch = [&](const int64_t fr, float (&xn)[NPL], float& x0n) {
        const LT* __restrict__ x = logits + fr * in_stride + in_off;
        if (full) ob_load<NPL>(x + col0, xn);
        if (partial) {
#pragma unroll
            for (int k = 0; k < NPL; ++k)
                if (real[k]) xn[k] = ob_ld(&x[col0 + k]);
        }
        if (MODE == 1) x0n = ob_ld(&logits[fr * in_stride]);
    };
    if (f < n_frames) fetch(f, xq[0], x0q[0]);
    if (f + fstep < n_frames) fetch(f + fstep, xq[1], x0q[1]);
    auto process = [&](const int64_t f, float (&xn)[NPL], float& x0n) {
        ET* __restrict__ o = out + f * S;
        float a[NA];
        const float x0f = x0n;
#pragma unroll
        for (int k = 0; k < NPL; ++k) a[SPW + k] = xn[k];
        if (f + 2 * fstep < n_frames) fetch(f + 2 * fstep, xn, x0n);
#include "obs_frame_body.inc"
        if (full) ob_store<NPL>(o + col0, v);
        if (partial) {
#pragma unroll
            for (int k = 0; k < NPL; ++k)
                if (real[k]) ob_st(v[k], &o[col0 + k]);
        }
        if (MODE == 2) last *= rprior_u;                 // (a peak-less frame: 1 / prior)
        if (lane == 0) ob_st(ob_log(last + kTiny), &o[U]);
    };
    for (; f < n_frames; f += 2 * fstep) {
        process(f, xq[0], x0q[0]);
        if (f + fstep < n_frames) process(f + fstep, xq[1], x0q[1]);
    }
}

// ---------------------------------------------------------------------------------------
// Device-resident hand-off from the acoustic model (SURVEY.md 8f rank 4; tonet/for_paper.py:2282-2302 does this on the
// host after a .cpu().numpy() copy): a batch of snippets [n, C, F] (C = n_bins + 1 channel rows, channel 0 = unvoiced,
// F frames) becomes n*F time-major logit rows appended to a recording's buffer on the GPU --
//   mode 0 ("shaun"):   row[b] = snip[b+1][f] - snip[0][f]   (n_bins columns: logits relative to the unvoiced channel)
//   mode 1 ("softmax"): row[c] = snip[c][f]                  (n_bins + 1 columns, unvoiced first)
// Only the first `rows` (= n*F - padded_frames) rows are written.  A 64 x 64 tile goes through LDS so that both the
// frame-contiguous reads and the channel-contiguous writes are coalesced.
// ---------------------------------------------------------------------------------------
// LT: the snippets' storage type (float or __half, widened at the load); the subtraction and the rows are float32.
template <typename LT>
__global__ void __launch_bounds__(256) snippets_append_kernel(const LT* __restrict__ snips, int n, int C, int F, int mode,
                                                              float* __restrict__ out, int64_t rows) {
    __shared__ float tile[64][65];
    __shared__ float ch0[64];
    const int sn = blockIdx.z, c0 = blockIdx.y * 64, f0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // 64 x 4
    const LT* __restrict__ src = snips + (size_t)sn * C * F;
    const int cols = mode == 0 ? C - 1 : C;
    const int coff = mode == 0 ? 1 : 0;                         // first channel that becomes a column
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r + coff, f = f0 + tx;
        tile[r][tx] = (c < C && f < F) ? ob_ld(&src[(size_t)c * F + f]) : 0.f;
    }
    if (mode == 0 && threadIdx.x < 64) ch0[tx] = f0 + tx < F ? ob_ld(&src[f0 + tx]) : 0.f;
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int f = f0 + r, col = c0 + tx;
        const int64_t row = (int64_t)sn * F + f;
        if (f < F && col < cols && row < rows) out[row * cols + col] = mode == 0 ? tile[tx][r] - ch0[r] : tile[tx][r];
    }
}

namespace {

template <int NPL, int SPW, int MODE, typename LT, typename ET>
hipError_t launch_obs_reg(const LT* logits, int64_t n_frames, int U, double thr, double off, double sc, const float* prior,
                          ET* out, int n_cus, hipStream_t st) {
    int64_t blocks = (n_frames + 3) / 4;
    if (blocks > (int64_t)n_cus * 8) blocks = (int64_t)n_cus * 8;      // eight waves per SIMD: the resident capacity, every wave walks its frames
    hipLaunchKernelGGL((observation_reg_kernel<NPL, SPW, MODE, LT, ET>), dim3((int)blocks), dim3(256), 0, st, logits, n_frames, U, thr, off, sc, prior, out);
    return hipGetLastError();
}

template <int MODE, typename LT, typename ET>
hipError_t launch_obs(const LT* logits, int64_t n_frames, int U, int spw, double thr, double off, double sc,
                      const float* prior, ET* out, hipStream_t st) {
    if (n_frames <= 0) return hipSuccess;
    if (spw < 1 || spw >= U || spw > 64 || U > 768) return hipErrorInvalidValue;
    int64_t blocks = (n_frames + kObsWaves - 1) / kObsWaves;
    static int n_cus = 0;                         // (no plan at this entry point: ask the device once)
    if (n_cus == 0) {
        int dev = 0, cus = 0;
        n_cus = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) ? cus : 256;
    }
    // the register form for the reference's geometries (spw 5 / 15; 5, 6, 8 or 12 bins per lane)
    if ((spw == 5 || spw == 15) && U > 64 && U > 2 * spw) {
#define VIT_OBS_REG(N) return spw == 5 ? launch_obs_reg<N, 5, MODE, LT, ET>(logits, n_frames, U, thr, off, sc, prior, out, n_cus, st) \
                                      : launch_obs_reg<N, 15, MODE, LT, ET>(logits, n_frames, U, thr, off, sc, prior, out, n_cus, st)
        if (U <= 64 * 5) VIT_OBS_REG(5);
        if (U <= 64 * 6) VIT_OBS_REG(6);
        if (U <= 64 * 8) VIT_OBS_REG(8);
        if (U <= 64 * 12) VIT_OBS_REG(12);
#undef VIT_OBS_REG
    }
    if (blocks > (int64_t)n_cus * 6) blocks = (int64_t)n_cus * 6;   // six workgroups of four frames' LDS fit a CU: one resident wave per frame slot, no second round
    const size_t lds = sizeof(float) * kObsWaves * 4 * (U + 2 * spw + 1);
    if (U <= 384)
        hipLaunchKernelGGL((observation_kernel<6, MODE, LT, ET>), dim3((int)blocks), dim3(kObsWaves * 64), lds, st, logits, n_frames, U,
                           spw, thr, off, sc, prior, out);
    else
        hipLaunchKernelGGL((observation_kernel<12, MODE, LT, ET>), dim3((int)blocks), dim3(kObsWaves * 64), lds, st, logits, n_frames, U,
                           spw, thr, off, sc, prior, out);
    return hipGetLastError();
}

}  // namespace
