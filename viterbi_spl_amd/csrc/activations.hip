// activations.hip -- activation front-end of imm's decoder: NMF source activations HF0 -> log-emissions, the step right
// upstream of the decoder for the dense Durrieu matrix.  In the reference this is host NumPy, once per recording
// (Viterbi.process_HF0_fn, imm/tf_imm.py:70-88):
//   t    = min(HF0[HF0 > 0]);  if log(t) < -87: t = exp(-87)
//   E    = log(HF0 + t)                      [U, N]
//   _min = min(E);  pad one unvoiced row filled with _min;  transpose -> [N, U + 1]
// Here B recordings lie side by side along the frame axis of one [U, N_total] matrix (row stride ld, recording b owns columns
// offsets[b] .. offsets[b+1]-1) and every statistic is per recording.  Four launches on the caller's stream:
//   act_init_kernel    stats[b] = {+inf, +inf, 0, +inf}
//   act_stats_kernel   pass 1: per recording the minimum over entries > 0 and over all entries, reduced on the BIT PATTERNS
//                      (non-negative floats order like unsigned integers: exact, order-independent, and a subnormal counts as
//                      positive whatever the float mode -- "positive" is "bits != 0", found as the minimum of bits - 1)
//   act_log_kernel     pass 2: t from the statistics and two host-derived constants (the clamp decision is an integer compare
//                      of bit patterns: the device's log has no say in it), out[n][u] = log(hf0[u][n] + t) through padded
//                      64 x 64 LDS tiles (frame-contiguous reads, state-contiguous writes, 128-bit where the rows allow), and
//                      the minimum of the WRITTEN values per recording
//   act_fill_kernel    column U of every row = that minimum.  It is reduced from the computed values rather than taken as
//                      log(min + t): the two agree only if logf is monotone, which nothing promises.
// A tile of 64 frames may straddle recordings: every frame of a tile looks its recording up in the device copy of offsets.
// Vector memory operations and plain C++ only.
#include "device_common.hpp"

namespace vit {

constexpr int kActTile = 64;                 // frames and bins of one tile
constexpr int kActPitch = kActTile + 1;      // tile[bin][frame], padded: both the row-wise stores and the column-wise reads
                                             // of a wave touch 64 different banks
constexpr unsigned kActInf = 0x7f800000u;    // +inf: the identity of every minimum kept in stats

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// recording of frame c: the largest b in [0, B) with offsets[b] <= c (always a valid index, whatever offsets holds)
__device__ __forceinline__ int act_find_rec(const int64_t* __restrict__ offsets, int B, int64_t c) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// minimum over the 16 lanes of a DPP row, in every lane of the row
__device__ __forceinline__ float act_row16_min(float x) {
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0xB1, 0xf, 0xf, false)));    // quad_perm [1,0,3,2]
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x4E, 0xf, 0xf, false)));    // quad_perm [2,3,0,1]
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x141, 0xf, 0xf, false)));   // row_half_mirror
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x140, 0xf, 0xf, false)));   // row_mirror
    return x;
}

// float minimum into a word that starts at +inf: non-negative values order like signed integers, negative ones in reverse
// like unsigned integers, and any negative value beats any non-negative one under the unsigned maximum
__device__ __forceinline__ void act_atomic_min_f32(unsigned* addr, float v) {
    const unsigned b = __float_as_uint(v);
    if (b & 0x80000000u) atomicMax(addr, b);
    else atomicMin(reinterpret_cast<int*>(addr), (int)b);
}

__global__ void act_init_kernel(unsigned* __restrict__ stats, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 * B) stats[i] = (i & 3) == 2 ? 0u : kActInf;
}

// Tile geometry shared by both passes: tile bx covers frames c0 .. c0 + 63 with c0 = 64 bx - shift, where shift is the
// misalignment (in floats) of hf0's first element -- with ld a multiple of 4 every row of every tile then starts on a 16-byte
// boundary.  Local frames [plo, phi) exist.
struct ActTile {
    int64_t c0;
    int plo, phi;
};
__device__ __forceinline__ ActTile act_tile(const float* hf0, int64_t total) {
    const int shift = (int)((reinterpret_cast<uintptr_t>(hf0) >> 2) & 3);
    ActTile t;
    t.c0 = (int64_t)blockIdx.x * kActTile - shift;
    t.plo = t.c0 < 0 ? (int)-t.c0 : 0;
    const int64_t left = total - t.c0;
    t.phi = left < kActTile ? (int)left : kActTile;
    return t;
}

// ---- pass 1.  256 threads: thread (r = tid / 16, j = tid % 16) reads frames 4j .. 4j+3 of bin rows r, r + 16 gridDim.y, ...
__global__ void __launch_bounds__(256) act_stats_kernel(const float* __restrict__ hf0, int64_t ld, int U, int B,
                                                        const int64_t* __restrict__ offsets, int64_t total,
                                                        unsigned* __restrict__ stats) {
    __shared__ int s_rec[kActTile];
    __shared__ unsigned s_pos[kActTile], s_all[kActTile];
    const ActTile tl = act_tile(hf0, total);
    const int tid = threadIdx.x;
    if (tid < kActTile) {
        s_rec[tid] = (tid >= tl.plo && tid < tl.phi) ? act_find_rec(offsets, B, tl.c0 + tid) : -1;
        s_pos[tid] = ~0u;
        s_all[tid] = ~0u;
    }
    __syncthreads();
    const int rec0 = s_rec[tl.plo];
    const bool one_rec = rec0 == s_rec[tl.phi - 1];          // (recordings are contiguous: equal ends, equal everywhere)
    const int j = tid & 15, r = tid >> 4;
    const int p0 = 4 * j;
    const bool inside = p0 >= tl.plo && p0 + 3 < tl.phi;
    unsigned mpos = ~0u, mall = ~0u;                         // mpos: minimum of bits - 1 (a zero wraps to the identity)
    const int64_t rstep = 16 * (int64_t)gridDim.y;
    for (int64_t u = r + 16 * (int64_t)blockIdx.y; u < U; u += rstep) {
        const float* __restrict__ row = hf0 + u * ld + tl.c0;
        unsigned v[4] = {~0u, ~0u, ~0u, ~0u};
        bool have[4] = {false, false, false, false};
        if (inside && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(row + p0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = __float_as_uint(x[k]);
                have[k] = true;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                have[k] = p0 + k >= tl.plo && p0 + k < tl.phi;
                if (have[k]) v[k] = __float_as_uint(row[p0 + k]);
            }
        }
        if (one_rec) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (have[k]) {
                    mall = min(mall, v[k]);
                    mpos = min(mpos, v[k] - 1u);
                }
        } else {                                             // a tile across a recording boundary: per-frame minima in LDS
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (have[k]) {
                    atomicMin(&s_all[p0 + k], v[k]);
                    atomicMin(&s_pos[p0 + k], v[k] - 1u);
                }
        }
    }
    if (one_rec) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mall = min(mall, (unsigned)__shfl_xor((int)mall, off, 64));
            mpos = min(mpos, (unsigned)__shfl_xor((int)mpos, off, 64));
        }
        if ((tid & 63) == 0) {
            if (mpos != ~0u) atomicMin(&stats[4 * rec0 + 0], mpos + 1u);
            if (mall != ~0u) atomicMin(&stats[4 * rec0 + 1], mall);
        }
    } else {
        __syncthreads();
        if (tid >= tl.plo && tid < tl.phi) {
            const int rec = s_rec[tid];
            if (s_pos[tid] != ~0u) atomicMin(&stats[4 * rec + 0], s_pos[tid] + 1u);
            if (s_all[tid] != ~0u) atomicMin(&stats[4 * rec + 1], s_all[tid]);
        }
    }
}

// ---- pass 2.  The block walks the 64-bin tiles k = blockIdx.y, blockIdx.y + gridDim.y, ... of its 64 frames.
//   load  : thread (r, j) reads frames 4j .. 4j+3 of bins 64k + r + 16i (i < 4) into registers -- the next tile's loads are in
//           flight while this one is written out -- and stores them to tile[bin][frame]
//   store : thread (r, j) owns frames r + 16i; of each it writes one 4-element group of the out row, cut so that the group starts
//           on a 4-element boundary of the OUTPUT (float32: 16 bytes, float16: 8 bytes; rows of S = U + 1 elements start at
//           every alignment): group g covers tile bins 4g - a .. 4g - a + 3 with a the row's misalignment, lane j takes
//           g = j, lane 0 also the partial group g = 16.
template <typename OT>
__global__ void __launch_bounds__(256) act_log_kernel(const float* __restrict__ hf0, int64_t ld, int U, int B,
                                                      const int64_t* __restrict__ offsets, int64_t total, unsigned clamp_below_bits,
                                                      float clamp_to, unsigned* __restrict__ stats, OT* __restrict__ out) {
    __shared__ float tile[kActTile * kActPitch];
    __shared__ float s_t[kActTile], s_min[kActTile];
    __shared__ int s_rec[kActTile];
    const ActTile tl = act_tile(hf0, total);
    const int tid = threadIdx.x;
    const int S = U + 1;
    if (tid < kActTile) {
        int rec = -1;
        float t = 0.f;
        if (tid >= tl.plo && tid < tl.phi) {
            rec = act_find_rec(offsets, B, tl.c0 + tid);
            const unsigned mp = stats[4 * rec + 0];
            t = mp < clamp_below_bits ? clamp_to : __uint_as_float(mp);
            if (blockIdx.y == 0 && offsets[rec] == tl.c0 + tid) reinterpret_cast<float*>(stats)[4 * rec + 2] = t;
        }
        s_rec[tid] = rec;
        s_t[tid] = t;
        s_min[tid] = INFINITY;
    }
    __syncthreads();
    const int j = tid & 15, r = tid >> 4;
    const int p0 = 4 * j;
    const bool inside = p0 >= tl.plo && p0 + 3 < tl.phi;
    const int nk = (U + kActTile - 1) / kActTile;
    float tf[4];                                              // t of this thread's four frames
    bool fok[4];
    float vmin[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = r + 16 * i;
        fok[i] = n >= tl.plo && n < tl.phi;
        tf[i] = s_t[n];
        vmin[i] = INFINITY;
    }
    float x[4][4];
    auto fetch = [&](const int k) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = k * kActTile + r + 16 * i;
#pragma unroll
            for (int q = 0; q < 4; ++q) x[i][q] = 0.f;
            if (u < U) {
                const float* __restrict__ row = hf0 + (int64_t)u * ld + tl.c0;
                if (inside && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row + p0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) x[i][q] = v[q];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (p0 + q >= tl.plo && p0 + q < tl.phi) x[i][q] = row[p0 + q];
                }
            }
        }
    };
    int k = blockIdx.y;
    if (k < nk) fetch(k);
    for (; k < nk; k += gridDim.y) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) tile[(r + 16 * i) * kActPitch + p0 + q] = x[i][q];
        __syncthreads();
        if (k + (int)gridDim.y < nk) fetch(k + gridDim.y);
        const int u0 = k * kActTile;
        const int ulen = U - u0 < kActTile ? U - u0 : kActTile;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = r + 16 * i;
            if (fok[i]) {
                OT* __restrict__ orow = out + (tl.c0 + n) * (int64_t)S + u0;
                const int a = (int)((reinterpret_cast<uintptr_t>(orow) / sizeof(OT)) & 3);
                for (int g = j; g < 17; g += 16) {
                    const int q0 = 4 * g - a;
                    if (q0 >= 0 && q0 + 3 < ulen) {
                        float y[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            y[q] = logf(tile[(q0 + q) * kActPitch + n] + tf[i]);
                            vmin[i] = fminf(vmin[i], y[q]);
                        }
                        if constexpr (sizeof(OT) == 4) {
                            f32x4 w = {y[0], y[1], y[2], y[3]};
                            *reinterpret_cast<f32x4*>(orow + q0) = w;
                        } else {
                            f16x4 w = {(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
                            *reinterpret_cast<f16x4*>(orow + q0) = w;
                        }
                    } else {
                        for (int q = 0; q < 4; ++q)
                            if (q0 + q >= 0 && q0 + q < ulen) {
                                const float y = logf(tile[(q0 + q) * kActPitch + n] + tf[i]);
                                vmin[i] = fminf(vmin[i], y);
                                orow[q0 + q] = (OT)y;
                            }
                    }
                }
            }
        }
        __syncthreads();
    }
    // minimum of the written values, per frame, then per recording
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float m = act_row16_min(vmin[i]);
        if (j == 0) s_min[r + 16 * i] = m;
    }
    __syncthreads();
    if (tid < kActTile) {
        const bool ok = tid >= tl.plo && tid < tl.phi;
        float m = ok ? s_min[tid] : INFINITY;
        const int rec0 = s_rec[tl.plo];
        if (rec0 == s_rec[tl.phi - 1]) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, 64));
            if (tid == 0 && m < INFINITY) act_atomic_min_f32(&stats[4 * rec0 + 3], m);
        } else if (ok && m < INFINITY) {
            act_atomic_min_f32(&stats[4 * s_rec[tid] + 3], m);
        }
    }
}

template <typename OT>
__global__ void __launch_bounds__(256) act_fill_kernel(int U, int B, const int64_t* __restrict__ offsets, int64_t total,
                                                       const float* __restrict__ stats, OT* __restrict__ out) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n < total) out[n * (int64_t)(U + 1) + U] = (OT)stats[4 * act_find_rec(offsets, B, n) + 3];
}

hipError_t launch_activations(const float* hf0, int64_t ld, int U, int B, const int64_t* offsets, int64_t total,
                              uint32_t clamp_below_bits, float clamp_to, float* stats, void* out, bool f16, hipStream_t st) {
    unsigned* us = reinterpret_cast<unsigned*>(stats);
    const int64_t shift = (int64_t)((reinterpret_cast<uintptr_t>(hf0) >> 2) & 3);
    const int64_t nx = (total + shift + kActTile - 1) / kActTile;
    // few frames: split the bins over blockIdx.y so that a single recording still fills the device
    const int nk = (U + kActTile - 1) / kActTile, nr = (U + 15) / 16;
    const int64_t want = (4096 + nx - 1) / nx;
    const int ny1 = (int)(want < 1 ? 1 : (want > nr ? nr : want));
    const int ny2 = (int)(want < 1 ? 1 : (want > nk ? nk : want));
    hipLaunchKernelGGL(act_init_kernel, dim3((4 * B + 255) / 256), dim3(256), 0, st, us, B);
    hipLaunchKernelGGL(act_stats_kernel, dim3((unsigned)nx, ny1), dim3(256), 0, st, hf0, ld, U, B, offsets, total, us);
    const dim3 fill((unsigned)((total + 255) / 256));
    if (f16) {
        hipLaunchKernelGGL(act_log_kernel<_Float16>, dim3((unsigned)nx, ny2), dim3(256), 0, st, hf0, ld, U, B, offsets, total,
                           clamp_below_bits, clamp_to, us, reinterpret_cast<_Float16*>(out));
        hipLaunchKernelGGL(act_fill_kernel<_Float16>, fill, dim3(256), 0, st, U, B, offsets, total, stats, reinterpret_cast<_Float16*>(out));
    } else {
        hipLaunchKernelGGL(act_log_kernel<float>, dim3((unsigned)nx, ny2), dim3(256), 0, st, hf0, ld, U, B, offsets, total,
                           clamp_below_bits, clamp_to, us, reinterpret_cast<float*>(out));
        hipLaunchKernelGGL(act_fill_kernel<float>, fill, dim3(256), 0, st, U, B, offsets, total, stats, reinterpret_cast<float*>(out));
    }
    return hipGetLastError();
}

}  // namespace vit
