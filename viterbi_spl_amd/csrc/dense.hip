// dense.hip -- dense forward kernels (any matrix): the streaming form and the matrix-resident form.
#include "device_common.hpp"

namespace vit {

// ---------------------------------------------------------------------------------------
// Dense forward kernel (any matrix): NS songs per workgroup; every thread owns one target state
// and walks all S sources four at a time.  A4[q][j][0..3] = logA_T[j][4q..4q+3] is a coalesced
// 16-byte load per lane (L2 resident, 4*S*S bytes per frame), reused for the NS songs; the delta
// vectors are read from LDS as wave-uniform (broadcast) 16-byte reads.  Value-only: two packed
// adds and two max3 per four sources.
// ---------------------------------------------------------------------------------------
template <int NS, typename ET, int KT = 1>
__global__ void __launch_bounds__(KT == 2 ? 1024 : dense_max_threads(NS)) dense_forward_kernel(FwdArgs a) {
    // KT = 2: two threads per target, each walks half of the sources (twice the waves = twice the transition loads in
    // flight: the kernel is bound by the latency of streaming the matrix through L2, not by arithmetic); the halves meet
    // through LDS once per frame.
    extern __shared__ __align__(16) unsigned char smem[];
    const int S = a.S, SP = a.SP, S4 = a.S4, T = a.T, SD = a.SD;
    float* dl = reinterpret_cast<float*>(smem);  // [2][NS][SD]
    float* part = dl + 2 * NS * SD;              // [NS][SP] partial maxima of the upper half (KT == 2)
    VI* tot = reinterpret_cast<VI*>(part + (KT == 2 ? NS * SP : 0) + ((2 * NS * SD + (KT == 2 ? NS * SP : 0)) & 1));

    const int half = KT == 2 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >= (unsigned)SP)) : 0;   // SP is a multiple of 64
    const int j = threadIdx.x - half * SP;
    const bool lead = half == 0;                 // the thread that owns target j
    const int nw = blockDim.x >> 6;
    const int song0 = blockIdx.x * NS;
    const float4* __restrict__ A4 = reinterpret_cast<const float4*>(a.image + a.off_A4);
    const float* __restrict__ log_pi = reinterpret_cast<const float*>(a.image + a.off_logpi);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE);
    const int qmid = KT == 2 ? (S4 + 1) / 2 : S4;
    const int q_lo = half ? qmid : 0, q_hi = half ? S4 : qmid;

    int Tb[NS];
    bool live[NS];
    int Tmax = 1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        live[s] = song0 + s < a.B;
        Tb[s] = live[s] ? song_length(a.lengths, song0 + s, T) : 1;
        Tmax = Tb[s] > Tmax ? Tb[s] : Tmax;
    }

    float enext[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const size_t base = (size_t)(song0 + s) * T * S;
        float d = -INFINITY;
        if (lead && live[s] && j < S) {
            d = log_pi[j] + load_e<ET>(E + base + j);
            a.hist[(size_t)(song0 + s) * T * SD + j] = d;
        }
        if (lead && j < SD) { dl[(0 * NS + s) * SD + j] = d; dl[(1 * NS + s) * SD + j] = -INFINITY; }
        enext[s] = (lead && live[s] && j < S && Tb[s] > 1) ? load_e<ET>(E + base + S + j) : 0.f;
    }
    __syncthreads();

    int cur = 0;
    for (int t = 1; t < Tmax; ++t) {
        float ecur[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            ecur[s] = enext[s];
            if (lead && live[s] && j < S && t + 1 < Tb[s])
                enext[s] = load_e<ET>(E + ((size_t)(song0 + s) * T + t + 1) * S + j);
        }
        float b0[NS], b1[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) { b0[s] = -INFINITY; b1[s] = -INFINITY; }
        const float* dcur = dl + cur * NS * SD;
#pragma unroll 8
        for (int q = q_lo; q < q_hi; ++q) {
            const float4 av = A4[(size_t)q * SP + j];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float4 dv = *reinterpret_cast<const float4*>(dcur + s * SD + 4 * q);
                b0[s] = fmaxf(fmaxf(b0[s], dv.x + av.x), dv.y + av.y);
                b1[s] = fmaxf(fmaxf(b1[s], dv.z + av.z), dv.w + av.w);
            }
        }
        if (KT == 2) {
            if (!lead) {
#pragma unroll
                for (int s = 0; s < NS; ++s) part[s * SP + j] = fmaxf(b0[s], b1[s]);
            }
            __syncthreads();
            if (lead) {
#pragma unroll
                for (int s = 0; s < NS; ++s) b0[s] = fmaxf(b0[s], part[s * SP + j]);
            }
        }
        float* dnxt = dl + (cur ^ 1) * NS * SD;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (lead && j < S) {
                if (live[s] && t < Tb[s]) {
                    const float dn = fmaxf(b0[s], b1[s]) + ecur[s];
                    dnxt[s * SD + j] = dn;
                    a.hist[((size_t)(song0 + s) * T + t) * SD + j] = dn;
                } else {
                    dnxt[s * SD + j] = dcur[s * SD + j];
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }

#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (live[s]) {
            const bool valid = lead && j < S;
            const float dj = valid ? dl[(cur * NS + s) * SD + j] : -INFINITY;
            terminal_argmax(dj, j, valid, tot, nw, a.last_state, a.loglik, song0 + s);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------
// Dense forward kernel with the matrix RESIDENT on the CU (any matrix, 64 < S <= 368; one song per workgroup).
//
// dense_forward_kernel streams 4*S*S bytes of transition entries per frame and workgroup through a 64 B/clk vector L1:
// ~8100 cycles per frame at S = 361, four times the ~2000 its S*S packed adds and maxima take.  But a CU owns 512 KB of
// vector registers and 160 KB of LDS and the matrix is 521 KB: two threads per target, each holding its half row (HS = 184
// sources) as WRG = 132 registers + 13 float4 in LDS (conflict-free [q][thread] layout), keep every entry on the CU for the
// whole song.  A frame then reads only delta_{t-1}: the half row's 46 float4 as LDS broadcast reads (the even and the odd
// lanes of a wave read two addresses), 92 packed adds + 92 max3 per thread, one DPP exchange between the two lanes of a
// target, one barrier.  Same sums, same maxima as the streaming kernel: bit-identical history rows.
// ---------------------------------------------------------------------------------------
template <int HS, int WRG, int PF, typename ET>
__global__ void __launch_bounds__(768) dense_resident_forward_kernel(FwdArgs a) {
    static_assert(HS % 4 == 0 && WRG % 4 == 0 && WRG <= HS && PF % 2 == 0, "half rows in whole quads");
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NT = 4 * HS;                   // threads that own a half row: two for each of up to 2*HS targets
    constexpr int QR = WRG / 4, QL = (HS - WRG) / 4;
    f32x4* awl = reinterpret_cast<f32x4*>(smem);             // [QL][NT]  the half rows' last QL quads
    float* dl = reinterpret_cast<float*>(awl + QL * NT);     // [2][2*HS] delta, double-buffered (entries >= S: -inf)
    VI* tot = reinterpret_cast<VI*>(dl + 4 * HS);
    const int S = a.S, SP = a.SP, S4 = a.S4, T = a.T, SD = a.SD;

    const int tid = threadIdx.x;
    const int j = tid >> 1, h = tid & 1;                     // target, half: lanes 2j and 2j+1 share target j
    const bool tvalid = j < S;
    const bool writer = tvalid && h == 0;
    const int song = blockIdx.x;
    const int Tb = song_length(a.lengths, song, T);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (size_t)song * T * S;
    float* __restrict__ hist = a.hist + (size_t)song * T * SD;
    const int jc = tvalid ? j : S - 1;

    // ---------------- the half row: quads h*HS/4 .. of row j (quads beyond S4 and idle threads: -inf)
    const f32x4 ninf4 = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    f32x4 aw[QR];
    {
        const f32x4* __restrict__ A4 = reinterpret_cast<const f32x4*>(a.image + a.off_A4);
        const int q0 = h * (HS / 4);
#pragma unroll
        for (int q = 0; q < QR; ++q) aw[q] = (tvalid && q0 + q < S4) ? A4[(size_t)(q0 + q) * SP + j] : ninf4;
        if (tid < NT) {
#pragma unroll
            for (int q = 0; q < QL; ++q) awl[q * NT + tid] = (tvalid && q0 + QR + q < S4) ? A4[(size_t)(q0 + QR + q) * SP + j] : ninf4;
        }
    }
    const int tl = tid < NT ? tid : 0;                       // (threads beyond NT own no target: j >= 2*HS >= S)
    for (int k = tid; k < 4 * HS; k += blockDim.x) dl[k] = -INFINITY;
    __syncthreads();

    // ---------------- frame 0
    {
        const float d0 = reinterpret_cast<const float*>(a.image + a.off_logpi)[jc] + load_e<ET>(E + jc);
        if (writer) { hist[j] = d0; dl[j] = d0; }
    }
    float er[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) er[k] = load_e<ET>(E + (size_t)(1 + k < Tb ? 1 + k : Tb - 1) * S + jc);
#pragma unroll
    for (int q = 0; q < QR; ++q) asm volatile("" ::"v"(aw[q].x), "v"(aw[q].y), "v"(aw[q].z), "v"(aw[q].w));
    __syncthreads();

    auto frame = [&](const int t, float& e_slot, const int RB) {
        const f32x4* __restrict__ dcur = reinterpret_cast<const f32x4*>(dl + RB * 2 * HS + h * HS);
        float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
        auto fold = [&](const f32x4 d, const f32x4 w, float& ma, float& mb) {
            const f32x2 c0_ = f32x2{d.x, d.y} + f32x2{w.x, w.y};
            const f32x2 c1_ = f32x2{d.z, d.w} + f32x2{w.z, w.w};
            ma = fmaxf(fmaxf(ma, c0_.x), c0_.y);
            mb = fmaxf(fmaxf(mb, c1_.x), c1_.y);
        };
        // Reads run one stage ahead of their use and never more: 132 weight registers leave ~16 for data in flight.
        // Register-resident weights: stages of two delta quads; weights in LDS: stages of one delta quad + its weight quad.
        {
            constexpr int NST = (QR + 1) / 2;
            f32x4 dv[2][2];
            auto issue = [&](const int c) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (2 * c + u < QR) dv[c & 1][u] = dcur[2 * c + u];
            };
            issue(0);
#pragma unroll
            for (int c = 0; c < NST; ++c) {
                if (c + 1 < NST) issue(c + 1);
                asm volatile("" ::: "memory");
                fold(dv[c & 1][0], aw[2 * c], m0, m1);
                if (2 * c + 1 < QR) fold(dv[c & 1][1], aw[2 * c + 1 < QR ? 2 * c + 1 : 0], m2, m3);
            }
        }
        {
            f32x4 dv[2], wv[2];
            auto issue = [&](const int c) {
                dv[c & 1] = dcur[QR + c];
                wv[c & 1] = awl[c * NT + tl];
            };
            if (QL > 0) issue(0);
#pragma unroll
            for (int c = 0; c < QL; ++c) {
                if (c + 1 < QL) issue(c + 1);
                asm volatile("" ::: "memory");
                if (c & 1) fold(dv[c & 1], wv[c & 1], m2, m3); else fold(dv[c & 1], wv[c & 1], m0, m1);
            }
        }
        float m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
        // the other half of the row: the neighbouring lane (quad_perm [1,0,3,2])
        m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(m), __float_as_int(m), 0xB1, 0xf, 0xf, false)));
        const float dn = m + e_slot;
        const int tn = t + PF < Tb ? t + PF : Tb - 1;
        if (writer) {
            dl[(RB ^ 1) * 2 * HS + j] = dn;
            hist[(size_t)t * SD + j] = dn;
        }
        e_slot = load_e<ET>(E + (size_t)tn * S + jc);
        __syncthreads();
    };
    int t = 1;
    for (; t + PF - 1 < Tb; t += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) frame(t + k, er[k], k & 1);
    }
#pragma unroll
    for (int k = 0; k < PF - 1; ++k)
        if (t + k < Tb) frame(t + k, er[k], k & 1);

    const int fb = (Tb - 1) & 1;                             // buffer holding delta_{Tb-1}
    terminal_argmax(writer ? dl[fb * 2 * HS + j] : -INFINITY, j, writer, tot, (int)(blockDim.x >> 6), a.last_state, a.loglik, song);
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
template <int NS, typename ET, int KT = 1>
static hipError_t launch_dense_t(const FwdArgs& a, hipStream_t st) {
    const size_t lds = sizeof(float) * (2 * NS * a.SD + (KT == 2 ? NS * a.SP : 0) + 1) + sizeof(VI) * 16;
    const int grid = (int)((a.B + NS - 1) / NS);
    hipLaunchKernelGGL((dense_forward_kernel<NS, ET, KT>), dim3(grid), dim3(KT * a.SP), lds, st, a);
    return hipGetLastError();
}

// matrix-resident dense kernel: instantiated for half rows of 64, 128 and 184 sources (64 < S <= 368)
bool dense_resident_applies(const FwdArgs& a) { return a.S > 64 && a.S <= 368 && a.dense_form != 1; }

template <int HS, int WRG>
static hipError_t launch_dense_resident_t(const FwdArgs& a, bool f16, hipStream_t st) {
    constexpr int PF = 2;
    const int threads = (2 * a.S + 63) / 64 * 64;
    const size_t lds = sizeof(float) * 4 * ((HS - WRG) / 4) * (4 * HS) + sizeof(float) * 4 * HS + sizeof(VI) * 16;
    if (f16)
        hipLaunchKernelGGL((dense_resident_forward_kernel<HS, WRG, PF, __half>), dim3((int)a.B), dim3(threads), lds, st, a);
    else
        hipLaunchKernelGGL((dense_resident_forward_kernel<HS, WRG, PF, float>), dim3((int)a.B), dim3(threads), lds, st, a);
    return hipGetLastError();
}

static hipError_t launch_dense_resident(const FwdArgs& a, bool f16, hipStream_t st) {
    // half rows of 128 sources live in registers alone (eight waves); 184 sources: 132 registers + 13 float4 in LDS (twelve waves)
    if (a.S <= 128) return launch_dense_resident_t<64, 64>(a, f16, st);
    return a.S <= 256 ? launch_dense_resident_t<128, 128>(a, f16, st) : launch_dense_resident_t<184, 132>(a, f16, st);
}

hipError_t launch_dense(const FwdArgs& a, int ns, bool f16, hipStream_t st) {
    if (dense_resident_applies(a)) return launch_dense_resident(a, f16, st);
    while (ns > 1 && a.SP > dense_max_threads(ns)) ns >>= 1;
    // one song per workgroup: two threads per target when the workgroup still fits (S <= 512)
    if (ns == 1 && 2 * a.SP <= 1024 && !a.dense_kt1)
        return f16 ? launch_dense_t<1, __half, 2>(a, st) : launch_dense_t<1, float, 2>(a, st);
    if (f16) {
        if (ns >= 8) return launch_dense_t<8, __half>(a, st);
        if (ns >= 4) return launch_dense_t<4, __half>(a, st);
        if (ns >= 2) return launch_dense_t<2, __half>(a, st);
        return launch_dense_t<1, __half>(a, st);
    }
    if (ns >= 8) return launch_dense_t<8, float>(a, st);
    if (ns >= 4) return launch_dense_t<4, float>(a, st);
    if (ns >= 2) return launch_dense_t<2, float>(a, st);
    return launch_dense_t<1, float>(a, st);
}

}  // namespace vit
