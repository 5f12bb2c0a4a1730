// step.hip -- forward kernels for step-structured matrices (plan.step_ok).
#include "device_common.hpp"

namespace vit {

// ---------------------------------------------------------------------------------------
// Step-structured forward kernel (plan.step_ok: the Durrieu matrix of imm's own decoder, S = 722).
//
// For voiced source i and voiced target j, logA_T[j][i] = C[min(|i-j| / BW, KB)][i]: column i is piecewise constant in
// distance bands of BW bins and constant from distance KB*BW on.  So fl(delta_i + logA_T[j][i]) takes only KB+1 values
// per source: every thread publishes V_k[i] = fl(delta_i + C[k][i]) for its own state, and target j takes the max of
// the band windows V_k[j + k*BW .. j + k*BW + BW) and V_k(j - k*BW - BW .. j - k*BW] -- exactly the sums the dense
// recursion forms.  The far sources (distance >= KB*BW) reduce to ONE number, M = max_i V_KB[i]: if its arg-max is far
// from j it IS the far term, if it is near, its near-band value is >= M (no near band of a column is below the far
// value: checked by the plan; rounding is monotone) and every far term is <= M.  The unvoiced source contributes one
// value to every voiced target and joins M; the unvoiced target's row is arbitrary and gets a wave of its own.
// 2*KB*BW window reads per target instead of S global transition entries: the matrix is never streamed.
// One workgroup per song.  Value-only like every forward kernel here; the generic back-trace follows.
//
// Four targets per lane, one wave per lane group (step_form 3).
//
// Same arithmetic as the one-target-per-lane form it replaced, which was bound by the LDS return path
// (359 four-byte window reads per target and frame).  With lane p owning states 4p .. 4p+3, the band windows of its four
// targets overlap in 17 of 20 sources, start on 16-byte boundaries (BW is a multiple of 4) and are read as contiguous
// float4s -- the ideal LDS pattern, a single copy of every V_k, 3.4x fewer bytes -- and the shared 17 sources are reduced
// once: ~15 instead of 40 max3 per band side for the four targets.  Three voiced waves + the unvoiced wave: one wave per SIMD.
// ---------------------------------------------------------------------------------------
template <int BW, int KB, int PF, typename ET>
__global__ void __launch_bounds__(256) step4_forward_kernel(FwdArgs a) {
    static_assert(BW == 20 && PF % 2 == 0, "written for 20-bin bands");
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NW4 = 3;                        // voiced waves: 192 lanes x 4 states
    constexpr int NPV = NW4 * 256;                // padded voiced states
    constexpr int PAD = KB * BW + BW;             // -inf margin on both sides of every V_k (multiple of 4)
    constexpr int VLEN = NPV + 2 * PAD;
    constexpr int DLEN = NPV + 64;
    constexpr int FLEN = VLEN / 4;                // quads per V_k (PAD and NPV are multiples of 4)
    float* V = reinterpret_cast<float*>(smem);    // [2][KB][VLEN]
    float* F = V + 2 * KB * VLEN;                 // [2][KB][FLEN]  F_k[u] = max of the quad V_k[4u .. 4u+3]
    float* dl = F + 2 * KB * FLEN;                // [2][DLEN]  delta of the voiced states (for the unvoiced target's row)
    float* wm = dl + 2 * DLEN;                    // [2][4]     wave maxima of V_KB, slot 3 = the unvoiced source's candidate
    float* dun = wm + 2 * 4;                      // [2]        delta of the unvoiced state
    VI* tot = reinterpret_cast<VI*>(dun + 2 + 2);
    const int S = a.S, SP = a.SP, T = a.T, SD = a.SD;
    const int n = S - 1;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int song = blockIdx.x;
    const int Tb = song_length(a.lengths, song, T);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (size_t)song * T * S;
    float* __restrict__ hist = a.hist + (size_t)song * T * SD;
    const float* __restrict__ lpi = reinterpret_cast<const float*>(a.image + a.off_logpi);

    for (int k = tid; k < 2 * KB * VLEN + 2 * KB * FLEN + 2 * DLEN + 2 * 4 + 4; k += 256) V[k] = -INFINITY;
    __syncthreads();

    const bool voiced_wave = wv < NW4;
    const int j0 = 4 * tid;                                               // voiced lanes: first of the four own states
    bool val[4];
    int col[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        val[q] = voiced_wave && j0 + q < n;
        col[q] = voiced_wave ? (j0 + q < n ? j0 + q : n - 1) : n;          // emission column loaded (unvoiced wave: column n)
    }
    const bool all4 = voiced_wave && j0 + 3 < n;
    f32x4 c[KB + 1];
    {
        const float* __restrict__ sc = reinterpret_cast<const float*>(a.image + a.off_stepC);
#pragma unroll
        for (int k = 0; k <= KB; ++k) {
            c[k].x = val[0] ? sc[(size_t)k * SP + j0 + 0] : -INFINITY;
            c[k].y = val[1] ? sc[(size_t)k * SP + j0 + 1] : -INFINITY;
            c[k].z = val[2] ? sc[(size_t)k * SP + j0 + 2] : -INFINITY;
            c[k].w = val[3] ? sc[(size_t)k * SP + j0 + 3] : -INFINITY;
        }
    }
    constexpr int NQ = 13;                                                // sources per lane of the unvoiced target's wave
    float rown[NQ];
    {
        const float* __restrict__ ar = reinterpret_cast<const float*>(a.image + a.off_Arow) + (size_t)n * SP;
#pragma unroll
        for (int q = 0; q < NQ; ++q) rown[q] = (!voiced_wave && lane + 64 * q < SP) ? ar[lane + 64 * q] : -INFINITY;
    }
    const float cn = a.step_cn;

    auto load4 = [&](const int row) -> f32x4 {
        const ET* __restrict__ r = E + (size_t)row * S;
        return f32x4{load_e<ET>(r + col[0]), load_e<ET>(r + col[1]), load_e<ET>(r + col[2]), load_e<ET>(r + col[3])};
    };
    auto store4 = [&](const int row, const f32x4 d) {
        float* __restrict__ h = hist + (size_t)row * SD;
        if (all4) {
            *reinterpret_cast<f32x4*>(h + j0) = d;
        } else if (voiced_wave) {
            if (val[0]) h[j0] = d.x;
            if (val[1]) h[j0 + 1] = d.y;
            if (val[2]) h[j0 + 2] = d.z;
        } else if (lane == 0) {
            h[n] = d.x;
        }
    };
    const f32x4 ninf4 = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    auto mask4 = [&](const f32x4 d) -> f32x4 {
        if (!voiced_wave) return d;
        return f32x4{val[0] ? d.x : -INFINITY, val[1] ? d.y : -INFINITY, val[2] ? d.z : -INFINITY, val[3] ? d.w : -INFINITY};
    };

    f32x4 dn;                                                             // delta of the own states (unvoiced wave: .x = state n, every lane)
    {
        const f32x4 e0 = load4(0);
        dn = mask4(f32x4{lpi[col[0]], lpi[col[1]], lpi[col[2]], lpi[col[3]]} + e0);
        store4(0, dn);
    }
    f32x4 er[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) er[k] = load4(1 + k < Tb ? 1 + k : Tb - 1);

    auto mx3 = [](float acc, float x, float y) { return fmaxf(fmaxf(acc, x), y); };

#ifdef VIT_TIMING_HOOKS
    const bool prof = (a.debug & 256) != 0;      // phase stamps: publish | barrier | consume | store + prefetch -> scratch[song][4*wave ..]
#else
    constexpr bool prof = false;
#endif
    unsigned long long ph0 = 0, ph1 = 0, ph2 = 0, ph3 = 0;
    auto stamp = [&]() -> unsigned long long {
        unsigned long long v;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");
        return v;
    };
    auto frame = [&](const int t, f32x4& e_slot, const int b) {
        const unsigned long long s0 = prof ? stamp() : 0ull;
        // ---- publish delta_{t-1} into buffer b
        if (voiced_wave) {
            float* vb = V + b * KB * VLEN + PAD + j0;
            float* fb = F + b * KB * FLEN + PAD / 4 + tid;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const f32x4 vq = dn + c[k];
                *reinterpret_cast<f32x4*>(vb + k * VLEN) = vq;
                fb[k * FLEN] = fmaxf(fmaxf(fmaxf(vq.x, vq.y), vq.z), vq.w);
            }
            *reinterpret_cast<f32x4*>(dl + b * DLEN + j0) = dn;
            const f32x4 vf = dn + c[KB];
            const float inc = wave_scan_max(fmaxf(fmaxf(vf.x, vf.y), fmaxf(vf.z, vf.w)));
            if (lane == 63) wm[b * 4 + wv] = inc;
        } else if (lane == 0) {
            dun[b] = dn.x;
            wm[b * 4 + 3] = dn.x + cn;
        }
        const unsigned long long s1 = prof ? stamp() : 0ull;
        __syncthreads();
        const unsigned long long s2 = prof ? stamp() : 0ull;
        // ---- consume
        f32x4 m = ninf4;
        if (voiced_wave) {
            const float* rb = V + b * KB * VLEN + PAD + j0;                 // 16-byte aligned; offsets below are relative to state j0
            const float* fr = F + b * KB * FLEN + PAD / 4 + tid;          // own quad's slot in F_0
            // A stage is one 24-source read window (six quads Q0 .. Q5 from a 16-byte aligned base): the four targets share the
            // four inner quads whole, so those arrive as their published maxima F (four floats) and only Q0 and Q5 are read in
            // full -- 2 ds_read_b128 + 4 ds_read_b32 and ~9 max operations per stage instead of 6 ds_read_b128 and ~19.
            // Stage 0, 1: band 0 (left-type window ending at the target, right-type window starting at it; the target's own
            // source is in both, which a maximum does not mind); stage 2k, 2k+1: band k right, left.
            // One wave per SIMD: nothing else covers the LDS latency, so the reads run LA stages ahead of the maxima.
            constexpr int LA = 3;                                         // stages in flight ahead of the one being reduced
            f32x4 q0[LA + 1], q5[LA + 1], fq[LA + 1];
            auto issue = [&](const int st) {
                const int k = st >> 1;
                const int qrel = st == 0 ? -5 : (st == 1 ? 0 : ((st & 1) ? -5 * k - 5 : 5 * k));     // first quad, relative to the own one
                const float* base = rb + k * VLEN + 4 * qrel;
                const float* fbase = fr + k * FLEN + qrel;
                q0[st % (LA + 1)] = *reinterpret_cast<const f32x4*>(base);
                q5[st % (LA + 1)] = *reinterpret_cast<const f32x4*>(base + 20);
                fq[st % (LA + 1)] = f32x4{fbase[1], fbase[2], fbase[3], fbase[4]};
            };
            float core = -INFINITY;                                       // sources every one of the four targets takes
            // right-type window (sources base .. base+23): target q takes read offsets q .. q+19
            auto reduce_right = [&](const int st) {
                const f32x4 a0 = q0[st % (LA + 1)], a5 = q5[st % (LA + 1)], f = fq[st % (LA + 1)];
                core = mx3(mx3(core, a0.w, f.x), f.y, fmaxf(f.z, f.w));
                const float lo2 = fmaxf(a0.y, a0.z), hi2 = fmaxf(a5.x, a5.y);
                m.x = mx3(m.x, a0.x, lo2);
                m.y = mx3(m.y, lo2, a5.x);
                m.z = mx3(m.z, a0.z, hi2);
                m.w = mx3(m.w, hi2, a5.z);
                // the element no target takes stays live up to here: a register that is dead on arrival is handed to the next
                // stage's address arithmetic, which then has to wait for this read to land (a queue drain per stage)
                asm volatile("" ::"v"(a5.w));
            };
            // left-type window (sources c-20 .. c+3, c the target-0 end of the window): target q takes read offsets q+1 .. q+20
            auto reduce_left = [&](const int st) {
                const f32x4 a0 = q0[st % (LA + 1)], a5 = q5[st % (LA + 1)], f = fq[st % (LA + 1)];
                core = mx3(mx3(core, a5.x, f.x), f.y, fmaxf(f.z, f.w));
                const float lo2 = fmaxf(a0.z, a0.w), hi2 = fmaxf(a5.y, a5.z);
                m.x = mx3(m.x, a0.y, lo2);
                m.y = mx3(m.y, lo2, a5.y);
                m.z = mx3(m.z, a0.w, hi2);
                m.w = mx3(m.w, hi2, a5.w);
                asm volatile("" ::"v"(a0.x));
            };
#pragma unroll
            for (int st = 0; st < LA; ++st) issue(st);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int st = 0; st < 2 * KB; ++st) {
                if (st + LA < 2 * KB) issue(st + LA);
                asm volatile("" ::: "memory");
                if (st & 1) {
                    if (st == 1) reduce_right(st); else reduce_left(st);
                } else {
                    if (st == 0) reduce_left(st); else reduce_right(st);
                }
            }
            m = f32x4{fmaxf(m.x, core), fmaxf(m.y, core), fmaxf(m.z, core), fmaxf(m.w, core)};
            // the far sources and the unvoiced source: one maximum
            const f32x4 w = *reinterpret_cast<const f32x4*>(wm + b * 4);
            const float M = fmaxf(fmaxf(w.x, w.y), fmaxf(w.z, w.w));
            m = f32x4{fmaxf(m.x, M), fmaxf(m.y, M), fmaxf(m.z, M), fmaxf(m.w, M)};
        } else {
            // the unvoiced target: every source through its own (arbitrary) row
            float mm = -INFINITY;
            const float du = dun[b];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int i = lane + 64 * q;                               // < DLEN; entries n .. DLEN-1 of dl hold -inf
                const float d = i == n ? du : dl[b * DLEN + i];
                mm = fmaxf(mm, d + rown[q]);
            }
            m.x = wave_max_all(mm);
        }
        dn = mask4(m + e_slot);
        const unsigned long long s3 = prof ? stamp() : 0ull;
        const int tn = t + PF < Tb ? t + PF : Tb - 1;
        store4(t, dn);
        e_slot = load4(tn);
        if (prof) {
            const unsigned long long s4 = stamp();
            ph0 += s1 - s0; ph1 += s2 - s1; ph2 += s3 - s2; ph3 += s4 - s3;
        }
    };
    int t = 1;
    for (; t + PF - 1 < Tb; t += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) frame(t + k, er[k], (k + 1) & 1);
    }
#pragma unroll
    for (int k = 0; k < PF - 1; ++k)
        if (t + k < Tb) frame(t + k, er[k], (k + 1) & 1);
    if (prof && lane == 0 && Tb > 1) {
        float* o = a.fmax + (size_t)song * 64 + 4 * wv;
        const float nf = (float)(Tb - 1);
        o[0] = (float)ph0 / nf; o[1] = (float)ph1 / nf; o[2] = (float)ph2 / nf; o[3] = (float)ph3 / nf;
    }

    // terminal state: lowest-index argmax; a voiced lane holds four adjacent states
    __syncthreads();
    {
        VI x = vi_identity();
        if (voiced_wave) {
            if (val[0]) x = VI{dn.x, j0};
            if (val[1]) x = op_fwd(x, VI{dn.y, j0 + 1});
            if (val[2]) x = op_fwd(x, VI{dn.z, j0 + 2});
            if (val[3]) x = op_fwd(x, VI{dn.w, j0 + 3});
        } else if (lane == 0) {
            x = VI{dn.x, n};
        }
        x = wave_scan<false>(x);
        if (lane == 63) tot[wv] = x;
        __syncthreads();
        if (tid == 0) {
            VI acc = vi_identity();
            for (int bq = 0; bq < 4; ++bq) acc = op_fwd(acc, tot[bq]);
            if (acc.i == kBig) acc.i = 0;
            a.last_state[song] = acc.i;
            if (a.loglik) a.loglik[song] = acc.v;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Step-structured forward kernel, four targets per lane, the bands split over two waves per lane group (what runs for
// the Durrieu matrix).
//
// Same arithmetic as step4_forward_kernel.  With one workgroup per CU (B = 256 on 256 CUs) that kernel has one wave per
// SIMD, and a lone wave issues one vector instruction per ~4 cycles: its ~50 publish and ~270 consume instructions ARE the
// frame time.  Here every group of 192 lanes x 4 states exists twice: waves 0-2 (half A) publish V_k and F_k for the bands
// k = 0..4 and delta itself and reduce the read stages 0..9, waves 3-5 (half B) take k = 5..8, the far-band maximum and the
// stages 10..17; the halves swap their partial maxima through LDS (one float4 each way) behind a second barrier and both form
// delta_t.  Two waves per SIMD issue alternately (2 cycles per instruction), each half moves half the bytes through the LDS
// store path, and with a barrier on either side of the reads V needs no second buffer: 60 KB of LDS instead of 112.
// ---------------------------------------------------------------------------------------
// LDS of step4s_forward_kernel, in floats: what the kernel carves and what its launchers ask for
template <int BW, int KB>
struct Step4sLds {
    static constexpr int NQL = 192;                      // lanes per half: 192 x 4 states
    static constexpr int NPV = 4 * NQL;                  // padded voiced states
    static constexpr int PAD = KB * BW + BW;             // -inf margin on both sides of every V_k (multiple of 4)
    static constexpr int VLEN = NPV + 2 * PAD;
    static constexpr int FLEN = VLEN / 4;
    static constexpr int DLEN = NPV + 64;
    static constexpr int V = 0;                          // [KB][VLEN]
    static constexpr int F = V + KB * VLEN;              // [KB][FLEN]  F_k[u] = max of the quad V_k[4u .. 4u+3]
    static constexpr int dl = F + KB * FLEN;             // [DLEN]      delta of the voiced states (for the unvoiced target's row)
    static constexpr int X = dl + DLEN;                  // [2][NQL] f32x4: partial maxima of the two halves
    static constexpr int wm = X + 2 * NQL * 4;           // [4]  wave maxima of V_KB (half B), slot 3 = the unvoiced source's candidate
    static constexpr int dun = wm + 4;                   // [1 (+3)]    delta of the unvoiced state
    static constexpr int reset = dun + 4;                // floats that go to -inf before a song: everything up to here
    static constexpr int tot = reset;                    // [16] VI
    static constexpr int end = tot + 16 * (int)(sizeof(VI) / sizeof(float));
    static_assert(sizeof(float) * end <= kLdsBytes, "one workgroup's LDS");
    static constexpr size_t bytes() { return sizeof(float) * end; }
};

// WV = Packed is the packed variant (vit_decode_packed): the workgroup is a slot and decodes the songs
// slot_songs[slot_begin[w] .. slot_begin[w+1]) back to back, rows of a song at offsets[song] of the packed buffers.  The band
// tables c[] and rown[] stay in registers; V, F, dl, X, wm and dun go back to -inf between two songs, behind a barrier.
// WV = Ckpt is the checkpoint / resume variant (vit_decode_checkpointed), driven by the FwdArgs fields the wave form uses.  The only
// state this kernel carries from frame to frame is dn (V, F, dl, X, wm and dun are published anew every frame), so
//   pass 1 (ckpt_every = K > 0): every frame; frame mK - 1 is stored to row m - 1 of the song's hist_rows rows, every other frame to
//     its last row (scratch);
//   segment (ckpt_every = 0): frames t_begin .. min(length, t_end) - 1, row t stored at t - t_begin; t_begin > 0 loads dn from
//     init_rows[song] = delta_{t_begin - 1} instead of forming log_pi + e_0.  A workgroup whose song ended before t_begin leaves
//     without writing; the terminal state is pass 1's business.
// WV = PackedCkpt is the packed-checkpoint variant (vit_decode_packed_bounded), the slot walk of Packed joined with the stores of Ckpt, in two modes
// told apart by a.unit_song (uniform over the launch):
//   pass 1 (unit_song null): the workgroup is a slot and walks its songs as in Packed; of song b only the rows in front of its segments
//     1 .. n_b - 1 are kept (frames t with (t + 1) % K == 0 and t + 1 < T_b, K = ckpt_every), at rows ckpt_base[b] .. of a.hist; every
//     other store goes to the slot's scratch row hist_rows + slot; the terminal state and the log-likelihood are written per song;
//   unit (unit_song set): Ckpt's segment per workgroup: workgroup u runs the K frames of segment unit_seg[u] of song unit_song[u] (emission
//     rows at offsets[song]) from row ckpt_base[song] + segment - 1 of init_rows (segment 0: from the prior) into rows u * hist_rows ..
// WV = Stream is the session variant (vit_stream_append): the workgroup's song gets its next cnt frames t0 .. t0 + cnt - 1 (wg_cursor.inc;
// cnt = 0 leaves without writing) from the rows of its chunk; rows are stored at their absolute index as Plain stores them, t0 > 0 loads
// dn from row t0 - 1 of the song's own rows, and the terminal state and log-likelihood are written after every launch.
// WV = Plain compiles to the code it was before the variants existed.  (PK / CK / PC / ST below: WV is that variant; PKx / CKx: what the
// packed-checkpoint variant shares with the packed and with the checkpoint / resume variant; RSx: CKx or ST.)
template <int BW, int KB, int PF, typename ET, WgVariant WV = WgVariant::Plain>
__global__ void __launch_bounds__(448) step4s_forward_kernel(FwdArgs a) {
    static_assert(BW == 20 && KB == 9 && PF % 2 == 0, "written for nine 20-bin bands");
    using L = Step4sLds<BW, KB>;
    constexpr bool PK = WV == WgVariant::Packed, CK = WV == WgVariant::Ckpt, PC = WV == WgVariant::PackedCkpt;
    constexpr bool PKx = PK || PC;                // the song loop and its per-song preamble
    constexpr bool CKx = CK || PC;                // the row selection of the stores, the resumed first frame
    constexpr bool ST = WV == WgVariant::Stream;  // the frames of one launch of a session, rows at their absolute index
    constexpr bool RSx = CKx || ST;               // the frame loop starts at t1 (a launch may resume a song)
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NQL = L::NQL, PAD = L::PAD, VLEN = L::VLEN, FLEN = L::FLEN;
    constexpr int KA = 5;                         // half A: bands 0 .. KA-1; half B: KA .. KB-1 and the far band KB
    constexpr int NST = 2 * KB, STA = 10;         // read stages; half A takes 0 .. STA-1 (half B also reduces the far band and scans)
    float* V = reinterpret_cast<float*>(smem) + L::V;
    float* F = V + L::F;
    float* dl = V + L::dl;
    f32x4* X = reinterpret_cast<f32x4*>(V + L::X);
    float* wm = V + L::wm;
    float* dun = V + L::dun;
    VI* tot = reinterpret_cast<VI*>(V + L::tot);
    const int S = a.S, SP = a.SP, T = a.T, SD = a.SD;
    const int n = S - 1;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wv < 3 ? 0 : (wv < 6 ? 1 : 2);                        // 2: the unvoiced state's wave
    const int ql = tid - NQL * (half == 1 ? 1 : 0);                       // lane within the half (halves 0, 1)
    constexpr int kPast = 0, kRowBias = 0;        // a segment ends with its last frame; rows are stored at their own index
#define VIT_WG_CURSOR 1
#include "wg_cursor.inc"
    const float* __restrict__ lpi = reinterpret_cast<const float*>(a.image + a.off_logpi);
#define VIT_WG_CURSOR 2
#include "wg_cursor.inc"

    for (int k = tid; k < L::reset; k += 448) V[k] = -INFINITY;
    __syncthreads();

    const bool voiced_wave = half < 2;
    const int j0 = 4 * ql;                                                // voiced lanes: first of the four own states
    bool val[4];
    int col[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        val[q] = voiced_wave && j0 + q < n;
        col[q] = voiced_wave ? (j0 + q < n ? j0 + q : n - 1) : n;          // emission column loaded (unvoiced wave: column n)
    }
    const bool all4 = voiced_wave && j0 + 3 < n;
    const int k0 = half == 1 ? KA : 0;                                    // first band of this half
    f32x4 c[KA];                                                          // half A: C_0 .. C_4; half B: C_5 .. C_8 and the far band C_9
    {
        const float* __restrict__ sc = reinterpret_cast<const float*>(a.image + a.off_stepC);
#pragma unroll
        for (int i = 0; i < KA; ++i) {
            const int k = k0 + i;
            c[i].x = val[0] ? sc[(size_t)k * SP + j0 + 0] : -INFINITY;
            c[i].y = val[1] ? sc[(size_t)k * SP + j0 + 1] : -INFINITY;
            c[i].z = val[2] ? sc[(size_t)k * SP + j0 + 2] : -INFINITY;
            c[i].w = val[3] ? sc[(size_t)k * SP + j0 + 3] : -INFINITY;
        }
    }
    constexpr int NQ = 13;                                                // sources per lane of the unvoiced target's wave
    float rown[NQ];
    {
        const float* __restrict__ ar = reinterpret_cast<const float*>(a.image + a.off_Arow) + (size_t)n * SP;
#pragma unroll
        for (int q = 0; q < NQ; ++q) rown[q] = (!voiced_wave && lane + 64 * q < SP) ? ar[lane + 64 * q] : -INFINITY;
    }
    const float cn = a.step_cn;

    auto load4 = [&](const int row) -> f32x4 {
        const ET* __restrict__ r = E + (size_t)row * S;
        return f32x4{load_e<ET>(r + col[0]), load_e<ET>(r + col[1]), load_e<ET>(r + col[2]), load_e<ET>(r + col[3])};
    };
    auto store4 = [&](const int row, const f32x4 d) {                     // half A and the unvoiced wave only
        float* __restrict__ h = hist + (size_t)row * SD;
        if (half == 0) {
            if (all4) {
                *reinterpret_cast<f32x4*>(h + j0) = d;
            } else {
                if (val[0]) h[j0] = d.x;
                if (val[1]) h[j0 + 1] = d.y;
                if (val[2]) h[j0 + 2] = d.z;
            }
        } else if (half == 2 && lane == 0) {
            h[n] = d.x;
        }
    };
    auto mask4 = [&](const f32x4 d) -> f32x4 {
        if (!voiced_wave) return d;
        return f32x4{val[0] ? d.x : -INFINITY, val[1] ? d.y : -INFINITY, val[2] ? d.z : -INFINITY, val[3] ? d.w : -INFINITY};
    };
    auto mx3 = [](float acc, float x, float y) { return fmaxf(fmaxf(acc, x), y); };

    f32x4 dn;                                                             // delta of the own states (unvoiced wave: .x = state n, every lane)
    if constexpr (CKx) {                                                  // frame 0 (pass 1: into the scratch row), or the checkpoint row
        if (t0 > 0) {
            const float* __restrict__ ir = PC ? pc_init : a.init_rows + (size_t)song * a.init_stride;
            dn = mask4(f32x4{ir[col[0]], ir[col[1]], ir[col[2]], ir[col[3]]});
        } else {
            const f32x4 e0 = load4(0);
            dn = mask4(f32x4{lpi[col[0]], lpi[col[1]], lpi[col[2]], lpi[col[3]]} + e0);
            store4(ck_every > 0 ? ck_scratch : 0, dn);
        }
    } else if constexpr (ST) {                                            // frame 0, or the song's own row in front of this launch's first frame
        if (t0 > 0) {
            const float* __restrict__ ir = hist + (size_t)(t0 - 1) * SD;
            dn = mask4(f32x4{ir[col[0]], ir[col[1]], ir[col[2]], ir[col[3]]});
        } else {
            const f32x4 e0 = load4(0);
            dn = mask4(f32x4{lpi[col[0]], lpi[col[1]], lpi[col[2]], lpi[col[3]]} + e0);
            store4(0, dn);
        }
    } else {
        const f32x4 e0 = load4(0);
        dn = mask4(f32x4{lpi[col[0]], lpi[col[1]], lpi[col[2]], lpi[col[3]]} + e0);
        store4(0, dn);
    }
    f32x4 er[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) er[k] = load4((RSx ? t1 : 1) + k < Tb ? (RSx ? t1 : 1) + k : Tb - 1);

#ifdef VIT_TIMING_HOOKS
    const bool prof = !PKx && !CKx && (a.debug & 256) != 0;      // phase stamps: publish | barrier | reads | exchange + store -> scratch[song][4*wave ..]
#else
    constexpr bool prof = false;
#endif
    unsigned long long ph0 = 0, ph1 = 0, ph2 = 0, ph3 = 0;
    auto stamp = [&]() -> unsigned long long {
        unsigned long long v;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");
        return v;
    };

    const float* rb = V + PAD + j0;                                       // own quad in V_0 (16-byte aligned)
    const float* fr = F + PAD / 4 + ql;                                   // own quad's slot in F_0

    // reads of one stage (see step4_forward_kernel): Q0, Q5 in full, the four inner quads as their maxima
    struct Stage { f32x4 q0, q5, f; };
    auto issue = [&](const int st) -> Stage {
        const int k = st >> 1;
        const int qrel = st == 0 ? -5 : (st == 1 ? 0 : ((st & 1) ? -5 * k - 5 : 5 * k));
        const float* base = rb + k * VLEN + 4 * qrel;
        const float* fbase = fr + k * FLEN + qrel;
        Stage r;
        r.q0 = *reinterpret_cast<const f32x4*>(base);
        r.q5 = *reinterpret_cast<const f32x4*>(base + 20);
        r.f = f32x4{fbase[1], fbase[2], fbase[3], fbase[4]};
        return r;
    };

    auto frame = [&](const int t, f32x4& e_slot) {
        const unsigned long long s0 = prof ? stamp() : 0ull;
        // ---- publish delta_{t-1}
        if (voiced_wave) {
            float* vb = V + PAD + j0 + k0 * VLEN;
            float* fb = F + PAD / 4 + ql + k0 * FLEN;
#pragma unroll
            for (int i = 0; i < KA; ++i) {
                if (i < KA - 1 || half == 0) {                            // half B's fifth constant is the far band
                    const f32x4 vq = dn + c[i];
                    *reinterpret_cast<f32x4*>(vb + i * VLEN) = vq;
                    fb[i * FLEN] = fmaxf(fmaxf(fmaxf(vq.x, vq.y), vq.z), vq.w);
                }
            }
            if (half == 0) *reinterpret_cast<f32x4*>(dl + j0) = dn;
            if (half == 1) {
                const f32x4 vf = dn + c[KA - 1];
                const float inc = wave_scan_max(fmaxf(fmaxf(vf.x, vf.y), fmaxf(vf.z, vf.w)));
                if (lane == 63) wm[wv - 3] = inc;
            }
        } else if (lane == 0) {
            dun[0] = dn.x;
            wm[3] = dn.x + cn;
        }
        const unsigned long long s1 = prof ? stamp() : 0ull;
        __syncthreads();
        const unsigned long long s2 = prof ? stamp() : 0ull;
        // ---- reads
        f32x4 m = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (voiced_wave) {
            float core = -INFINITY;                                       // sources every one of the four targets takes
            auto reduce_right = [&](const Stage& r) {                     // target q takes read offsets q .. q+19
                const f32x4 a0 = r.q0, a5 = r.q5, f = r.f;
                core = mx3(mx3(core, a0.w, f.x), f.y, fmaxf(f.z, f.w));
                const float lo2 = fmaxf(a0.y, a0.z), hi2 = fmaxf(a5.x, a5.y);
                m.x = mx3(m.x, a0.x, lo2);
                m.y = mx3(m.y, lo2, a5.x);
                m.z = mx3(m.z, a0.z, hi2);
                m.w = mx3(m.w, hi2, a5.z);
                asm volatile("" ::"v"(a5.w));                             // (keeps a dead-on-arrival register out of the address arithmetic)
            };
            auto reduce_left = [&](const Stage& r) {                      // target q takes read offsets q+1 .. q+20
                const f32x4 a0 = r.q0, a5 = r.q5, f = r.f;
                core = mx3(mx3(core, a5.x, f.x), f.y, fmaxf(f.z, f.w));
                const float lo2 = fmaxf(a0.z, a0.w), hi2 = fmaxf(a5.y, a5.z);
                m.x = mx3(m.x, a0.y, lo2);
                m.y = mx3(m.y, lo2, a5.y);
                m.z = mx3(m.z, a0.w, hi2);
                m.w = mx3(m.w, hi2, a5.w);
                asm volatile("" ::"v"(a0.x));
            };
            constexpr int LA = 2;                                         // stages in flight ahead of the one being reduced
            auto run = [&](auto first, auto last) {
                constexpr int ST0 = decltype(first)::value, ST1 = decltype(last)::value;
                Stage buf[LA + 1];
#pragma unroll
                for (int st = ST0; st < ST0 + LA; ++st) buf[(st - ST0) % (LA + 1)] = issue(st);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int st = ST0; st < ST1; ++st) {
                    if (st + LA < ST1) buf[(st + LA - ST0) % (LA + 1)] = issue(st + LA);
                    asm volatile("" ::: "memory");
                    const bool left = st == 0 || (st >= 2 && (st & 1));
                    if (left) reduce_left(buf[(st - ST0) % (LA + 1)]); else reduce_right(buf[(st - ST0) % (LA + 1)]);
                }
            };
            if (half == 0) {
                run(std::integral_constant<int, 0>{}, std::integral_constant<int, STA>{});
            } else {
                run(std::integral_constant<int, STA>{}, std::integral_constant<int, NST>{});
                const f32x4 w = *reinterpret_cast<const f32x4*>(wm);        // the far sources and the unvoiced source: one maximum
                core = fmaxf(core, fmaxf(fmaxf(w.x, w.y), fmaxf(w.z, w.w)));
            }
            m = f32x4{fmaxf(m.x, core), fmaxf(m.y, core), fmaxf(m.z, core), fmaxf(m.w, core)};
            X[half * NQL + ql] = m;
        } else {
            // the unvoiced target: every source through its own (arbitrary) row
            float mm = -INFINITY;
            const float du = dun[0];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int i = lane + 64 * q;                               // < DLEN; entries n .. DLEN-1 of dl hold -inf
                const float d = i == n ? du : dl[i];
                mm = fmaxf(mm, d + rown[q]);
            }
            m.x = wave_max_all(mm);
        }
        const unsigned long long s3 = prof ? stamp() : 0ull;
        __syncthreads();
        // ---- both halves form delta_t
        if (voiced_wave) {
            const f32x4 o = X[(1 - half) * NQL + ql];
            m = f32x4{fmaxf(m.x, o.x), fmaxf(m.y, o.y), fmaxf(m.z, o.z), fmaxf(m.w, o.w)};
        }
        dn = mask4(m + e_slot);
        const int tn = t + PF < Tb ? t + PF : Tb - 1;
        if constexpr (CKx) {        // a segment stores frame t at t - t0, pass 1 at the next checkpoint row or the scratch row (scalar selects)
            int row = t - t0;
#define VIT_WG_CURSOR 3
#include "wg_cursor.inc"
            store4(row, dn);
        } else {
            store4(t, dn);
        }
        e_slot = load4(tn);
        if (prof) {
            const unsigned long long s4 = stamp();
            ph0 += s1 - s0; ph1 += s2 - s1; ph2 += s3 - s2; ph3 += s4 - s3;
        }
    };
    // ---------------- one pass per song (PK: the songs of the slot, back to back)
    for (;;) {
        int t = RSx ? t1 : 1;
        for (; t + PF - 1 < Tb; t += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) frame(t + k, er[k]);
        }
#pragma unroll
        for (int k = 0; k < PF - 1; ++k)
            if (t + k < Tb) frame(t + k, er[k]);
        if (prof && lane == 0 && Tb > 1) {
            float* o = a.fmax + (size_t)song * 64 + 4 * wv;
            const float nf = (float)(Tb - 1);
            o[0] = (float)ph0 / nf; o[1] = (float)ph1 / nf; o[2] = (float)ph2 / nf; o[3] = (float)ph3 / nf;
        }

        // terminal state: lowest-index argmax over half A's lanes (four adjacent states each) and the unvoiced state
        // (CK: pass 1 only -- a uniform test, every thread reaches the barriers or none does)
        __syncthreads();
        if (!CKx || ck_every > 0) {
            VI x = vi_identity();
            if (half == 0) {
                if (val[0]) x = VI{dn.x, j0};
                if (val[1]) x = op_fwd(x, VI{dn.y, j0 + 1});
                if (val[2]) x = op_fwd(x, VI{dn.z, j0 + 2});
                if (val[3]) x = op_fwd(x, VI{dn.w, j0 + 3});
            } else if (half == 2 && lane == 0) {
                x = VI{dn.x, n};
            }
            x = wave_scan<false>(x);
            if (lane == 63) tot[wv] = x;
            __syncthreads();
            if (tid == 0) {
                VI acc = vi_identity();
                for (int bq = 0; bq < 7; ++bq) acc = op_fwd(acc, tot[bq]);
                if (acc.i == kBig) acc.i = 0;
                a.last_state[song] = acc.i;
                if (a.loglik) a.loglik[song] = acc.v;
            }
        }
        if constexpr (!PKx) {
            break;
        } else {
            if (++si >= si_end) break;                                        // (PC, unit: si_end = 1)
            take_song();
            // every wave is past its last read of the song before V, F, dl, X, wm and dun go back to -inf, and none publishes
            // frame 0 of the next song before they have
            __syncthreads();
            for (int k = tid; k < L::reset; k += 448) V[k] = -INFINITY;
            __syncthreads();
            {                                                             // frame 0 and the first PF emission rows, as above
                const f32x4 e0 = load4(0);
                int cq[4] = {col[0], col[1], col[2], col[3]};             // (opaque: the prior's addresses are formed here, per song)
                asm volatile("" : "+v"(cq[0]), "+v"(cq[1]), "+v"(cq[2]), "+v"(cq[3]));
                dn = mask4(f32x4{lpi[cq[0]], lpi[cq[1]], lpi[cq[2]], lpi[cq[3]]} + e0);
                store4(PC ? ck_scratch : 0, dn);                          // (PC reaches here in pass 1 only)
            }
#pragma unroll
            for (int k = 0; k < PF; ++k) er[k] = load4(1 + k < Tb ? 1 + k : Tb - 1);
        }
    }
}

// step4s_forward_kernel<.., WV = V>: one workgroup per song (Plain, Ckpt), per slot (Packed, PackedCkpt pass 1) or per unit (PackedCkpt,
// a.unit_song set); with `per_cu` the occupancy query of that instantiation instead of the launch
template <WgVariant V>
static hipError_t step4s_launch(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu) {
    constexpr int BW = 20, KB = 9, PF = 2;
    constexpr size_t ldss = Step4sLds<BW, KB>::bytes();
    const bool per_song = V == WgVariant::Plain || V == WgVariant::Ckpt || V == WgVariant::Stream || (V == WgVariant::PackedCkpt && a.unit_song);
    auto go = [&](auto kern) -> hipError_t {
        if (per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, 448, ldss);
        hipLaunchKernelGGL(kern, dim3(per_song ? (int)a.B : a.n_slots), dim3(448), ldss, st, a);
        return hipGetLastError();
    };
    return f16 ? go(step4s_forward_kernel<BW, KB, PF, __half, V>) : go(step4s_forward_kernel<BW, KB, PF, float, V>);
}
// (defined at the end of the file: the Stream kernels are emitted behind every earlier kernel, whose code then keeps its place)
static hipError_t step_stream(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu);
static hipError_t step_variant(const FwdArgs& a, WgVariant v, bool f16, hipStream_t st, int* per_cu) {
    if (!step_kernel_instantiated(a.S, a.step_bw, a.step_kb)) return hipErrorInvalidConfiguration;
    switch (v) {
        case WgVariant::Packed: return step4s_launch<WgVariant::Packed>(a, f16, st, per_cu);
        case WgVariant::Ckpt: return step4s_launch<WgVariant::Ckpt>(a, f16, st, per_cu);
        case WgVariant::PackedCkpt: return step4s_launch<WgVariant::PackedCkpt>(a, f16, st, per_cu);
        case WgVariant::Stream: return step_stream(a, f16, st, per_cu);
        default: return hipErrorInvalidValue;   // (Plain is launch_step's)
    }
}

hipError_t launch_step_variant(const FwdArgs& a, WgVariant v, bool f16, hipStream_t st) {
    // (the checkpoint / resume entry has always asked for the instantiation first, the packed ones for their arguments)
    if (v == WgVariant::Ckpt && !step_kernel_instantiated(a.S, a.step_bw, a.step_kb)) return hipErrorInvalidConfiguration;
    if (!wg_variant_args_ok(a, v, 0)) return hipErrorInvalidValue;
    return step_variant(a, v, f16, st, nullptr);
}

hipError_t step_variant_resident(const FwdArgs& a, WgVariant v, bool f16, int* per_cu) { return step_variant(a, v, f16, nullptr, per_cu); }

hipError_t launch_step(const FwdArgs& a, bool f16, hipStream_t st) {
    constexpr int BW = 20, KB = 9, PF = 2;
    if (!step_kernel_instantiated(a.S, a.step_bw, a.step_kb)) return hipErrorInvalidConfiguration;
    // four targets per lane, bands split over two waves (step_form 3: one wave)
    if (a.step_form != 3) return step4s_launch<WgVariant::Plain>(a, f16, st, nullptr);
    constexpr int VL4 = 768 + 2 * (KB * BW + BW);
    const size_t lds4 = sizeof(float) * (2 * KB * VL4 + 2 * KB * (VL4 / 4) + 2 * (768 + 64) + 2 * 4 + 4) + sizeof(VI) * 16;
    if (f16)
        hipLaunchKernelGGL((step4_forward_kernel<BW, KB, PF, __half>), dim3((int)a.B), dim3(256), lds4, st, a);
    else
        hipLaunchKernelGGL((step4_forward_kernel<BW, KB, PF, float>), dim3((int)a.B), dim3(256), lds4, st, a);
    return hipGetLastError();
}

static hipError_t step_stream(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu) { return step4s_launch<WgVariant::Stream>(a, f16, st, per_cu); }

}  // namespace vit
