// banded_floor.inc -- the one-target floor-max forward kernel (banded_floor_forward_kernel), its device helpers, its LDS layout and the
// launch of its variants, shared by the translation units that instantiate it: banded.hip (plain, packed and checkpoint / resume
// variants) and banded_pc.hip (the packed-checkpoint variant).  Included inside namespace vit, after device_common.hpp.  The scheme is
// described in banded.hip.
// Global row access with a wave-uniform row base: a raw buffer descriptor (stride 0, no range limit) built on the SALU and
// the lane's 32-bit byte offset -- no 64-bit per-lane address arithmetic on the VALU.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void* row) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(row), (short)0, -1, 0x00020000);
}
// `soff` is the instruction's scalar byte offset (wave-uniform): a kernel that keeps one descriptor for a round of frames passes the
// frame's row distance here instead of rebuilding the descriptor per frame (the split kernel, banded.hip).
__device__ __forceinline__ void row_store_f32(float* row, unsigned off, float v, unsigned soff = 0) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), row_rsrc(row), off, soff, 0);
}
template <typename ET>
__device__ __forceinline__ float row_load_e(const ET* row, unsigned off, unsigned soff = 0);
template <>
__device__ __forceinline__ float row_load_e<float>(const float* row, unsigned off, unsigned soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(row_rsrc(row), off, soff, 0));
}
template <>
__device__ __forceinline__ float row_load_e<__half>(const __half* row, unsigned off, unsigned soff) {
    return __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(row_rsrc(row), off, soff, 0)));
}

// Frame-maximum slots of the floor-max kernel: a two-step DPP max over each quad of lanes, then lane l adds into slot
// 4 * (l & 3) + ((l >> 2) & 3) -- slots 0..3 between them see all sixteen quads; slots 4..15 are written and never read.
inline constexpr int kFmGroups = 4;                       // slot groups in rotation (written, read, being reset, idle)
inline constexpr int kFmGroupFloats = 64;                 // a group's 16 slots + the rest of the reset wave's 64 lanes
inline constexpr int kFmSlots = 4;                        // slots read back per frame
__device__ __forceinline__ int fm_slot(int lane) { return 4 * (lane & 3) + ((lane >> 2) & 3); }
// max over the lane's quad, then a no-return ds_max_f32 into its slot
__device__ __forceinline__ void fm_publish(float* slot, float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xb1, 0xf, 0xf, false)));   // quad_perm:[1,0,3,2]
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4e, 0xf, 0xf, false)));   // quad_perm:[2,3,0,1]
    __hip_atomic_fetch_max(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

#ifdef VIT_TIMING_HOOKS
// Per-wave probe of the floor kernels (timing option 64; hooks builds only, the <.., WPR = true> instantiations of the
// S = 361 production shape).  Every wave accumulates over its frames
//   work = s_memtime at "last max3 done" (just before the publication) - s_memtime right after the preceding barrier
//   wait = s_memtime after the barrier release - s_memtime after the s_waitcnt lgkmcnt(0) in front of the barrier
//   data = s_memtime behind the frame's first s_waitcnt (M's slot quad, in the trimmed full waves together with the first pair of window
//          quads) - s_memtime right after the preceding barrier: barrier release to first usable data (the split kernel only)
// and lane 0 of wave w leaves {SIMD_ID of HW_REG_HW_ID, mean work, mean wait, frames} in scratch floats 4w .. 4w+3 of its song and
// mean data in float 48 + w.  A frame is then data | work - data (first data to last max3) | wait (publication, stores and barrier).
// The two s_memtime around the barrier return behind it (one more s_waitcnt per frame, the same for every wave): compare
// waves with each other, and take the frame time from a run without the probe.  (With the data stamp's scalar load in flight the
// compiler makes the next stated lgkmcnt of the frame a wait for everything: the probed full wave's second pair waits as the last one.)
struct WaveProbe {
    unsigned long long t_rel = 0, t_pub = 0, t_dat = 0, work = 0, wait = 0, data = 0;
    __device__ __forceinline__ void start() { t_rel = t_dat = __builtin_amdgcn_s_memtime(); }   // (a kernel without the data stamp reports 0)
    // behind the frame's first wait: `first` is a value that wait delivered
    template <typename V>
    __device__ __forceinline__ void first_data(V& first) {
        asm volatile("" : "+v"(first));
        __builtin_amdgcn_sched_barrier(0);
        t_dat = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void before_publish(float dn) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::"v"(dn));
        t_pub = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void barrier() {
        unsigned long long t_in, t_out;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_barrier\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(t_in), "=&s"(t_out) : "s"(t_pub), "s"(t_dat) : "memory");
        work += t_pub - t_rel;
        data += t_dat - t_rel;
        wait += t_out - t_in;
        t_rel = t_dat = t_out;
    }
    __device__ __forceinline__ void finish(float* scratch, int wv, int lane, int frames) const {
        if (lane != 0) return;
        const float n = (float)(frames > 0 ? frames : 1);
        scratch[4 * wv + 0] = (float)__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4);   // HW_REG_HW_ID bits 5:4 = SIMD_ID
        scratch[4 * wv + 1] = (float)work / n;
        scratch[4 * wv + 2] = (float)wait / n;
        scratch[4 * wv + 3] = n;
        scratch[48 + wv] = (float)data / n;
    }
};
#endif

// LDS of the one-target floor kernel (and, with the copy stride of its 384 state slots, of the split kernel), in floats from the start
// of the dynamic segment: what the kernel carves and what its launchers ask for.
// W = 128 with twelve waves (S > 512) leaves 168 registers per thread: the last W - WR window weights then live in LDS
// ([(W - WR) / 4][NP] float4-interleaved, read with conflict-free 16-byte reads next to the delta window)
// (variants: WR = 88 -- the song loop / the row selection keep a few more values alive, and 168 registers leave nothing to spill into)
template <int W, int NWT, WgVariant V = WgVariant::Plain>
struct FloorLds {
    static constexpr int NP = NWT * 64;
    static constexpr int DC = NP + 16;                   // copy stride (see banded_forward_kernel)
    static constexpr int BUF = 4 * DC;                   // floats per delta buffer
    static constexpr int WR = (W == 128 && NWT > 8) ? (V != WgVariant::Plain ? 88 : 96) : W;   // register-resident window weights
    static constexpr int dls = 0;                        // [2][4][DC] delta buffers
    static constexpr int fmg = dls + 2 * BUF;            // [kFmGroups][kFmGroupFloats] frame-maximum slot groups
    static constexpr int reset = fmg + kFmGroups * kFmGroupFloats;   // floats that go to -inf before a song: everything up to here
    static constexpr int tot = reset;                    // [16] VI: terminal argmax scratch
    static constexpr int awl = tot + 16 * (int)(sizeof(VI) / sizeof(float));   // [(W - WR) / 4][NP] f32x4: window weights WR .. W - 1
    static constexpr int end = awl + (W - WR) / 4 * 4 * NP;
    static_assert(sizeof(float) * end <= kLdsBytes, "one workgroup's LDS");
    static constexpr size_t bytes() { return sizeof(float) * end; }
};
// Where a lane writes: from its own entry of copy 0 (wp = dls + 4 + sh + j), copy c's entry lies floor_copy_off(DC, c) floats on; an
// upper lane of the split kernel's half waves writes copies 2 and 3, so its wp starts split_upper_off(DC) floats further on.  (Shared
// with floor_lds_check.hip, which holds them against where the readers look.)
// (floor_copy_off, split_upper_off, the half waves' lane map and the split kernel's slot map: plan.hpp, where the host library's replay
// of a frame's LDS conflicts, split_lds_conflicts, is written with them)
// the split kernel (banded.hip): four full waves and four half-window waves over 384 target slots, in the six-wave kernel's LDS
using FloorSplitLds = FloorLds<32, kSplitStates / 64>;   // the six-wave kernel's LDS, byte for byte
static_assert(FloorSplitLds::DC == kSplitCopyStride && FloorSplitLds::fmg == kSplitSlotGroups, "plan.hpp replays this layout");
// Lane map of a half wave: the two lanes of a target are l and l ^ 8, partners under the DPP control row_ror:8, so that the two halves
// of a window are joined by one v_max_f32_dpp (max_lane_xor8).  Lanes with bit 3 clear hold the lower half of the window, and the 32
// of them take the wave's 32 targets in ascending lane order.  A target's quad mates are the same in both halves.
// (Shared with floor_lds_check.hip, which replays the map against the LDS layout and the ds_read_b128 lane groups.)
// Frame-maximum slots of the split kernel where the extra column leaves M by address (XQ): the lane with l & 3 == r of quad q adds into
// slot 4 r + q % 3, so slots 0 .. 2 see all sixteen quads of every wave and M is one v_max3_f32 of them.  Slot 3, the fourth float of the
// same 16-byte read, belongs to the extra column x: its two lanes (r = 0, quad mates idle) add delta[x] into it and into nothing else, and
// a ds_max_f32 into a slot that was reset to -inf leaves exactly the value added.  Slots 4 .. 15 are written and never read.

// V = Packed is the packed variant (vit_decode_packed, plans without the wave form): the workgroup is a SLOT and decodes the
// songs slot_songs[slot_begin[w] .. slot_begin[w+1]) back to back, as a wave does in wave.hip.  Emission and history rows of
// a song start at row offsets[song] of the packed buffers (row strides S and SD; T plays no role).  The per-lane tables and
// the LDS-resident weights are loaded once; between two songs both delta buffers and every slot group go back to -inf behind
// a barrier.  The history layout is the unpacked one (the frame maximum of row t in pad column S of row t), so a song
// writes its own rows only.
// V = Ckpt is the checkpoint / resume variant (vit_decode_checkpointed, plans without the wave form), driven by the FwdArgs fields
// the wave form uses:
//   pass 1 (ckpt_every = K > 0): every frame of the song; frame mK - 1 goes to row m - 1 of the song's hist_rows rows, every other
//     frame to its last row (scratch).  The store stays unconditional, only its row base is selected (on the SALU).  The frame maximum
//     is not kept (lane S writes it into pad column S + 1 of the row being stored, which nothing reads): a resumed segment re-forms
//     it from the delta values.
//   segment (ckpt_every = 0): frames t_begin .. min(length, t_end + 1) - 1 -- one frame past the segment where the song goes on, so
//     that M of the segment's last row is stored too.  t_begin > 0 publishes init_rows[song] = delta_{t_begin - 1} instead of
//     log_pi + e_0; row t is stored at t - t_begin.  Lane S stores M of frame t - 1 into row t - 1 - t_begin: for the first frame
//     that is the row IN FRONT of a.hist, which the caller must own (the segment buffer starts one row before a.hist).  A workgroup
//     whose song ended before t_begin leaves without writing; the terminal state is pass 1's business.
// V = PackedCkpt is the packed-checkpoint variant (vit_decode_packed_bounded, plans without the wave form; instantiated in banded_pc.hip):
// the slot walk of Packed joined with the stores of Ckpt, in two modes told apart by a.unit_song (uniform over the launch):
//   pass 1 (unit_song null): the workgroup is a slot and walks its songs as in Packed; of song b only the rows in front of its segments
//     1 .. n_b - 1 are kept (frames t with (t + 1) % K == 0 and t + 1 < T_b, K = ckpt_every), at rows ckpt_base[b] .. of a.hist; every
//     other store goes to the slot's scratch row hist_rows + slot.  Stores, lane S and the frame maximum as in Ckpt's pass 1; the
//     terminal state and the log-likelihood are written per song.
//   unit (unit_song set): Ckpt's segment with the song, the segment and the rows taken per workgroup: workgroup u runs frames
//     unit_seg[u] * K .. of song unit_song[u] (emission rows at offsets[song]) from row ckpt_base[song] + segment - 1 of init_rows
//     (segment 0: from the prior) into rows u * hist_rows .. of a.hist, one frame past the segment where the song goes on; the row in
//     front of those rows takes the first frame's frame-maximum store (the caller passes a.hist one row into the unit's K + 2 rows).
// V = Stream is the session variant (vit_stream_append; instantiated in banded_stream.hip): the workgroup's song gets its next cnt
// frames t0 .. t0 + cnt - 1 (per song from the launch's tables, or the same for every song: wg_cursor.inc; cnt = 0 leaves without
// writing).  Emission row t is row t - t0 of the song's chunk, and the prefetch is clamped to the chunk's last row for this song.  History
// rows sit at their absolute index in the Plain layout, and Plain's stores are the ones used: frame t writes row t and, from lane S, M of
// frame t - 1 into pad column S of row t - 1.  t0 > 0 publishes row t0 - 1 of the song's own rows instead of log_pi + e_0 and so
// re-forms M of that frame, as Ckpt's segment does -- its first frame therefore completes the row the launch before ended with.  No
// frame is run past the chunk: M of the newest row is stored by the next launch, and the back-trace of a song of n frames reads the
// pad column of rows 0 .. n - 2 only.  The terminal state and the log-likelihood are Plain's, written after every launch.
// V = StreamRing is Stream over a ring session (vit_stream_open_ring; instantiated in banded_stream_ring.hip): the song owns a.hist_rows = R
// rows and frame t lives in row t mod R.  Frames stay absolute (emission rows, t0, Tb); only the row bases differ: a scalar cursor rs holds
// the slot of row t - 1, the launch resumes from slot (t0 - 1) mod R, and the frame whose row t - 1 sits in slot R - 1 stores M there and
// its own row into slot 0.  Everything else is Stream's, instruction for instruction.
// V = Plain compiles to the code it was before the variants existed.  (PK / CK / PC / ST below: V is that variant; PKx / CKx: what the
// packed-checkpoint variant shares with the packed and with the checkpoint / resume variant; RSx: CKx or ST.)
template <int W, int NWT, int NXT, int PF, typename ET, WgVariant V = WgVariant::Plain, bool WPR = false>
__global__ void __launch_bounds__(NWT * 64) banded_floor_forward_kernel(FwdArgs a) {
    static_assert(!WPR || V == WgVariant::Plain, "the per-wave probe exists for the plain kernel only");
    using L = FloorLds<W, NWT, V>;
    constexpr bool PK = V == WgVariant::Packed, CK = V == WgVariant::Ckpt, PC = V == WgVariant::PackedCkpt;
    constexpr bool PKx = PK || PC;                // the song loop and its per-song preamble
    constexpr bool CKx = CK || PC;                // the row selection of the stores, the resumed first frame
    constexpr bool RG = V == WgVariant::StreamRing;        // Stream with row t at t mod a.hist_rows (the row cursor rs below)
    constexpr bool ST = V == WgVariant::Stream || RG;      // the frames of one launch of a session, rows at their absolute index
    constexpr bool RSx = CKx || ST;               // the frame loop starts at t1 (a launch may resume a song)
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NP = L::NP, DC = L::DC, BUF = L::BUF, WR = L::WR;
    float* dls = reinterpret_cast<float*>(smem) + L::dls;
    float* fmg = dls + L::fmg;
    VI* tot = reinterpret_cast<VI*>(dls + L::tot);
    f32x4* awl = reinterpret_cast<f32x4*>(dls + L::awl);
    const int S = a.S, SP = a.SP, T = a.T, SD = a.SD;
    constexpr bool GEN = NXT < 0;
    constexpr int NXL = GEN ? kMaxExtras : NXT;
    const int nx = GEN ? a.n_extras : NXT;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int kPast = 1, kRowBias = 1;        // a segment runs one frame on; the lanes' row offsets are relative to row t - 1
#define VIT_WG_CURSOR 1
#include "wg_cursor.inc"
#define VIT_WG_CURSOR 2
#include "wg_cursor.inc"
    // (StreamRing) the song's ring and the row cursor: the slot of the row in front of the first frame the loop computes.  Scalars.
    [[maybe_unused]] int ring_rows = 0, rs = 0;
    if constexpr (RG) {
        ring_rows = (int)a.hist_rows;
        hist = a.hist + (size_t)song * (size_t)ring_rows * SD;
        rs = (int)((unsigned)(t1 - 1) % (unsigned)ring_rows);
    }

    // ---------------- per-lane constants.  Idle lanes (j >= S) carry -inf tables: their delta stays -inf.
    const int j = tid;
    const bool tvalid = j < S;
    const int jc = tvalid ? j : 0;
    const int jld = tvalid ? j : S - 1;                                   // emission column an idle lane (harmlessly) loads
    // history store of frame t, relative to row t-1: own column of row t | lane S: M into pad column S of row t-1
    // | other idle lanes: pad column S+1 of row t (never read)
    // (CK, pass 1: lane S joins the other idle lanes -- the row before the one being stored is not this frame's to write)
    const unsigned hoff = tvalid ? (unsigned)(SD + j) : ((j == S && !(CKx && ck_every > 0)) ? (unsigned)S : (unsigned)(SD + S + 1));
    const bool is_fm = j == S;
    const unsigned hoffb = 4u * hoff, eoffb = (unsigned)(sizeof(ET) * jld);   // per-lane byte offsets from the frame's row bases
    const int lo = reinterpret_cast<const int32_t*>(a.image + a.off_lo)[jc];
    const float cj = tvalid ? reinterpret_cast<const float*>(a.image + a.off_rowc)[jc] : -INFINITY;
    float aw[WR];
    float xa[NXL > 0 ? NXL : 1];
    int xcol[NXL > 0 ? NXL : 1];
    bool is_x = false;                                                    // this lane's state is an extra column: not part of M
    {
        const float* __restrict__ tab = reinterpret_cast<const float*>(a.image + a.off_tabA);
        const float* __restrict__ xaT = reinterpret_cast<const float*>(a.image + a.off_extraA);
#pragma unroll
        for (int w = 0; w < WR; ++w) aw[w] = tvalid ? tab[(size_t)w * SP + jc] : -INFINITY;
#pragma unroll
        for (int q = 0; q < (W - WR) / 4; ++q) {
            f32x4 wv4;
            wv4.x = tvalid ? tab[(size_t)(WR + 4 * q + 0) * SP + jc] : -INFINITY;
            wv4.y = tvalid ? tab[(size_t)(WR + 4 * q + 1) * SP + jc] : -INFINITY;
            wv4.z = tvalid ? tab[(size_t)(WR + 4 * q + 2) * SP + jc] : -INFINITY;
            wv4.w = tvalid ? tab[(size_t)(WR + 4 * q + 3) * SP + jc] : -INFINITY;
            awl[q * NP + j] = wv4;
        }
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            xcol[k] = k < nx ? a.extras[k] : 0;
            xa[k] = (tvalid && k < nx) ? xaT[(size_t)k * SP + jc] : -INFINITY;
            is_x |= (k < nx && j == xcol[k]);
        }
    }
    // delta[i] lives at float position 4 + sh + i - c of copy c (sh = a.win_shift): lane j reads its window from the copy
    // that makes delta[lo_j] 16-byte aligned.  With sh = lo_off mod 4 the sixteen lanes of one LDS read group start on
    // sixteen different 4-bank groups; without it the first and the last lane of a group collide (2-way conflict on
    // every ds_read_b128: 128 instead of 256 B/clk).
    const int sh = a.win_shift;
    const int lov = (tvalid ? lo : 0) + sh;
    const float* rp = dls + 4 + (lov & 3) * DC + (lov & ~3);              // window start in the copy that aligns it
    float* wp = dls + 4 + sh + j;                                         // own entry of copy 0 (copy c: + c*DC - c)
    float* fmp = fmg + fm_slot(lane);                                     // own frame-maximum slot in group 0 (group g: + g*kFmGroupFloats)

    for (int k = tid; k < L::reset; k += NWT * 64) dls[k] = -INFINITY;
    __syncthreads();

    // produce(): publish a new delta value -- four shifted copies into buffer WB and the lane's share of M into slot group G --
    // and reset slot group Z for the frame after next
    auto produce = [&](const float dn, const int WB, const int G, const int Z) {
#pragma unroll
        for (int c = 0; c < 4; ++c) wp[WB * BUF + floor_copy_off(DC, c)] = dn;
        fm_publish(fmp + G * kFmGroupFloats, (NXL > 0 && is_x) ? -INFINITY : dn);
        int w = wv;
        asm volatile("" : "+s"(w));   // a fresh SGPR test per frame: hoisted, the wave test became two VALU instructions a frame
        if (w == NWT - 1) fmg[Z * kFmGroupFloats + lane] = -INFINITY;
    };

    // ---------------- one pass per song (PK: the songs of the slot, back to back)
    for (;;) {
        // ---------------- frame 0
        // (PK: the lane's column index is made opaque once per song, so that the 64-bit addresses of this preamble are formed here
        // and do not stay in registers across the frame loop for the next song -- W = 128 with twelve waves has none to spare)
        int jf = j;
        if constexpr (PKx) asm volatile("" : "+v"(jf));
        const bool tvf = PKx ? jf < S : tvalid;
        const int jldf = PKx ? (tvf ? jf : S - 1) : jld;
        if constexpr (CKx) {         // frame 0 (pass 1: into the scratch row), or the checkpoint row in front of this segment
            float d0 = -INFINITY;
            if (t0 > 0) {
                if (tvf) d0 = PC ? pc_init[jf] : a.init_rows[(size_t)song * a.init_stride + jf];
            } else if (tvf) {
                d0 = reinterpret_cast<const float*>(a.image + a.off_logpi)[jf] + load_e<ET>(E + jf);
                hist[(size_t)(ck_every > 0 ? ck_scratch : 0) * SD + jf] = d0;
            }
            produce(d0, 0, 0, 1);
        } else if constexpr (ST) {   // frame 0, or the song's own row in front of this launch's first frame (M is re-formed from it)
            float d0 = -INFINITY;
            if (t0 > 0) {
                if (tvf) d0 = hist[(size_t)(RG ? rs : t0 - 1) * SD + jf];
            } else if (tvf) {
                d0 = reinterpret_cast<const float*>(a.image + a.off_logpi)[jf] + load_e<ET>(E + jf);
                hist[jf] = d0;
            }
            produce(d0, 0, 0, 1);
        } else {
            const float d0 = tvf ? reinterpret_cast<const float*>(a.image + a.off_logpi)[jf] + load_e<ET>(E + jf) : -INFINITY;
            if (tvf) hist[jf] = d0;
            produce(d0, 0, 0, 1);   // (group 1 is still -inf)
        }
        // Emission rows are fetched PF frames ahead (PF even): a global load takes ~2 us under load, several frame times,
        // and the s_waitcnt before a frame's "+ e" must not be what paces the recursion.
        float er[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) er[k] = load_e<ET>(E + (size_t)((RSx ? t1 : 1) + k < Tb ? (RSx ? t1 : 1) + k : Tb - 1) * S + jldf);
#pragma unroll
        for (int w = 0; w < WR; ++w) asm volatile("" ::"v"(aw[w]));
#pragma unroll
        for (int k = 0; k < NXL; ++k) asm volatile("" ::"v"(xa[k]));
        asm volatile("" ::"v"(cj));
        __syncthreads();

        // frame t = 1 + PF*n + u: delta buffers u & 1 (read) / (u & 1) ^ 1 (write); slot groups u % 4 read, (u + 1) % 4 written,
        // (u + 2) % 4 reset (PF % 4 == 0: every index is a compile-time constant)
        static_assert(PF % 2 == 0 && PF % kFmGroups == 0, "the unrolled frames must cycle through whole buffer and slot-group rounds");
#ifdef VIT_TIMING_HOOKS
        constexpr bool wprobe = WPR;   // per-wave probe (see WaveProbe): an instantiation of its own, the loop without it is the release loop
        WaveProbe wp_;
#endif
        auto frame = [&](const int t, float& e_slot, const int u) {
            const int RB = u & 1, WB = RB ^ 1;
            const int GR = u % kFmGroups, GW = (u + 1) % kFmGroups, GZ = (u + 2) % kFmGroups;
            // ---- everything this frame reads from LDS: the window, the extra columns, the frame-maximum slots
            const f32x4* __restrict__ win = reinterpret_cast<const f32x4*>(rp + RB * BUF);
            float xd[NXL > 0 ? NXL : 1];
            f32x4 fq[kFmSlots / 4];
            // The small reads go out first and the first chunk of the window right behind them, and only then is M reduced: left to
            // itself the compiler reduces M before it issues the window reads -- a full LDS round trip with nothing else in flight.
            // (M reduced last instead lengthens the dependent tail after the last window read lands: measured slower.)
            auto small_reads = [&]() {
#pragma unroll
                for (int k = 0; k < NXL; ++k) xd[k] = dls[4 + sh + RB * BUF + xcol[k]];
#pragma unroll
                for (int q = 0; q < kFmSlots / 4; ++q) fq[q] = reinterpret_cast<const f32x4*>(fmg + GR * kFmGroupFloats)[q];
            };
            // the window in chunks of 32 sources (8 reads): wide windows (W = 96, 128) must not hold all their data at once
            float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
            float M = -INFINITY;
            small_reads();
            asm volatile("" ::: "memory");
#pragma unroll
            for (int w0 = 0; w0 < W; w0 += 32) {
            // W > 64: one chunk of reads in flight at a time (W register-resident weights leave no room for more; with
            // twelve waves per workgroup the other waves of the SIMD cover the read latency)
            if ((W > 64 || (W == 64 && NWT > 8)) && w0 > 0) asm volatile("" : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3)::"memory");
            f32x4 dw[8];
#ifdef VIT_ABL_READS
            // result-breaking ablation (make TIMING=1 ABL=n builds only): read n of every chunk's window quads, the others reuse them --
            // what does the LDS return path cost a frame?
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (w0 + 4 * q < W) { if (q < VIT_ABL_READS) dw[q] = win[w0 / 4 + q]; else dw[q] = dw[q % VIT_ABL_READS]; }
#else
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (w0 + 4 * q < W) dw[q] = win[w0 / 4 + q];
#endif
            if (w0 == 0) {
                __builtin_amdgcn_sched_barrier(0);
                // M = max of delta_{t-1} over the non-extra sources
                M = fmaxf(fmaxf(fq[0].x, fq[0].y), fmaxf(fq[0].z, fq[0].w));
#pragma unroll
                for (int q = 1; q < kFmSlots / 4; ++q) M = fmaxf(fmaxf(fmaxf(M, fq[q].x), fq[q].y), fmaxf(fq[q].z, fq[q].w));
                m0 = M + cj;
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int w = w0; w + 7 < W && w < w0 + 32; w += 8) {
                const f32x4 da = dw[(w - w0) / 4], db = dw[(w - w0) / 4 + 1];
                f32x4 wa, wb;
                if (w < WR) {
                    wa = f32x4{aw[w < WR ? w + 0 : 0], aw[w < WR ? w + 1 : 0], aw[w < WR ? w + 2 : 0], aw[w < WR ? w + 3 : 0]};
                    wb = f32x4{aw[w < WR ? w + 4 : 0], aw[w < WR ? w + 5 : 0], aw[w < WR ? w + 6 : 0], aw[w < WR ? w + 7 : 0]};
                } else {
                    wa = awl[((w - WR) / 4) * NP + j];
                    wb = awl[((w - WR) / 4 + 1) * NP + j];
                }
                f32x2 c0_ = f32x2{da.x, da.y} + f32x2{wa.x, wa.y};
                f32x2 c1_ = f32x2{da.z, da.w} + f32x2{wa.z, wa.w};
                f32x2 c2_ = f32x2{db.x, db.y} + f32x2{wb.x, wb.y};
                f32x2 c3_ = f32x2{db.z, db.w} + f32x2{wb.z, wb.w};
                // (W <= 32: all of a group's sums before its maxima.  Left alone, the compiler folds each sum into its chain at once,
                // and a max3 right behind the packed add it reads needs an s_nop: eleven a frame.)
                if (W <= 32) asm volatile("" : "+v"(c0_), "+v"(c1_), "+v"(c2_), "+v"(c3_));
                m0 = fmaxf(fmaxf(m0, c0_.x), c0_.y);
                m1 = fmaxf(fmaxf(m1, c1_.x), c1_.y);
                m2 = fmaxf(fmaxf(m2, c2_.x), c2_.y);
                m3 = fmaxf(fmaxf(m3, c3_.x), c3_.y);
            }
            if (W % 8 == 4 && w0 + 32 >= W) {          // W = 84: the last four sources (one read, two packed adds)
                static_assert(W % 8 != 4 || W <= WR, "an odd float4 count only with register-resident weights");
                const f32x4 da = dw[((W - 4 - w0) / 4) & 7];
                const f32x2 c0_ = f32x2{da.x, da.y} + f32x2{aw[W - 4], aw[W - 3]};
                const f32x2 c1_ = f32x2{da.z, da.w} + f32x2{aw[W - 2], aw[W - 1]};
                m2 = fmaxf(fmaxf(m2, c0_.x), c0_.y);
                m3 = fmaxf(fmaxf(m3, c1_.x), c1_.y);
            }
            }
#pragma unroll
            for (int k = 0; k < NXL; ++k) m1 = fmaxf(m1, xd[k] + xa[k]);
            const float dn = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3)) + e_slot;
#ifdef VIT_TIMING_HOOKS
            if constexpr (wprobe) wp_.before_publish(dn);
#endif
            produce(dn, WB, GW, GZ);
            asm volatile("" ::: "memory");   // keep the global store / prefetch behind the frame-maximum publication: they fill
                                             // the wait for the LDS write acknowledgement before the barrier (-2 %)
            // Unconditional store + prefetch: exact in-order vmcnt accounting (see banded_forward_kernel).  Row bases are
            // scalar index arithmetic on purpose: the SALU is idle, the VALU is not (running 64-bit per-lane pointers
            // measured 3.5% slower).  Both are buffer instructions: a descriptor built on the SALU from the row base plus the lane's
            // fixed 32-bit byte offset, no per-frame 64-bit address add on the VALU.
            const int tn = t + PF < Tb ? t + PF : Tb - 1;
            if constexpr (CKx) {
                // the row in front of the one this frame's delta goes to (the lanes' offsets are relative to row t - 1): a segment
                // stores frame t at t - t0, pass 1 at the next checkpoint row or the scratch row.  Scalar selects, the store as ever.
                long long row = (long long)t - 1 - t0;
#define VIT_WG_CURSOR 3
#include "wg_cursor.inc"
                row_store_f32(hist + row * SD, hoffb, is_fm ? M : dn);
            } else if constexpr (RG) {
                // rs = the slot of row t - 1.  Row t is the next slot, and the lanes' offsets reach it from there -- but for the frame whose
                // row t - 1 sits in the last slot: there lane S stores M into that slot and every other lane from slot 0 (a uniform branch
                // taken once per ring_rows frames; the cursor is a scalar increment with a scalar compare-and-reset)
                if (rs != ring_rows - 1) {
                    row_store_f32(hist + (size_t)rs * SD, hoffb, is_fm ? M : dn);
                    ++rs;
                } else {
                    // (two stores with a uniform row base each, kept apart: joined into one store the row base is a per-lane select, the
                    // descriptor lives in VGPRs and the store becomes a waterfall loop)
                    // (the offsets from slot 0 are formed here, from an opaque copy: hoisted out of the loop they cost every frame a VGPR)
                    unsigned hoff0 = hoffb;
                    asm volatile("" : "+v"(hoff0));
                    if (!is_fm) row_store_f32(hist, hoff0 - 4u * (unsigned)SD, dn);
                    asm volatile("" ::: "memory");
                    if (is_fm) row_store_f32(hist + (size_t)rs * SD, hoffb, M);
                    rs = 0;
                }
            } else {
                row_store_f32(hist + (size_t)(t - 1) * SD, hoffb, is_fm ? M : dn);
            }
            e_slot = row_load_e<ET>(E + (size_t)tn * S, eoffb);
#ifdef VIT_TIMING_HOOKS
            if constexpr (wprobe) wp_.barrier(); else
#endif
            __syncthreads();
        };
#ifdef VIT_TIMING_HOOKS
        const bool probe = !PKx && !CKx && (a.debug & 48) != 0;
        if constexpr (wprobe) wp_.start();
#else
        constexpr bool probe = false;   // cycle probe: VIT_TIMING_HOOKS builds only; it writes the per-song scratch, never an output
#endif
        const unsigned long long clk0 = probe ? __builtin_amdgcn_s_memtime() : 0ull;
        const unsigned long long rt0 = probe ? __builtin_amdgcn_s_memrealtime() : 0ull;
        int t = RSx ? t1 : 1;
        for (; t + PF - 1 < Tb; t += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) frame(t + k, er[k], k);
        }
#pragma unroll
        for (int k = 0; k < PF - 1; ++k)
            if (t + k < Tb) frame(t + k, er[k], k);

        const int fb = (Tb - (RSx ? t1 : 1)) & 1;                             // buffer holding delta_{Tb-1}
        if constexpr (PC) {         // pass 1 only, per song (uniform test)
            if (ck_every > 0) terminal_argmax_w(tvalid ? dls[4 + sh + fb * BUF + j] : -INFINITY, j, tvalid, tot, NWT, wv, lane, a.last_state, a.loglik, song);
        } else
        if constexpr (CK) {         // the terminal state and the log-likelihood come from pass 1 (uniform test: every thread reaches the barrier inside)
            if (ck_every > 0) terminal_argmax(tvalid ? dls[4 + sh + fb * BUF + j] : -INFINITY, j, tvalid, tot, NWT, a.last_state, a.loglik, song);
        } else
        if constexpr (PK) terminal_argmax_w(tvalid ? dls[4 + sh + fb * BUF + j] : -INFINITY, j, tvalid, tot, NWT, wv, lane, a.last_state, a.loglik, song);
        else terminal_argmax(tvalid ? dls[4 + sh + fb * BUF + j] : -INFINITY, j, tvalid, tot, NWT, a.last_state, a.loglik, song);
        if (probe && tid == 0) {  // timing experiments only: cycles (16) or 100 MHz ticks (32) per frame -> scratch slot 63
            const unsigned long long d = (a.debug & 16) ? __builtin_amdgcn_s_memtime() - clk0 : __builtin_amdgcn_s_memrealtime() - rt0;
            a.fmax[(size_t)song * 64 + 63] = (float)d / (float)(Tb > 1 ? Tb - 1 : 1);
        }
#ifdef VIT_TIMING_HOOKS
        if constexpr (wprobe) wp_.finish(a.fmax + (size_t)song * 64, wv, lane, Tb - 1);
#endif
        if constexpr (!PKx) {
            break;
        } else {
            if (++si >= si_end) break;                                        // (PC, unit: si_end = 1)
            take_song();
            // every wave has read the last delta row (terminal_argmax) before both buffers and all slot groups go back to -inf,
            // and no wave starts frame 0 of the next song before they have
            __syncthreads();
            for (int k = tid; k < L::reset; k += NWT * 64) dls[k] = -INFINITY;
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------
// launch helpers of the floor form (host)
// ---------------------------------------------------------------------------------------
// f(std::integral_constant<int, W>) for the instantiated window width W / for the target waves of S states
template <typename F>
static hipError_t dispatch_width(int W, F&& f) {
    static_assert(sizeof(kBandedWidths) / sizeof(int) == 6, "one case per instantiated window width");
    switch (W) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 84: return f(std::integral_constant<int, 84>{});
        case 96: return f(std::integral_constant<int, 96>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidConfiguration;
    }
}
template <typename F>
static hipError_t dispatch_waves(int S, F&& f) {
    switch (banded_waves_for(S)) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 12: return f(std::integral_constant<int, 12>{});
        default: return hipErrorInvalidConfiguration;
    }
}
// emission rows in flight (see launch_floor_t)
template <int W>
constexpr int floor_pf() { return W <= 32 ? 12 : 4; }
// f(std::integral_constant<int, NXT>): the compile-time extras count of the one-target kernel -- 1 for the reference's matrices (band +
// unvoiced column) at the widths they come in, else the run-time count
template <int W, typename F>
static hipError_t with_nxt(int n_extras, F&& f) {
    if constexpr (W == 32 || W >= 84) {
        if (n_extras == 1) return f(std::integral_constant<int, 1>{});
    }
    return f(std::integral_constant<int, -1>{});
}

// A variant of the one-target floor kernel: one workgroup per slot (Packed, PackedCkpt pass 1), per song (Ckpt, Stream) or per unit
// (PackedCkpt, a.unit_song set).  With `per_cu` the launch is replaced by the occupancy query of that instantiation at its dynamic LDS size.
template <int W, int NWT, typename ET, WgVariant V>
static hipError_t floor_variant_t(const FwdArgs& a, hipStream_t st, int* per_cu) {
    constexpr size_t ldsf = FloorLds<W, NWT, V>::bytes();
    const int groups = V == WgVariant::Ckpt || V == WgVariant::Stream || V == WgVariant::StreamRing || (V == WgVariant::PackedCkpt && a.unit_song) ? (int)a.B : a.n_slots;
    return with_nxt<W>(a.n_extras, [&](auto nxt) -> hipError_t {
        auto kern = banded_floor_forward_kernel<W, NWT, decltype(nxt)::value, floor_pf<W>(), ET, V>;
        if (per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, NWT * 64, ldsf);
        hipLaunchKernelGGL(kern, dim3(groups), dim3(NWT * 64), ldsf, st, a);
        return hipGetLastError();
    });
}
// the (W, NWT) pairs a variant is instantiated for: Packed and Stream every pair of the floor form, the checkpoint variants floor_ckpt_pair's
template <typename ET, WgVariant V>
static hipError_t floor_variant_e(const FwdArgs& a, hipStream_t st, int* per_cu) {
    constexpr bool packed = V == WgVariant::Packed || V == WgVariant::Stream || V == WgVariant::StreamRing;    // (floor_stream_applies is floor_packed_applies)
    if (!(packed ? floor_packed_applies(a.S, a.W, a.floor_ok != 0, a.n_dense) : floor_ckpt_applies(a.S, a.W, a.floor_ok != 0, a.n_dense)))
        return hipErrorInvalidConfiguration;
    return dispatch_width(a.W, [&](auto w) {
        return dispatch_waves(a.S, [&](auto n) -> hipError_t {
            constexpr int W = decltype(w)::value, NWT = decltype(n)::value;
            if constexpr (packed || floor_ckpt_pair(W, NWT)) return floor_variant_t<W, NWT, ET, V>(a, st, per_cu);
            return hipErrorInvalidConfiguration;
        });
    });
}
