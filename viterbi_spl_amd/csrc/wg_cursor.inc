// wg_cursor.inc -- the song / segment bookkeeping of the two workgroup forward kernels that have variants (WgVariant, kernels.hpp):
// banded_floor_forward_kernel (banded_floor.inc) and step4s_forward_kernel (step.hip).  Included as text (see wave_frame_body.inc):
// as a helper the same statements are simplified on their own before they are inlined, and the variant kernels then come out
// with other register counts (profiles/README.md, wg_refactor).  Scalars only, all of them wave-uniform.  The kernels keep their
// frame bodies, LDS resets, barriers and stores.
//
// VIT_WG_CURSOR == 1 and 2, one after the other at kernel top level (the early returns are the kernel's; the step kernel forms its
// prior pointer between them, where its kernel-argument loads have always been): which song the workgroup decodes, its rows, the
// frames of this launch and the checkpoint counters.
//   In scope: a, S, T, SD, ET, PK / CK / PC / PKx / ST; kPast = 1 where a segment runs one frame past its end if the song goes on (the
//   floor kernel stores the frame maximum of row t with frame t + 1), 0 where it ends with the segment (the step kernel).  (Stream
//   runs no frame past its chunk: the next launch's first frame stores that maximum.)
//   Declares: song, Tb, E, hist (1); si, si_end, take_song() (slot walks: `if (++si >= si_end) break; take_song();`), t0, t1,
//   ck_every, ck_scratch, ck_next, ck_row, pc_init (2).
// VIT_WG_CURSOR == 3, in the frame: the row select of a checkpoint variant's pass 1.
//   In scope: t; row = the row frame t is stored to in a segment (t - t0, less kRowBias), overwritten here in pass 1 with the next
//   checkpoint row or the scratch row (scalar selects; the store itself stays unconditional).
#if VIT_WG_CURSOR == 1
    // the song being decoded: the workgroup's own, or (slot walks) the slot's songs one after the other
    int song = blockIdx.x;
    int Tb = PKx ? 1 : song_length(a.lengths, song, T);
    const ET* __restrict__ E = reinterpret_cast<const ET*>(a.logE) + (PKx || ST ? (size_t)0 : (size_t)song * T * S);
    float* __restrict__ hist = a.hist + (PKx ? (size_t)0 : (CK ? (size_t)song * (size_t)a.hist_rows * SD : (size_t)song * T * SD));
#elif VIT_WG_CURSOR == 2
    // (Ckpt) first frame of this launch, first frame the loop computes, pass 1's segment length and its row bookkeeping
    // (PackedCkpt: t0 and t1 belong to the unit; ck_every is K in pass 1 and 0 in a unit launch; the scratch row is the slot's)
    [[maybe_unused]] const bool pc_unit = PC && a.unit_song != nullptr;
    [[maybe_unused]] int t0 = CK ? a.t_begin : 0;
    [[maybe_unused]] int t1 = CK && t0 > 0 ? t0 : 1;
    [[maybe_unused]] const int ck_every = CK ? a.ckpt_every : (PC && !pc_unit ? a.ckpt_every : 0);
    [[maybe_unused]] const int ck_scratch = CK ? (int)a.hist_rows - 1 : (PC ? (int)a.hist_rows + (int)blockIdx.x : 0);
    [[maybe_unused]] int ck_next = ck_every - 1, ck_row = 0;              // the next frame that is a checkpoint, and its row
    [[maybe_unused]] const float* __restrict__ pc_init = nullptr;         // (PackedCkpt, unit) the checkpoint row in front of the unit's segment
    if constexpr (CK) {
        const int stop = ck_every > 0 || a.t_end >= T ? T : a.t_end + kPast;
        Tb = Tb < stop ? Tb : stop;
        if (Tb <= t0) return;                                             // (segments: the song ended before this one)
    }
    if constexpr (ST) {
        // (Stream) the frames of this launch: t0 .. t0 + cnt - 1 of the song's T rows; E is moved so that row t of it is row t - t0 of the
        // song's chunk, and the kernel goes on indexing emission rows by frame
        // (two branches, and the loaded values declared uniform: as one select between a table entry and a kernel argument the
        // compiler loads per lane, and t0, Tb and the row bases then live in VGPRs -- a waterfall loop at every store and prefetch)
        int cnt = a.t_end - a.t_begin;
        t0 = a.t_begin;
        if (a.unit_song) {
            t0 = __builtin_amdgcn_readfirstlane(a.unit_song[song]);
            cnt = __builtin_amdgcn_readfirstlane(a.unit_seg[song]);
        }
        if (cnt <= 0) return;                                           // (nothing appended to this song)
        t1 = t0 > 0 ? t0 : 1;
        Tb = t0 + cnt;
        E += (ptrdiff_t)song * (ptrdiff_t)a.init_stride - (ptrdiff_t)t0 * S;
    }
    [[maybe_unused]] int si = 0, si_end = 1;                              // (slot walks) position in slot_songs, end of the slot's list
    // (slot walks) the song at si: its emission rows; Packed: its history rows; PackedCkpt: its first checkpoint row (a.hist is the
    // checkpoint area).  Wave-uniform: scalar loads.
    [[maybe_unused]] auto take_song = [&]() {
        song = a.slot_songs[si];
        const long long r0 = a.offsets[song];
        Tb = (int)(a.offsets[song + 1] - r0);
        E = reinterpret_cast<const ET*>(a.logE) + (size_t)r0 * S;
        if constexpr (PK) hist = a.hist + (size_t)r0 * SD;
        if constexpr (PC) {
            ck_next = ck_every - 1;
            ck_row = (int)a.ckpt_base[song];
        }
    };
    if constexpr (PK) {
        si = a.slot_begin[blockIdx.x];
        si_end = a.slot_begin[blockIdx.x + 1];
        if (si >= si_end) return;                                         // an empty slot (the host makes none)
        take_song();
    }
    if constexpr (PC) {
        hist = a.hist;
        if (pc_unit) {                                                    // one unit: its song, segment, frames and rows
            song = a.unit_song[blockIdx.x];
            const int useg = a.unit_seg[blockIdx.x];
            const long long r0 = a.offsets[song];
            const int Ts = (int)(a.offsets[song + 1] - r0);
            t0 = useg * a.ckpt_every;
            t1 = t0 > 0 ? t0 : 1;
            Tb = t0 + a.ckpt_every >= Ts ? Ts : t0 + a.ckpt_every + kPast;
            E = reinterpret_cast<const ET*>(a.logE) + (size_t)r0 * S;
            hist = a.hist + (size_t)blockIdx.x * (size_t)a.hist_rows * SD;
            pc_init = a.init_rows + (size_t)(a.ckpt_base[song] + useg - 1) * SD;
            if (Tb <= t0) return;                                         // (the host lists no such unit)
        } else {
            si = a.slot_begin[blockIdx.x];
            si_end = a.slot_begin[blockIdx.x + 1];
            if (si >= si_end) return;                                     // an empty slot (the host makes none)
            take_song();
        }
    }
#elif VIT_WG_CURSOR == 3
            if (ck_every > 0) {
                // (PackedCkpt: a song's last frame is no checkpoint -- the row behind its last one is the next song's first)
                const bool hit = PC ? (t == ck_next && t + 1 < Tb) : t == ck_next;
                row = (hit ? ck_row : ck_scratch) - kRowBias;
                ck_next += hit ? ck_every : 0;
                ck_row += hit ? 1 : 0;
            }
#endif
#undef VIT_WG_CURSOR
