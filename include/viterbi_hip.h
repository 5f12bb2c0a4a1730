/*
 * viterbi_hip.h -- C ABI of libviterbi_hip.so (MI355X / gfx950 Viterbi decoder).
 *
 * This is the drop-in boundary for the hot path of drwangxian/viterbi_spl: the
 * float32 log-domain Viterbi forward recursion + argmax back-trace.  Plain
 * pointers and sizes only; no torch types; no exceptions cross this ABI (every
 * entry point returns a vit_status).  All device buffers are caller-owned; the
 * library never allocates device memory and never synchronises the host inside
 * vit_decode().
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   - viterbi_numba.core(B, prob_init, probs) -> int64[T]
 *       dcnet/aot_viterbi_core.py:8-54, call site dcnet/tf_viterbi_decoding.py:147-151
 *       ('i8[:](f4[:, ::1], f4[:], f4[:, ::1])': B is [S,S] "target <- source",
 *        C-contiguous; probs is [T,S] C-contiguous).
 *   - viterbi_librosa_fn(*, log_transition_matrix_T, log_prob_init, log_probs_st)
 *       imm/tf_viterbi.py:75-109 (the log-domain core this ABI mirrors).
 *   - the in-class copies Viterbi.viterbi_librosa_fn / SoftMaxViterbi.viterbi_librosa_fn
 *       tonet/for_paper.py:1833-1870, :1999-2037 (after their host-side log step).
 *
 * Differences from the reference boundary, all deliberate:
 *   - inputs are NEVER mutated (the Numba core logs its arguments in place,
 *     dcnet/aot_viterbi_core.py:23-25);
 *   - the contract starts at log-domain tensors: the prob -> log step stays on
 *     the host in the Python adapters, because NumPy's float32 log is the one
 *     operation whose last bit is not reproducible on a GPU;
 *   - songs are batched ([B,T,S]) and may be ragged (lengths);
 *   - states come back as int32 (the Python adapters widen to int64);
 *   - the terminal log-likelihood delta_{T-1}[s_{T-1}] is returned as well
 *     (the unused `p` at dcnet/tf_viterbi_decoding.py:255).
 *
 * NaN inputs are outside the contract.  -inf entries are accepted.  A candidate of -inf never beats the running best
 * (the comparison is strict), so a frame whose delta row is all -inf resolves every back-pointer to state 0, and a song
 * that reaches such a frame returns state 0 from that frame on and log-likelihood -inf -- what the oracle
 * (oracle/viterbi_oracle.c) and np.argmax do.
 */
#ifndef VITERBI_HIP_H_
#define VITERBI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIT_ABI_VERSION 4

typedef enum vit_status {
    VIT_OK = 0,
    VIT_EINVAL = -1,       /* bad argument (null pointer, size out of range) */
    VIT_ENOMEM = -2,       /* host allocation failed */
    VIT_EHIP = -3,         /* a HIP runtime call failed (see vit_last_hip_error) */
    VIT_EWORKSPACE = -4,   /* workspace smaller than vit_workspace_bytes() */
    VIT_EUNSUPPORTED = -5, /* shape/algorithm combination not supported */
    VIT_ENOTUPLOADED = -6, /* vit_decode() before vit_plan_upload() */
    VIT_ENOFORWARD = -7    /* vit_backtrace() on a workspace without a matching vit_forward() on record */
} vit_status;

/* storage type of the emission tensor (arithmetic is always float32) */
typedef enum vit_dtype { VIT_F32 = 0, VIT_F16 = 1 } vit_dtype;

/* forward-kernel selection */
typedef enum vit_algo {
    VIT_ALGO_AUTO = 0,   /* banded if the plan proved the structure, else dense */
    VIT_ALGO_DENSE = 1,  /* S*S max-plus per frame, any matrix */
    VIT_ALGO_BANDED = 2, /* exact row-constant + window + extra-column decomposition; the form (one song per
                            workgroup / one song per wavefront) is chosen from the batch size */
    VIT_ALGO_WAVE = 3,   /* banded, one song per wavefront (throughput form; VIT_EUNSUPPORTED if the plan lacks it) */
    VIT_ALGO_GROUP = 4   /* banded, one song per workgroup (latency form) */
} vit_algo;

typedef struct vit_plan vit_plan; /* opaque: analysed transition matrix + prior */
typedef void *vit_stream;         /* hipStream_t */

typedef struct vit_plan_info {
    int64_t S;
    int32_t banded_ok;      /* 1 if the banded kernel may be used for this matrix */
    int32_t n_consts;       /* distinct row constants */
    int32_t n_extras;       /* extra exception columns shared by most rows */
    int32_t max_window;     /* widest per-row exception window */
    int32_t group_window;   /* window width the banded kernel evaluates per target */
    int32_t reserved[3];    /* [0] dense rows, [1] one-maximum ("floor") form proven, [2] bit 0: window start affine in the target, bit 1: pair windows proven, bit 2: step structure (dense matrix, piecewise-constant columns), bit 3: wave form (one song per wavefront) available.
                             * Bit 2 means "step structure proven AND the forward step kernel is instantiated for it" (20-bin bands, 9 near bands,
                             * 705..768 voiced states); a step-structured plan without it (another band width or count, another state count)
                             * runs the dense forward kernel and still reads the band table, not the matrix rows, in its back-trace. */
    float consts[4];
    int32_t extras[4];
} vit_plan_info;

int vit_abi_version(void);
const char *vit_status_string(int status);
/* last hipError_t seen by this library on the calling thread (0 = hipSuccess) */
int vit_last_hip_error(void);

/*
 * Analyse a transition matrix on the host.
 *   logA_T : host, [S,S] float32 C-order, row j = log-probabilities INTO target j
 *            (same orientation the reference passes to its core,
 *            dcnet/tf_viterbi_decoding.py:144, imm/tf_viterbi.py:77-80)
 *   log_pi : host, [S] float32
 * 1 <= S <= 1024.
 */
int vit_plan_create(const float *logA_T, const float *log_pi, int64_t S, vit_plan **out);
void vit_plan_destroy(vit_plan *plan);
int vit_plan_query(const vit_plan *plan, vit_plan_info *info);

/*
 * Kernel-selection overrides, per plan.  Every setting decodes the same bits -- they exist so that tests and timing
 * scripts can reach each kernel form (the library reads NO environment variables).  Keys:
 *   "forward_form"     banded plans: 0 by batch size | 1 one target per lane | 2 two targets per lane | 3 scan form |
 *                      4 wave form | 5 never the wave form | 6 floor form, split windows over eight waves (window 32 wide,
 *                      256 < S < 384: the six-wave grids; what 0 picks there up to 256 songs with fp32 emissions.  Elsewhere 6 runs the
 *                      one-target kernel, as 2 does for a plan without pair_ok)
 *   "backtrace_form"   0 auto | 1 generic kernel | 2 whole-row kernels (no sparse fetch) | 4 one (song, chunk) stream per LANE
 *                      instead of per wavefront (banded plans, full history; up to 256 chunks per song; VIT_EUNSUPPORTED elsewhere:
 *                      from vit_decode() before anything is enqueued, from vit_backtrace() behind a vit_forward() that has run)
 *   "dense_songs"      songs per workgroup of the dense kernel (0 auto); "dense_one_thread" 1 = one thread per target;
 *                      "dense_form" 0 = matrix-resident dense kernel where it applies (64 < S <= 368), 1 = always stream the matrix
 *   "step_form"        step-structured kernel, four targets per lane: 0 bands split over two waves | 3 one wave per lane group
 *                      (VIT_ALGO_DENSE is the plain dense kernel)
 *   "bt_chunks", "bt_warm"   time-parallel back-trace: chunks per song (0 auto), warm-up frames (-1 default); "bt_fast_rows" 1 = every
 *                      row through the general code of the sparse kernels (0: the unexceptional rows run in a loop of their own)
 *   "bt_block_waves"   half history's back-trace: waves per workgroup, 0 = 16 | 8 | 4.  Eight-wave workgroups (208 registers per SIMD) can start
 *                      on a CU whose SIMDs each hold one 256-register forward wave, i.e. beside the next batch's forward pass at up to
 *                      4 x CUs songs in flight (the two-stream schedule); sixteen-wave ones cannot
 *   "win_shift"        LDS window shift 0..3 (-1 from the plan); "wave_min_batch" (0 default), "wave_two" 1 | 2 (register budget of
 *                      the wave kernel) + 4 = a full-history row carries its own scalars only (default: also those of the two frames
 *                      before it, so that the back-trace touches one scalar line per three frames; A/B and tests)
 *   "wave_history"     wave form: 0 / 1 = store every delta row | 2 = store the rows of even frames only (the back-trace rebuilds
 *                      the 32 values an odd frame needs from the row before it and the emissions): half the workspace and a
 *                      faster forward pass for a slower back-trace; VIT_EUNSUPPORTED where the plan does not
 *                      allow it (window 32 wide with an affine start, <= 2 extra columns, S <= 378)
 *   "wave_uniform"     wave form: 0 = specialised variants where the plan proves them -- the one extra column is the last state (every
 *                      matrix the reference builds), and a lane's slots 0..4 share the row constant and the extra-column weight
 *                      (its 361-state matrices; for its 321-state ones three groups of slots do) | 1 = neither | 2 = the first only |
 *                      3 = the three-group form also where two groups would do
 *   "floor_live_window"   split-window floor kernel (what "forward_form" 6 forces): 0 = its full-window waves evaluate only the window
 *                      entries the plan proves live for their targets (rows 0 .. 255: the trailing entries that equal the row constant or
 *                      are an extra column are covered by the frame-maximum candidate and the extra-column path; 29 of 32 on the
 *                      reference's 361-state grid, 25 on its 321-state grids) | 1 = always the whole window
 *   "f64_units_per_cu" vit_decode_f64_packed_checkpointed(): (recording, segment) units per compute unit and launch, 1 .. 4 (0 = the forward
 *                      instantiation's own); it changes vit_f64_packed_bounded_units() and the workspace size with it
 *   "timing"           ablation / probe mask: accepted only by a -DVIT_TIMING_HOOKS build (VIT_EUNSUPPORTED otherwise;
 *                      those bits change results)
 *   "reset"            back to the defaults
 * Not thread-safe against concurrent decodes on the same plan.
 */
int vit_plan_set_option(vit_plan *plan, const char *key, int64_t value);

/* Device image of the plan: the caller allocates vit_plan_image_bytes() bytes of
 * device memory (256-byte aligned) and uploads once; the copy is enqueued on `stream`. */
size_t vit_plan_image_bytes(const vit_plan *plan);
int vit_plan_upload(vit_plan *plan, void *device_image, size_t bytes, vit_stream stream);

/* Bytes of device workspace vit_decode() needs for a [B,T,S] batch (float32 delta history
 * [B,T,SD] + per-song terminals; SD = ceil((S+2)/4)*4 with the per-frame maximum in pad column S, or 64*ceil(S/64) in slot
 * order for the wave form -- the size covers whichever form runs).  256-byte aligned base required. */
size_t vit_workspace_bytes(const vit_plan *plan, int64_t B, int64_t T);
/* The same for ONE algo (what vit_forward / vit_decode check a workspace against): smaller than vit_workspace_bytes() where
 * the chosen kernel keeps a narrower or a half history -- the wave form stores [B, ceil(T/2), 64*ceil(S/64)] floats.  The
 * answer depends on B (VIT_ALGO_AUTO / _BANDED pick the form by batch size) and on the plan's options; 0 = algo unsupported. */
size_t vit_workspace_bytes_for(const vit_plan *plan, int64_t B, int64_t T, int algo);

/*
 * Decode B songs.
 *   logE      : device, [B,T,S] C-order, float32 or float16 (emis_dtype)
 *   lengths   : device, [B] int64 or NULL; song b uses frames [0, clamp(lengths[b],1,T))
 *   workspace : device, >= vit_workspace_bytes(plan,B,T)
 *   states    : device, [B,T] int32; frames past a song's length are set to -1
 *   loglik    : device, [B] float32 or NULL
 * Enqueues kernels on `stream` and returns; no host synchronisation.
 *
 * ALIGNMENT, for this and every other entry point of this header: a data pointer needs the alignment of its element type and
 * nothing more -- logE 4 bytes (VIT_F32) or 2 bytes (VIT_F16), logits, logE_out, hf0, stats, notes and float32 loglik 4 bytes,
 * states and bins 4 bytes, the float64 loglik 8 bytes, voiced 1 byte.  A tensor may start anywhere inside a larger buffer; rows of
 * S = 361 or 722 elements start at every alignment anyway.  The kernels read and write these buffers with element-aligned vector
 * types and 16- / 32-bit buffer accesses; no access is wider than its proven alignment.  The two exceptions are the buffers the
 * library lays out itself: `workspace` and the plan's device image need a 256-byte aligned base, and a workspace pointer that is not
 * is refused with VIT_EINVAL before anything is enqueued.
 *
 * OUTPUTS NEED NOT BE INITIALISED: every call that returns VIT_OK writes every states[b][t], t < len_b (the path), and -1 into every
 * states[b][t], len_b <= t < T (the packed decodes: every entry of states, no -1), and every loglik[b]; what the buffers held before
 * the call has no influence on the result (the verify pass of the time-parallel back-trace reads back `states`, but only entries
 * this call has written).  Nothing is written outside [states, states + B * T), [loglik, loglik + B) and [workspace, workspace +
 * the bytes the size query of the call returns), and what an earlier call left in the workspace has no influence either.  A call that returns VIT_EINVAL, VIT_EWORKSPACE, VIT_EUNSUPPORTED or
 * VIT_ENOTUPLOADED has written nothing; vit_decode() included where "backtrace_form" 4 does not apply to the plan.
 */
int vit_decode(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, int64_t T,
               const int64_t *lengths, void *workspace, size_t workspace_bytes,
               int32_t *states, float *loglik, int algo, vit_stream stream);

/* Forward pass only / back-trace only; used by bench.py to time the two kernels separately and to run the back-trace
 * of one batch on another stream.  vit_decode() == forward then backtrace.  vit_forward records, per plan and workspace
 * pointer, which kernel family filled the workspace and how its history rows are laid out; vit_backtrace reads that
 * record (its `algo` argument is ignored) and returns VIT_ENOFORWARD when this workspace has no forward pass of the same
 * (B, T) on record.  The caller orders the two calls (same stream, or an event).  A plan keeps the records of the 64
 * workspaces most recently written; a failed vit_forward leaves none for its workspace.
 *
 * LIFETIME RULE: the emission tensor handed to vit_forward must stay valid and UNCHANGED until vit_backtrace has run -- a half
 * history (wave form, "wave_history" 2) re-reads 32 emission values of every odd frame through the pointer vit_forward
 * recorded.  vit_backtrace_checked() takes the emission pointer and storage type again and returns VIT_EINVAL when they are
 * not the ones on record (a double-buffered caller that refilled or swapped its emission buffer between the two phases);
 * the Python host always calls that form. */
int vit_forward(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, int64_t T,
                const int64_t *lengths, void *workspace, size_t workspace_bytes,
                float *loglik, int algo, vit_stream stream);
int vit_backtrace(const vit_plan *plan, int64_t B, int64_t T, const int64_t *lengths,
                  void *workspace, size_t workspace_bytes, int32_t *states, int algo, vit_stream stream);
int vit_backtrace_checked(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, int64_t T,
                          const int64_t *lengths, void *workspace, size_t workspace_bytes, int32_t *states,
                          int algo, vit_stream stream);

/* Which forward kernel family vit_forward() would launch for (plan, options, algo, batch size): 1 dense / step-structured,
 * 2 banded with one song per workgroup, 3 banded with one song per wavefront; a negative vit_status when the algo is not
 * available for this plan.  (The thresholds scale with the device's compute units; callers should ask, not guess.) */
int vit_forward_family(const vit_plan *plan, int64_t B, int algo);

/*
 * Bounded-workspace decode: the same result as vit_decode() with a workspace of about (T / segment_frames + segment_frames)
 * delta rows per song instead of T (the reference keeps its work buffers T1 / T2 for one song at a time,
 * tonet/for_paper.py:1852-1853; vit_decode keeps a history for the whole batch).  Pass 1 runs the forward recursion and keeps
 * one row per segment of segment_frames frames; pass 2 re-runs it segment by segment from the last to the first and
 * back-traces each.  Exact by construction; about twice the forward work.  64 <= segment_frames <= 2^24 (values above T act
 * like T; out of range: VIT_EINVAL, size 0).  Three kinds of plan are served, whatever VIT_ALGO_* a normal decode would take:
 *   - plans with the wave form (vit_plan_info reserved[2] bit 3): the general wave kernel with a full history of the segment and
 *     the sparse back-trace.  Honoured options: "bt_fast_rows", "wave_two"; ignored: "wave_history", "wave_uniform",
 *     "backtrace_form", "bt_chunks", "bt_warm".
 *   - banded plans without the wave form whose floor form is proven (reserved[1]) and that have no dense rows (the 722-state jdc
 *     grids): one song per workgroup, always the one-target floor kernel, and the sparse back-trace over its rows (the lane form
 *     where the sparse one does not apply).  Window widths >= 64 or more than 384 states.
 *   - step-structured plans (reserved[2] bit 2, the Durrieu matrix): the step kernel with the bands split over two waves, and
 *     the generic back-trace with the chunk count taken from the segment length.
 *   For the last two, honoured: "bt_fast_rows", "bt_warm", "win_shift"; ignored: "forward_form", "step_form", "backtrace_form",
 *   "bt_chunks".
 * Every other plan (unstructured matrices, banded plans with only the scan form or with dense rows) gets size 0 and
 * VIT_EUNSUPPORTED, before anything is enqueued.  The workspace holds per song T / segment_frames checkpoint rows and
 * segment_frames + 1 rows (wave form; 64 * ceil(S / 64) floats each) or segment_frames + 2 rows (the other two; ceil((S + 2) / 4) * 4
 * floats each) of the segment being walked.  The library does not record this call for vit_backtrace().
 */
size_t vit_workspace_bytes_checkpointed(const vit_plan *plan, int64_t B, int64_t T, int64_t segment_frames);
int vit_decode_checkpointed(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, int64_t T,
                            const int64_t *lengths, void *workspace, size_t workspace_bytes, int32_t *states,
                            float *loglik, int64_t segment_frames, vit_stream stream);

/*
 * Packed (ragged) decode: B songs of DIFFERENT lengths without padding.  The reference decodes every recording whole with its
 * own T (tonet/for_paper.py:2304-2309, one viterbi(logits) call per recording).
 *   logE    : device, [offsets[B], S] C-order: the emission rows of song b are rows offsets[b] .. offsets[b+1]-1
 *   offsets : HOST, [B+1] int64, offsets[0] = 0, strictly increasing (every song holds at least one frame)
 *   states  : device, [offsets[B]] int32, packed like the emission rows
 *   loglik  : device, [B] float32 or NULL
 * Which plans: (a) plans with the wave form (vit_plan_info reserved[2] bit 3): the forward pass runs min(B, 8 x compute units)
 * wavefronts, each decoding a host-packed list of songs back to back (longest-first greedy bins by frame count), so a launch
 * costs (total frames / wavefronts), not its longest song, and neither memory nor time is spent on padding; the back-trace cuts
 * every song into chunks of about equal length, one chunk per lane ("backtrace_form" 4's kernels).  (b) Banded plans without the
 * wave form whose floor form is proven (reserved[1]; the 722-state jdc grids): the same scheme with one WORKGROUP per slot -- as
 * many slots as workgroups of the floor kernel are resident at once (an occupancy query x compute units), at most B and at most
 * total frames / longest song --, history rows in the workgroup layout (stride ceil((S+2)/4)*4, state i in column i, the frame
 * maximum in column S), the same lane back-trace.  (c) Step-structured plans (reserved[2] bit 2; the Durrieu matrix): the step
 * kernel per slot and the generic (lazy) back-trace with at most 32 chunks per song, none shorter than 1024 frames.  Every other
 * plan (unstructured matrices, banded plans that only have the scan form) gets 0 from vit_workspace_bytes_packed and
 * VIT_EUNSUPPORTED from vit_decode_packed, before anything is enqueued; a size > 0 means the decode launches.  Of the plan's
 * options the packed decode of (b) / (c) honours "bt_warm" and "win_shift" and ignores "forward_form", "step_form",
 * "backtrace_form" and "bt_chunks".
 * The library builds the slot and chunk tables on
 * the host from `offsets` and uploads them through a pinned staging buffer it owns (it waits for the previous call's upload
 * before reusing it; otherwise no host synchronisation; the first packed decode of a plan of (b) / (c) asks the runtime for the
 * kernel's occupancy).  Bit-identical to vit_decode() of each song alone.  Not thread-safe against
 * concurrent packed decodes on the same plan (one staging buffer per plan); `lengths`-style padding does not exist here, so states
 * carries no -1 entries.
 */
size_t vit_workspace_bytes_packed(const vit_plan *plan, int64_t B, int64_t total_frames);
int vit_decode_packed(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, const int64_t *offsets,
                      void *workspace, size_t workspace_bytes, int32_t *states, float *loglik, vit_stream stream);

/*
 * Packed decode under a workspace budget: vit_decode_packed() with the bounded workspace of vit_decode_checkpointed().  The
 * reference decodes one recording at a time, each with its own length (tonet/for_paper.py:2304-2309), and keeps its work buffers
 * T1 / T2 for that one recording (:1852-1853); vit_decode_packed keeps a delta row for every frame it is handed.
 *   logE, offsets, states, loglik : exactly as for vit_decode_packed (offsets on the HOST; states packed, no -1 entries)
 *   segment_frames : the rule of vit_decode_checkpointed: 64 <= K <= 2^24, a value above the longest song acts like that length
 *                    (out of range: VIT_EINVAL, size 0)
 * Segments are per song: song b has n_b = ceil(T_b / K).  Pass 1 is the packed forward pass (min(B, 8 x compute units, total frames /
 * longest song) wavefronts walking host-packed song lists) and keeps the delta row in front of every segment but a song's first --
 * sum (n_b - 1) <= total frames / K rows -- and every song's terminal state and log-likelihood.  Pass 2 works on (song, segment)
 * units, one wavefront each: the units of a song run from its last segment to its first, units of different songs are independent;
 * the host lists the launches up front, each with up to n_units = min(B, 8 x compute units) units, at most one per song, the songs
 * with the most segments left first -- about max(longest n_b, total units / n_units) launches.  A launch re-runs the forward
 * recursion of its units from their checkpoint rows into K + 1 rows per unit and back-traces them (the sparse back-trace of
 * vit_decode_checkpointed).  States and log-likelihoods are bit-identical to vit_decode_packed on the same input, hence to
 * vit_decode() of each song alone; about twice the forward work.
 * Workspace: n_units x (K + 1) rows + sum (n_b - 1) checkpoint rows + one scratch row per wavefront of pass 1, 64 * ceil(S / 64)
 * floats each, + the tables: it depends on the lengths, so the size function takes `offsets` (256-byte aligned base required).
 * Which plans: plans with the wave form (vit_plan_info reserved[2] bit 3): the reference's 321- and 361-state matrices.  Every
 * other plan (the 722-state floor and step plans, unstructured matrices, scan-only banded plans) gets size 0 and VIT_EUNSUPPORTED
 * before anything is enqueued; a size > 0 means the decode launches.  Honoured options: "wave_uniform", "wave_two",
 * "bt_fast_rows"; ignored: "wave_history", "forward_form", "backtrace_form", "bt_chunks", "bt_warm", "wave_min_batch".
 * VIT_EINVAL: a null pointer, offsets that do not start at 0 or do not increase strictly, K out of range, a bad dtype;
 * VIT_EWORKSPACE: a workspace below the size function's answer.  The tables (slot lists, unit lists, checkpoint bases) are built on
 * the host and go through the plan's pinned staging buffer in one upload: the call waits for the previous upload from that buffer
 * (this call's or vit_decode_packed's) and synchronises nowhere else; no device allocation.  Not thread-safe against concurrent
 * packed decodes on the same plan.  The library does not record this call for vit_backtrace().
 */
size_t vit_workspace_bytes_packed_checkpointed(const vit_plan *plan, int64_t B, const int64_t *offsets /* HOST, [B+1] */,
                                               int64_t segment_frames);
int vit_decode_packed_checkpointed(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, const int64_t *offsets,
                                   void *workspace, size_t workspace_bytes, int32_t *states, float *loglik,
                                   int64_t segment_frames, vit_stream stream);

/*
 * Packed decode under a workspace budget for EVERY plan with a packed decode: a superset of vit_decode_packed_checkpointed(), whose
 * entry points keep their behaviour (size 0 / VIT_EUNSUPPORTED for plans without the wave form).  Arguments, argument rules, status
 * codes, the staging of the tables and the thread-safety note are those of vit_decode_packed_checkpointed(): 64 <= K <= 2^24 (a
 * value above the longest song acts like that length), offsets on the HOST from 0 with no empty song, a 256-byte aligned workspace,
 * B = 0 is VIT_OK and enqueues nothing.  States and log-likelihoods are bit-identical to vit_decode_packed() on the same input.
 * Which plans, and what runs:
 *   - plans with the wave form: forwarded to vit_decode_packed_checkpointed() -- the same size, the same bits;
 *   - banded plans without it whose floor form is proven (the 722- and 721-state grids of jdc and imm): the scheme above with a
 *     WORKGROUP where it has a wavefront.  Pass 1 is vit_decode_packed's slot walk and keeps the row in front of every segment but a
 *     song's first; pass 2 runs one workgroup per (song, segment) unit into K + 2 rows of its own and back-traces the units with the
 *     sparse kernel.  Requires the sparse back-trace over the workgroup rows: a plan that only the lane form could back-trace
 *     (vit_decode_checkpointed serves it) gets size 0 here;
 *   - step plans (the Durrieu matrices, 705 .. 768 voiced states): the same with K + 1 rows per unit and the lazy back-trace;
 *   - everything else (unstructured matrices, scan-only banded plans): size 0 and VIT_EUNSUPPORTED before anything is enqueued.
 * A size > 0 means the decode launches.  vit_packed_bounded_units(): the units one pass-2 launch takes, min(B, u x compute units)
 * with u = 8 (wave form), 1 (floor plans) or 2 (step plans); 0 for plans the decode does not serve.  Every unit owns its rows, so u
 * is tuning, not correctness.  Compute units: of the device the plan was uploaded to, 256 before the upload.
 * Workspace of the workgroup forms: units x (K + 2 | K + 1) segment rows + sum (n_b - 1) checkpoint rows + one scratch row per
 * pass-1 slot (min(B, 8 x compute units) of them are provided for), (S + 5) / 4 * 4 floats each, + the tables of
 * vit_decode_packed_checkpointed().  Honoured options: "bt_fast_rows", "bt_warm", "win_shift".
 */
size_t vit_workspace_bytes_packed_bounded(const vit_plan *plan, int64_t B, const int64_t *offsets /* HOST, [B+1] */,
                                          int64_t segment_frames);
int vit_decode_packed_bounded(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, const int64_t *offsets,
                              void *workspace, size_t workspace_bytes, int32_t *states, float *loglik,
                              int64_t segment_frames, vit_stream stream);
int64_t vit_packed_bounded_units(const vit_plan *plan, int64_t B);

/*
 * Float64-accumulating decode: the reference's float64 Viterbi variant, dcnet/tf_viterbi_decoding.py:209-263 (viterbi_librosa_fn
 * there; its parameters and emissions are float32, only T1 is float64; the unused `p` at :255 is the log-likelihood returned here).
 * Inputs are the library's: the plan's float32 logA_T and log_pi, float32 or float16 log-emissions (float16 is widened to float32
 * first; every widening below is exact), lengths.  Bit for bit, with A[j][i] = logA_T[j][i]:
 *   d_0[j]  = f64( fl32(log_pi[j] + E_0[j]) )            the reference adds two float32 arrays, THEN stores into its float64 T1
 *   m_j     = max_i fl64( d_{t-1}[i] + f64(A[j][i]) )     psi_t[j] = LOWEST i attaining m_j
 *   d_t[j]  = fl64( m_j + f64(E_t[j]) )
 *   s_{T-1} = lowest argmax_j d_{T-1}[j];   s_t = psi_{t+1}[s_{t+1}];   loglik = d_{T-1}[s_{T-1}]   (a double)
 * -inf follows the rules of vit_decode(): the compare is strict, a dead song yields state 0 and a log-likelihood of -inf; NaN is
 * outside the contract.  On long inputs the path differs from vit_decode()'s in a few frames out of thousands (the float32 running
 * sum drifts); this one is the better-scoring path.
 * Plans served: banded plans whose one-maximum ("floor") form is proven, without dense rows, at an instantiated window width
 * (16 / 32 / 64 / 84 / 96 / 128) and at most 768 states -- every banded matrix the reference builds (321, 361, the 721- / 722-state
 * bands of jdc and imm).  Unstructured matrices, the Durrieu (step) matrices and scan-only or dense-row plans get size 0 and
 * VIT_EUNSUPPORTED before anything is enqueued; a size > 0 means the decode launches.
 * Argument checks, status codes and their order, the 256-byte workspace alignment, lengths clamped to [1, T] and states[b, t] = -1
 * past a song's end are vit_decode()'s; B = 0 is VIT_OK.  The call does not synchronise the host and allocates nothing.  It
 * overwrites the workspace: the record an earlier vit_forward() left for it is dropped and none is written, so a vit_backtrace()
 * on that workspace afterwards is VIT_ENOFORWARD.  Workspace: B x T rows of (S + 3) / 2 * 2 doubles (every d row and the frame maximum) + tables.
 * Honoured options: "bt_chunks", "bt_warm"; every other option is ignored.
 */
size_t vit_workspace_bytes_f64(const vit_plan *plan, int64_t B, int64_t T);
int vit_decode_f64(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, int64_t T, const int64_t *lengths,
                   void *workspace, size_t workspace_bytes, int32_t *states, double *loglik /* [B] or NULL */, vit_stream stream);

/*
 * The same over recordings of different lengths without padding: vit_decode_packed()'s buffers (logE [offsets[B], S], states
 * [offsets[B]], recording b in rows offsets[b] .. offsets[b+1] - 1; offsets on the HOST) with vit_decode_f64()'s recursion.  States
 * and log-likelihoods are bit for bit those of vit_decode_f64() of each recording alone.  The reference decodes recording by
 * recording, each with its own length (tonet/for_paper.py:2304-2309).
 * Plans served: exactly those of vit_decode_f64() (one predicate behind both); every other plan gets size 0 and VIT_EUNSUPPORTED
 * before anything is enqueued, and a size > 0 means the decode launches.
 * Argument rules, status codes and their order are vit_decode_packed()'s: null plan / offsets / workspace, B out of range,
 * a misaligned workspace or a bad dtype VIT_EINVAL (VIT_ENOTUPLOADED in its place); then VIT_EUNSUPPORTED; then bad offsets
 * (offsets[0] != 0, a recording with fewer than 1 or more than 2^30 frames) VIT_EINVAL; B = 0 VIT_OK; null logE / states VIT_EINVAL;
 * a workspace below vit_workspace_bytes_f64_packed(plan, B, offsets[B]) VIT_EWORKSPACE.
 * Forward: one workgroup per slot, min(B, resident workgroups of the packed kernel x compute units, max(1, total frames /
 * longest recording)) slots, each walking its recordings back to back; recordings go longest first into the lightest slot.  The
 * occupancy answer is asked of the device once per plan and emission type.
 * Back-trace: one wave per (recording, chunk).  With N = total frames and tmax = the longest recording,
 *   cf = max(ceil(N / (8 x compute units)), 8 * 128, ceil(tmax / 32))
 * and recording b gets clamp(T_b / cf, 1, 32) chunks (the division rounds down: no chunk is shorter than cf frames); a second pass
 * per recording verifies every chunk's entry state and repairs what was guessed wrong.  The chunk rule is tuning: the states do not
 * depend on it.
 * The slot and chunk tables go through the plan's pinned staging buffer with one upload: like vit_decode_packed() the call is not
 * thread-safe against other packed decodes on the same plan, may wait for the previous packed call's upload, does no other host
 * synchronisation and no device allocation.  It drops the workspace's vit_forward() record as vit_decode_f64() does.
 * Workspace: offsets[B] rows of (S + 3) / 2 * 2 doubles + per-recording terminal states + chunk entries + the tables.
 * Honoured options: "bt_warm"; "bt_chunks" and every other option are ignored.
 */
size_t vit_workspace_bytes_f64_packed(const vit_plan *plan, int64_t B, int64_t total_frames);
int vit_decode_f64_packed(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, const int64_t *offsets /* HOST, [B+1] */,
                          void *workspace, size_t workspace_bytes, int32_t *states /* [offsets[B]] */,
                          double *loglik /* [B] or NULL */, vit_stream stream);

/*
 * vit_decode_f64() under a workspace budget: the scheme of vit_decode_checkpointed() with the float64 kernels.  States and
 * log-likelihoods are bit for bit those of vit_decode_f64() on the same arguments (-1 past a song's length, lengths clamped to
 * [1, T], the -inf rules and the float16 widening included).  The reference keeps T1 / T2 for one recording at a time.
 * Plans served: exactly those of vit_decode_f64() (one predicate behind all float64 entry points); every other plan gets size 0
 * and VIT_EUNSUPPORTED before anything is enqueued, and a size > 0 means the decode launches.
 * segment_frames = K: 64 <= K <= 2^24, a value above T acts like T; out of range VIT_EINVAL and size 0.
 * Argument checks, status codes and their order are vit_decode_f64()'s, with the K check behind the dtype check and in front of
 * VIT_EUNSUPPORTED (where vit_decode_checkpointed() has it); B = 0 is VIT_OK; a workspace one byte below the size function's answer
 * is VIT_EWORKSPACE and nothing is written.  No host synchronisation, no device allocation, O(T / K) launches on `stream`.  It
 * drops the workspace's vit_forward() record and writes none.
 * Pass 1 runs the forward recursion over all T frames, one workgroup per song, and keeps the d row of the frame in front of every
 * segment but a song's first, plus every song's terminal state and log-likelihood.  Pass 2 walks the segments from the last to the
 * first: the forward kernel resumed from the checkpoint row into the song's segment rows, then the segment's back-trace from the
 * state decided just behind it (a song's last segment: from the terminal state); a song that ends before a segment starts is
 * skipped in it.  About twice the forward work.
 * Workspace, with K = min(segment_frames, T), nseg = ceil(T / K), SD = (S + 3) / 2 * 2 and r(x) = x rounded up to 256:
 *   r(B * nseg * SD * 8)        checkpoint rows: nseg - 1 per song and one more (where K divides T, pass 1 stores frame T - 1)
 * + r(B * (K + 1) * SD * 8)     segment rows: ONE IN FRONT of the segment, which receives the frame maximum M of the checkpoint
 *                               frame (written, never read), and the K of the segment.  M of the segment's last row is formed behind
 *                               the segment's last frame from what that frame published: no frame past the segment is run.
 * + r(4 B) + r(128 B) + r(8 B) + r(4 B)   terminal states, chunk entries, the sub-problems' lengths and start states.
 * A segment's back-trace runs min(32, ceil(2048 / B), frames / max(2 * warm, 64)) chunks per song (at least one) with a warm-up of
 * 64 frames, and the verify / repair pass of vit_decode_f64(); the chunk rule is tuning: the states do not depend on it.
 * Honoured options: "bt_chunks", "bt_warm" (per segment); every other option is ignored.
 */
size_t vit_workspace_bytes_f64_checkpointed(const vit_plan *plan, int64_t B, int64_t T, int64_t segment_frames);
int vit_decode_f64_checkpointed(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B, int64_t T, const int64_t *lengths,
                                void *workspace, size_t workspace_bytes, int32_t *states, double *loglik /* [B] or NULL */,
                                int64_t segment_frames, vit_stream stream);

/*
 * vit_decode_f64_packed() under a workspace budget: recordings of different lengths, unpadded, with segments per recording -- the
 * scheme of vit_decode_packed_bounded() with the float64 kernels.  Buffers are vit_decode_f64_packed()'s: logE [offsets[B], S], states
 * [offsets[B]] (no -1 entries), offsets on the HOST.  States and log-likelihoods are bit for bit those of vit_decode_f64_packed() on
 * the same input, hence those of vit_decode_f64() of each recording alone.
 * Plans served: exactly those of vit_decode_f64() (one predicate behind all float64 entry points); every other plan gets size 0,
 * vit_f64_packed_bounded_units() 0 and VIT_EUNSUPPORTED before anything is enqueued; a size > 0 means the decode launches.
 * segment_frames = K: 64 <= K <= 2^24, a value above the longest recording acts like that length.  Recording b has
 * n_b = ceil(T_b / K) segments.
 * Checks, in this order (vit_decode_packed_bounded()'s): null plan / offsets / workspace, B out of range, a misaligned workspace or a
 * bad dtype VIT_EINVAL (VIT_ENOTUPLOADED in its place); K out of range VIT_EINVAL; VIT_EUNSUPPORTED; bad offsets VIT_EINVAL; B = 0
 * VIT_OK; null logE / states VIT_EINVAL; a workspace below the size function's answer VIT_EWORKSPACE.  A refused call writes nothing.
 * Pass 1 is vit_decode_f64_packed()'s slot walk; it keeps the d row of the frame in front of every segment but a recording's first
 * (sum (n_b - 1) rows, nothing else) and every recording's terminal state and log-likelihood.  Pass 2 works on (recording, segment)
 * units, a recording's from its last segment to its first, at most one unit per recording in a launch: the forward kernel resumed
 * from the unit's checkpoint row into the unit's own rows, then the units' back-trace, which writes states[offsets[b] + segment * K ..].
 * vit_f64_packed_bounded_units(): the units one launch takes, n_units = min(B, u x compute units); u is a constant of the forward
 * instantiation (window width W, target waves n = 2 / 4 / 6 / 8 / 12, the least with 64 n >= S): 1 on twelve waves, else the workgroups
 * whose waves one compute unit's registers hold, min(4, 4 r / n) with r = 4, 3, 2 waves per SIMD at W = 16, 32, wider -- 2 at S = 361
 * ("f64_units_per_cu" 1 .. 4 overrides it, for measurements; it changes the size).  Every unit owns its rows:
 * u is tuning, not correctness.  Compute units: of the device the plan was uploaded to, 256 before the upload.
 * Workspace, with K = min(segment_frames, longest recording), SD = (S + 3) / 2 * 2, U = sum n_b and r(x) = x rounded up to 256:
 *   r(sum (n_b - 1) * SD * 8)        checkpoint rows
 * + r(n_units * (K + 1) * SD * 8)    unit rows: one in front of the segment (it receives M of the checkpoint frame: written, never
 *                                    read) and the K of the segment; no frame past the segment is run
 * + r(4 B) + r(n_units * 32 * 4)     terminal states, chunk entries
 * + r(8 n_units) + r(4 n_units) + r(8 n_units)   the units' lengths, start states and first entries in `states`
 * + r(8 (B + 1)) + r(8 (B + 1)) + r(4 (min(B, 8 x compute units) + 1)) + r(4 B) + r(4 U) + r(4 U)
 *                                    the tables: offsets, checkpoint bases, pass 1's slots and their recordings, the units' recordings
 *                                    and segments in launch order -- staged in the plan's pinned buffer and sent in one upload.
 * A launch back-traces its n units in min(32, ceil(2048 / n), (K + 1) / max(2 * warm, 64)) chunks each (at least one), warm-up 64.
 * Like vit_decode_f64_packed() the call is not thread-safe against other packed decodes on the same plan, may wait for the previous
 * packed call's upload, does no other host synchronisation and no device allocation; it drops the workspace's vit_forward() record and
 * writes none.  Honoured options: "bt_chunks", "bt_warm" (per unit), "f64_units_per_cu"; every other option is ignored.
 */
size_t vit_workspace_bytes_f64_packed_checkpointed(const vit_plan *plan, int64_t B, const int64_t *offsets /* HOST, [B+1] */,
                                                   int64_t segment_frames);
int vit_decode_f64_packed_checkpointed(const vit_plan *plan, const void *logE, int emis_dtype, int64_t B,
                                       const int64_t *offsets /* HOST, [B+1] */, void *workspace, size_t workspace_bytes,
                                       int32_t *states /* [offsets[B]] */, double *loglik /* [B] or NULL */, int64_t segment_frames,
                                       vit_stream stream);
int64_t vit_f64_packed_bounded_units(const vit_plan *plan, int64_t B);

/*
 * Fused logits -> path decode: what callers of the reference run is Viterbi.__call__ (tonet/for_paper.py:1817-1831) -- pitch
 * logits -> observation log-probabilities -> Viterbi decode.  vit_obs_*() + vit_decode() do that with a [B,T,S] float32
 * emission tensor written to and read back from device memory (2 x 4 S bytes per frame, 44 GB for [1024, 30000, 361]); here the
 * emission rows are built inside the forward pass, in the workgroup that consumes them, and exist in LDS only.
 *   obs       : HOST, the arguments of vit_obs_shaun (mode 0) / vit_obs_softmax (1) / vit_obs_softmax_scaled (2); obs->prior is a
 *               device pointer.  obs->n_bins + 1 must be the plan's S (VIT_EINVAL otherwise).
 *   logits    : device, [B,T,n_bins] float32 (mode 1: [B,T,n_bins+1], unvoiced column first), C-order
 *   lengths, workspace, states, loglik : as for vit_decode(); workspace >= vit_workspace_bytes_logits(plan, obs, B, T) -- a full
 *               delta history in the wave layout (64 * 6 floats per frame and song) and nothing for emissions
 *   logE_out  : NULL, or device [B,T,S] float32: the emission rows are ALSO written there (frames inside a song's length only),
 *               bit for bit what vit_obs_*() writes
 * States and log-likelihoods are bit-identical to vit_obs_*() into a buffer followed by vit_decode(..., VIT_ALGO_WAVE).
 * Which plans and builders: plans with the wave form (vit_plan_info reserved[2] bit 3) whose one extra column is the last state
 * (the reference's 321- and 361-state matrices), n_bins 320 or 360, and the reference's three builder geometries -- mode 0 with
 * spw 5, mode 1 with spw 15, mode 2 with spw 5.  Everything else (no wave form, the 722-state grids, two extra columns, other
 * peak widths, "wave_uniform" 1) gets 0 from vit_workspace_bytes_logits and VIT_EUNSUPPORTED from vit_decode_logits before
 * anything is enqueued; a size > 0 means the decode launches.  Honoured options: "bt_chunks", "bt_warm", "bt_fast_rows",
 * "bt_block_waves", "backtrace_form", "wave_uniform"; ignored: "wave_history" (a half history re-reads emissions, which do not exist
 * here), "forward_form", "wave_two".  No host synchronisation, no allocation.  The library does not record this call for
 * vit_backtrace().
 */
typedef struct vit_obs_params {
    int32_t mode;                    /* 0 shaun | 1 softmax (logits [.., n_bins+1], unvoiced first) | 2 scaled softmax */
    int32_t n_bins, spw;
    double threshold_logit;          /* mode 0: threshold logit; mode 2: the unvoiced logit */
    double offset, scale;            /* mode 0 */
    const float *prior;              /* mode 2: device [n_bins+1] or NULL */
} vit_obs_params;
size_t vit_workspace_bytes_logits(const vit_plan *plan, const vit_obs_params *obs, int64_t B, int64_t T);
int vit_decode_logits(const vit_plan *plan, const float *logits, const vit_obs_params *obs, int64_t B, int64_t T,
                      const int64_t *lengths, void *workspace, size_t workspace_bytes, float *logE_out,
                      int32_t *states, float *loglik, vit_stream stream);

/*
 * The fused logits -> path decode with a bounded workspace: vit_decode_checkpointed()'s scheme with the fused workgroup as its
 * forward launch.  Pass 1 builds every emission row once, in LDS, and keeps one delta row per segment of K = segment_frames frames
 * plus the terminal state and the log-likelihood; pass 2 walks the segments from the last to the first: the fused workgroup builds
 * the segment's emission rows AGAIN from the logits (the builders work per frame: the same bits), resumes the recursion from the
 * segment's checkpoint row into K rows per song, and the segment is back-traced from the state the segment behind it decided.
 * Neither a [B,T,S] emission tensor nor a [B,T] delta history exists: besides logits and outputs only the workspace is resident,
 * 1.7 GB for [1024, 30000, 361] at K = 1024 where vit_decode_logits() takes 47 GB.  About twice the forward work.
 *   arguments : as for vit_decode_logits(), without logE_out (the rows are built twice; the call exists to save memory), and
 *               segment_frames as for vit_decode_checkpointed(): 64 .. 2^24, a value above T acts like T.
 *   workspace >= vit_workspace_bytes_logits_checkpointed(plan, obs, B, T, segment_frames), which equals
 *               vit_workspace_bytes_checkpointed(plan, B, T, segment_frames) wherever it is not 0.
 * States and log-likelihoods are bit-identical to vit_decode_logits() and so to vit_obs_*() + vit_decode(..., VIT_ALGO_WAVE).
 * Which plans and builders: those of vit_decode_logits().  Everything else, and a segment length out of range, gets 0 from the size
 * function; a size > 0 means the decode launches.  Status, in this order: NULL plan or obs VIT_EINVAL; VIT_ENOTUPLOADED; NULL or
 * misaligned workspace, B or T out of range VIT_EINVAL; a bad obs or obs->n_bins + 1 != S VIT_EINVAL; segment_frames out of range
 * VIT_EINVAL; VIT_EUNSUPPORTED; NULL logits or states with B > 0 VIT_EINVAL; VIT_EWORKSPACE; B = 0 VIT_OK.  A refused call enqueues
 * and writes nothing.  Honoured options: "wave_uniform", "bt_fast_rows"; ignored: "bt_chunks", "bt_warm" (every segment warms up 64
 * frames, as in vit_decode_checkpointed() for wave-form plans), "bt_block_waves", "backtrace_form", "wave_history", "forward_form",
 * "wave_two".  No host synchronisation, no allocation; the call drops the workspace's vit_forward() record and writes none.
 */
size_t vit_workspace_bytes_logits_checkpointed(const vit_plan *plan, const vit_obs_params *obs, int64_t B, int64_t T,
                                               int64_t segment_frames);
int vit_decode_logits_checkpointed(const vit_plan *plan, const float *logits, const vit_obs_params *obs, int64_t B, int64_t T,
                                   const int64_t *lengths, void *workspace, size_t workspace_bytes, int32_t *states,
                                   float *loglik, int64_t segment_frames, vit_stream stream);

/*
 * Streaming decode: the forward pass advances as chunks of emission rows arrive, the back-trace runs whenever a path is wanted.
 * The callers of the reference's decoders receive a recording batch by batch (tonet/for_paper.py:2246-2327) and decode behind the
 * last one; a session spends the forward recursion beside the acoustic model instead of behind it.  History rows, back-trace and
 * results are exactly those of vit_decode() of the same recordings: states and log-likelihoods are bit-identical for any chunking.
 *
 *   vit_workspace_bytes_stream(plan, B, T_cap)  bytes of a session of B recordings of at most T_cap frames each: the [B, T_cap] delta
 *               rows, terminal states and log-likelihoods, device lengths, the per-launch tables and the back-trace's chunk entries,
 *               flags and counters.  0 = the plan is not served (or NULL plan, B < 1, T_cap < 1, either above 2^30).
 *   vit_stream_open()       the session: host memory only (plan, workspace pointer, per-song positions, emission type).  The
 *               workspace is caller-owned, 256-byte aligned, and must outlive the session, as must the plan.  Nothing is enqueued.
 *   vit_stream_append()     logE: device [B, n, S] of emis_dtype, rows [b][0 .. counts[b]) are the next counts[b] frames of recording b
 *               (counts: HOST [B], 0 <= counts[b] <= n; NULL = n for every recording).  One kernel launch on `stream`; where the
 *               recordings are not all at one position with one count, also one upload of two int32 [B] tables through the plan's
 *               pinned staging buffer, which first waits on the host for the upload before it (as vit_decode_packed()).  No other
 *               host synchronisation.  Emission rows are never read again: the chunk buffer may be reused once the append's kernel
 *               has run in stream order.  The emission type is fixed by the first append (vit_stream_reset() frees it).
 *   vit_stream_lengths()    frames appended per recording so far, HOST [B].
 *   vit_stream_backtrace()  decodes the recordings AS THEY STAND: states[b][0 .. len_b) = the best path of the len_b frames so far,
 *               states[b][len_b .. states_stride) = -1, loglik[b] (device [B], may be NULL) = its log-likelihood.  The session stays
 *               open: more frames may follow, and a later back-trace supersedes this one.
 *   vit_stream_reset()      every position back to 0 (host only); the workspace is reused as it is.
 *   vit_stream_close()      frees the session (not the workspace).  NULL is allowed.
 * The caller orders the calls of one session -- appends, back-traces and whatever rewrites a chunk or the workspace -- on one stream
 * or by events, as for vit_forward() / vit_backtrace().  Two sessions of one plan may run on two streams from one thread.
 *
 * Which plans: those with a stream instantiation of their workgroup forward kernel -- banded plans whose one-maximum ("floor") form
 * is proven, without dense rows, with an instantiated window width and an idle target slot (the reference's 321- and 361-state grids,
 * the 721- / 722-state grids of jdc and imm's wide matrix), and step-structured plans of the Durrieu geometry.  Unstructured
 * matrices, banded plans that only have the scan form and plans with dense rows get size 0 and VIT_EUNSUPPORTED.  A session always
 * runs one recording per workgroup, whatever B: it is meant for a few recordings at a time.  float32 history only.
 *
 * Status.  vit_stream_open(): NULL plan / out / workspace, B or T_cap out of range, misaligned workspace VIT_EINVAL; then
 * VIT_ENOTUPLOADED; then VIT_EUNSUPPORTED; then VIT_EWORKSPACE.  vit_stream_append(): NULL session or logE, a bad emis_dtype, n < 1,
 * an emis_dtype other than the first append's, a count outside [0, n] or pos[b] + counts[b] > T_cap for any b: VIT_EINVAL, with
 * nothing enqueued and no position moved.  vit_stream_backtrace(): NULL session or states, a recording still at length 0,
 * states_stride < max len_b: VIT_EINVAL; "backtrace_form" 4 where the lane kernel does not apply: VIT_EUNSUPPORTED.  A refused call
 * enqueues and writes nothing.  Honoured options: "bt_chunks", "bt_warm", "bt_fast_rows", "win_shift", and "backtrace_form" 4 (banded
 * plans); ignored: "forward_form", "step_form", "wave_*", "backtrace_form" 1 / 2 (the back-trace is the sparse kernel, the lane form
 * where that does not serve the rows, the lazy kernel for step plans).  No vit_forward() record is written; the one the workspace
 * carried is dropped by vit_stream_open().
 */
typedef struct vit_session vit_session; /* opaque: one streaming session */
size_t vit_workspace_bytes_stream(const vit_plan *plan, int64_t B, int64_t T_cap);
int vit_stream_open(const vit_plan *plan, int64_t B, int64_t T_cap, void *workspace, size_t workspace_bytes, vit_session **out);
int vit_stream_append(vit_session *s, const void *logE /* device [B, n, S] */, int emis_dtype, int64_t n,
                      const int64_t *counts /* HOST [B], 0 <= counts[b] <= n, or NULL = n for every song */, vit_stream stream);
int vit_stream_lengths(const vit_session *s, int64_t *lengths /* HOST [B] */);
int vit_stream_backtrace(vit_session *s, int32_t *states /* device [B, states_stride] */, int64_t states_stride,
                         float *loglik /* device [B] or NULL */, vit_stream stream);
int vit_stream_reset(vit_session *s);
void vit_stream_close(vit_session *s);

/* The commit point of a session: the path prefix that no later frame can change, and incremental output.
 *
 * For one recording with n frames appended and f frames committed so far (f = 0 after vit_stream_commit_begin() and after
 * vit_stream_reset()): psi_t[j] = the lowest-index argmax of vit_decode()'s recursion, U_{n-1} = all S states, U_{t-1} = psi_t[U_t].
 * With L = max_lookback, c = the LARGEST t with max(f, n-1-L) <= t <= n-2 and |U_t| = 1, s_c = its element.  If c exists the new
 * frontier is f' = c + 1 and states[f .. c] are written (s_c at frame c, s_{t-1} = psi_t[s_t] below it); otherwise, or with n < 2,
 * f' = f and nothing is written.  Exact, not a fixed-lag rule: every path through frame n-1, whatever is appended later, passes
 * frame c in state s_c, because a back-pointer is a function of the delta row below it and rows never change once written.
 *
 *   vit_workspace_bytes_stream_commit(plan, B)  bytes of the commit state (device frontiers [B], the call's length table, the
 *               committed ranges' first rows, lengths and start states, the back-trace's chunk entries and flags): a separate
 *               caller-owned, 256-byte-aligned buffer; the session's own workspace and its size are what they were.  0 where the plan
 *               is not served.
 *   vit_stream_commit_begin()  binds the buffer to the session and marks every frontier as 0.  Host only.
 *   vit_stream_commit()  for every recording b: states[b][f_b .. f'_b) and committed[b] = f'_b (device int64 [B]), NOTHING else of
 *               `states` (no -1 fill, nothing below f_b or from f'_b on).  A recording of 0 or 1 frames commits nothing and is no
 *               error.  No host synchronisation and no host read of a frontier: one upload (the lengths, through the plan's pinned
 *               staging buffer as in vit_stream_backtrace(), with the thread-safety of that call) and a constant number of launches on
 *               `stream`: the survivor merge kernel, then the lane back-trace (chunk flags' memset, speculative pass, verify, repair)
 *               over the committed ranges, whose bounds stay on the device.
 *               max_lookback bounds the frames the merge is looked for in (a call that finds none commits nothing; a later one may);
 *               the frames committed are walked whatever their number.
 * vit_stream_backtrace() is unchanged and may be called at any time; its prefix [0, f') equals what the commits wrote.
 *
 * Which plans: the banded session plans (every (window, waves) pair a session serves: the 321-, 361-, 721- and 722-state grids).
 * Step-structured plans (the Durrieu matrix) get size 0 and VIT_EUNSUPPORTED: their back-pointer decision is a whole-row kernel,
 * not a per-lane one.
 *
 * Status.  vit_stream_commit_begin(): NULL session, NULL or misaligned buffer VIT_EINVAL; then VIT_EUNSUPPORTED; then VIT_EWORKSPACE.
 * vit_stream_commit(): NULL session / states / committed, max_lookback < 1 or > 2^30: VIT_EINVAL; no vit_stream_commit_begin() on this
 * session: VIT_EINVAL; states_stride < max n_b: VIT_EINVAL.  A refused call enqueues and writes nothing. */
size_t vit_workspace_bytes_stream_commit(const vit_plan *plan, int64_t B);
int vit_stream_commit_begin(vit_session *s, void *commit_ws, size_t bytes);
int vit_stream_commit(vit_session *s, int32_t *states /* device [B, states_stride] */, int64_t states_stride,
                      int64_t *committed /* device [B] */, int64_t max_lookback, vit_stream stream);

/* Ring sessions: recordings of any length in a fixed window of history rows.
 *
 * No commit and no back-trace of the frames from the frontier f on ever reads a row below f (the proof above).  A ring session keeps
 * R = ring_rows history rows per recording, frame t in row t mod R of its recording, and a recording may grow to 2^30 frames.  The
 * results are those of vit_decode() of the whole recording, bit for bit: the concatenated vit_stream_commit_rel() outputs followed
 * by one vit_stream_tail().
 *
 *   vit_workspace_bytes_stream_ring(plan, B, ring_rows)  the layout of vit_workspace_bytes_stream() with ring_rows in place of T_cap:
 *               [B][ring_rows] delta rows, then the same counters, chunk flags, terminal states, log-likelihoods, chunk entries,
 *               device lengths and per-launch tables.  64 <= ring_rows <= 2^30, else 0.  0 where the plan is not served.
 *   vit_stream_open_ring()  as vit_stream_open().  Served: exactly the plans vit_stream_commit() serves (a ring advances by commits
 *               only); every other plan, step plans included: size 0 / VIT_EUNSUPPORTED.
 *   vit_stream_append()  on a ring session: the same call, still ONE kernel launch, also where the frames wrap.  Residency: rows
 *               [f_b, n_b) must stay in the ring.  The library never reads a frontier from the device; it keeps a HOST lower bound a_b
 *               of every frontier, 0 until the caller reports more with vit_stream_commit_ack().  pos[b] + counts[b] - a_b > R for
 *               any b: VIT_EWORKSPACE, nothing enqueued, no position moved -- acknowledge newer frontiers, or open with a larger R.
 *               pos[b] + counts[b] > 2^30: VIT_EINVAL.  STALL: where the survivors of a recording do not merge inside R frames its
 *               frontier stands, and once n_b - a_b = R the session cannot advance.  Merges come within tens of frames on the
 *               reference's matrices (the longest merge walk measured is 147 frames); choose R well above that plus the append size.
 *   vit_stream_commit_ack(s, frontiers)  HOST int64 [B]: frontiers the caller has READ BACK from the `committed` buffer of an earlier
 *               commit of this session.  Host only: no device access, no synchronisation.  A value below the last acknowledged one
 *               or above pos[b], or a session that is not a ring session: VIT_EINVAL, nothing changed.  A caller that acknowledges
 *               values it did not read lets appends overwrite rows a commit still needs: it gets WRONG STATES, but never an access
 *               outside the buffers (every row index is taken mod R, every range is cut to R frames).
 *   vit_stream_commit_rel()  vit_stream_commit()'s definition word for word, with a window-relative output: states[b][0 .. f'_b - f_b)
 *               = the states of frames f_b .. f'_b - 1, first[b] = f_b, committed[b] = f'_b (device int64 [B] each), NOTHING else.
 *               states_stride >= min(max n_b, R) suffices on a ring session (max n_b on a linear one).  Valid on ring and linear
 *               sessions after vit_stream_commit_begin(); vit_stream_commit()'s launch shape (one lengths upload, merge, flags'
 *               memset, speculative pass, verify, repair), no host synchronisation.
 *   vit_stream_tail()  the frames behind the frontier: states[b][0 .. n_b - f_b) = the best path of the n_b frames so far restricted
 *               to frames f_b .. n_b - 1, from the terminal state the last append wrote; first[b] = f_b; loglik as in
 *               vit_stream_backtrace().  Nothing else is written and the frontier does not move.  Before any commit f_b = 0: the call
 *               then equals vit_stream_backtrace() without the -1 fill.  Valid on both session kinds after vit_stream_commit_begin()
 *               (it uses the commit buffer's sub-problem tables: order it with the session's commits).  Range lengths and first rows
 *               are formed on the device from the frontier and the uploaded lengths: no host read.
 *   On a ring session vit_stream_backtrace() and vit_stream_commit() (absolute output) return VIT_EUNSUPPORTED before anything is
 *   enqueued; vit_stream_reset() also zeroes the acknowledged frontiers; vit_stream_lengths() and vit_stream_close() work as before.
 *
 * Status.  vit_stream_open_ring(): vit_stream_open()'s order (ring_rows outside [64, 2^30] is VIT_EINVAL).  vit_stream_commit_rel():
 * vit_stream_commit()'s, with NULL first VIT_EINVAL and states_stride below the bound above VIT_EINVAL.  vit_stream_tail(): NULL
 * session / states / first, no vit_stream_commit_begin(), a recording with 0 frames, states_stride below the longest possible tail
 * (min(max n_b, R) on a ring, max n_b on a linear session): VIT_EINVAL.  A refused call enqueues and writes nothing. */
size_t vit_workspace_bytes_stream_ring(const vit_plan *plan, int64_t B, int64_t ring_rows);
int vit_stream_open_ring(const vit_plan *plan, int64_t B, int64_t ring_rows, void *workspace, size_t workspace_bytes, vit_session **out);
int vit_stream_commit_ack(vit_session *s, const int64_t *frontiers /* HOST [B] */);
int vit_stream_commit_rel(vit_session *s, int32_t *states /* device [B, states_stride] */, int64_t states_stride,
                          int64_t *first /* device [B] */, int64_t *committed /* device [B] */, int64_t max_lookback, vit_stream stream);
int vit_stream_tail(vit_session *s, int32_t *states /* device [B, states_stride] */, int64_t states_stride,
                    int64_t *first /* device [B] */, float *loglik /* device [B] or NULL */, vit_stream stream);

/* Event counts of the last vit_backtrace() on this workspace (banded plans; all zero for the kernels that do not count):
 * *offset = byte offset, inside the workspace, of an int32 [B][*n_per_song] device array (valid once the back-trace has run
 * on its stream): per song [0] tiles fetched, [1] span misses (the path left the fetched columns), [2] whole-row evaluations
 * (the bound fl(M_t + c_j) could not exclude the row constant), [3] of those: odd rows of a half history rebuilt in full,
 * [4] chunks repaired by the verify pass, [5] frames rewritten by repairs.  The data-dependent part of the back-trace's cost;
 * bench.py reports it per 1000 frames. */
int vit_backtrace_counters(const vit_plan *plan, int64_t B, int64_t T, const void *workspace, size_t *offset,
                           int32_t *n_per_song);

/* Fused epilogue of Viterbi.__call__ (tonet/for_paper.py:1828-1829):
 * voiced = state < n_bins ; bins = min(state, n_bins-1).  n entries, device pointers.
 * Negative states (ragged padding) give voiced = 0, bins = -1. */
int vit_voicing_map(const int32_t *states, int64_t n, int32_t n_bins, uint8_t *voiced, int32_t *bins,
                    vit_stream stream);

/* The same map plus the bin -> note lookup the metrics consume (tonet/for_paper.py:2106-2115 est_notes_360_fn, :2207):
 * notes = note_range[bins], notes_voiced = voiced ? notes : 0.  note_range: device, [n_bins] float32.  Any of the four
 * outputs may be NULL. */
int vit_voicing_notes(const int32_t *states, int64_t n, int32_t n_bins, const float *note_range, uint8_t *voiced,
                      int32_t *bins, float *notes, float *notes_voiced, vit_stream stream);

/*
 * Device-resident hand-off from the acoustic model (replaces the host round trip at tonet/for_paper.py:2282-2302): a
 * batch of snippets [n_snippets, n_channels, n_frames] float32 (channel 0 = unvoiced) is transposed into time-major logit
 * rows appended at rows_out (device; the caller advances the pointer recording by recording):
 *   mode 0 ("shaun"):   n_channels-1 columns, channel 0 subtracted (:2296-2297);  mode 1 ("softmax"): n_channels columns.
 * Only the first n_rows <= n_snippets * n_frames rows are written (the last batch of a recording is padded, :2299-2300).
 */
int vit_snippets_append(const float *snippets, int32_t n_snippets, int32_t n_channels, int32_t n_frames, int32_t mode,
                        float *rows_out, int64_t n_rows, vit_stream stream);

/*
 * Emission builders (the step upstream of the decoder): pitch logits -> log(p + tiny)
 * observation log-probabilities in the [n_frames, n_bins+1] layout vit_decode() reads (unvoiced state last).
 *   vit_obs_shaun   : Viterbi.observation_probs_fn, tonet/for_paper.py:1733-1778 -- logits [n_frames, n_bins];
 *                     threshold_logit = log(th/(1-th)), offset = log(p/(1-p)), scale (:1697-1699, :1743-1745);
 *                     spw = single-side peak width (5).
 *   vit_obs_softmax : SoftMaxViterbi.observation_probs_fn, tonet/for_paper.py:1911-1944 -- logits
 *                     [n_frames, n_bins+1] with column 0 = unvoiced; spw = 15.
 *   vit_obs_softmax_scaled : dcnet's SoftMaxViterbi.observation_probs_fn, dcnet/softmax_viterbi.py:2530-2579 -- logits
 *                     [n_frames, n_bins]; the unvoiced logit is the constant unvoiced_logit = log(vth/(1-vth)) (:2548-2550);
 *                     every softmax probability is divided by its state prior ("scaled likelihood", values may exceed 1,
 *                     i.e. positive log-emissions); prior: device, [n_bins+1] float32 in state order (unvoiced last), or NULL
 *                     for the unscaled variant; a frame without peaks gets 1 / prior[unvoiced] (:2562-2565); spw = 5.
 * exp/log run on the GPU: probabilities agree with the reference to a few ulp, structural zeros are exact.
 */
int vit_obs_shaun(const float *logits, int64_t n_frames, int32_t n_bins, int32_t spw, double threshold_logit,
                  double offset, double scale, float *logE, vit_stream stream);
int vit_obs_softmax(const float *logits, int64_t n_frames, int32_t n_bins, int32_t spw, float *logE,
                    vit_stream stream);
int vit_obs_softmax_scaled(const float *logits, int64_t n_frames, int32_t n_bins, int32_t spw, double unvoiced_logit,
                           const float *prior, float *logE, vit_stream stream);

/*
 * The three builders with typed buffers: float32 or float16 pitch logits in, float32 or float16 log-emissions out, so that a model
 * under autocast hands its logits over as they are and the decoder (which reads float16 rows in every form) gets rows of half the
 * size without a float32 emission tensor ever existing.
 *   obs          : HOST, as for vit_decode_logits(): mode 0 = vit_obs_shaun (threshold_logit, offset, scale), 1 = vit_obs_softmax,
 *                  2 = vit_obs_softmax_scaled (threshold_logit = the unvoiced logit; obs->prior device [n_bins+1] float32 or NULL)
 *   logits       : device, [n_frames, n_bins] (mode 1: [n_frames, n_bins+1], unvoiced first) of logits_dtype (VIT_F32 / VIT_F16)
 *   logE         : device, [n_frames, n_bins+1] of emis_dtype (VIT_F32 / VIT_F16); buffers need their element's alignment only
 * Rounding contract, bit for bit: a float16 logit is widened exactly where it is loaded and all arithmetic is the float32 builder's,
 * so with logits_dtype VIT_F16 the rows are those of the float32 entry point on the widened logits; the float32 result is rounded to
 * nearest even where it is stored (float16 subnormals kept; the emission range [-87.34, ~+9] cannot overflow), so with emis_dtype
 * VIT_F16 the rows are the float32 entry point's rows after that rounding.  Float16 rows are a different decoder input: a decode of
 * them is the reference decoder's result on the rounded rows, not on the float32 rows.
 * With both dtypes VIT_F32 the call launches exactly what vit_obs_shaun / _softmax / _softmax_scaled launch; every geometry those
 * serve is served in all four combinations by the same kernel form, and one they refuse gets the status they return
 * (VIT_EUNSUPPORTED).  VIT_EINVAL: NULL obs, a bad mode or dtype, n_frames < 0, n_bins < 2, a null buffer with n_frames > 0.
 * n_frames == 0 is VIT_OK and launches nothing.  A refused call writes nothing.  One kernel launch on `stream`; no host
 * synchronisation, no allocation.
 */
int vit_obs_build(const vit_obs_params *obs, const void *logits, int logits_dtype, int64_t n_frames, void *logE, int emis_dtype,
                  vit_stream stream);
/* vit_snippets_append() for float16 snippets (device; a model under autocast): each value is widened exactly, mode 0's subtraction of
 * channel 0 is a float32 subtraction and the rows are float32 -- bit-equal to vit_snippets_append() on the widened snippets. */
int vit_snippets_append_f16(const void *snippets /* device float16 */, int32_t n_snippets, int32_t n_channels, int32_t n_frames,
                            int32_t mode, float *rows_out, int64_t n_rows, vit_stream stream);

/*
 * Activation front-end of imm's decoder (Viterbi.process_HF0_fn, imm/tf_imm.py:70-88; the decoder it feeds is
 * Viterbi.__call__, :129-135): NMF source activations -> log-emissions in the [frames, n_bins+1] layout vit_decode() /
 * vit_decode_packed() read (unvoiced state last).  Per recording the reference takes t = the smallest positive entry
 * (replaced by exp(-87) when log(t) < -87), E = log(HF0 + t), pads one unvoiced row filled with min(E) and transposes.
 *   hf0          : device, float32 [n_bins, total_frames] bins x frames with row stride ld >= total_frames (elements); B
 *                  recordings side by side along the frame axis, recording b owns columns offsets[b] .. offsets[b+1]-1
 *   offsets_dev  : DEVICE, [B+1] int64, offsets[0] = 0, strictly increasing, offsets[B] = total_frames (not checked: the call
 *                  does not read device memory on the host; whatever it holds, no access leaves the buffers)
 *   clamp_below, clamp_to : t = (min positive < clamp_below) ? clamp_to : min positive.  The caller derives both on the host --
 *                  clamp_to = float32(exp(-87)), clamp_below = the smallest float32 x with not (log(x) < -87) under the log
 *                  it wants to match -- so the clamp decision is a compare of bit patterns and never the device's log
 *   stats        : device float32 [B][4] = {min positive, min, t, _min}, written by the call (valid once it has run on its
 *                  stream; _min = the minimum of the values written to columns 0 .. n_bins-1 of that recording's rows)
 *   logE         : device [total_frames, n_bins+1] float32 or float16 (out_dtype; the float16 value is the float32 value
 *                  rounded to nearest even).  logE[offsets[b] + n][u] = log(hf0[u][n] + t_b) for u < n_bins -- a float32 add
 *                  and the device's accurate logf, a few ulp from NumPy's --, column n_bins = _min_b, bit-equal to the minimum
 *                  of the recording's other columns.  The minima are reduced on bit patterns: exact, order-independent, a
 *                  subnormal counts as positive.
 * Every statistic is per recording, as the reference calls the function once per recording.  Contract: entries finite and >= 0,
 * at least one positive entry per recording (the reference raises otherwise; here the output is then unspecified, nothing
 * faults), 1 <= n_bins <= 1023, every recording holds at least one frame.  VIT_EINVAL: a null pointer, ld < total_frames,
 * n_bins out of range, B < 1, total_frames < B, a bad out_dtype.  Four kernel launches on `stream`; no host synchronisation,
 * no allocation.
 */
int vit_obs_activations(const float *hf0, int64_t ld, int32_t n_bins, int64_t B, const int64_t *offsets_dev,
                        int64_t total_frames, float clamp_below, float clamp_to, float *stats, void *logE, int out_dtype,
                        vit_stream stream);

/* Self-test hook of the wave-wide DPP scan primitives the kernels are built on (tests/test_gpu_parity.py): vals [n_waves*64]
 * device float32; mode 0 / 1 ordered (value, index) first-maximum scan forward / reverse, 2 value-only prefix maximum, 3 the
 * prefix maximum shifted up one lane, 4 wave-wide maximum; out_v / out_i [n_waves*64]. */
int vit_debug_scan(const float *vals, int n_waves, int mode, float *out_v, int32_t *out_i, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VITERBI_HIP_H_ */
