// capi.hip -- extern "C" entry points declared in include/viterbi_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <queue>
#include <new>
#include <utility>
#include <vector>

#include "../../include/viterbi_hip.h"
#include "kernels.hpp"
#include "plan.hpp"

// Kernel-selection overrides (vit_plan_set_option).  Every combination decodes the same bits; they exist so that tests and
// timing scripts can reach each kernel form.  `timing` carries the ablation / probe mask of a -DVIT_TIMING_HOOKS build and
// is refused by a release build (those bits DO change results).
// Which of them the checkpointed decodes consult is said once, at segment_backtrace and above vit_decode_checkpointed; in short: the
// kernels are fixed by the plan's family, and bt_warm reaches the segment back-traces of the step and group families only.
struct Tuning {
    int forward_form = 0;      // banded plans: 0 by batch size | 1 one target per lane | 2 two targets per lane | 3 scan form | 6 split windows
                               //               | 4 wave form (one song per wavefront) | 5 never the wave form
    int backtrace_form = 0;    // 0 auto (sparse fetch, one stream per wavefront, where it applies) | 1 generic (lazy) kernel | 2 whole-row kernels |
                               // 4 one stream per LANE (backtrace_lane.hip; VIT_EUNSUPPORTED where it does not apply)
    int dense_songs = 0;       // songs per workgroup of the dense kernel (0 = by batch size)
    int dense_one_thread = 0;  // 1: one thread per target in the dense kernel even where two fit
    int dense_form = 0;        // 0: matrix-resident dense kernel where it applies (64 < S <= 368) | 1: always the streaming kernel
    int step_form = 0;         // step-structured kernel, four targets per lane: 0 bands split over two waves | 3 one wave
    int bt_chunks = 0;         // time-parallel back-trace: chunks per song (0 = auto)
    int bt_warm = -1;          //                            warm-up frames (-1 = default; NOT consulted by the wave family's segment back-traces)
    int win_shift = -1;        // LDS window shift of the floor kernels (-1 = from the plan)
    int wave_min_batch = 0;    // batch size from which banded plans take the wave form (0 = default)
    int wave_two = 0;          // wave kernel: 1 always the 256-register instantiation (the default but for two extra columns) | 2 the 512-register
                               // one up to 1024 songs
    int wave_uniform = 0;      // wave form: 0 = the last-state / uniform-lane variants where the plan proves them (wave.hip UV) | 1 = neither |
                               // 2 = the last-state variant only | 3 = the three-group form where the two-group one would run (it is valid there too)
    int bt_fast_rows = 0;      // sparse / half back-trace: 0 = the unexceptional rows in their own loop | 1 = every row through the general code
    int bt_block_waves = 0;    // half back-trace: waves per workgroup, 0 = 16 | 8 | 4 (to start beside the next batch's resident forward waves)
    int floor_live_window = 0; // split floor kernel: 0 = the full waves evaluate the window entries the plan proves live | 1 = always the whole window
    int wave_history = 0;      // wave form: 0 / 1 every delta row | 2 the rows of even frames only (VIT_EUNSUPPORTED where the plan does not allow it)
    int f64_units_per_cu = 0;  // vit_decode_f64_packed_checkpointed: units per CU and launch, 1 .. 4 (0 = the instantiation's own, f64_pckpt_units_per_cu)
    int timing = 0;
};
// The bt_chunks / bt_warm overrides applied to a default (test hooks: they force the chunking / warm-up so that the verify-and-repair
// pass is exercised).  cap: the most chunks per song the kernel that runs takes (kLaneMaxChunks for the lane form).
inline int tuned_chunks(const Tuning& tn, int chunks, int cap = vit::kBtMaxChunks) { return tn.bt_chunks >= 1 && tn.bt_chunks <= cap ? tn.bt_chunks : chunks; }
inline int tuned_warm(const Tuning& tn, int warm) { return tn.bt_warm >= 0 ? tn.bt_warm : warm; }

// Forward kernel families.  The values are public: vit_forward_family returns them and FwdStamp::family stores them.
enum Family : int {
    kFamNone = 0,              // (the answer of the *_family predicates for a plan an entry point does not serve)
    kFamStep = 1,              // dense / step kernels: any matrix, or the step-structured one
    kFamGroup = 2,             // banded, one song per workgroup
    kFamWave = 3,              // banded, one song per wavefront
};
// the forward launch of a packed / checkpointed decode: the workgroup kernels take a variant; the wave form ignores it and reads its
// mode from the arguments (wave_hist_of, wave_common.hpp: which of ckpt_base / unit_song, offsets, ckpt_every, t_begin / t_end, hist_half mean which mode)
inline hipError_t launch_family(int family, vit::WgVariant v, const vit::FwdArgs& a, bool f16, hipStream_t st) {
    if (family == kFamWave) return vit::launch_wave(a, f16, st);
    return family == kFamGroup ? vit::launch_banded_variant(a, v, f16, st) : vit::launch_step_variant(a, v, f16, st);
}
// ... and the occupancy query of a workgroup family's variant
inline hipError_t family_resident(int family, vit::WgVariant v, const vit::FwdArgs& a, bool f16, int* per_cu) {
    return family == kFamGroup ? vit::banded_variant_resident(a, v, f16, per_cu) : vit::step_variant_resident(a, v, f16, per_cu);
}
// The packed forward kernels whose launches are sized by their occupancy (vit_plan::resident): the Packed and the PackedCkpt variant of
// the plan's workgroup family, the Packed variant of the float64 kernel.  kResNone: nothing to ask (the wave family).
enum ResidentKey : int { kResNone = -1, kResPacked = 0, kResPackedCkpt = 1, kResF64Packed = 2, kResF64PackedCkpt = 3, kResKeys = 4 };

// Where a state's column, the frame maximum and the copies of the extra columns sit in a history row: hist_layout(plan, family).
struct HistLayout {
    int SD = 0;                // row stride, floats
    int col0 = 0, mcol = 0;    // state i in column col0 + i, the frame maximum in column mcol
    int xcol0 = -1;            // >= 0: column xcol0 + k holds a copy of delta of extra column k
    int have_fmax = 0;         // column mcol of every history row holds a bound on max_i delta_t[i]
};

// What the last vit_forward left in a workspace: vit_backtrace reads the layout from here, not from its arguments.
struct FwdStamp {
    const void* ws = nullptr;
    int64_t B = 0, T = 0;
    int family = 0;            // Family
    HistLayout lay;            // the history rows the forward kernel wrote
    int aux_frames = 1;        // frames whose scalars a row carries (BtArgs::aux_frames)
    int half = 0;              // wave form, even rows only: the back-trace re-reads the emissions
    const void* logE = nullptr;
    int e_f16 = 0;
};

struct vit_plan {
    int S = 0;
    vit::BandedPlan bp;
    vit::ImageLayout L;
    std::vector<uint8_t> host_image;
    const uint8_t* dev_image = nullptr;
    int wave_u5 = 0;           // the wave kernel's uniform-lane form applies (wave.hip U5)
    int n_cus = 256;           // compute units of the device the image was uploaded to (vit_plan_upload): kernel-selection thresholds scale with it
    Tuning tune;
    mutable std::mutex mu;
    mutable std::vector<FwdStamp> stamps;   // most recent first, at most kMaxStamps
    // vit_decode_packed: pinned host staging of the slot / chunk tables, and the event of the copy that last read it
    mutable void* pk_host = nullptr;
    mutable size_t pk_host_bytes = 0;
    mutable hipEvent_t pk_event = nullptr;
    // workgroups per CU of the packed forward kernels, by kernel (ResidentKey) and emission type (fp32 / fp16); 0 = not asked yet
    // (resident_per_cu)
    mutable int resident[kResKeys][2] = {};
    ~vit_plan() {
        if (pk_event) (void)hipEventDestroy(pk_event);
        if (pk_host) (void)hipHostFree(pk_host);
    }
};

namespace {

thread_local int g_last_hip_error = 0;

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline int hist_stride(int S) { return (S + 5) / 4 * 4; }   // rows 16-byte aligned, at least two pad columns (frame max, scratch)
// The history row layout of one forward family: the ONE place that knows it.  Workgroup kernels (step, group): state i in column i,
// the frame maximum (banded kernels only) in pad column S.  Wave form: rows in slot order, 64 * npl floats, the states at the end,
// the frame maximum in column 0 and the extra columns' copies behind it.
HistLayout hist_layout(const vit_plan* p, int family) {
    HistLayout h;
    if (family == kFamWave) {
        h.SD = vit::wave_hist_stride(p->bp.wave_npl);
        h.col0 = h.SD - p->S;
        h.mcol = 0;
        h.xcol0 = 1;
        h.have_fmax = 1;
    } else {
        h.SD = hist_stride(p->S);
        h.col0 = 0;
        h.mcol = p->S;
        h.xcol0 = -1;
        h.have_fmax = family == kFamGroup ? 1 : 0;
    }
    return h;
}
void hist_layout_apply(const HistLayout& h, vit::BtArgs& b) {     // (aux_frames is the caller's: it depends on what was stored, not on the family)
    b.SD = h.SD;
    b.col0 = h.col0;
    b.mcol = h.mcol;
    b.xcol0 = h.xcol0;
    b.have_fmax = h.have_fmax;
}
// widest history row any forward kernel of this plan writes
inline int hist_stride_ws(const vit_plan* p) {
    const int sd = hist_layout(p, kFamStep).SD;
    const int sw = (p->bp.ok && p->bp.wave_ok) ? hist_layout(p, kFamWave).SD : 0;
    return sd > sw ? sd : sw;
}
constexpr size_t kMaxStamps = 64;    // workspaces with a forward pass on record per plan (include/viterbi_hip.h, vit_forward)
// From two workgroups per CU + 1 songs on, one song per wavefront beats one song per workgroup (256 CUs: two workgroups per CU hold 512
// songs, B = 512: 18.8 vs 14.2 ms forward; the 513th starts a second round, B = 576: 18.8 vs 19.8 ms, B = 1024: 20.0 vs 25-27 ms;
// DESIGN.md 6).
inline int64_t wave_min_batch(const vit_plan* p) { return 2 * (int64_t)p->n_cus + 1; }

void stamp_erase(const vit_plan* p, const void* ws) {
    std::lock_guard<std::mutex> g(p->mu);
    for (size_t k = 0; k < p->stamps.size(); ++k)
        if (p->stamps[k].ws == ws) { p->stamps.erase(p->stamps.begin() + k); break; }
}
void stamp_put(const vit_plan* p, const FwdStamp& st) {
    stamp_erase(p, st.ws);
    std::lock_guard<std::mutex> g(p->mu);
    p->stamps.insert(p->stamps.begin(), st);
    if (p->stamps.size() > kMaxStamps) p->stamps.pop_back();
}
bool stamp_get(const vit_plan* p, const void* ws, FwdStamp* out) {
    std::lock_guard<std::mutex> g(p->mu);
    for (const FwdStamp& st : p->stamps)
        if (st.ws == ws) { *out = st; return true; }
    return false;
}

int hip_fail(hipError_t e) {
    g_last_hip_error = (int)e;
    return VIT_EHIP;
}
inline int hip_status(hipError_t e) { return e == hipSuccess ? VIT_OK : hip_fail(e); }
// a HIP call or launch in a function that returns a status: on failure record the error (vit_last_hip_error) and return VIT_EHIP
#define VIT_TRY(expr)                                               \
    do {                                                            \
        const hipError_t vit_try_e_ = (expr);                       \
        if (vit_try_e_ != hipSuccess) return hip_fail(vit_try_e_);  \
    } while (0)

struct WsLayout {
    size_t off_hist, off_fmax, off_cnt, off_mask, off_last, off_entry, bytes;
};

// history floats per song: `rows` rows of `stride` floats
WsLayout ws_layout_hist(int64_t B, size_t rows, size_t stride) {
    WsLayout w;
    w.off_hist = 0;
    w.off_fmax = align256((size_t)B * rows * stride * sizeof(float));
    w.off_cnt = w.off_fmax + align256((size_t)B * 64 * sizeof(float));    // (off_fmax: timing-experiment scratch of the forward kernels)
    w.off_mask = w.off_cnt + align256((size_t)B * vit::kBtCounters * sizeof(int32_t));   // the back-trace's event counters, then its chunk flags:
    w.off_last = w.off_mask + align256((size_t)B * vit::kLaneMaskWords * sizeof(uint32_t));   // one memset covers both
    w.off_entry = w.off_last + align256((size_t)B * sizeof(int32_t));
    w.bytes = w.off_entry + align256((size_t)B * vit::kLaneMaxChunks * sizeof(int32_t));
    return w;
}
// the layout that covers every forward kernel of the plan (vit_workspace_bytes)
WsLayout ws_layout(const vit_plan* p, int64_t B, int64_t T) { return ws_layout_hist(B, (size_t)T, (size_t)hist_stride_ws(p)); }

// Does the wave form of this plan store a half history (even frames only)?  The back-trace kernel for it
// (backtrace_half.hip) is asked with the layout the forward kernel would write.
bool wave_half_applies(const vit_plan* p, int64_t T) {
    if (!(p->bp.ok && p->bp.wave_ok) || p->tune.wave_history != 2 || T < 2) return false;
    vit::BtArgs b{};                 // a probe: only what half_backtrace_applies reads, NOT bt_args_from_plan
    hist_layout_apply(hist_layout(p, kFamWave), b);
    b.S = p->S;
    b.SP = p->L.SP;
    b.W = p->bp.W;
    b.banded = 1;
    b.n_extras = p->bp.n_extras;
    b.n_dense = p->bp.n_dense;
    b.lo_affine = p->bp.lo_affine ? 1 : 0;
    b.lo_off = p->bp.lo_off;
    return vit::half_backtrace_applies(b);
}
// the workspace of one forward family
WsLayout ws_layout_family(const vit_plan* p, int family, int64_t B, int64_t T) {
    const bool half = family == kFamWave && wave_half_applies(p, T);
    return ws_layout_hist(B, (size_t)(half ? (T + 1) / 2 : T), (size_t)hist_layout(p, family).SD);
}

int check_common(const vit_plan* plan, int64_t B, int64_t T, const void* ws) {
    if (!plan || !ws) return VIT_EINVAL;
    if (B < 0 || T < 1 || T > (int64_t)1 << 30 || B > (int64_t)1 << 30) return VIT_EINVAL;
    if (!plan->dev_image) return VIT_ENOTUPLOADED;
    if (((uintptr_t)ws & 255) != 0) return VIT_EINVAL;
    return VIT_OK;
}
// the segment lengths the checkpointed decodes take
inline bool ck_segment_ok(int64_t K) { return K >= 64 && K <= (int64_t)1 << 24; }

}  // namespace

extern "C" {

int vit_abi_version(void) { return VIT_ABI_VERSION; }

const char* vit_status_string(int status) {
    switch (status) {
        case VIT_OK: return "ok";
        case VIT_EINVAL: return "invalid argument";
        case VIT_ENOMEM: return "out of host memory";
        case VIT_EHIP: return "HIP runtime error";
        case VIT_EWORKSPACE: return "workspace too small";
        case VIT_EUNSUPPORTED: return "unsupported shape or algorithm";
        case VIT_ENOTUPLOADED: return "plan image not uploaded";
        case VIT_ENOFORWARD: return "no forward pass on record for this workspace";
        default: return "unknown status";
    }
}

int vit_last_hip_error(void) { return g_last_hip_error; }

int vit_plan_create(const float* logA_T, const float* log_pi, int64_t S, vit_plan** out) {
    if (!logA_T || !log_pi || !out) return VIT_EINVAL;
    if (S < 1 || S > 1024) return VIT_EINVAL;
    vit_plan* p = new (std::nothrow) vit_plan();
    if (!p) return VIT_ENOMEM;
    try {
        p->S = (int)S;
        p->bp = vit::analyze_banded(logA_T, (int)S);
        if (!p->bp.ok) vit::analyze_step(logA_T, (int)S, p->bp);
        p->L = vit::make_layout((int)S, p->bp);
        p->host_image.resize(p->L.bytes);
        vit::fill_image(logA_T, log_pi, p->bp, p->L, p->host_image.data());
        // wave form, uniform-lane variant: six states per lane, ONE extra column = the last state, and for every lane the row constant
        // and the extra-column weight of its slots 0..4 agree bit for bit (idle slots count as -inf)
        if (p->bp.ok && p->bp.wave_ok && p->bp.n_extras == 1 && p->bp.extras[0] == (int)S - 1) p->wave_u5 = 1;     // (the extra column is the last state)
        if (p->wave_u5 == 1 && p->bp.wave_npl == 6) {
            const float* xa = reinterpret_cast<const float*>(p->host_image.data() + p->L.off_extraA);
            const int o = 384 - (int)S;
            auto uniform = [&](const int k0, const int k1) {       // slots k0 .. k1-1 of every lane agree in row constant and extra-column weight
                for (int l = 0; l < 64; ++l) {
                    uint32_t c_ref = 0, x_ref = 0;
                    for (int k = k0; k < k1; ++k) {
                        const int j = 6 * l + k - o;
                        const float cv = j >= 0 ? p->bp.rowc[j] : -INFINITY, xv = j >= 0 ? xa[j] : -INFINITY;
                        uint32_t cb, xb;
                        std::memcpy(&cb, &cv, 4);
                        std::memcpy(&xb, &xv, 4);
                        if (k == k0) { c_ref = cb; x_ref = xb; }
                        if (cb != c_ref || xb != x_ref) return false;
                    }
                }
                return true;
            };
            if (uniform(0, 5)) p->wave_u5 = 2;                      // S = 361: the idle slots end at a lane boundary + 5
            else if (uniform(0, 3) && uniform(3, 5)) p->wave_u5 = 3;   // S = 321: they end in the middle of a lane
        }
    } catch (const std::bad_alloc&) {
        delete p;
        return VIT_ENOMEM;
    }
    *out = p;
    return VIT_OK;
}

void vit_plan_destroy(vit_plan* plan) { delete plan; }

int vit_plan_query(const vit_plan* plan, vit_plan_info* info) {
    if (!plan || !info) return VIT_EINVAL;
    std::memset(info, 0, sizeof(*info));
    info->S = plan->S;
    info->banded_ok = plan->bp.ok ? 1 : 0;
    info->n_consts = plan->bp.ok ? 1 : 0;
    info->n_extras = plan->bp.n_extras;
    info->max_window = plan->bp.max_window;
    info->group_window = plan->bp.W;
    info->reserved[0] = plan->bp.n_dense;
    info->reserved[1] = plan->bp.ok && plan->bp.floor_ok ? 1 : 0;
    info->reserved[2] = (plan->bp.ok && plan->bp.lo_affine ? 1 : 0) | (plan->bp.ok && plan->bp.pair_ok ? 2 : 0) |
                        (plan->bp.step_ok && vit::step_kernel_instantiated(plan->S, plan->bp.step_bw, plan->bp.step_kb) ? 4 : 0) |
                        (plan->bp.ok && plan->bp.wave_ok ? 8 : 0);
    info->consts[0] = plan->bp.c0;
    for (int k = 0; k < vit::kMaxExtras; ++k) info->extras[k] = k < plan->bp.n_extras ? plan->bp.extras[k] : -1;
    return VIT_OK;
}

size_t vit_plan_image_bytes(const vit_plan* plan) { return plan ? plan->L.bytes : 0; }

int vit_plan_upload(vit_plan* plan, void* device_image, size_t bytes, vit_stream stream) {
    if (!plan || !device_image) return VIT_EINVAL;
    if (bytes < plan->L.bytes || ((uintptr_t)device_image & 255) != 0) return VIT_EINVAL;
    VIT_TRY(hipMemcpyAsync(device_image, plan->host_image.data(), plan->L.bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    plan->dev_image = static_cast<const uint8_t*>(device_image);
    int dev = 0, cus = 0;      // the thresholds below are "how many workgroups / waves fit the chip at once": from the device, not from "256"
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        plan->n_cus = cus;
    return VIT_OK;
}

size_t vit_workspace_bytes(const vit_plan* plan, int64_t B, int64_t T) {
    if (!plan || B < 0 || T < 1) return 0;
    return ws_layout(plan, B, T).bytes;
}

// options of vit_plan_set_option
static int* tuning_field(Tuning& t, const char* key) {
    struct { const char* k; int Tuning::*f; } const tab[] = {
        {"forward_form", &Tuning::forward_form}, {"backtrace_form", &Tuning::backtrace_form},
        {"dense_songs", &Tuning::dense_songs}, {"dense_one_thread", &Tuning::dense_one_thread}, {"dense_form", &Tuning::dense_form},
        {"step_form", &Tuning::step_form}, {"bt_chunks", &Tuning::bt_chunks}, {"bt_warm", &Tuning::bt_warm},
        {"win_shift", &Tuning::win_shift}, {"wave_min_batch", &Tuning::wave_min_batch}, {"wave_two", &Tuning::wave_two},
        {"bt_fast_rows", &Tuning::bt_fast_rows}, {"bt_block_waves", &Tuning::bt_block_waves}, {"wave_history", &Tuning::wave_history}, {"wave_uniform", &Tuning::wave_uniform},
        {"floor_live_window", &Tuning::floor_live_window}, {"f64_units_per_cu", &Tuning::f64_units_per_cu}, {"timing", &Tuning::timing},
    };
    for (const auto& e : tab)
        if (std::strcmp(e.k, key) == 0) return &(t.*(e.f));
    return nullptr;
}

int vit_plan_set_option(vit_plan* plan, const char* key, int64_t value) {
    if (!plan || !key) return VIT_EINVAL;
    if (std::strcmp(key, "reset") == 0) { plan->tune = Tuning(); return VIT_OK; }
    int* f = tuning_field(plan->tune, key);
    if (!f || value < -1 || value > (int64_t)1 << 30) return VIT_EINVAL;
#ifndef VIT_TIMING_HOOKS
    if (f == &plan->tune.timing && value != 0) return VIT_EUNSUPPORTED;   // result-breaking ablations: timing builds only
#endif
    *f = (int)value;
    return VIT_OK;
}

// forward kernel family (Family) for (plan, algo, batch); < 0 = status
static int resolve_family(const vit_plan* plan, int algo, int64_t B) {
    const int nwt = vit::banded_waves_for(plan->S);
    const bool group_ok = plan->bp.ok && (vit::scan_form_instantiated(plan->bp.W, nwt) ||
                                          (plan->bp.floor_ok && plan->S < nwt * 64 && vit::floor_form_instantiated(plan->bp.W, nwt)));
    const bool wave_ok = plan->bp.ok && plan->bp.wave_ok;
    const int ff = plan->tune.forward_form;
    const int64_t wmin = plan->tune.wave_min_batch > 0 ? plan->tune.wave_min_batch : wave_min_batch(plan);
    if (algo == VIT_ALGO_DENSE) return kFamStep;
    if (algo == VIT_ALGO_WAVE) return wave_ok ? kFamWave : VIT_EUNSUPPORTED;
    if (algo == VIT_ALGO_GROUP) return group_ok ? kFamGroup : VIT_EUNSUPPORTED;
    if (algo != VIT_ALGO_AUTO && algo != VIT_ALGO_BANDED) return VIT_EINVAL;
    const bool want_wave = wave_ok && ff != 5 && (ff == 4 || (ff == 0 && B >= wmin) || !group_ok);
    if (want_wave) return kFamWave;
    if (group_ok) return kFamGroup;
    return algo == VIT_ALGO_AUTO ? kFamStep : VIT_EUNSUPPORTED;
}

// the fields of FwdArgs that depend on the plan and its options only
static void fwd_args_from_plan(const vit_plan* plan, vit::FwdArgs& a) {
    const Tuning& tn = plan->tune;
    a.image = plan->dev_image;
    a.S = plan->S;
    a.SP = plan->L.SP;
    a.S4 = plan->L.S4;
    a.SD = hist_stride(plan->S);
    a.W = plan->bp.W;
    a.n_extras = plan->bp.ok ? plan->bp.n_extras : 0;
    a.n_dense = plan->bp.ok ? plan->bp.n_dense : 0;
    for (int k = 0; k < vit::kMaxExtras; ++k) a.extras[k] = plan->bp.extras[k];
    a.c0 = plan->bp.c0;
    a.debug = tn.timing;          // 0 unless built with -DVIT_TIMING_HOOKS (vit_plan_set_option refuses it otherwise)
    a.fwd_form = (tn.forward_form >= 1 && tn.forward_form <= 3) || tn.forward_form == 6 ? tn.forward_form : 0;
    a.dense_kt1 = tn.dense_one_thread;
    a.dense_form = tn.dense_form;
    a.step_form = tn.step_form;
    a.off_logpi = plan->L.off_logpi;
    a.off_A4 = plan->L.off_A4;
    a.off_lo = plan->L.off_lo;
    a.off_kind = plan->L.off_kind;
    a.off_tabA = plan->L.off_tabA;
    a.off_extraA = plan->L.off_extraA;
    a.off_denseA = plan->L.off_denseA;
    a.off_rowc = plan->L.off_rowc;
    a.off_lo2 = plan->L.off_lo2;
    a.off_tabP = plan->L.off_tabP;
    a.pair_ok = plan->bp.ok && plan->bp.pair_ok ? 1 : 0;
    a.floor_ok = plan->bp.ok && plan->bp.floor_ok ? 1 : 0;
    a.step_ok = plan->bp.step_ok ? 1 : 0;
    a.step_bw = plan->bp.step_bw;
    a.step_kb = plan->bp.step_kb;
    a.step_cn = plan->bp.step_cn;
    a.off_stepC = plan->L.off_stepC;
    a.off_Arow = plan->L.off_Arow;
    a.off_tabV = plan->L.off_tabV;
    a.wave_ok = plan->bp.ok && plan->bp.wave_ok ? 1 : 0;
    a.wave_npl = plan->bp.wave_npl;
    a.wave_dk = plan->bp.wave_dk;
    a.wave_u5 = tn.wave_uniform == 1 ? 0 : (tn.wave_uniform == 2 ? (plan->wave_u5 >= 1 ? 1 : 0) : (tn.wave_uniform == 3 && plan->wave_u5 == 2 ? 3 : plan->wave_u5));
    a.wave_flags = ((tn.wave_two & 3) == 1 ? 1 : ((tn.wave_two & 3) == 2 ? 2 : 0)) | (tn.wave_two & 4);   // (bit 2: a row carries its own scalars only -- A/B)
    a.win_shift = (plan->bp.ok && plan->bp.lo_affine) ? (plan->bp.lo_off & 3) : 0;
    a.win_shift2 = (plan->bp.ok && plan->bp.pair_ok && plan->bp.lo2_affine) ? (plan->bp.lo2_off & 3) : 0;
    if (tn.win_shift >= 0) a.win_shift = a.win_shift2 = tn.win_shift & 3;   // every value is functionally correct
    a.floor_live = tn.floor_live_window == 0 ? vit::floor_live_width(plan->bp, vit::kSplitFullRows) : plan->bp.W;
}

size_t vit_workspace_bytes_for(const vit_plan* plan, int64_t B, int64_t T, int algo) {
    if (!plan || B < 0 || T < 1) return 0;
    const int family = resolve_family(plan, algo, B);
    if (family < 0) return 0;
    return ws_layout_family(plan, family, B, T).bytes;
}

static void bt_args_from_plan(const vit_plan* plan, vit::BtArgs& b);

// vit_forward; then_backtrace: the call is vit_decode's, which refuses BEFORE anything is enqueued what its back-trace would refuse
// behind the forward pass ("backtrace_form" 4 where the lane kernel does not apply) -- a refused decode writes nothing.  The check sits
// behind every other one, so that a call with two defects is answered as it always was.
static int forward_impl(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T,
                        const int64_t* lengths, void* workspace, size_t workspace_bytes, float* loglik, int algo,
                        vit_stream stream, bool then_backtrace) {
    int rc = check_common(plan, B, T, workspace);
    if (rc != VIT_OK) return rc;
    if (!logE) return VIT_EINVAL;
    if (emis_dtype != VIT_F32 && emis_dtype != VIT_F16) return VIT_EINVAL;
    const int family = resolve_family(plan, algo, B);
    if (family < 0) return family;
    const Tuning& tn = plan->tune;
    const bool half = family == kFamWave && wave_half_applies(plan, T);
    if (family == kFamWave && tn.wave_history == 2 && !half && T >= 2) return VIT_EUNSUPPORTED;
    const WsLayout w = ws_layout_family(plan, family, B, T);
    if (workspace_bytes < w.bytes) return VIT_EWORKSPACE;
    if (B == 0) return VIT_OK;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    if (then_backtrace && tn.backtrace_form == 4 && !half) {      // backtrace_impl's own test, on the layout this pass would record
        vit::BtArgs b{};
        bt_args_from_plan(plan, b);
        hist_layout_apply(hist_layout(plan, family), b);
        b.mask = reinterpret_cast<uint32_t*>(ws + w.off_mask);
        if (!vit::lane_backtrace_applies(b)) return VIT_EUNSUPPORTED;
    }
    stamp_erase(plan, workspace);      // whatever this workspace held is gone once the kernel below starts; re-stamped on success

    vit::FwdArgs a{};
    fwd_args_from_plan(plan, a);
    a.logE = logE;
    a.lengths = lengths;
    a.hist = reinterpret_cast<float*>(ws + w.off_hist);
    a.fmax = reinterpret_cast<float*>(ws + w.off_fmax);
    a.last_state = reinterpret_cast<int32_t*>(ws + w.off_last);
    a.loglik = loglik;
    a.B = B;
    a.T = (int)T;
    a.hist_half = half ? 1 : 0;
    a.hist_rows = half ? (T + 1) / 2 : T;
    a.t_begin = 0;
    a.t_end = (int)T;

    FwdStamp st;
    st.ws = workspace;
    st.B = B;
    st.T = T;
    st.family = family;
    st.lay = hist_layout(plan, family);
    st.logE = logE;
    st.e_f16 = emis_dtype == VIT_F16 ? 1 : 0;
    hipError_t e;
    if (family == kFamWave) {
        st.aux_frames = half || (a.wave_flags & 4) ? 1 : vit::wave_aux_frames(plan->bp.wave_npl, plan->S, a.n_extras);
        st.half = half ? 1 : 0;
        e = vit::launch_wave(a, emis_dtype == VIT_F16, (hipStream_t)stream);
    } else if (family == kFamGroup) {
        e = vit::launch_banded(a, emis_dtype == VIT_F16, (hipStream_t)stream);
    } else if (algo == VIT_ALGO_AUTO && a.step_ok && vit::step_kernel_instantiated(a.S, a.step_bw, a.step_kb)) {
        // dense matrix with step structure (Durrieu): VIT_ALGO_DENSE still means the plain dense kernel
        e = vit::launch_step(a, emis_dtype == VIT_F16, (hipStream_t)stream);
    } else {
        // songs per workgroup share the streamed matrix (measured at S = 361, B = 1024: 1 -> 57, 2 -> 64, 4 -> 48 Mframes/s)
        const int ns = tn.dense_songs > 0 ? tn.dense_songs : (B >= 512 ? 2 : 1);
        e = vit::launch_dense(a, ns, emis_dtype == VIT_F16, (hipStream_t)stream);
    }
    VIT_TRY(e);
    stamp_put(plan, st);
    return VIT_OK;
}

int vit_forward(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T,
                const int64_t* lengths, void* workspace, size_t workspace_bytes, float* loglik, int algo,
                vit_stream stream) {
    return forward_impl(plan, logE, emis_dtype, B, T, lengths, workspace, workspace_bytes, loglik, algo, stream, false);
}

// the fields of BtArgs that depend on the plan and its options only
static void bt_args_from_plan(const vit_plan* plan, vit::BtArgs& b) {
    b.image = plan->dev_image;
    b.S = plan->S;
    b.SP = plan->L.SP;
    b.W = plan->bp.ok ? plan->bp.W : 0;
    b.banded = plan->bp.ok ? 1 : 0;
    b.n_extras = plan->bp.ok ? plan->bp.n_extras : 0;
    b.n_dense = plan->bp.ok ? plan->bp.n_dense : 0;
    for (int k = 0; k < vit::kMaxExtras; ++k) b.extras[k] = plan->bp.extras[k];
    b.c0 = plan->bp.c0;
    b.bt_form = plan->tune.backtrace_form;
    b.no_fast_rows = plan->tune.bt_fast_rows == 1 ? 1 : 0;
    b.block_waves = plan->tune.bt_block_waves;
    b.lo_affine = plan->bp.lo_affine ? 1 : 0;
    b.lo_off = plan->bp.lo_off;
    for (int d = 0; d < vit::kMaxDenseRows; ++d) b.dense_rows[d] = d < plan->bp.n_dense ? plan->bp.dense_rows[d] : -1;
    b.off_lo = plan->L.off_lo;
    b.off_kind = plan->L.off_kind;
    b.off_tabA = plan->L.off_tabA;
    b.off_extraA = plan->L.off_extraA;
    b.off_tabX = plan->L.off_tabX;
    b.off_stepC = plan->L.off_stepC;
    b.step_ok = 0;
    if (plan->bp.step_ok) {   // band = dist / bw as a multiply-shift, verified here for every distance that can occur
        const int bw = plan->bp.step_bw;
        const int mult = (65536 + bw - 1) / bw;
        bool exact = true;
        for (int d = 0; d < 1024 && exact; ++d) exact = ((unsigned)(d * mult) >> 16) == (unsigned)(d / bw);
        if (exact) { b.step_ok = 1; b.step_kb = plan->bp.step_kb; b.step_mult = mult; b.step_cn = plan->bp.step_cn; }
    }
    b.off_denseA = plan->L.off_denseA;
    b.off_Arow = plan->L.off_Arow;
    b.off_rowc = plan->L.off_rowc;
}

int vit_forward_family(const vit_plan* plan, int64_t B, int algo) {
    if (!plan || B < 0) return VIT_EINVAL;
    return resolve_family(plan, algo, B);
}

static int backtrace_impl(const vit_plan* plan, const void* logE, int emis_dtype, bool check_e, int64_t B, int64_t T, const int64_t* lengths,
                          void* workspace, size_t workspace_bytes, int32_t* states, vit_stream stream);

int vit_backtrace(const vit_plan* plan, int64_t B, int64_t T, const int64_t* lengths, void* workspace,
                  size_t workspace_bytes, int32_t* states, int algo, vit_stream stream) {
    (void)algo;   // kept for ABI compatibility: the layout comes from what vit_forward recorded for this workspace
    return backtrace_impl(plan, nullptr, 0, false, B, T, lengths, workspace, workspace_bytes, states, stream);
}

int vit_backtrace_checked(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T, const int64_t* lengths,
                          void* workspace, size_t workspace_bytes, int32_t* states, int algo, vit_stream stream) {
    (void)algo;
    if (!logE || (emis_dtype != VIT_F32 && emis_dtype != VIT_F16)) return VIT_EINVAL;
    return backtrace_impl(plan, logE, emis_dtype, true, B, T, lengths, workspace, workspace_bytes, states, stream);
}

static int backtrace_impl(const vit_plan* plan, const void* logE, int emis_dtype, bool check_e, int64_t B, int64_t T, const int64_t* lengths,
                          void* workspace, size_t workspace_bytes, int32_t* states, vit_stream stream) {
    int rc = check_common(plan, B, T, workspace);
    if (rc != VIT_OK) return rc;
    if (!states) return VIT_EINVAL;
    if (B == 0) return VIT_OK;
    FwdStamp st;
    if (!stamp_get(plan, workspace, &st) || st.B != B || st.T != T) return VIT_ENOFORWARD;   // no matching vit_forward
    // the emission tensor must be the one the forward pass decoded (a half history reads it again through the recorded pointer)
    if (check_e && (st.logE != logE || st.e_f16 != (emis_dtype == VIT_F16 ? 1 : 0))) return VIT_EINVAL;
    const Tuning& tn = plan->tune;
    const WsLayout w = ws_layout_hist(B, (size_t)(st.half ? (T + 1) / 2 : T), (size_t)st.lay.SD);
    if (workspace_bytes < w.bytes) return VIT_EWORKSPACE;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    vit::BtArgs b{};
    b.hist = reinterpret_cast<const float*>(ws + w.off_hist);
    b.last_state = reinterpret_cast<const int32_t*>(ws + w.off_last);
    b.lengths = lengths;
    b.states = states;
    b.entry = reinterpret_cast<int32_t*>(ws + w.off_entry);
    b.B = B;
    b.T = (int)T;
    bt_args_from_plan(plan, b);
    hist_layout_apply(st.lay, b);
    b.aux_frames = st.aux_frames;
    b.states_stride = T;
    if (st.family == kFamWave && !(b.banded && b.n_dense == 0)) return VIT_EINVAL;   // (cannot happen: wave_ok implies both)
    b.hist_rows = T;
    b.counters = reinterpret_cast<int32_t*>(ws + w.off_cnt);          // event counts of this back-trace, chunk flags of the lane form
    b.mask = reinterpret_cast<uint32_t*>(ws + w.off_mask);
    VIT_TRY(hipMemsetAsync(ws + w.off_cnt, 0, w.off_last - w.off_cnt, (hipStream_t)stream));
    if (st.half) {
        b.hist_half = 1;
        b.hist_rows = (T + 1) / 2;
        b.mcol_odd = 1 + b.n_extras;
        b.xcol0_odd = 2 + b.n_extras;
        b.logE = st.logE;
        b.e_f16 = st.e_f16;
    }
    if (st.half) {
        b.chunks = tuned_chunks(tn, vit::sparse_backtrace_chunks(B, (int)T, plan->n_cus));
        b.warm = tuned_warm(tn, vit::kBtWarmSparse);
        return hip_status(vit::launch_backtrace_half(b, (hipStream_t)stream));
    }
    if (b.bt_form == 4) {                                             // one (song, chunk) stream per lane
        if (!vit::lane_backtrace_applies(b)) return VIT_EUNSUPPORTED;
        b.warm = tuned_warm(tn, vit::kBtWarmSparse);
        b.chunks = tuned_chunks(tn, vit::lane_backtrace_chunks(B, (int)T, plan->n_cus, b.warm), vit::kLaneMaxChunks);   // (one stream per lane: its own cap)
        return hip_status(vit::launch_backtrace_lane(b, (hipStream_t)stream));
    }
    const bool sparse = b.bt_form == 0 && vit::sparse_backtrace_applies(b);
    b.chunks = tuned_chunks(tn, sparse ? vit::sparse_backtrace_chunks(B, (int)T, plan->n_cus) : vit::backtrace_chunks(B, (int)T));
    b.warm = tuned_warm(tn, sparse ? vit::kBtWarmSparse : vit::kBtWarm);
    return hip_status(vit::launch_backtrace(b, (hipStream_t)stream));
}

int vit_backtrace_counters(const vit_plan* plan, int64_t B, int64_t T, const void* workspace, size_t* offset, int32_t* n_per_song) {
    if (!plan || !workspace || !offset || !n_per_song) return VIT_EINVAL;
    FwdStamp st;
    if (!stamp_get(plan, workspace, &st) || st.B != B || st.T != T) return VIT_ENOFORWARD;
    *offset = ws_layout_hist(B, (size_t)(st.half ? (T + 1) / 2 : T), (size_t)st.lay.SD).off_cnt;
    *n_per_song = vit::kBtCounters;
    return VIT_OK;
}

int vit_decode(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T,
               const int64_t* lengths, void* workspace, size_t workspace_bytes, int32_t* states, float* loglik,
               int algo, vit_stream stream) {
    if (!states) return VIT_EINVAL;
    int rc = forward_impl(plan, logE, emis_dtype, B, T, lengths, workspace, workspace_bytes, loglik, algo, stream, true);
    if (rc != VIT_OK) return rc;
    return vit_backtrace(plan, B, T, lengths, workspace, workspace_bytes, states, algo, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Float64-accumulating decode (f64.hip): the reference's float64 variant, dcnet/tf_viterbi_decoding.py:209-263.  The forward and the
// back-trace kernel of that file, nothing else: of the plan's options only bt_chunks and bt_warm are consulted.  No forward pass is
// put on record and the record an earlier vit_forward left for the workspace is dropped (vit_backtrace knows nothing of this history).
namespace {

inline bool f64_applies(const vit_plan* p) {
    return vit::f64_decode_applies(p->S, p->bp.W, p->bp.ok, p->bp.ok && p->bp.floor_ok, p->bp.ok ? p->bp.n_dense : 0);
}
struct F64Layout {
    size_t off_hist, off_last, off_entry, bytes;
};
F64Layout f64_layout(const vit_plan* p, int64_t B, int64_t T) {
    F64Layout w;
    w.off_hist = 0;
    w.off_last = align256((size_t)B * (size_t)T * (size_t)vit::f64_hist_stride(p->S) * sizeof(double));
    w.off_entry = w.off_last + align256((size_t)B * sizeof(int32_t));
    w.bytes = w.off_entry + align256((size_t)B * vit::kBtMaxChunks * sizeof(int32_t));
    return w;
}
// The argument checks the two padded float64 decodes start with, in this order (segment_frames: null for vit_decode_f64).
int check_f64(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T, const void* ws, const int32_t* states,
              const int64_t* segment_frames = nullptr) {
    if (!states) return VIT_EINVAL;
    const int rc = check_common(plan, B, T, ws);
    if (rc != VIT_OK) return rc;
    if (!logE) return VIT_EINVAL;
    if (emis_dtype != VIT_F32 && emis_dtype != VIT_F16) return VIT_EINVAL;
    if (segment_frames && !ck_segment_ok(*segment_frames)) return VIT_EINVAL;
    return f64_applies(plan) ? VIT_OK : VIT_EUNSUPPORTED;
}
// what the float64 kernels read of the plan (vit_decode_f64, vit_decode_f64_packed)
void f64_args_from_plan(const vit_plan* plan, vit::F64Args& a) {
    a.image = plan->dev_image;
    a.S = plan->S;
    a.SP = plan->L.SP;
    a.SD64 = vit::f64_hist_stride(plan->S);
    a.W = plan->bp.W;
    a.n_extras = plan->bp.n_extras;
    for (int k = 0; k < vit::kMaxExtras; ++k) a.extras[k] = plan->bp.extras[k];
    a.off_logpi = plan->L.off_logpi;
    a.off_lo = plan->L.off_lo;
    a.off_tabA = plan->L.off_tabA;
    a.off_extraA = plan->L.off_extraA;
    a.off_rowc = plan->L.off_rowc;
    a.off_tabX = plan->L.off_tabX;
}

}  // namespace

size_t vit_workspace_bytes_f64(const vit_plan* plan, int64_t B, int64_t T) {
    if (!plan || B < 0 || T < 1 || T > (int64_t)1 << 30 || B > (int64_t)1 << 30 || !f64_applies(plan)) return 0;
    return f64_layout(plan, B, T).bytes;
}

int vit_decode_f64(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T, const int64_t* lengths, void* workspace,
                   size_t workspace_bytes, int32_t* states, double* loglik, vit_stream stream) {
    const int rc = check_f64(plan, logE, emis_dtype, B, T, workspace, states);
    if (rc != VIT_OK) return rc;
    const F64Layout w = f64_layout(plan, B, T);
    if (workspace_bytes < w.bytes) return VIT_EWORKSPACE;
    if (B == 0) return VIT_OK;
    stamp_erase(plan, workspace);      // whatever vit_forward left in this workspace is gone once the kernels below start: vit_backtrace must not find it
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    vit::F64Args a{};
    f64_args_from_plan(plan, a);
    a.logE = logE;
    a.lengths = lengths;
    a.hist = reinterpret_cast<double*>(ws + w.off_hist);
    a.last_state = reinterpret_cast<int32_t*>(ws + w.off_last);
    a.loglik = loglik;
    a.states = states;
    a.entry = reinterpret_cast<int32_t*>(ws + w.off_entry);
    a.B = B;
    a.T = (int)T;
    a.chunks = tuned_chunks(plan->tune, vit::backtrace_chunks(B, (int)T));
    a.warm = tuned_warm(plan->tune, vit::kBtWarm);
    VIT_TRY(vit::launch_f64_forward(a, vit::F64Variant::Plain, emis_dtype == VIT_F16, (hipStream_t)stream));
    return hip_status(vit::launch_f64_backtrace(a, vit::F64Variant::Plain, (hipStream_t)stream));
}

// ---------------------------------------------------------------------------------------------------------------------
// Bounded-workspace decode.  The reference keeps T1 / T2 for ONE song (tonet/for_paper.py:1852-1853); the
// batched decode above keeps a delta history for the whole batch (46 MB per song at T = 30000, 87 MB with 722 states).  Here the
// history never exists at once: pass 1 runs the forward recursion over all T frames and keeps one delta row per segment of K frames
// (the row in front of the segment) plus the terminal state; pass 2 walks the segments from the last to the first, re-runs the
// forward kernel over one segment from its checkpoint row into a buffer of about K rows and back-traces it from the state the
// segment behind it decided at its first frame.  Exact by construction (the same kernels, the same sums); twice the forward work.
// Three families (ck_family, Family): plans with the wave form (wave.hip WaveHist::CkptPass / Segment, the sparse back-trace); banded plans without it whose
// floor form is proven (banded_floor_forward_kernel<.., WgVariant::Ckpt>, the sparse back-trace over the workgroup layout, or the lane form);
// step plans (step4s_forward_kernel<.., WgVariant::Ckpt>, the lazy back-trace).  The workgroup families always run that one kernel:
// forward_form, step_form, backtrace_form and bt_chunks are not consulted; bt_fast_rows, bt_warm and win_shift are.
namespace {

// the sparse back-trace serves the history layout a checkpointed decode of this plan writes (kFamWave: the wave layout, kFamGroup: workgroup rows)
bool ck_sparse_applies(const vit_plan* p, int family) {
    vit::BtArgs b{};                 // a probe: only what sparse_backtrace_applies reads, NOT bt_args_from_plan (lo_affine stays 0)
    hist_layout_apply(hist_layout(p, family), b);
    b.S = p->S;
    b.SP = p->L.SP;
    b.W = p->bp.W;
    b.banded = 1;
    b.n_extras = p->bp.n_extras;
    b.n_dense = p->bp.n_dense;
    return vit::sparse_backtrace_applies(b);
}
// the lane back-trace does (lane_backtrace_applies for the workgroup rows: width instantiated, W <= S, no dense rows)
bool ck_lane_applies(const vit_plan* p) { return p->bp.n_dense == 0 && vit::banded_width_instantiated(p->bp.W) && p->bp.W <= p->S; }
inline bool step_applies(const vit_plan* p) { return p->bp.step_ok && vit::step_kernel_instantiated(p->S, p->bp.step_bw, p->bp.step_kb); }

// The forward family a checkpointed decode of this plan runs, kFamNone = none: the ONE predicate behind
// vit_workspace_bytes_checkpointed and vit_decode_checkpointed, so that a size > 0 implies a decode that launches.
int ck_family(const vit_plan* p) {
    if (p->bp.ok && p->bp.wave_ok) return ck_sparse_applies(p, kFamWave) ? kFamWave : kFamNone;
    if (p->bp.ok)      // banded, no wave form: the floor form (no dense rows) and a back-trace over its rows
        return vit::floor_ckpt_applies(p->S, p->bp.W, p->bp.floor_ok, p->bp.n_dense) && (ck_sparse_applies(p, kFamGroup) || ck_lane_applies(p)) ? kFamGroup : kFamNone;
    return step_applies(p) ? kFamStep : kFamNone;
}

struct CkLayout {
    int64_t nseg, seg_rows;
    size_t off_ckpt, off_seg, off_cnt, off_mask, off_last, off_entry, off_slen, off_slast, bytes;
};
// The wave family keeps the byte counts it had when it was the only one.  The workgroup families: the segment
// buffer holds K + 2 rows per song -- one in FRONT of the segment (the banded kernel stores the frame maximum of frame t - 1 into row
// t - 1 while it computes frame t: for a resumed segment's first frame that is the checkpoint's place) and one behind it (the
// forward pass runs one frame past the segment where the song goes on, for the frame maximum of its last row).  kFamGroup may
// back-trace with the lane form: its chunk flags and kLaneMaxChunks entries per song.
CkLayout ck_layout(const vit_plan* p, int family, int64_t B, int64_t T, int64_t K) {
    CkLayout c;
    K = K > T ? T : K;                                                           // (a segment longer than the songs: one segment of T frames)
    const size_t sd = (size_t)hist_layout(p, family).SD * sizeof(float);
    c.nseg = (T + K - 1) / K;
    c.seg_rows = family == kFamWave ? K + 1 : K + 2;
    c.off_ckpt = 0;                                                              // [B][nseg] rows: nseg - 1 checkpoints + the scratch row
    c.off_seg = align256((size_t)B * (size_t)c.nseg * sd);                       // [B][seg_rows] rows of the segment being walked
    c.off_cnt = c.off_seg + align256((size_t)B * (size_t)c.seg_rows * sd);
    c.off_mask = c.off_cnt + align256((size_t)B * 64 * sizeof(float));           // (counters; timing builds: the forward kernels' scratch)
    c.off_last = c.off_mask + (family == kFamGroup ? align256((size_t)B * vit::kLaneMaskWords * sizeof(uint32_t)) : 0);
    c.off_entry = c.off_last + align256((size_t)B * sizeof(int32_t));
    c.off_slen = c.off_entry + align256((size_t)B * (family == kFamGroup ? vit::kLaneMaxChunks : vit::kBtMaxChunks) * sizeof(int32_t));
    c.off_slast = c.off_slen + align256((size_t)B * sizeof(int64_t));
    c.bytes = c.off_slast + align256((size_t)B * sizeof(int32_t));
    return c;
}

// The back-trace of one segment of a checkpointed decode -- b.B sub-problems of b.T frames: the songs of vit_decode_checkpointed, the
// units of one launch of the packed budgeted decode -- and of a streaming session (vit_stream_backtrace: the recordings as they stand).
// Step plans: the lazy kernel, one wave per (sub-problem, chunk); banded plans: the sparse kernel, or the lane form where the caller
// found that the sparse one does not serve the rows (lane_bt; b.mask set).  tune_chunks: "bt_chunks" is honoured (sessions only).
hipError_t segment_backtrace(const vit_plan* plan, int family, bool lane_bt, vit::BtArgs& b, hipStream_t st, bool tune_chunks = false) {
    const Tuning& tn = plan->tune;      // (bt_chunks is not consulted by the checkpointed decodes)
    auto chunks_of = [&](int chunks, int cap) { return tune_chunks ? tuned_chunks(tn, chunks, cap) : chunks; };
    if (family == kFamStep) {
        b.chunks = chunks_of(vit::backtrace_chunks(b.B, b.T), vit::kBtMaxChunks);
        b.warm = tuned_warm(tn, vit::kBtWarm);
        return vit::launch_backtrace_rows_segment(b, st);
    }
    if (lane_bt) {
        b.warm = tuned_warm(tn, vit::kBtWarmSparse);
        b.chunks = chunks_of(vit::lane_backtrace_chunks(b.B, b.T, plan->n_cus, b.warm), vit::kLaneMaxChunks);
        if (b.chunks > 1) {         // the chunk flags of this segment
            const hipError_t e = hipMemsetAsync(b.mask, 0, (size_t)b.B * vit::kLaneMaskWords * sizeof(uint32_t), st);
            if (e != hipSuccess) return e;
        }
        return vit::launch_backtrace_lane(b, st);
    }
    b.chunks = chunks_of(vit::sparse_backtrace_chunks(b.B, b.T, plan->n_cus), vit::kBtMaxChunks);
    // KNOWN ASYMMETRY, kept: the wave family always warms up kBtWarmSparse frames and does NOT consult bt_warm; kFamGroup does
    b.warm = family == kFamWave ? vit::kBtWarmSparse : tuned_warm(tn, vit::kBtWarmSparse);
    return vit::launch_backtrace_sparse(b, st);
}

}  // namespace

size_t vit_workspace_bytes_checkpointed(const vit_plan* plan, int64_t B, int64_t T, int64_t segment_frames) {
    if (!plan || B < 0 || T < 1 || !ck_segment_ok(segment_frames)) return 0;
    const int family = ck_family(plan);
    if (family == kFamNone) return 0;
    return ck_layout(plan, family, B, T, segment_frames).bytes;
}

namespace {
extern "C++" {      // (a template over the forward callable: no C linkage)
// The checkpointed decode of a padded batch once its entry point has accepted the call -- the driver of vit_decode_checkpointed and
// vit_decode_logits_checkpointed, which differ in what a forward launch is: forward(f, segment) -> hipError_t runs pass 1 (segment
// false: f.ckpt_every = K) or one segment (f.t_begin / f.t_end, resumed from f.init_rows) of `family` over the rows of c = ck_layout(plan,
// family, B, T, K), K <= T; f.logE is the caller's `logE` (the fused launch has none).  The steps: the memset of `states` where lengths
// are given, pass 1, then the segments from the last to the first with launch_segment_prep and segment_backtrace.
template <typename Forward>
int ck_decode(const vit_plan* plan, int family, const CkLayout& c, int64_t K, const void* logE, int64_t B, int64_t T, const int64_t* lengths,
              void* workspace, int32_t* states, float* loglik, hipStream_t st, Forward&& forward) {
    stamp_erase(plan, workspace);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const HistLayout lay = hist_layout(plan, family);
    const bool lane_bt = family == kFamGroup && !ck_sparse_applies(plan, kFamGroup);
    if (lengths)       // frames past a song's end: -1 (segments a song does not reach are skipped, not written)
        VIT_TRY(hipMemsetAsync(states, 0xff, (size_t)B * (size_t)T * sizeof(int32_t), st));
    int32_t* counters = reinterpret_cast<int32_t*>(ws + c.off_cnt);
    VIT_TRY(hipMemsetAsync(counters, 0, (size_t)B * vit::kBtCounters * sizeof(int32_t), st));

    // ---- pass 1: checkpoint rows + terminal state
    vit::FwdArgs a{};
    fwd_args_from_plan(plan, a);          // (a.SD: the workgroup kernels' row stride; the wave kernel has its own)
    a.logE = logE;
    a.lengths = lengths;
    a.hist = reinterpret_cast<float*>(ws + c.off_ckpt);
    a.fmax = reinterpret_cast<float*>(ws + c.off_cnt);
    a.last_state = reinterpret_cast<int32_t*>(ws + c.off_last);
    a.loglik = loglik;
    a.B = B;
    a.T = (int)T;
    a.hist_rows = c.nseg;
    a.ckpt_every = (int)K;
    a.t_begin = 0;
    a.t_end = (int)T;
    VIT_TRY(forward(a, false));

    // ---- pass 2: segments, last to first
    vit::BtArgs b{};
    bt_args_from_plan(plan, b);
    hist_layout_apply(lay, b);
    b.aux_frames = 1;       // (a segment's sub-problem ends one frame behind the rows it decides from: every frame's scalars from its own row)
    // workgroup families: the segment's row 0 is the buffer's second row (ck_layout)
    float* seg = reinterpret_cast<float*>(ws + c.off_seg) + (family == kFamWave ? 0 : lay.SD);
    b.hist = seg;
    b.hist_rows = c.seg_rows;
    b.last_state = reinterpret_cast<const int32_t*>(ws + c.off_slast);
    b.lengths = reinterpret_cast<const int64_t*>(ws + c.off_slen);
    b.entry = reinterpret_cast<int32_t*>(ws + c.off_entry);
    b.B = B;
    b.states_stride = T;
    b.skip_nonpositive = 1;
    b.counters = counters;
    b.mask = family == kFamGroup ? reinterpret_cast<uint32_t*>(ws + c.off_mask) : nullptr;
    b.bt_form = family == kFamStep ? 1 : (lane_bt ? 4 : 0);
    if (lane_bt && !vit::lane_backtrace_applies(b)) return VIT_EUNSUPPORTED;      // (cannot happen: ck_family asked the same predicates)
    for (int64_t sgm = c.nseg - 1; sgm >= 0; --sgm) {
        const int64_t s0 = sgm * K, e0 = s0 + K < T ? s0 + K : T;
        vit::FwdArgs f = a;
        f.ckpt_every = 0;
        f.hist = seg;
        f.hist_rows = c.seg_rows;
        f.loglik = nullptr;
        f.t_begin = (int)s0;
        f.t_end = (int)e0;
        f.init_rows = sgm > 0 ? reinterpret_cast<const float*>(ws + c.off_ckpt) + (size_t)(sgm - 1) * lay.SD : nullptr;
        f.init_stride = (int64_t)c.nseg * lay.SD;
        VIT_TRY(forward(f, true));
        VIT_TRY(vit::launch_segment_prep(lengths, B, (int)T, (int)s0, (int)e0, states, reinterpret_cast<const int32_t*>(ws + c.off_last),
                                         reinterpret_cast<int64_t*>(ws + c.off_slen), reinterpret_cast<int32_t*>(ws + c.off_slast), st));
        b.T = (int)(e0 < T ? e0 - s0 + 1 : e0 - s0);      // the frame behind the segment is the sub-problem's terminal frame
        b.states = states + s0;
        VIT_TRY(segment_backtrace(plan, family, lane_bt, b, st));
    }
    return VIT_OK;
}
}  // extern "C++"
}  // namespace

int vit_decode_checkpointed(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T, const int64_t* lengths,
                            void* workspace, size_t workspace_bytes, int32_t* states, float* loglik, int64_t segment_frames,
                            vit_stream stream) {
    int rc = check_common(plan, B, T, workspace);
    if (rc != VIT_OK) return rc;
    if (!logE || !states) return VIT_EINVAL;
    if (emis_dtype != VIT_F32 && emis_dtype != VIT_F16) return VIT_EINVAL;
    if (!ck_segment_ok(segment_frames)) return VIT_EINVAL;
    const int family = ck_family(plan);             // (everything that can refuse the plan is asked here, before anything is enqueued)
    if (family == kFamNone) return VIT_EUNSUPPORTED;
    const int64_t K = segment_frames > T ? T : segment_frames;
    const CkLayout c = ck_layout(plan, family, B, T, K);
    if (workspace_bytes < c.bytes) return VIT_EWORKSPACE;
    if (B == 0) return VIT_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool f16 = emis_dtype == VIT_F16;
    return ck_decode(plan, family, c, K, logE, B, T, lengths, workspace, states, loglik, st, [&](const vit::FwdArgs& f, bool) {
        return launch_family(family, vit::WgVariant::Ckpt, f, f16, st);
    });
}


// ---------------------------------------------------------------------------------------------------------------------
// Bounded-workspace float64 decode: the scheme above with vit_decode_f64's kernels in their Ckpt variant (f64.hip).  Pass 1 keeps the d
// row in front of every segment but a song's first and the terminal state and log-likelihood; pass 2 walks the segments from the
// last to the first: the forward kernel resumed from the checkpoint row into K + 1 rows per song, segment_prep_kernel, the
// back-trace of the sub-problems.  The plans are vit_decode_f64's (f64_applies); bt_chunks and bt_warm are honoured per segment.
namespace {

struct F64CkLayout {
    int64_t nseg, seg_rows;
    size_t off_ckpt, off_seg, off_last, off_entry, off_slen, off_slast, bytes;
};
// Checkpoint rows: nseg per song -- the rows in front of segments 1 .. nseg - 1 and, where K divides T, the place pass 1 stores frame
// T - 1 at.  Segment rows: K + 1 per song -- one in FRONT of the segment (the forward kernel stores the frame maximum of frame t - 1
// next to row t - 1 while it computes frame t: for a resumed segment's first frame that is the checkpoint's place) and the K of the
// segment; M of the segment's last row is formed from what the last frame published, so no frame past the segment is run.
F64CkLayout f64_ck_layout(const vit_plan* p, int64_t B, int64_t T, int64_t K) {
    F64CkLayout c;
    K = K > T ? T : K;
    const size_t sd = (size_t)vit::f64_hist_stride(p->S) * sizeof(double);
    c.nseg = (T + K - 1) / K;
    c.seg_rows = K + 1;
    c.off_ckpt = 0;
    c.off_seg = align256((size_t)B * (size_t)c.nseg * sd);
    c.off_last = c.off_seg + align256((size_t)B * (size_t)c.seg_rows * sd);
    c.off_entry = c.off_last + align256((size_t)B * sizeof(int32_t));
    c.off_slen = c.off_entry + align256((size_t)B * vit::kBtMaxChunks * sizeof(int32_t));
    c.off_slast = c.off_slen + align256((size_t)B * sizeof(int64_t));
    c.bytes = c.off_slast + align256((size_t)B * sizeof(int32_t));
    return c;
}
// Chunks of one segment's back-trace.  backtrace_chunks() keeps a chunk at eight warm-ups of 128 frames and so gives a segment of
// 1024 frames ONE chunk: every song then walks its K frames step by step in every segment, T dependent steps in all where the
// whole-history decode walks T / 32.  Here: enough (song, chunk) waves to cover the chip twice over, chunks no shorter than two
// warm-ups of kBtWarmSparse frames (a wrong guess costs a repair that ends where the paths meet).  Tuning: the states do not depend on it.
int f64_segment_chunks(int64_t B, int frames, int warm) {
    const int shortest = 2 * warm > 64 ? 2 * warm : 64;
    long long c = (2 * 1024 + B - 1) / B;
    c = c > frames / shortest ? frames / shortest : c;
    c = c > vit::kBtMaxChunks ? vit::kBtMaxChunks : c;
    return c < 1 ? 1 : (int)c;
}

}  // namespace

size_t vit_workspace_bytes_f64_checkpointed(const vit_plan* plan, int64_t B, int64_t T, int64_t segment_frames) {
    if (!plan || B < 0 || T < 1 || T > (int64_t)1 << 30 || B > (int64_t)1 << 30 || !ck_segment_ok(segment_frames) || !f64_applies(plan)) return 0;
    return f64_ck_layout(plan, B, T, segment_frames).bytes;
}

int vit_decode_f64_checkpointed(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, int64_t T, const int64_t* lengths,
                                void* workspace, size_t workspace_bytes, int32_t* states, double* loglik, int64_t segment_frames,
                                vit_stream stream) {
    const int rc = check_f64(plan, logE, emis_dtype, B, T, workspace, states, &segment_frames);
    if (rc != VIT_OK) return rc;
    const int64_t K = segment_frames > T ? T : segment_frames;
    const F64CkLayout c = f64_ck_layout(plan, B, T, K);
    if (workspace_bytes < c.bytes) return VIT_EWORKSPACE;
    if (B == 0) return VIT_OK;
    stamp_erase(plan, workspace);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const bool f16 = emis_dtype == VIT_F16;
    if (lengths)       // frames past a song's end: -1 (segments a song does not reach are skipped, not written)
        VIT_TRY(hipMemsetAsync(states, 0xff, (size_t)B * (size_t)T * sizeof(int32_t), st));

    // ---- pass 1: checkpoint rows + terminal state and log-likelihood
    vit::F64Args a{};
    f64_args_from_plan(plan, a);
    a.logE = logE;
    a.lengths = lengths;
    a.hist = reinterpret_cast<double*>(ws + c.off_ckpt);
    a.hist_song_stride = c.nseg * (int64_t)a.SD64;
    a.last_state = reinterpret_cast<int32_t*>(ws + c.off_last);
    a.loglik = loglik;
    a.entry = reinterpret_cast<int32_t*>(ws + c.off_entry);
    a.B = B;
    a.T = (int)T;
    a.ckpt_every = (int)K;
    a.t_begin = 0;
    a.t_end = (int)T;
    VIT_TRY(vit::launch_f64_forward(a, vit::F64Variant::Ckpt, f16, st));

    // ---- pass 2: segments, last to first
    int64_t* seg_len = reinterpret_cast<int64_t*>(ws + c.off_slen);
    int32_t* seg_last = reinterpret_cast<int32_t*>(ws + c.off_slast);
    const Tuning& tn = plan->tune;
    for (int64_t sgm = c.nseg - 1; sgm >= 0; --sgm) {
        const int64_t s0 = sgm * K, e0 = s0 + K < T ? s0 + K : T;
        vit::F64Args f = a;
        f.ckpt_every = 0;
        f.hist = reinterpret_cast<double*>(ws + c.off_seg) + a.SD64;      // the segment's row 0 is the buffer's second row
        f.hist_song_stride = c.seg_rows * (int64_t)a.SD64;
        f.loglik = nullptr;
        f.t_begin = (int)s0;
        f.t_end = (int)e0;
        f.init_rows = sgm > 0 ? reinterpret_cast<const double*>(ws + c.off_ckpt) + (size_t)(sgm - 1) * a.SD64 : nullptr;
        f.init_stride = a.hist_song_stride;
        VIT_TRY(vit::launch_f64_forward(f, vit::F64Variant::Ckpt, f16, st));
        VIT_TRY(vit::launch_segment_prep(lengths, B, (int)T, (int)s0, (int)e0, states, a.last_state, seg_len, seg_last, st));
        const int sub_T = (int)(e0 < T ? e0 - s0 + 1 : e0 - s0);           // the frame behind the segment is the sub-problem's terminal frame
        f.seg_len = seg_len;
        f.seg_last = seg_last;
        f.states = states + s0;
        f.warm = tuned_warm(tn, vit::kBtWarmSparse);
        f.chunks = tuned_chunks(tn, f64_segment_chunks(B, sub_T, f.warm));
        VIT_TRY(vit::launch_f64_backtrace(f, vit::F64Variant::Ckpt, st));
    }
    return VIT_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// Packed (ragged) decode.  The reference decodes every recording whole with its own T (tonet/for_paper.py:2304-2309); a padded
// [B, T_max, S] tensor wastes memory on the padding and a launch with one wavefront per song costs its LONGEST song.  Here the
// emissions of B songs are one [sum T_b, S] buffer, the history and the states are packed the same way, and the forward pass
// runs n_slots <= 8 waves per CU, each walking a host-packed list of songs back to back (longest-first greedy bins by frames:
// the rule of sharded.shard_by_length), so that every wave carries about the same number of frames.  The back-trace is the lane
// form (backtrace_lane.hip): every song is cut into chunks of about equal length (total frames / resident LANES), one lane per
// chunk -- the one-stream-per-wavefront kernels hold 16 streams per CU, fewer than a ragged batch of thousands of songs needs
// (3250 songs: a second round of waves, 14 instead of 6 ms).
// Plans without the wave form (the 722-state grids) run the same scheme with a WORKGROUP per slot: banded plans with the floor
// form proven take banded_floor_forward_kernel<.., WgVariant::Packed> and the lane back-trace over the workgroup history layout, step plans take
// step4s_forward_kernel<.., WgVariant::Packed> and the lazy back-trace over per-song chunk lists.  Slots: as many workgroups as are resident at once.
namespace {

// The forward family a packed decode of this plan runs, kFamNone = none: the ONE predicate behind
// vit_workspace_bytes_packed and vit_decode_packed, so that a size > 0 implies a decode that launches.
int pk_family(const vit_plan* p) {
    if (p->bp.ok && p->bp.wave_ok) return kFamWave;
    if (p->bp.ok)      // banded, no wave form: the floor form and the lane back-trace (lane_backtrace_applies: width instantiated, W <= S)
        return vit::floor_packed_applies(p->S, p->bp.W, p->bp.floor_ok, p->bp.n_dense) && p->bp.W <= p->S ? kFamGroup : kFamNone;
    return step_applies(p) ? kFamStep : kFamNone;
}

// The argument checks every packed decode starts with, in this order.
int check_packed(const vit_plan* plan, int64_t B, const int64_t* offsets, const void* workspace, int emis_dtype) {
    if (!plan || !workspace || !offsets) return VIT_EINVAL;
    if (B < 0 || B > (int64_t)1 << 30) return VIT_EINVAL;
    if (!plan->dev_image) return VIT_ENOTUPLOADED;
    if (((uintptr_t)workspace & 255) != 0) return VIT_EINVAL;
    if (emis_dtype != VIT_F32 && emis_dtype != VIT_F16) return VIT_EINVAL;
    return VIT_OK;
}
// B + 1 frame offsets from 0, every song with 1 .. 2^30 frames; *tmax: the longest song (1 for an empty batch)
bool offsets_ok(const int64_t* offsets, int64_t B, int64_t* tmax) {
    if (!offsets || offsets[0] != 0) return false;
    *tmax = 1;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t tb = offsets[b + 1] - offsets[b];
        if (tb < 1 || tb > (int64_t)1 << 30) return false;
        *tmax = std::max(*tmax, tb);
    }
    return true;
}

// The chunk table (vit::packed_chunk_table) of the packed back-traces that run one WAVE per chunk -- the lazy kernel over step plans,
// the float64 kernel: about eight waves per CU (tuning), chunks no shorter than the 8 * kBtWarm frames of backtrace_chunks, at most
// kBtMaxChunks per song, counts rounded down (no chunk shorter than that).  At most B + pk_wave_streams entries: sum of
// max(1, T_b / cf) <= B + N / cf, cf >= N / streams.
inline int64_t pk_wave_streams(const vit_plan* p) { return 8 * (int64_t)p->n_cus; }
inline bool pk_wave_chunk_table(const vit_plan* p, const int64_t* offsets, int64_t B, int64_t capacity, int32_t* chunk_base, int32_t* wave_song,
                                int64_t* largest) {
    return vit::packed_chunk_table(offsets, B, pk_wave_streams(p), vit::kBtMaxChunks, 8 * vit::kBtWarm, false, capacity, chunk_base, wave_song, largest);
}

struct PkLayout {
    int64_t n_slots, max_waves;
    size_t off_hist, off_cnt, off_mask, off_last, off_entry, off_offsets, off_slot_begin, off_slot_songs, off_wave_song, off_chunk_base, bytes;
    size_t tables_bytes;      // offsets .. chunk_base: one contiguous upload
};
inline int64_t pk_slots(const vit_plan* p, int64_t B) { const int64_t cap = 8 * (int64_t)p->n_cus; return B < cap ? B : cap; }
inline int64_t pk_max_waves(const vit_plan* p, int64_t B) { return B + 16 * 64 * (int64_t)p->n_cus; }     // (song, chunk) streams of the back-trace: one per lane
// n_slots is an upper bound here (it sizes slot_begin): the decode lowers it (pk_lower_slots)
PkLayout pk_layout(const vit_plan* p, int family, int64_t B, int64_t N) {
    PkLayout k;
    const size_t sd = (size_t)hist_layout(p, family).SD * sizeof(float);
    k.n_slots = pk_slots(p, B);
    k.max_waves = pk_max_waves(p, B);
    k.off_hist = 0;
    k.off_cnt = align256((size_t)N * sd);
    k.off_mask = k.off_cnt + align256((size_t)B * vit::kBtCounters * sizeof(int32_t));
    k.off_last = k.off_mask + align256((size_t)B * vit::kLaneMaskWords * sizeof(uint32_t));
    k.off_entry = k.off_last + align256((size_t)B * sizeof(int32_t));
    k.off_offsets = k.off_entry + align256((size_t)k.max_waves * sizeof(int32_t));
    k.off_slot_begin = k.off_offsets + align256((size_t)(B + 1) * sizeof(int64_t));
    k.off_slot_songs = k.off_slot_begin + align256((size_t)(k.n_slots + 1) * sizeof(int32_t));
    k.off_wave_song = k.off_slot_songs + align256((size_t)B * sizeof(int32_t));
    k.off_chunk_base = k.off_wave_song + align256((size_t)k.max_waves * sizeof(int32_t));
    k.bytes = k.off_chunk_base + align256((size_t)(B + 1) * sizeof(int32_t));
    k.tables_bytes = k.bytes - k.off_offsets;
    return k;
}

extern "C++" {      // (two templates over the query callable: no C linkage)
// Workgroups one CU holds of a packed forward kernel (key: which; not kResNone) -- the occupancy of that instantiation, asked of the
// device once per emission type (query(&per_cu) -> hipError_t) and remembered in the plan.
template <typename Query>
int resident_per_cu(const vit_plan* plan, int key, bool f16, Query&& query, int* per_cu) {
    int& cached = plan->resident[key][f16 ? 1 : 0];
    {
        std::lock_guard<std::mutex> g(plan->mu);
        *per_cu = cached;
    }
    if (*per_cu >= 1) return VIT_OK;
    const hipError_t eq = query(per_cu);
    if (eq == hipErrorInvalidConfiguration) return VIT_EUNSUPPORTED;    // (cannot happen: the predicate of the entry point asked the same)
    VIT_TRY(eq);
    if (*per_cu < 1) return VIT_EUNSUPPORTED;
    std::lock_guard<std::mutex> g(plan->mu);
    cached = *per_cu;
    return VIT_OK;
}
// The forward slots of a packed batch of N frames whose longest song has tmax: at most `bound` (*n_slots on entry); workgroup forms
// (key, query: as in resident_per_cu): one per workgroup that is resident at once; and no more than N / tmax -- a slot's load should
// not fall below the longest song, which bounds the launch anyway (1623 songs of 7500..30000 frames: 1024 slots of ~30000 frames, one
// wave per SIMD, instead of 1623 waves of which the longest share their SIMDs to the end).
template <typename Query>
int pk_lower_slots(const vit_plan* plan, int key, bool f16, Query&& query, int64_t N, int64_t tmax, int64_t* n_slots) {
    if (key != kResNone) {      // (kResNone, the wave family: min(pk_slots, max(1, N / tmax)) with no occupancy query)
        int per_cu;
        const int rc = resident_per_cu(plan, key, f16, query, &per_cu);
        if (rc != VIT_OK) return rc;
        *n_slots = std::min<int64_t>(*n_slots, (int64_t)per_cu * plan->n_cus);
    }
    *n_slots = std::min<int64_t>(*n_slots, std::max<int64_t>(1, N / tmax));
    return VIT_OK;
}
}  // extern "C++"

// The plan's pinned staging buffer with room for `bytes` of host tables, zeroed (the packed decodes): waits for the upload of the call
// before, which read it; pk_upload() sends it and records the next wait.
int pk_stage(const vit_plan* plan, size_t bytes) {
    std::lock_guard<std::mutex> g(plan->mu);
    if (plan->pk_event) VIT_TRY(hipEventSynchronize(plan->pk_event));
    else VIT_TRY(hipEventCreateWithFlags(&plan->pk_event, hipEventDisableTiming));
    if (plan->pk_host_bytes < bytes) {
        if (plan->pk_host) (void)hipHostFree(plan->pk_host);
        plan->pk_host = nullptr;
        plan->pk_host_bytes = 0;
        VIT_TRY(hipHostMalloc(&plan->pk_host, bytes, hipHostMallocDefault));
        plan->pk_host_bytes = bytes;
    }
    std::memset(plan->pk_host, 0, bytes);
    return VIT_OK;
}
int pk_upload(const vit_plan* plan, void* dst, size_t bytes, hipStream_t st) {
    VIT_TRY(hipMemcpyAsync(dst, plan->pk_host, bytes, hipMemcpyHostToDevice, st));
    VIT_TRY(hipEventRecord(plan->pk_event, st));
    return VIT_OK;
}

// forward slots of a packed batch: longest song first into the slot with the fewest frames (ties: fewest songs, lowest slot);
// slot sl walks songs slot_songs[slot_begin[sl] .. slot_begin[sl+1]), longest first (the rule of sharded.shard_by_length)
void pk_fill_slots(const int64_t* offsets, int64_t B, int64_t n_slots, int32_t* h_slot_begin, int32_t* h_slot_songs) {
    std::vector<int32_t> order((size_t)B);
    for (int64_t b = 0; b < B; ++b) order[(size_t)b] = (int32_t)b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return offsets[x + 1] - offsets[x] > offsets[y + 1] - offsets[y]; });
    typedef std::pair<std::pair<int64_t, int32_t>, int32_t> Load;       // ((frames, songs), slot)
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
    for (int32_t sl = 0; sl < (int32_t)n_slots; ++sl) heap.push(Load{{0, 0}, sl});
    std::vector<int32_t> slot_of((size_t)B);
    std::vector<int32_t> count((size_t)n_slots, 0);
    for (int32_t sng : order) {
        Load l = heap.top();
        heap.pop();
        slot_of[(size_t)sng] = l.second;
        ++count[(size_t)l.second];
        l.first.first += offsets[sng + 1] - offsets[sng];
        ++l.first.second;
        heap.push(l);
    }
    h_slot_begin[0] = 0;
    for (int64_t sl = 0; sl < n_slots; ++sl) h_slot_begin[sl + 1] = h_slot_begin[sl] + count[(size_t)sl];
    std::vector<int32_t> fill(h_slot_begin, h_slot_begin + n_slots);
    for (int32_t sng : order) h_slot_songs[fill[(size_t)slot_of[(size_t)sng]]++] = sng;     // a slot walks its songs longest first
}

// The tables every packed decode starts with, in the plan's pinned staging buffer (pk_stage: `bytes` of it, zeroed): the offsets at
// its start, the forward slots at rel_slot_begin / rel_slot_songs (the tables' workspace offsets less that of the offsets).  *hb: the buffer.
int pk_stage_common(const vit_plan* plan, size_t bytes, const int64_t* offsets, int64_t B, int64_t n_slots, size_t rel_slot_begin,
                    size_t rel_slot_songs, uint8_t** hb) {
    const int rc = pk_stage(plan, bytes);
    if (rc != VIT_OK) return rc;
    *hb = static_cast<uint8_t*>(plan->pk_host);
    std::memcpy(*hb, offsets, (size_t)(B + 1) * sizeof(int64_t));
    try {
        pk_fill_slots(offsets, B, n_slots, reinterpret_cast<int32_t*>(*hb + rel_slot_begin), reinterpret_cast<int32_t*>(*hb + rel_slot_songs));
    } catch (const std::bad_alloc&) {
        return VIT_ENOMEM;
    }
    return VIT_OK;
}

// the fields of a packed forward pass that do not depend on which packed decode runs it
void fwd_args_packed(vit::FwdArgs& a, const void* logE, int64_t B, float* loglik) {
    a.logE = logE;
    a.lengths = nullptr;
    a.fmax = nullptr;
    a.loglik = loglik;
    a.B = B;
    a.T = 1;                      // (unused by the packed kernels: a song's rows come from the offsets)
    a.t_begin = 0;
    a.t_end = 1;
}

}  // namespace

size_t vit_workspace_bytes_packed(const vit_plan* plan, int64_t B, int64_t total_frames) {
    if (!plan || B < 0 || total_frames < 0) return 0;
    const int family = pk_family(plan);
    if (family == kFamNone) return 0;
    return pk_layout(plan, family, B, total_frames).bytes;
}

int vit_decode_packed(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, const int64_t* offsets, void* workspace,
                      size_t workspace_bytes, int32_t* states, float* loglik, vit_stream stream) {
    int rc = check_packed(plan, B, offsets, workspace, emis_dtype);
    if (rc != VIT_OK) return rc;
    const int family = pk_family(plan);
    if (family == kFamNone) return VIT_EUNSUPPORTED;
    int64_t tmax;
    if (!offsets_ok(offsets, B, &tmax)) return VIT_EINVAL;
    const int64_t N = offsets[B];
    if (B == 0) return VIT_OK;
    if (!logE || !states) return VIT_EINVAL;
    PkLayout k = pk_layout(plan, family, B, N);
    if (workspace_bytes < k.bytes) return VIT_EWORKSPACE;
    const bool f16 = emis_dtype == VIT_F16;
    vit::FwdArgs a{};
    fwd_args_from_plan(plan, a);
    rc = pk_lower_slots(plan, family == kFamWave ? kResNone : kResPacked, f16,
                        [&](int* n) { return family_resident(family, vit::WgVariant::Packed, a, f16, n); }, N, tmax, &k.n_slots);
    if (rc != VIT_OK) return rc;
    stamp_erase(plan, workspace);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);

    // ---- host tables in the plan's pinned staging buffer (the previous call's upload must have read it): offsets, forward slots
    // (greedy bins by frames) and the back-trace's chunk table.  Banded plans: one stream per LANE (backtrace_lane.hip) -- chunks of
    // about (total frames / resident lanes) frames, never shorter than four warm-ups, at most kLaneMaxChunks per song, counts rounded
    // to nearest.  Step plans, lazy back-trace: one WAVE per chunk (pk_wave_chunk_table).
    uint8_t* hb;
    rc = pk_stage_common(plan, k.tables_bytes, offsets, B, k.n_slots, k.off_slot_begin - k.off_offsets, k.off_slot_songs - k.off_offsets, &hb);
    if (rc != VIT_OK) return rc;
    int32_t* h_chunk_base = reinterpret_cast<int32_t*>(hb + (k.off_chunk_base - k.off_offsets));
    int32_t* h_wave_song = reinterpret_cast<int32_t*>(hb + (k.off_wave_song - k.off_offsets));
    int64_t max_chunks;
    if (!(family == kFamStep ? pk_wave_chunk_table(plan, offsets, B, k.max_waves, h_chunk_base, h_wave_song, &max_chunks)
                             : vit::packed_chunk_table(offsets, B, 16 * 64 * (int64_t)plan->n_cus, vit::kLaneMaxChunks, 4 * vit::kBtWarmSparse, true,
                                                       k.max_waves, h_chunk_base, h_wave_song, &max_chunks)))
        return VIT_EINVAL;      // (cannot happen: sum of round(T_b / cf) <= B + N / cf <= B + 16 * 64 n_cus)
    const int n_waves = h_chunk_base[B];
    rc = pk_upload(plan, ws + k.off_offsets, k.tables_bytes, st);
    if (rc != VIT_OK) return rc;
    VIT_TRY(hipMemsetAsync(ws + k.off_cnt, 0, k.off_last - k.off_cnt, st));

    // ---- forward: one wave (wave form) or one workgroup per slot
    fwd_args_packed(a, logE, B, loglik);
    a.hist = reinterpret_cast<float*>(ws + k.off_hist);
    a.last_state = reinterpret_cast<int32_t*>(ws + k.off_last);
    a.hist_rows = 0;
    a.offsets = reinterpret_cast<const int64_t*>(ws + k.off_offsets);
    a.n_slots = (int)k.n_slots;
    a.slot_begin = reinterpret_cast<const int32_t*>(ws + k.off_slot_begin);
    a.slot_songs = reinterpret_cast<const int32_t*>(ws + k.off_slot_songs);
    VIT_TRY(launch_family(family, vit::WgVariant::Packed, a, f16, st));

    // ---- back-trace: one lane (banded plans) or one wave (step plans) per (song, chunk)
    vit::BtArgs b{};
    bt_args_from_plan(plan, b);
    hist_layout_apply(hist_layout(plan, family), b);
    b.aux_frames = family != kFamWave || (a.wave_flags & 4) ? 1 : vit::wave_aux_frames(plan->bp.wave_npl, plan->S, b.n_extras);    // (a full wave history)
    b.hist = reinterpret_cast<const float*>(ws + k.off_hist);
    b.hist_rows = 0;
    b.last_state = reinterpret_cast<const int32_t*>(ws + k.off_last);
    b.lengths = nullptr;
    b.states = states;
    b.states_stride = 0;
    b.entry = reinterpret_cast<int32_t*>(ws + k.off_entry);
    b.B = B;
    b.T = 1;
    b.counters = reinterpret_cast<int32_t*>(ws + k.off_cnt);
    b.mask = reinterpret_cast<uint32_t*>(ws + k.off_mask);
    b.offsets = a.offsets;
    b.wave_song = reinterpret_cast<const int32_t*>(ws + k.off_wave_song);
    b.chunk_base = reinterpret_cast<const int32_t*>(ws + k.off_chunk_base);
    b.n_waves = n_waves;
    b.chunks = (int)max_chunks;
    if (family == kFamStep) {
        b.warm = tuned_warm(plan->tune, vit::kBtWarm);
        b.bt_form = 1;
        return hip_status(vit::launch_backtrace_rows_packed(b, st));
    }
    b.warm = tuned_warm(plan->tune, vit::kBtWarmSparse);
    b.bt_form = 4;
    if (!vit::lane_backtrace_applies(b)) return VIT_EUNSUPPORTED;
    return hip_status(vit::launch_backtrace_lane(b, st));
}

// ---------------------------------------------------------------------------------------------------------------------
// Packed float64-accumulating decode: vit_decode_f64's kernels (f64.hip, their Packed variant) over vit_decode_packed's buffers.  A WORKGROUP
// per forward slot walks its songs back to back; the back-trace runs one wave per (song, chunk) over per-song chunk lists, the scheme
// of the step plans' lazy back-trace above.  The plans served are vit_decode_f64's (f64_applies).
namespace {

// Tables first, the history behind them: the size less the N history rows does not depend on N.
struct F64PkLayout {
    int64_t n_slots, max_waves;
    size_t off_last, off_entry, off_offsets, off_slot_begin, off_slot_songs, off_wave_song, off_chunk_base, off_hist, bytes;
    size_t tables_bytes;      // offsets .. chunk_base: one contiguous upload
};
// n_slots is an upper bound here (it sizes slot_begin): the decode lowers it
F64PkLayout f64_pk_layout(const vit_plan* p, int64_t B, int64_t N) {
    F64PkLayout k;
    k.n_slots = pk_slots(p, B);
    k.max_waves = B + pk_wave_streams(p);            // (pk_wave_chunk_table)
    k.off_last = 0;
    k.off_entry = k.off_last + align256((size_t)B * sizeof(int32_t));
    k.off_offsets = k.off_entry + align256((size_t)k.max_waves * sizeof(int32_t));
    k.off_slot_begin = k.off_offsets + align256((size_t)(B + 1) * sizeof(int64_t));
    k.off_slot_songs = k.off_slot_begin + align256((size_t)(k.n_slots + 1) * sizeof(int32_t));
    k.off_wave_song = k.off_slot_songs + align256((size_t)B * sizeof(int32_t));
    k.off_chunk_base = k.off_wave_song + align256((size_t)k.max_waves * sizeof(int32_t));
    k.off_hist = k.off_chunk_base + align256((size_t)(B + 1) * sizeof(int32_t));
    k.tables_bytes = k.off_hist - k.off_offsets;
    k.bytes = k.off_hist + (size_t)N * (size_t)vit::f64_hist_stride(p->S) * sizeof(double);
    return k;
}

}  // namespace

size_t vit_workspace_bytes_f64_packed(const vit_plan* plan, int64_t B, int64_t total_frames) {
    if (!plan || B < 0 || B > (int64_t)1 << 30 || total_frames < 0 || !f64_applies(plan)) return 0;
    return f64_pk_layout(plan, B, total_frames).bytes;
}

int vit_decode_f64_packed(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, const int64_t* offsets, void* workspace,
                          size_t workspace_bytes, int32_t* states, double* loglik, vit_stream stream) {
    int rc = check_packed(plan, B, offsets, workspace, emis_dtype);
    if (rc != VIT_OK) return rc;
    if (!f64_applies(plan)) return VIT_EUNSUPPORTED;
    int64_t tmax;
    if (!offsets_ok(offsets, B, &tmax)) return VIT_EINVAL;
    const int64_t N = offsets[B];
    if (B == 0) return VIT_OK;
    if (!logE || !states) return VIT_EINVAL;
    F64PkLayout k = f64_pk_layout(plan, B, N);
    if (workspace_bytes < k.bytes) return VIT_EWORKSPACE;
    const bool f16 = emis_dtype == VIT_F16;
    vit::F64Args a{};
    f64_args_from_plan(plan, a);
    // forward slots: min(B, workgroups resident at once, max(1, N / tmax))
    rc = pk_lower_slots(plan, kResF64Packed, f16, [&](int* n) { return vit::f64_forward_resident(a, vit::F64Variant::Packed, f16, n); }, N, tmax,
                        &k.n_slots);
    if (rc != VIT_OK) return rc;
    stamp_erase(plan, workspace);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);

    // ---- host tables in the plan's pinned staging buffer (the previous call's upload must have read it): offsets, forward slots
    // (greedy bins by frames), and the back-trace's chunk table: one wave per (song, chunk), the step plans' rule of vit_decode_packed
    uint8_t* hb;
    rc = pk_stage_common(plan, k.tables_bytes, offsets, B, k.n_slots, k.off_slot_begin - k.off_offsets, k.off_slot_songs - k.off_offsets, &hb);
    if (rc != VIT_OK) return rc;
    int32_t* h_chunk_base = reinterpret_cast<int32_t*>(hb + (k.off_chunk_base - k.off_offsets));
    int64_t max_chunks;
    if (!pk_wave_chunk_table(plan, offsets, B, k.max_waves, h_chunk_base, reinterpret_cast<int32_t*>(hb + (k.off_wave_song - k.off_offsets)), &max_chunks))
        return VIT_EINVAL;      // (cannot happen: see pk_wave_chunk_table)
    const int n_waves = h_chunk_base[B];
    rc = pk_upload(plan, ws + k.off_offsets, k.tables_bytes, st);
    if (rc != VIT_OK) return rc;

    a.logE = logE;
    a.lengths = nullptr;
    a.hist = reinterpret_cast<double*>(ws + k.off_hist);
    a.last_state = reinterpret_cast<int32_t*>(ws + k.off_last);
    a.loglik = loglik;
    a.states = states;
    a.entry = reinterpret_cast<int32_t*>(ws + k.off_entry);
    a.B = B;
    a.T = 1;                      // (unused by the packed kernels: a song's rows come from the offsets)
    a.offsets = reinterpret_cast<const int64_t*>(ws + k.off_offsets);
    a.n_slots = (int)k.n_slots;
    a.slot_begin = reinterpret_cast<const int32_t*>(ws + k.off_slot_begin);
    a.slot_songs = reinterpret_cast<const int32_t*>(ws + k.off_slot_songs);
    a.wave_song = reinterpret_cast<const int32_t*>(ws + k.off_wave_song);
    a.chunk_base = reinterpret_cast<const int32_t*>(ws + k.off_chunk_base);
    a.n_waves = n_waves;
    a.chunks = (int)max_chunks;
    a.warm = tuned_warm(plan->tune, vit::kBtWarm);
    VIT_TRY(vit::launch_f64_forward(a, vit::F64Variant::Packed, f16, st));
    return hip_status(vit::launch_f64_backtrace(a, vit::F64Variant::Packed, st));
}

// ---------------------------------------------------------------------------------------------------------------------
// Packed decode under a workspace budget: vit_decode_packed_checkpointed (wave-form plans) and vit_decode_packed_bounded (every plan
// with a packed decode; wave-form plans run the same code and get the same size) share ONE driver, decode_packed_budgeted.
// Segments are per song: song b has n_b = ceil(T_b / K) of them.  Pass 1 is the packed forward pass (slots walking their song lists)
// that keeps only the row in front of each segment 1 .. n_b - 1, packed into sum (n_b - 1) <= N / K checkpoint rows, and the terminal
// state and log-likelihood per song.  Pass 2 works on (song, segment) UNITS: the units of a song run from its last segment to its
// first, units of different songs are independent, and the host lists the launches up front (vit::packed_ckpt_schedule: up to n_units
// ready units per launch, at most one per song, most segments left first).  A launch resumes the forward kernel from every unit's
// checkpoint row into that unit's rows, sets every unit's length and start state (packed_segment_prep_kernel) and back-traces the
// units, which writes the states at offsets[b] + segment * K.  Exact by construction: the kernels and sums of vit_decode_packed.
// What differs by family (BudgetForm): the wave form runs a WAVEFRONT per slot and per unit (wave.hip WaveHist::PackedCkptPass / PackedSegment, K + 1 rows per
// unit, up to 8 units per CU and launch, the sparse back-trace); plans without it a WORKGROUP
// (banded_floor_forward_kernel / step4s_forward_kernel <.., WgVariant::PackedCkpt>; a.unit_song null = pass 1, set = pass 2).  The floor kernel's unit
// holds K + 2 rows (one in front for the first frame's frame-maximum store, one behind for the frame past the segment), 1 unit per CU
// (W = 128 on twelve waves takes 148 KB of LDS and 3 x 168 registers per SIMD), the sparse back-trace over the workgroup rows; the
// step kernel's K + 1 rows, 2 per CU (62 KB of LDS, seven waves of 128 registers), the lazy kernel's segment form.  Every unit owns
// its rows, so correctness does not depend on how many workgroups are resident; the units per launch are tuning.
namespace {

// the ONE predicate behind vit_workspace_bytes_packed_checkpointed and vit_decode_packed_checkpointed (a size > 0 implies a decode that launches)
bool pc_applies(const vit_plan* p) { return p->bp.ok && p->bp.wave_ok && ck_sparse_applies(p, kFamWave); }
int pc_family(const vit_plan* p) { return pc_applies(p) ? kFamWave : kFamNone; }
// The same behind vit_workspace_bytes_packed_bounded, vit_packed_bounded_units and vit_decode_packed_bounded.  kFamGroup back-traces
// its units with the sparse kernel only: a plan that the lane form alone could back-trace gets kFamNone.
int pb_family(const vit_plan* p) {
    if (p->bp.ok && p->bp.wave_ok) return pc_family(p);
    if (p->bp.ok)
        return vit::floor_pckpt_applies(p->S, p->bp.W, p->bp.floor_ok, p->bp.n_dense) && p->bp.W <= p->S && ck_sparse_applies(p, kFamGroup) ? kFamGroup : kFamNone;
    return step_applies(p) ? kFamStep : kFamNone;
}

// the choices of the budgeted packed decode that depend on the family: data, read at the top of the driver
struct BudgetForm {
    int units_per_cu;         // units per launch: min(B, units_per_cu x CUs)
    int extra_rows;           // rows a unit holds besides its K
    int front_rows;           // of those, in front of the unit's row 0 (BtArgs::hist, FwdArgs::hist point behind them)
};
BudgetForm budget_form(int family) {
    if (family == kFamWave) return {8, 1, 0};
    if (family == kFamGroup) return {1, 2, 1};
    return {2, 1, 0};
}
int64_t pb_units(const vit_plan* p, int family, int64_t B) {
    if (family == kFamNone) return 0;
    const int64_t cap = budget_form(family).units_per_cu * (int64_t)p->n_cus;
    return B < cap ? B : cap;
}

struct PcLayout {
    int64_t K, tmax, units, n_ckpt, n_units, n_slots;
    size_t off_ckpt, off_seg, off_last, off_entry, off_slen, off_slast, off_sbase;
    size_t off_offsets, off_ckpt_base, off_slot_begin, off_slot_songs, off_unit_song, off_unit_seg, bytes;
    size_t tables_bytes;      // offsets .. unit_seg: one contiguous upload
};
// What the layout takes from the kernels that run: the bytes of a history row, the units of one pass-2 launch, the rows a unit holds
// besides its K, and whether pass 1 needs a scratch row per slot behind the checkpoint rows.
struct PcRows {
    size_t row_bytes;
    int64_t n_units;
    int extra_rows;
    bool scratch;
};
PcRows pc_rows(const vit_plan* p, int family, int64_t B) {
    return {(size_t)hist_layout(p, family).SD * sizeof(float), pb_units(p, family, B), budget_form(family).extra_rows, true};
}
// false: bad offsets (offsets_ok), or more units than an int32 counts.  One layout for the three float32 families -- for a wave plan
// vit_workspace_bytes_packed_bounded IS vit_workspace_bytes_packed_checkpointed -- and for the float64 decode (f64_pc_rows).
bool pc_layout(const vit_plan* p, const PcRows& r, int64_t B, const int64_t* offsets, int64_t K, PcLayout& c) {
    if (!offsets_ok(offsets, B, &c.tmax)) return false;
    c.K = K > c.tmax ? c.tmax : K;                             // (a segment longer than every song: one segment per song)
    c.units = vit::packed_ckpt_units(offsets, B, c.K);
    if (c.units < 0 || c.units > 0x7fffffff) return false;
    c.n_ckpt = c.units - B;
    c.n_units = r.n_units;                                     // units per launch: at most one per song
    c.n_slots = pk_slots(p, B);                                // pass 1's slots (an upper bound, as in pk_layout): one scratch row each
    const size_t sd = r.row_bytes;
    c.off_ckpt = 0;                                            // [n_ckpt] checkpoint rows, then (r.scratch) [n_slots] scratch rows
    c.off_seg = align256((size_t)(c.n_ckpt + (r.scratch ? c.n_slots : 0)) * sd);   // [n_units][K + extra_rows] rows of the segments being walked
    c.off_last = c.off_seg + align256((size_t)c.n_units * (size_t)(c.K + r.extra_rows) * sd);
    c.off_entry = c.off_last + align256((size_t)B * sizeof(int32_t));
    c.off_slen = c.off_entry + align256((size_t)c.n_units * vit::kBtMaxChunks * sizeof(int32_t));
    c.off_slast = c.off_slen + align256((size_t)c.n_units * sizeof(int64_t));
    c.off_sbase = c.off_slast + align256((size_t)c.n_units * sizeof(int32_t));
    c.off_offsets = c.off_sbase + align256((size_t)c.n_units * sizeof(int64_t));
    c.off_ckpt_base = c.off_offsets + align256((size_t)(B + 1) * sizeof(int64_t));
    c.off_slot_begin = c.off_ckpt_base + align256((size_t)(B + 1) * sizeof(int64_t));
    c.off_slot_songs = c.off_slot_begin + align256((size_t)(c.n_slots + 1) * sizeof(int32_t));
    c.off_unit_song = c.off_slot_songs + align256((size_t)B * sizeof(int32_t));
    c.off_unit_seg = c.off_unit_song + align256((size_t)c.units * sizeof(int32_t));
    c.bytes = c.off_unit_seg + align256((size_t)c.units * sizeof(int32_t));
    c.tables_bytes = c.bytes - c.off_offsets;
    return true;
}
size_t budgeted_bytes(const vit_plan* plan, int (*family_of)(const vit_plan*), int64_t B, const int64_t* offsets, int64_t segment_frames) {
    if (!plan || !offsets || B < 0 || B > (int64_t)1 << 30 || !ck_segment_ok(segment_frames)) return 0;
    const int family = family_of(plan);
    PcLayout c;
    return family != kFamNone && pc_layout(plan, pc_rows(plan, family, B), B, offsets, segment_frames, c) ? c.bytes : 0;
}

// The host tables of a budgeted packed decode -- offsets, checkpoint bases, pass 1's slots, pass 2's units in launch order (sc) --
// staged in the plan's pinned buffer and sent to the workspace in one upload.
int pc_stage_tables(const vit_plan* plan, const PcLayout& c, const int64_t* offsets, int64_t B, int64_t n_slots, uint8_t* ws, hipStream_t st,
                    vit::PackedCkptSchedule& sc) {
    uint8_t* hb;
    const int rs = pk_stage_common(plan, c.tables_bytes, offsets, B, n_slots, c.off_slot_begin - c.off_offsets, c.off_slot_songs - c.off_offsets, &hb);
    if (rs != VIT_OK) return rs;
    try {
        vit::packed_ckpt_schedule(offsets, B, c.K, c.n_units, sc);
    } catch (const std::bad_alloc&) {
        return VIT_ENOMEM;
    }
    if ((int64_t)sc.unit_song.size() != c.units) return VIT_EINVAL;      // (cannot happen: the layout counted the same segments)
    std::memcpy(hb + (c.off_ckpt_base - c.off_offsets), sc.ckpt_base.data(), (size_t)(B + 1) * sizeof(int64_t));
    std::memcpy(hb + (c.off_unit_song - c.off_offsets), sc.unit_song.data(), (size_t)c.units * sizeof(int32_t));
    std::memcpy(hb + (c.off_unit_seg - c.off_offsets), sc.unit_seg.data(), (size_t)c.units * sizeof(int32_t));
    return pk_upload(plan, ws + c.off_offsets, c.tables_bytes, st);
}

// The driver behind both entry points; family_of is the entry point's predicate (pc_family / pb_family).
int decode_packed_budgeted(const vit_plan* plan, int (*family_of)(const vit_plan*), const void* logE, int emis_dtype, int64_t B,
                           const int64_t* offsets, void* workspace, size_t workspace_bytes, int32_t* states, float* loglik,
                           int64_t segment_frames, vit_stream stream) {
    int rc = check_packed(plan, B, offsets, workspace, emis_dtype);
    if (rc != VIT_OK) return rc;
    if (!ck_segment_ok(segment_frames)) return VIT_EINVAL;
    const int family = family_of(plan);                   // (everything that can refuse the plan is asked here, before anything is enqueued)
    if (family == kFamNone) return VIT_EUNSUPPORTED;
    PcLayout c;
    if (!pc_layout(plan, pc_rows(plan, family, B), B, offsets, segment_frames, c)) return VIT_EINVAL;
    if (B == 0) return VIT_OK;
    if (!logE || !states) return VIT_EINVAL;
    if (workspace_bytes < c.bytes) return VIT_EWORKSPACE;
    const BudgetForm form = budget_form(family);
    const HistLayout lay = hist_layout(plan, family);
    const int64_t N = offsets[B], K = c.K, seg_rows = K + form.extra_rows;
    const bool f16 = emis_dtype == VIT_F16;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    vit::FwdArgs a{};
    fwd_args_from_plan(plan, a);
    int64_t n_slots = c.n_slots;                          // pass 1's slots, as vit_decode_packed chooses them (the packed-checkpoint kernels' occupancy)
    rc = pk_lower_slots(plan, family == kFamWave ? kResNone : kResPackedCkpt, f16,
                        [&](int* n) { return family_resident(family, vit::WgVariant::PackedCkpt, a, f16, n); }, N, c.tmax, &n_slots);
    if (rc != VIT_OK) return rc;
    stamp_erase(plan, workspace);
    vit::PackedCkptSchedule sc;
    rc = pc_stage_tables(plan, c, offsets, B, n_slots, ws, st, sc);
    if (rc != VIT_OK) return rc;

    // ---- pass 1: checkpoint rows + terminal state, one wave / workgroup per slot
    fwd_args_packed(a, logE, B, loglik);
    a.hist = reinterpret_cast<float*>(ws + c.off_ckpt);
    a.last_state = reinterpret_cast<int32_t*>(ws + c.off_last);
    a.hist_rows = c.n_ckpt;       // the scratch row of slot w is row n_ckpt + w
    a.ckpt_every = (int)K;
    a.offsets = reinterpret_cast<const int64_t*>(ws + c.off_offsets);
    a.n_slots = (int)n_slots;
    a.slot_begin = reinterpret_cast<const int32_t*>(ws + c.off_slot_begin);
    a.slot_songs = reinterpret_cast<const int32_t*>(ws + c.off_slot_songs);
    a.ckpt_base = reinterpret_cast<const int64_t*>(ws + c.off_ckpt_base);
    a.unit_song = nullptr;
    VIT_TRY(launch_family(family, vit::WgVariant::PackedCkpt, a, f16, st));

    // ---- pass 2: the launches of the schedule; every unit's back-trace starts from what the launch before it wrote
    float* seg = reinterpret_cast<float*>(ws + c.off_seg) + (size_t)form.front_rows * lay.SD;
    vit::BtArgs b{};
    bt_args_from_plan(plan, b);
    hist_layout_apply(lay, b);
    b.aux_frames = 1;       // (a unit's sub-problem ends one frame behind the rows it decides from: every frame's scalars from its own row)
    b.hist = seg;
    b.hist_rows = seg_rows;
    b.last_state = reinterpret_cast<const int32_t*>(ws + c.off_slast);
    b.lengths = reinterpret_cast<const int64_t*>(ws + c.off_slen);
    b.unit_states = reinterpret_cast<const int64_t*>(ws + c.off_sbase);
    b.entry = reinterpret_cast<int32_t*>(ws + c.off_entry);
    b.states = states;
    b.states_stride = 0;
    b.T = (int)(K + 1);
    b.counters = nullptr;   // no event counts and no chunk flags in pass 2: the layout has no room for them
    b.mask = nullptr;
    b.bt_form = family == kFamStep ? 1 : 0;
    vit::FwdArgs f = a;
    f.hist = seg;
    f.hist_rows = seg_rows;
    f.loglik = nullptr;
    f.init_rows = reinterpret_cast<const float*>(ws + c.off_ckpt);
    const int32_t* d_unit_song = reinterpret_cast<const int32_t*>(ws + c.off_unit_song);
    const int32_t* d_unit_seg = reinterpret_cast<const int32_t*>(ws + c.off_unit_seg);
    for (size_t l = 0; l + 1 < sc.launch_begin.size(); ++l) {
        const int64_t u0 = sc.launch_begin[l], nu = sc.launch_begin[l + 1] - u0;
        if (nu < 1 || nu > c.n_units) return VIT_EINVAL;                  // (cannot happen: the schedule takes at most n_units per launch)
        f.B = nu;
        f.unit_song = d_unit_song + u0;
        f.unit_seg = d_unit_seg + u0;
        VIT_TRY(launch_family(family, vit::WgVariant::PackedCkpt, f, f16, st));
        VIT_TRY(vit::launch_packed_segment_prep(a.offsets, f.unit_song, f.unit_seg, (int)nu, (int)K, states, a.last_state,
                                                reinterpret_cast<int64_t*>(ws + c.off_slen), reinterpret_cast<int32_t*>(ws + c.off_slast),
                                                reinterpret_cast<int64_t*>(ws + c.off_sbase), st));
        b.B = nu;
        VIT_TRY(segment_backtrace(plan, family, false, b, st));
    }
    return VIT_OK;
}

}  // namespace

size_t vit_workspace_bytes_packed_checkpointed(const vit_plan* plan, int64_t B, const int64_t* offsets, int64_t segment_frames) {
    return budgeted_bytes(plan, pc_family, B, offsets, segment_frames);
}

int vit_decode_packed_checkpointed(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, const int64_t* offsets, void* workspace,
                                   size_t workspace_bytes, int32_t* states, float* loglik, int64_t segment_frames, vit_stream stream) {
    return decode_packed_budgeted(plan, pc_family, logE, emis_dtype, B, offsets, workspace, workspace_bytes, states, loglik, segment_frames, stream);
}

int64_t vit_packed_bounded_units(const vit_plan* plan, int64_t B) {
    if (!plan || B < 0 || B > (int64_t)1 << 30) return 0;
    return pb_units(plan, pb_family(plan), B);
}

size_t vit_workspace_bytes_packed_bounded(const vit_plan* plan, int64_t B, const int64_t* offsets, int64_t segment_frames) {
    return budgeted_bytes(plan, pb_family, B, offsets, segment_frames);
}

int vit_decode_packed_bounded(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, const int64_t* offsets, void* workspace,
                              size_t workspace_bytes, int32_t* states, float* loglik, int64_t segment_frames, vit_stream stream) {
    return decode_packed_budgeted(plan, pb_family, logE, emis_dtype, B, offsets, workspace, workspace_bytes, states, loglik, segment_frames, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Packed float64 decode under a workspace budget: the sibling of decode_packed_budgeted with vit_decode_f64's kernels in their PackedCkpt
// variant (f64.hip).  The scheme, the workspace layout (pc_layout over f64_pc_rows), the staged tables (pc_stage_tables) and the unit
// prep (launch_packed_segment_prep) are the float32 driver's; what differs: rows of doubles, K + 1 rows per unit (one in front for M of
// the checkpoint frame; M of the segment's last row is formed behind its last frame, so no frame past the segment is run), no scratch
// row in pass 1 (what is not kept is not stored), the float64 back-trace over the units with f64_segment_chunks chunks each.
namespace {

int f64_pc_units_per_cu(const vit_plan* p) {
    const int u = p->tune.f64_units_per_cu;
    return u >= 1 && u <= 4 ? u : vit::f64_pckpt_units_per_cu(p->bp.W, vit::banded_waves_for(p->S));
}
PcRows f64_pc_rows(const vit_plan* p, int64_t B) {
    const int64_t cap = f64_pc_units_per_cu(p) * (int64_t)p->n_cus;
    return {(size_t)vit::f64_hist_stride(p->S) * sizeof(double), B < cap ? B : cap, 1, false};
}

}  // namespace

int64_t vit_f64_packed_bounded_units(const vit_plan* plan, int64_t B) {
    if (!plan || B < 0 || B > (int64_t)1 << 30 || !f64_applies(plan)) return 0;
    return f64_pc_rows(plan, B).n_units;
}

size_t vit_workspace_bytes_f64_packed_checkpointed(const vit_plan* plan, int64_t B, const int64_t* offsets, int64_t segment_frames) {
    if (!plan || !offsets || B < 0 || B > (int64_t)1 << 30 || !ck_segment_ok(segment_frames) || !f64_applies(plan)) return 0;
    PcLayout c;
    return pc_layout(plan, f64_pc_rows(plan, B), B, offsets, segment_frames, c) ? c.bytes : 0;
}

int vit_decode_f64_packed_checkpointed(const vit_plan* plan, const void* logE, int emis_dtype, int64_t B, const int64_t* offsets, void* workspace,
                                       size_t workspace_bytes, int32_t* states, double* loglik, int64_t segment_frames, vit_stream stream) {
    int rc = check_packed(plan, B, offsets, workspace, emis_dtype);
    if (rc != VIT_OK) return rc;
    if (!ck_segment_ok(segment_frames)) return VIT_EINVAL;
    if (!f64_applies(plan)) return VIT_EUNSUPPORTED;
    PcLayout c;
    if (!pc_layout(plan, f64_pc_rows(plan, B), B, offsets, segment_frames, c)) return VIT_EINVAL;
    if (B == 0) return VIT_OK;
    if (!logE || !states) return VIT_EINVAL;
    if (workspace_bytes < c.bytes) return VIT_EWORKSPACE;
    const int64_t N = offsets[B], K = c.K;
    const bool f16 = emis_dtype == VIT_F16;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    vit::F64Args a{};
    f64_args_from_plan(plan, a);
    int64_t n_slots = c.n_slots;                          // pass 1's slots, as vit_decode_f64_packed chooses them (this variant's occupancy)
    rc = pk_lower_slots(plan, kResF64PackedCkpt, f16, [&](int* n) { return vit::f64_forward_resident(a, vit::F64Variant::PackedCkpt, f16, n); }, N, c.tmax,
                        &n_slots);
    if (rc != VIT_OK) return rc;
    stamp_erase(plan, workspace);
    vit::PackedCkptSchedule sc;
    rc = pc_stage_tables(plan, c, offsets, B, n_slots, ws, st, sc);
    if (rc != VIT_OK) return rc;

    // ---- pass 1: checkpoint rows + terminal state and log-likelihood, one workgroup per slot
    a.logE = logE;
    a.lengths = nullptr;
    a.hist = reinterpret_cast<double*>(ws + c.off_ckpt);
    a.last_state = reinterpret_cast<int32_t*>(ws + c.off_last);
    a.loglik = loglik;
    a.states = states;
    a.entry = reinterpret_cast<int32_t*>(ws + c.off_entry);
    a.B = B;
    a.T = 1;                      // (unused by the packed kernels: a song's rows come from the offsets)
    a.ckpt_every = (int)K;
    a.offsets = reinterpret_cast<const int64_t*>(ws + c.off_offsets);
    a.n_slots = (int)n_slots;
    a.slot_begin = reinterpret_cast<const int32_t*>(ws + c.off_slot_begin);
    a.slot_songs = reinterpret_cast<const int32_t*>(ws + c.off_slot_songs);
    a.ckpt_base = reinterpret_cast<const int64_t*>(ws + c.off_ckpt_base);
    a.unit_song = nullptr;
    VIT_TRY(vit::launch_f64_forward(a, vit::F64Variant::PackedCkpt, f16, st));

    // ---- pass 2: the launches of the schedule; every unit's back-trace starts from what the launch before it wrote
    vit::F64Args f = a;
    f.hist = reinterpret_cast<double*>(ws + c.off_seg) + a.SD64;          // a unit's row 0 is the second of its K + 1 rows
    f.hist_song_stride = (K + 1) * (int64_t)a.SD64;
    f.loglik = nullptr;
    f.init_rows = reinterpret_cast<const double*>(ws + c.off_ckpt);
    f.seg_len = reinterpret_cast<const int64_t*>(ws + c.off_slen);
    f.seg_last = reinterpret_cast<const int32_t*>(ws + c.off_slast);
    f.unit_states = reinterpret_cast<const int64_t*>(ws + c.off_sbase);
    f.warm = tuned_warm(plan->tune, vit::kBtWarmSparse);
    const int32_t* d_unit_song = reinterpret_cast<const int32_t*>(ws + c.off_unit_song);
    const int32_t* d_unit_seg = reinterpret_cast<const int32_t*>(ws + c.off_unit_seg);
    for (size_t l = 0; l + 1 < sc.launch_begin.size(); ++l) {
        const int64_t u0 = sc.launch_begin[l], nu = sc.launch_begin[l + 1] - u0;
        if (nu < 1 || nu > c.n_units) return VIT_EINVAL;                  // (cannot happen: the schedule takes at most n_units per launch)
        f.B = nu;
        f.unit_song = d_unit_song + u0;
        f.unit_seg = d_unit_seg + u0;
        VIT_TRY(vit::launch_f64_forward(f, vit::F64Variant::PackedCkpt, f16, st));
        VIT_TRY(vit::launch_packed_segment_prep(a.offsets, f.unit_song, f.unit_seg, (int)nu, (int)K, states, a.last_state,
                                                reinterpret_cast<int64_t*>(ws + c.off_slen), reinterpret_cast<int32_t*>(ws + c.off_slast),
                                                reinterpret_cast<int64_t*>(ws + c.off_sbase), st));
        f.chunks = tuned_chunks(plan->tune, f64_segment_chunks(nu, (int)(K + 1), f.warm));
        VIT_TRY(vit::launch_f64_backtrace(f, vit::F64Variant::PackedCkpt, st));
    }
    return VIT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused logits -> path decode (fused.hip): the emission builder and the wave-form forward recursion share a workgroup, the
// emission rows cross the CU through LDS and no [B, T, S] emission tensor exists.  Then the ordinary full-history back-trace of
// the wave layout.
namespace {

// the ONE predicate behind vit_workspace_bytes_logits and vit_decode_logits (a size > 0 implies a decode that launches)
bool lg_applies(const vit_plan* p, const vit_obs_params* obs) {
    vit::FwdArgs a{};
    fwd_args_from_plan(p, a);          // (wave_u5 after the "wave_uniform" option)
    return vit::fused_logits_applies(p->S, a.wave_ok, a.wave_npl, a.wave_dk, a.n_extras, a.wave_u5, obs->mode, obs->n_bins, obs->spw);
}

}  // namespace

size_t vit_workspace_bytes_logits(const vit_plan* plan, const vit_obs_params* obs, int64_t B, int64_t T) {
    if (!plan || !obs || B < 0 || T < 1) return 0;
    if (!lg_applies(plan, obs)) return 0;
    return ws_layout_hist(B, (size_t)T, (size_t)hist_layout(plan, kFamWave).SD).bytes;
}

int vit_decode_logits(const vit_plan* plan, const float* logits, const vit_obs_params* obs, int64_t B, int64_t T, const int64_t* lengths,
                      void* workspace, size_t workspace_bytes, float* logE_out, int32_t* states, float* loglik, vit_stream stream) {
    if (!plan || !obs) return VIT_EINVAL;
    if (!plan->dev_image) return VIT_ENOTUPLOADED;
    int rc = check_common(plan, B, T, workspace);
    if (rc != VIT_OK) return rc;
    if (obs->mode < 0 || obs->mode > 2 || obs->n_bins < 2 || (int64_t)obs->n_bins + 1 != plan->S) return VIT_EINVAL;
    if (!lg_applies(plan, obs)) return VIT_EUNSUPPORTED;      // (everything that can refuse the plan or the builder is asked here)
    if (B > 0 && (!logits || !states)) return VIT_EINVAL;
    const WsLayout w = ws_layout_hist(B, (size_t)T, (size_t)hist_layout(plan, kFamWave).SD);
    if (workspace_bytes < w.bytes) return VIT_EWORKSPACE;
    if (B == 0) return VIT_OK;
    stamp_erase(plan, workspace);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    vit::FusedArgs fa{};
    fwd_args_from_plan(plan, fa.f);
    fa.f.logE = nullptr;
    fa.f.lengths = lengths;
    fa.f.hist = reinterpret_cast<float*>(ws + w.off_hist);
    fa.f.fmax = reinterpret_cast<float*>(ws + w.off_fmax);
    fa.f.last_state = reinterpret_cast<int32_t*>(ws + w.off_last);
    fa.f.loglik = loglik;
    fa.f.B = B;
    fa.f.T = (int)T;
    fa.f.hist_half = 0;
    fa.f.hist_rows = T;
    fa.f.t_begin = 0;
    fa.f.t_end = (int)T;
    fa.logits = logits;
    fa.logE_out = logE_out;
    fa.mode = obs->mode;
    fa.n_bins = obs->n_bins;
    fa.spw = obs->spw;
    fa.threshold = obs->threshold_logit;
    fa.offset = obs->mode == 0 ? obs->offset : 0.0;
    fa.scale = obs->mode == 0 ? obs->scale : 0.0;
    fa.prior = obs->mode == 2 ? obs->prior : nullptr;
    hipError_t e = vit::launch_fused_logits(fa, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return VIT_EUNSUPPORTED;     // (cannot happen: lg_applies asked the same predicate)
    VIT_TRY(e);
    // the back-trace of a full wave-layout history, through the record vit_backtrace reads; the record does not outlive the call
    FwdStamp st;
    st.ws = workspace;
    st.B = B;
    st.T = T;
    st.family = kFamWave;
    st.lay = hist_layout(plan, kFamWave);
    st.aux_frames = vit::wave_aux_frames(plan->bp.wave_npl, plan->S, fa.f.n_extras);
    st.half = 0;
    stamp_put(plan, st);
    rc = backtrace_impl(plan, nullptr, 0, false, B, T, lengths, workspace, workspace_bytes, states, stream);
    stamp_erase(plan, workspace);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// The fused decode under a workspace budget: vit_decode_checkpointed's scheme and driver (ck_decode) with the fused workgroup
// (fused_ckpt.hip) as the forward launch of the wave family -- pass 1 builds every emission row once and keeps the checkpoint rows, each
// segment builds its rows again from the logits.  Plans and builders: vit_decode_logits's that the checkpointed decode serves in the
// wave family; the workspace is vit_decode_checkpointed's for the same plan.
namespace {

// the ONE predicate behind vit_workspace_bytes_logits_checkpointed and vit_decode_logits_checkpointed
bool lgck_applies(const vit_plan* p, const vit_obs_params* obs) { return lg_applies(p, obs) && ck_family(p) == kFamWave; }

}  // namespace

size_t vit_workspace_bytes_logits_checkpointed(const vit_plan* plan, const vit_obs_params* obs, int64_t B, int64_t T, int64_t segment_frames) {
    if (!plan || !obs || B < 0 || T < 1 || !ck_segment_ok(segment_frames)) return 0;
    if (!lgck_applies(plan, obs)) return 0;
    return ck_layout(plan, kFamWave, B, T, segment_frames).bytes;
}

int vit_decode_logits_checkpointed(const vit_plan* plan, const float* logits, const vit_obs_params* obs, int64_t B, int64_t T,
                                   const int64_t* lengths, void* workspace, size_t workspace_bytes, int32_t* states, float* loglik,
                                   int64_t segment_frames, vit_stream stream) {
    if (!plan || !obs) return VIT_EINVAL;
    if (!plan->dev_image) return VIT_ENOTUPLOADED;
    int rc = check_common(plan, B, T, workspace);
    if (rc != VIT_OK) return rc;
    if (obs->mode < 0 || obs->mode > 2 || obs->n_bins < 2 || (int64_t)obs->n_bins + 1 != plan->S) return VIT_EINVAL;
    if (!ck_segment_ok(segment_frames)) return VIT_EINVAL;
    if (!lgck_applies(plan, obs)) return VIT_EUNSUPPORTED;    // (everything that can refuse the plan or the builder is asked here)
    if (B > 0 && (!logits || !states)) return VIT_EINVAL;
    const int64_t K = segment_frames > T ? T : segment_frames;
    const CkLayout c = ck_layout(plan, kFamWave, B, T, K);
    if (workspace_bytes < c.bytes) return VIT_EWORKSPACE;
    if (B == 0) return VIT_OK;
    hipStream_t st = (hipStream_t)stream;
    vit::FusedArgs fa{};
    fa.logits = logits;
    fa.logE_out = nullptr;           // (the rows are built twice; the call exists to save memory)
    fa.mode = obs->mode;
    fa.n_bins = obs->n_bins;
    fa.spw = obs->spw;
    fa.threshold = obs->threshold_logit;
    fa.offset = obs->mode == 0 ? obs->offset : 0.0;
    fa.scale = obs->mode == 0 ? obs->scale : 0.0;
    fa.prior = obs->mode == 2 ? obs->prior : nullptr;
    return ck_decode(plan, kFamWave, c, K, nullptr, B, T, lengths, workspace, states, loglik, st, [&](const vit::FwdArgs& f, bool segment) {
        fa.f = f;
        fa.f.hist_half = 0;
        return vit::launch_fused_logits_ckpt(fa, segment, st);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// Streaming decode: a session owns [B, T_cap] history rows in the Plain layout of its workgroup family and advances the forward
// recursion by one chunk of emission rows per vit_stream_append (WgVariant::Stream of the floor and step kernels: the frames
// pos[b] .. pos[b] + counts[b] - 1 of song b, resumed from the song's own row pos[b] - 1).  Nothing reads an emission row twice, so
// the chunk is the caller's again once the append's kernel has run.  vit_stream_backtrace decodes the recordings as they stand, with
// the back-trace launches a checkpointed decode uses per segment (they take the song's row count apart from the frame count): the
// sparse kernel or the lane form for banded plans, the lazy kernel for step plans.  A session always runs the workgroup family.
// A ring session (vit_stream_open_ring) owns [B, R] rows instead, frame t in row t mod R (WgVariant::StreamRing), and
// returns its path by vit_stream_commit_rel and vit_stream_tail; its appends are checked against the acknowledged frontiers (ack).
struct vit_session {
    const vit_plan* plan = nullptr;
    int family = kFamNone;
    int64_t B = 0, T_cap = 0;
    uint8_t* ws = nullptr;
    int dtype = -1;                     // emission type of the first append (-1: none yet)
    std::vector<int64_t> pos;           // frames appended per song
    uint8_t* cws = nullptr;             // the commit state (vit_stream_commit_begin), or null
    bool commit_reset = true;           // the next commit counts every frontier as 0 (after commit_begin / reset: a host flag, nothing enqueued)
    // ring session (vit_stream_open_ring): ring = R > 0 history rows per song, frame t in row t mod R; T_cap = R (st_layout's rows).
    // ack[b] <= the song's frontier on the device: what the caller has reported (vit_stream_commit_ack).  Rows [ack[b], pos[b]) stay resident.
    int64_t ring = 0;
    std::vector<int64_t> ack;
};

namespace {

// The workgroup family a session of this plan runs, kFamNone = none: the ONE predicate behind vit_workspace_bytes_stream and
// vit_stream_open -- what has a Stream instantiation and a back-trace over the rows it writes.
int st_family(const vit_plan* p) {
    if (p->bp.ok)
        return vit::floor_stream_applies(p->S, p->bp.W, p->bp.floor_ok, p->bp.n_dense) && (ck_sparse_applies(p, kFamGroup) || ck_lane_applies(p)) ? kFamGroup : kFamNone;
    return step_applies(p) ? kFamStep : kFamNone;
}

struct StLayout {
    size_t off_hist, off_cnt, off_mask, off_last, off_loglik, off_entry, off_len, off_tab, bytes;
};
StLayout st_layout(const vit_plan* p, int family, int64_t B, int64_t T_cap) {
    StLayout s;
    s.off_hist = 0;                                                               // [B][T_cap] rows
    s.off_cnt = align256((size_t)B * (size_t)T_cap * (size_t)hist_layout(p, family).SD * sizeof(float));
    s.off_mask = s.off_cnt + align256((size_t)B * vit::kBtCounters * sizeof(int32_t));      // the back-trace's counters, then the lane form's chunk flags
    s.off_last = s.off_mask + align256((size_t)B * vit::kLaneMaskWords * sizeof(uint32_t));  // terminal states
    s.off_loglik = s.off_last + align256((size_t)B * sizeof(int32_t));             // log-likelihoods of the lengths so far
    s.off_entry = s.off_loglik + align256((size_t)B * sizeof(float));
    s.off_len = s.off_entry + align256((size_t)B * vit::kLaneMaxChunks * sizeof(int32_t));  // device lengths [B] (written by the back-trace call)
    s.off_tab = s.off_len + align256((size_t)B * sizeof(int64_t));                 // per-launch tables: positions [B], counts [B]
    s.bytes = s.off_tab + align256((size_t)B * 2 * sizeof(int32_t));
    return s;
}
inline bool st_shape_ok(int64_t B, int64_t T_cap) { return B >= 1 && T_cap >= 1 && B <= (int64_t)1 << 30 && T_cap <= (int64_t)1 << 30; }
constexpr int64_t kStMaxFrames = (int64_t)1 << 30;      // frames a recording of a ring session may grow to
constexpr int64_t kStMinRing = 64;
inline bool st_ring_ok(int64_t B, int64_t R) { return st_shape_ok(B, R) && R >= kStMinRing; }

// The commit state of a session (vit_stream_commit): its own caller-owned buffer, so that st_layout stays what it is.  Served: the
// banded session plans whose rows the per-lane decision reads (the lane back-trace's predicate); step plans decide by whole rows.
inline bool sc_served(const vit_plan* p) { return st_family(p) == kFamGroup && ck_lane_applies(p); }
struct ScLayout {
    size_t off_front, off_pos, off_first, off_len, off_last, off_mask, off_entry, bytes;
};
ScLayout sc_layout(int64_t B) {
    ScLayout c;
    c.off_front = 0;                                                              // frames committed so far [B]
    c.off_pos = align256((size_t)B * sizeof(int64_t));                            // per-call table: frames appended so far [B]
    c.off_first = c.off_pos + align256((size_t)B * sizeof(int64_t));              // the committed ranges as sub-problems of the lane back-trace:
    c.off_len = c.off_first + align256((size_t)B * sizeof(int64_t));              //   first rows, lengths,
    c.off_last = c.off_len + align256((size_t)B * sizeof(int64_t));               //   start states,
    c.off_mask = c.off_last + align256((size_t)B * sizeof(int32_t));              //   chunk flags
    c.off_entry = c.off_mask + align256((size_t)B * vit::kLaneMaskWords * sizeof(uint32_t));    // and chunk entries
    c.bytes = c.off_entry + align256((size_t)B * vit::kLaneMaxChunks * sizeof(int32_t));
    return c;
}

}  // namespace

size_t vit_workspace_bytes_stream(const vit_plan* plan, int64_t B, int64_t T_cap) {
    if (!plan || !st_shape_ok(B, T_cap)) return 0;
    const int family = st_family(plan);
    if (family == kFamNone) return 0;
    return st_layout(plan, family, B, T_cap).bytes;
}

namespace {
// vit_stream_open (ring = 0: T_cap rows per song) and vit_stream_open_ring (ring = T_cap = R rows per song): one status order
int st_open(const vit_plan* plan, int64_t B, int64_t T_cap, int64_t ring, void* workspace, size_t workspace_bytes, vit_session** out) {
    if (!plan || !out || !workspace || !(ring ? st_ring_ok(B, ring) : st_shape_ok(B, T_cap)) || ((uintptr_t)workspace & 255) != 0) return VIT_EINVAL;
    if (!plan->dev_image) return VIT_ENOTUPLOADED;
    const int family = ring && !sc_served(plan) ? kFamNone : st_family(plan);     // (a ring advances by commits only)
    if (family == kFamNone) return VIT_EUNSUPPORTED;
    if (workspace_bytes < st_layout(plan, family, B, T_cap).bytes) return VIT_EWORKSPACE;
    vit_session* s = new (std::nothrow) vit_session();
    if (!s) return VIT_ENOMEM;
    try {
        s->pos.assign((size_t)B, 0);
        if (ring) s->ack.assign((size_t)B, 0);
    } catch (const std::bad_alloc&) {
        delete s;
        return VIT_ENOMEM;
    }
    s->plan = plan;
    s->family = family;
    s->B = B;
    s->T_cap = T_cap;
    s->ring = ring;
    s->ws = static_cast<uint8_t*>(workspace);
    stamp_erase(plan, workspace);       // (whatever vit_forward left here is the session's to overwrite)
    *out = s;
    return VIT_OK;
}
}  // namespace

int vit_stream_open(const vit_plan* plan, int64_t B, int64_t T_cap, void* workspace, size_t workspace_bytes, vit_session** out) {
    return st_open(plan, B, T_cap, 0, workspace, workspace_bytes, out);
}

size_t vit_workspace_bytes_stream_ring(const vit_plan* plan, int64_t B, int64_t ring_rows) {
    if (!plan || !st_ring_ok(B, ring_rows) || !sc_served(plan)) return 0;
    return st_layout(plan, st_family(plan), B, ring_rows).bytes;
}

int vit_stream_open_ring(const vit_plan* plan, int64_t B, int64_t ring_rows, void* workspace, size_t workspace_bytes, vit_session** out) {
    if (ring_rows < 1) return VIT_EINVAL;
    return st_open(plan, B, ring_rows, ring_rows, workspace, workspace_bytes, out);
}

int vit_stream_commit_ack(vit_session* s, const int64_t* frontiers) {
    if (!s || !frontiers || !s->ring) return VIT_EINVAL;
    for (int64_t b = 0; b < s->B; ++b)
        if (frontiers[b] < s->ack[(size_t)b] || frontiers[b] > s->pos[(size_t)b]) return VIT_EINVAL;
    std::memcpy(s->ack.data(), frontiers, (size_t)s->B * sizeof(int64_t));
    return VIT_OK;
}

int vit_stream_append(vit_session* s, const void* logE, int emis_dtype, int64_t n, const int64_t* counts, vit_stream stream) {
    if (!s || !logE) return VIT_EINVAL;
    if (emis_dtype != VIT_F32 && emis_dtype != VIT_F16) return VIT_EINVAL;
    if (n < 1 || n > (int64_t)1 << 30) return VIT_EINVAL;
    if (s->dtype >= 0 && s->dtype != emis_dtype) return VIT_EINVAL;
    const vit_plan* plan = s->plan;
    const int64_t B = s->B;
    bool uniform = true;                // every song at the same position, taking the same count: two scalars instead of the tables
    int64_t any = 0;
    bool resident = true;               // (ring) rows [ack, pos + c) of every song fit its R rows
    for (int64_t b = 0; b < B; ++b) {
        const int64_t c = counts ? counts[b] : n;
        if (c < 0 || c > n || s->pos[(size_t)b] + c > (s->ring ? kStMaxFrames : s->T_cap)) return VIT_EINVAL;
        if (s->ring && s->pos[(size_t)b] + c - s->ack[(size_t)b] > s->ring) resident = false;
        uniform = uniform && c == (counts ? counts[0] : n) && s->pos[(size_t)b] == s->pos[0];
        any |= c;
    }
    if (!resident) return VIT_EWORKSPACE;   // (acknowledge newer frontiers, or open with more rows)
    if (any == 0) return VIT_OK;        // (nothing to append)
    hipStream_t st = (hipStream_t)stream;
    const StLayout L = st_layout(plan, s->family, B, s->T_cap);
    vit::FwdArgs a{};
    fwd_args_from_plan(plan, a);
    a.debug = 0;
    a.logE = logE;
    a.lengths = nullptr;
    a.hist = reinterpret_cast<float*>(s->ws + L.off_hist);
    a.fmax = nullptr;
    a.last_state = reinterpret_cast<int32_t*>(s->ws + L.off_last);
    a.loglik = reinterpret_cast<float*>(s->ws + L.off_loglik);
    a.B = B;
    a.T = (int)(s->ring ? kStMaxFrames : s->T_cap);     // (ring: frames are absolute, rows are taken mod hist_rows)
    a.hist_rows = s->T_cap;
    a.init_stride = n * (int64_t)plan->S;
    if (uniform) {
        a.t_begin = (int)s->pos[0];
        a.t_end = (int)(s->pos[0] + (counts ? counts[0] : n));
    } else {
        // the launch's tables through the plan's pinned staging buffer (the upload before must have read it)
        const size_t bytes = (size_t)B * 2 * sizeof(int32_t);
        const int rc = pk_stage(plan, bytes);
        if (rc != VIT_OK) return rc;
        int32_t* h = static_cast<int32_t*>(plan->pk_host);
        for (int64_t b = 0; b < B; ++b) {
            h[b] = (int32_t)s->pos[(size_t)b];
            h[B + b] = (int32_t)(counts ? counts[b] : n);
        }
        const int ru = pk_upload(plan, s->ws + L.off_tab, bytes, st);
        if (ru != VIT_OK) return ru;
        a.unit_song = reinterpret_cast<const int32_t*>(s->ws + L.off_tab);
        a.unit_seg = a.unit_song + B;
    }
    VIT_TRY(launch_family(s->family, s->ring ? vit::WgVariant::StreamRing : vit::WgVariant::Stream, a, emis_dtype == VIT_F16, st));
    for (int64_t b = 0; b < B; ++b) s->pos[(size_t)b] += counts ? counts[b] : n;
    s->dtype = emis_dtype;
    return VIT_OK;
}

int vit_stream_lengths(const vit_session* s, int64_t* lengths) {
    if (!s || !lengths) return VIT_EINVAL;
    std::memcpy(lengths, s->pos.data(), (size_t)s->B * sizeof(int64_t));
    return VIT_OK;
}

int vit_stream_backtrace(vit_session* s, int32_t* states, int64_t states_stride, float* loglik, vit_stream stream) {
    if (!s || !states) return VIT_EINVAL;
    if (s->ring) return VIT_EUNSUPPORTED;                   // (rows below the frontier are gone: vit_stream_commit_rel + vit_stream_tail)
    const vit_plan* plan = s->plan;
    const int64_t B = s->B;
    int64_t tmax = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (s->pos[(size_t)b] < 1) return VIT_EINVAL;       // (a song without a frame has no path)
        tmax = std::max(tmax, s->pos[(size_t)b]);
    }
    if (states_stride < tmax || states_stride > (int64_t)1 << 30) return VIT_EINVAL;
    const Tuning& tn = plan->tune;
    const StLayout L = st_layout(plan, s->family, B, s->T_cap);
    vit::BtArgs b{};
    bt_args_from_plan(plan, b);
    hist_layout_apply(hist_layout(plan, s->family), b);
    b.aux_frames = 1;
    b.hist = reinterpret_cast<const float*>(s->ws + L.off_hist);
    b.hist_rows = s->T_cap;
    b.last_state = reinterpret_cast<const int32_t*>(s->ws + L.off_last);
    b.lengths = reinterpret_cast<const int64_t*>(s->ws + L.off_len);
    b.states = states;
    b.states_stride = states_stride;
    b.entry = reinterpret_cast<int32_t*>(s->ws + L.off_entry);
    b.B = B;
    b.T = (int)tmax;                    // the frames the kernels walk and pad to; the caller's stride beyond: the memset below
    b.skip_nonpositive = 1;             // (the launches of a checkpointed decode's segments: rows by hist_rows, states by states_stride)
    b.counters = reinterpret_cast<int32_t*>(s->ws + L.off_cnt);
    b.mask = s->family == kFamGroup ? reinterpret_cast<uint32_t*>(s->ws + L.off_mask) : nullptr;
    const bool lane_bt = s->family == kFamGroup && (tn.backtrace_form == 4 || !ck_sparse_applies(plan, kFamGroup));
    b.bt_form = s->family == kFamStep ? 1 : (lane_bt ? 4 : 0);
    if (lane_bt && !vit::lane_backtrace_applies(b)) return VIT_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    // the lengths so far through the plan's pinned staging buffer
    const int rc = pk_stage(plan, (size_t)B * sizeof(int64_t));
    if (rc != VIT_OK) return rc;
    std::memcpy(plan->pk_host, s->pos.data(), (size_t)B * sizeof(int64_t));
    const int ru = pk_upload(plan, s->ws + L.off_len, (size_t)B * sizeof(int64_t), st);
    if (ru != VIT_OK) return ru;
    VIT_TRY(hipMemsetAsync(states, 0xff, (size_t)B * (size_t)states_stride * sizeof(int32_t), st));   // -1 behind every length
    VIT_TRY(hipMemsetAsync(s->ws + L.off_cnt, 0, L.off_mask - L.off_cnt, st));                       // the event counters
    VIT_TRY(segment_backtrace(plan, s->family, lane_bt, b, st, true));
    if (loglik) VIT_TRY(hipMemcpyAsync(loglik, s->ws + L.off_loglik, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, st));
    return VIT_OK;
}

int vit_stream_reset(vit_session* s) {
    if (!s) return VIT_EINVAL;
    std::fill(s->pos.begin(), s->pos.end(), (int64_t)0);
    std::fill(s->ack.begin(), s->ack.end(), (int64_t)0);
    s->dtype = -1;
    s->commit_reset = true;
    return VIT_OK;
}

size_t vit_workspace_bytes_stream_commit(const vit_plan* plan, int64_t B) {
    if (!plan || B < 1 || B > (int64_t)1 << 30 || !sc_served(plan)) return 0;
    return sc_layout(B).bytes;
}

int vit_stream_commit_begin(vit_session* s, void* commit_ws, size_t bytes) {
    if (!s || !commit_ws || ((uintptr_t)commit_ws & 255) != 0) return VIT_EINVAL;
    if (!sc_served(s->plan)) return VIT_EUNSUPPORTED;
    if (bytes < sc_layout(s->B).bytes) return VIT_EWORKSPACE;
    s->cws = static_cast<uint8_t*>(commit_ws);
    s->commit_reset = true;
    return VIT_OK;
}

namespace {
// The arguments vit_stream_commit, vit_stream_commit_rel and vit_stream_tail share: the merge kernel's (c) over the session's rows and
// commit state, and the lane back-trace's (b) over the sub-problems c.sub_* name.  rel: the states of a sub-problem start at its song's
// states_stride row, not at its first frame.  rows = the frames a sub-problem can hold: the chunk count's and the kernels' limit.
int sc_args(vit_session* s, int32_t* states, int64_t states_stride, int64_t rows, bool rel, vit::CommitArgs& c, vit::BtArgs& b) {
    const vit_plan* plan = s->plan;
    const int64_t B = s->B;
    const StLayout L = st_layout(plan, s->family, B, s->T_cap);
    const ScLayout C = sc_layout(B);
    bt_args_from_plan(plan, c.b);
    hist_layout_apply(hist_layout(plan, s->family), c.b);
    c.b.aux_frames = 1;
    c.b.hist = reinterpret_cast<const float*>(s->ws + L.off_hist);
    c.b.hist_rows = s->T_cap;
    c.b.states = states;
    c.b.states_stride = states_stride;
    c.b.B = B;
    c.b.T = (int)rows;
    c.pos = reinterpret_cast<const int64_t*>(s->cws + C.off_pos);
    c.frontier = reinterpret_cast<int64_t*>(s->cws + C.off_front);
    c.sub_first = reinterpret_cast<int64_t*>(s->cws + C.off_first);
    c.sub_len = reinterpret_cast<int64_t*>(s->cws + C.off_len);
    c.sub_last = reinterpret_cast<int32_t*>(s->cws + C.off_last);
    c.reset = s->commit_reset ? 1 : 0;
    if (!vit::stream_commit_applies(c.b)) return VIT_EUNSUPPORTED;
    // the ranges as sub-problems of the lane back-trace: first rows, lengths and start states stay on the device (a length of 0 is
    // skipped); the chunk count is that of the longest range there can be, the host knows no range
    b = c.b;
    b.first_row = c.sub_first;
    b.lengths = c.sub_len;
    b.last_state = c.sub_last;
    b.skip_nonpositive = 1;
    b.counters = nullptr;
    b.mask = reinterpret_cast<uint32_t*>(s->cws + C.off_mask);
    b.entry = reinterpret_cast<int32_t*>(s->cws + C.off_entry);
    b.bt_form = 4;
    b.ring_rows = s->ring;
    b.states_rel = rel ? 1 : 0;
    if (!vit::lane_backtrace_applies(b)) return VIT_EUNSUPPORTED;
    return VIT_OK;
}
// the lengths so far through the plan's pinned staging buffer: the call's only upload
int sc_upload_pos(vit_session* s, hipStream_t st) {
    const vit_plan* plan = s->plan;
    const size_t bytes = (size_t)s->B * sizeof(int64_t);
    const int rc = pk_stage(plan, bytes);
    if (rc != VIT_OK) return rc;
    std::memcpy(plan->pk_host, s->pos.data(), bytes);
    return pk_upload(plan, s->cws + sc_layout(s->B).off_pos, bytes, st);
}
inline int64_t sc_tmax(const vit_session* s) {
    int64_t tmax = 0;
    for (int64_t b = 0; b < s->B; ++b) tmax = std::max(tmax, s->pos[(size_t)b]);
    return tmax;
}

int sc_commit(vit_session* s, int32_t* states, int64_t states_stride, int64_t* first, int64_t* committed, int64_t max_lookback, bool rel,
              vit_stream stream) {
    if (!s || !states || !committed || (rel && !first) || max_lookback < 1 || max_lookback > (int64_t)1 << 30) return VIT_EINVAL;
    if (!s->cws) return VIT_EINVAL;
    if (s->ring && !rel) return VIT_EUNSUPPORTED;           // (absolute output over a ring: the stride would be the recording's length)
    const int64_t tmax = sc_tmax(s);
    const int64_t rows = s->ring ? std::min(tmax, s->ring) : tmax;      // the longest range: the resident rows
    if (states_stride < rows || states_stride > (int64_t)1 << 30) return VIT_EINVAL;
    vit::CommitArgs c{};
    vit::BtArgs b{};
    const int ra = sc_args(s, states, states_stride, rows, rel, c, b);
    if (ra != VIT_OK) return ra;
    c.committed = committed;
    c.first = rel ? first : nullptr;
    c.max_lookback = max_lookback;
    hipStream_t st = (hipStream_t)stream;
    const int ru = sc_upload_pos(s, st);
    if (ru != VIT_OK) return ru;
    VIT_TRY(vit::launch_stream_commit(c, st));
    s->commit_reset = false;
    if (tmax >= 2) VIT_TRY(segment_backtrace(s->plan, s->family, true, b, st));
    return VIT_OK;
}
}  // namespace

int vit_stream_commit(vit_session* s, int32_t* states, int64_t states_stride, int64_t* committed, int64_t max_lookback, vit_stream stream) {
    return sc_commit(s, states, states_stride, nullptr, committed, max_lookback, false, stream);
}

int vit_stream_commit_rel(vit_session* s, int32_t* states, int64_t states_stride, int64_t* first, int64_t* committed, int64_t max_lookback,
                          vit_stream stream) {
    return sc_commit(s, states, states_stride, first, committed, max_lookback, true, stream);
}

int vit_stream_tail(vit_session* s, int32_t* states, int64_t states_stride, int64_t* first, float* loglik, vit_stream stream) {
    if (!s || !states || !first) return VIT_EINVAL;
    if (!s->cws) return VIT_EINVAL;
    for (int64_t b = 0; b < s->B; ++b)
        if (s->pos[(size_t)b] < 1) return VIT_EINVAL;       // (a song without a frame has no path)
    const int64_t tmax = sc_tmax(s);
    const int64_t rows = s->ring ? std::min(tmax, s->ring) : tmax;      // the longest tail there can be
    if (states_stride < rows || states_stride > (int64_t)1 << 30) return VIT_EINVAL;
    vit::CommitArgs c{};
    vit::BtArgs b{};
    const int ra = sc_args(s, states, states_stride, rows, true, c, b);
    if (ra != VIT_OK) return ra;
    c.first = first;
    hipStream_t st = (hipStream_t)stream;
    const int ru = sc_upload_pos(s, st);
    if (ru != VIT_OK) return ru;
    const StLayout L = st_layout(s->plan, s->family, s->B, s->T_cap);
    VIT_TRY(vit::launch_stream_tail_prep(c, reinterpret_cast<const int32_t*>(s->ws + L.off_last), st));
    VIT_TRY(segment_backtrace(s->plan, s->family, true, b, st));
    if (loglik) VIT_TRY(hipMemcpyAsync(loglik, s->ws + L.off_loglik, (size_t)s->B * sizeof(float), hipMemcpyDeviceToDevice, st));
    return VIT_OK;
}

void vit_stream_close(vit_session* s) { delete s; }

int vit_voicing_map(const int32_t* states, int64_t n, int32_t n_bins, uint8_t* voiced, int32_t* bins,
                    vit_stream stream) {
    if (n < 0 || n_bins < 1 || (n > 0 && (!states || !voiced || !bins))) return VIT_EINVAL;
    return hip_status(vit::launch_voicing_map(states, n, n_bins, voiced, bins, (hipStream_t)stream));
}

int vit_obs_shaun(const float* logits, int64_t n_frames, int32_t n_bins, int32_t spw, double threshold_logit,
                  double offset, double scale, float* logE, vit_stream stream) {
    if (n_frames < 0 || n_bins < 2 || (n_frames > 0 && (!logits || !logE))) return VIT_EINVAL;
    hipError_t e = vit::launch_obs_shaun(logits, n_frames, n_bins, spw, threshold_logit, offset, scale, logE, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return VIT_EUNSUPPORTED;
    return hip_status(e);
}

int vit_obs_softmax(const float* logits, int64_t n_frames, int32_t n_bins, int32_t spw, float* logE, vit_stream stream) {
    if (n_frames < 0 || n_bins < 2 || (n_frames > 0 && (!logits || !logE))) return VIT_EINVAL;
    hipError_t e = vit::launch_obs_softmax(logits, n_frames, n_bins, spw, logE, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return VIT_EUNSUPPORTED;
    return hip_status(e);
}

int vit_obs_softmax_scaled(const float* logits, int64_t n_frames, int32_t n_bins, int32_t spw, double unvoiced_logit,
                           const float* prior, float* logE, vit_stream stream) {
    if (n_frames < 0 || n_bins < 2 || (n_frames > 0 && (!logits || !logE))) return VIT_EINVAL;
    hipError_t e = vit::launch_obs_softmax_scaled(logits, n_frames, n_bins, spw, unvoiced_logit, prior, logE, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return VIT_EUNSUPPORTED;
    return hip_status(e);
}

int vit_obs_build(const vit_obs_params* obs, const void* logits, int logits_dtype, int64_t n_frames, void* logE, int emis_dtype,
                  vit_stream stream) {
    if (!obs || obs->mode < 0 || obs->mode > 2) return VIT_EINVAL;
    if ((logits_dtype != VIT_F32 && logits_dtype != VIT_F16) || (emis_dtype != VIT_F32 && emis_dtype != VIT_F16)) return VIT_EINVAL;
    if (logits_dtype == VIT_F32 && emis_dtype == VIT_F32) {              // the float32 entry points themselves
        const float* x = static_cast<const float*>(logits);
        float* o = static_cast<float*>(logE);
        if (obs->mode == 0) return vit_obs_shaun(x, n_frames, obs->n_bins, obs->spw, obs->threshold_logit, obs->offset, obs->scale, o, stream);
        if (obs->mode == 1) return vit_obs_softmax(x, n_frames, obs->n_bins, obs->spw, o, stream);
        return vit_obs_softmax_scaled(x, n_frames, obs->n_bins, obs->spw, obs->threshold_logit, obs->prior, o, stream);
    }
    if (n_frames < 0 || obs->n_bins < 2 || (n_frames > 0 && (!logits || !logE))) return VIT_EINVAL;
    if (n_frames == 0) return VIT_OK;
    hipError_t e = vit::launch_obs_half(obs->mode, logits, logits_dtype == VIT_F16, n_frames, obs->n_bins, obs->spw, obs->threshold_logit,
                                        obs->offset, obs->scale, obs->mode == 2 ? obs->prior : nullptr, logE, emis_dtype == VIT_F16,
                                        (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return VIT_EUNSUPPORTED;
    return hip_status(e);
}

int vit_snippets_append_f16(const void* snippets, int32_t n_snippets, int32_t n_channels, int32_t n_frames, int32_t mode,
                            float* rows_out, int64_t n_rows, vit_stream stream) {
    if (n_snippets < 0 || n_channels < 2 || n_frames < 1 || (mode != 0 && mode != 1) || n_rows < 0 ||
        n_rows > (int64_t)n_snippets * n_frames || (n_rows > 0 && (!snippets || !rows_out)))
        return VIT_EINVAL;
    return hip_status(vit::launch_snippets_append_f16(snippets, n_snippets, n_channels, n_frames, mode, rows_out, n_rows, (hipStream_t)stream));
}

int vit_obs_activations(const float* hf0, int64_t ld, int32_t n_bins, int64_t B, const int64_t* offsets_dev, int64_t total_frames,
                        float clamp_below, float clamp_to, float* stats, void* logE, int out_dtype, vit_stream stream) {
    if (!hf0 || !offsets_dev || !stats || !logE) return VIT_EINVAL;
    if (n_bins < 1 || n_bins > 1023 || B < 1 || B > (int64_t)1 << 30 || total_frames < B || total_frames > (int64_t)1 << 36) return VIT_EINVAL;
    if (ld < total_frames) return VIT_EINVAL;
    if (out_dtype != VIT_F32 && out_dtype != VIT_F16) return VIT_EINVAL;
    uint32_t below_bits;
    memcpy(&below_bits, &clamp_below, sizeof(below_bits));
    return hip_status(vit::launch_activations(hf0, ld, n_bins, (int)B, offsets_dev, total_frames, below_bits, clamp_to, stats, logE,
                                           out_dtype == VIT_F16, (hipStream_t)stream));
}

int vit_snippets_append(const float* snippets, int32_t n_snippets, int32_t n_channels, int32_t n_frames, int32_t mode,
                        float* rows_out, int64_t n_rows, vit_stream stream) {
    if (n_snippets < 0 || n_channels < 2 || n_frames < 1 || (mode != 0 && mode != 1) || n_rows < 0 ||
        n_rows > (int64_t)n_snippets * n_frames || (n_rows > 0 && (!snippets || !rows_out)))
        return VIT_EINVAL;
    return hip_status(vit::launch_snippets_append(snippets, n_snippets, n_channels, n_frames, mode, rows_out, n_rows, (hipStream_t)stream));
}

int vit_voicing_notes(const int32_t* states, int64_t n, int32_t n_bins, const float* note_range, uint8_t* voiced,
                      int32_t* bins, float* notes, float* notes_voiced, vit_stream stream) {
    if (n < 0 || n_bins < 1 || (n > 0 && (!states || !note_range))) return VIT_EINVAL;
    return hip_status(vit::launch_voicing_notes(states, n, n_bins, note_range, voiced, bins, notes, notes_voiced, (hipStream_t)stream));
}

/* DPP scan self-test used by tests/test_gpu_parity.py */
int vit_debug_scan(const float* vals, int n_waves, int mode, float* out_v, int32_t* out_i, vit_stream stream) {
    if (!vals || !out_v || !out_i || n_waves < 1) return VIT_EINVAL;
    return hip_status(vit::launch_scan_selftest(vals, n_waves, mode, out_v, out_i, (hipStream_t)stream));
}

}  // extern "C"
