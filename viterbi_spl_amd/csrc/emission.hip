// emission.hip -- GPU emission builders: pitch logits -> log observation probabilities, the step right
// upstream of the Viterbi decoder.  In the reference these are Python loops over
// the frames of a song on the host:
//   Viterbi.observation_probs_fn          tonet/for_paper.py:1733-1778  (+ find_peaks :1714-1731, expit :1703-1712)
//   SoftMaxViterbi.observation_probs_fn   tonet/for_paper.py:1911-1944  (+ find_peaks :1890-1909)
//   SoftMaxViterbi.observation_probs_fn   dcnet/softmax_viterbi.py:2530-2579  ("scaled likelihood": p / prior, unvoiced
//                                         logit = the voicing-threshold logit; values may exceed 1)
// followed by log(p + tiny) in viterbi_librosa_fn (:1846-1847).  Here one wave builds one frame and
// writes log(p + tiny) directly in the [frames, n_bins+1] layout vit_decode() reads.
//
// Parity: peak picking and the voicing decision are exact (compares; the voicing logit in float64 like
// the reference); exp/log/sum are the GPU's, so probabilities agree to a few ulp, not bit for bit
// (tests compare with a tolerance and require the structural zeros -> log(tiny) to be exact).
#include "device_common.hpp"
#include "obs_frame.hpp"

namespace vit {

// the builder kernels (observation_kernel: the LDS form, observation_reg_kernel: the register form) and their launch table launch_obs:
// shared as text with emission_half.hip, which holds the float16 instantiations; here float32 logits -> float32 emissions
#include "obs_kernels.inc"

hipError_t launch_obs_shaun(const float* logits, int64_t n_frames, int U, int spw, double thr, double off, double sc,
                            float* out, hipStream_t st) {
    return launch_obs<0>(logits, n_frames, U, spw, thr, off, sc, nullptr, out, st);
}
hipError_t launch_obs_softmax(const float* logits, int64_t n_frames, int U, int spw, float* out, hipStream_t st) {
    return launch_obs<1>(logits, n_frames, U, spw, 0.0, 0.0, 0.0, nullptr, out, st);
}
hipError_t launch_obs_softmax_scaled(const float* logits, int64_t n_frames, int U, int spw, double unvoiced_logit,
                                     const float* prior, float* out, hipStream_t st) {
    return launch_obs<2>(logits, n_frames, U, spw, unvoiced_logit, 0.0, 0.0, prior, out, st);
}

hipError_t launch_snippets_append(const float* snips, int n, int C, int F, int mode, float* out, int64_t rows, hipStream_t st) {
    if (n <= 0 || rows <= 0) return hipSuccess;
    const int cols = mode == 0 ? C - 1 : C;
    hipLaunchKernelGGL(snippets_append_kernel<float>, dim3((F + 63) / 64, (cols + 63) / 64, n), dim3(256), 0, st, snips, n, C, F, mode, out, rows);
    return hipGetLastError();
}

// voiced = state < n_bins; bins = min(state, n_bins-1); notes = note_range[bins]; notes_v = voiced ? notes : 0
// (tonet/for_paper.py:1828-1829, :2106-2115 est_notes_360_fn, :2207)
__global__ void voicing_notes_kernel(const int32_t* __restrict__ states, int64_t n, int32_t n_bins,
                                     const float* __restrict__ note_range, uint8_t* __restrict__ voiced,
                                     int32_t* __restrict__ bins, float* __restrict__ notes, float* __restrict__ notes_v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = states[i];
        const bool v = s >= 0 && s < n_bins;
        const int32_t b = s < 0 ? -1 : (s < n_bins - 1 ? s : n_bins - 1);
        const float nt = b >= 0 ? note_range[b] : 0.f;
        if (voiced) voiced[i] = v ? 1 : 0;
        if (bins) bins[i] = b;
        if (notes) notes[i] = nt;
        if (notes_v) notes_v[i] = v ? nt : 0.f;
    }
}

hipError_t launch_voicing_notes(const int32_t* states, int64_t n, int32_t n_bins, const float* note_range, uint8_t* voiced,
                                int32_t* bins, float* notes, float* notes_v, hipStream_t st) {
    if (n == 0) return hipSuccess;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(voicing_notes_kernel, dim3((int)blocks), dim3(256), 0, st, states, n, n_bins, note_range, voiced, bins, notes, notes_v);
    return hipGetLastError();
}

// voiced = state < n_bins; bins = min(state, n_bins-1)  (tonet/for_paper.py:1828-1829)
__global__ void voicing_map_kernel(const int32_t* __restrict__ states, int64_t n, int32_t n_bins,
                                   uint8_t* __restrict__ voiced, int32_t* __restrict__ bins) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = states[i];
        voiced[i] = (s >= 0 && s < n_bins) ? 1 : 0;
        bins[i] = s < 0 ? -1 : (s < n_bins - 1 ? s : n_bins - 1);
    }
}

hipError_t launch_voicing_map(const int32_t* states, int64_t n, int32_t n_bins, uint8_t* voiced, int32_t* bins,
                              hipStream_t st) {
    if (n == 0) return hipSuccess;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(voicing_map_kernel, dim3((int)blocks), dim3(256), 0, st, states, n, n_bins, voiced, bins);
    return hipGetLastError();
}

}  // namespace vit
