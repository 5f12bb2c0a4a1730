// emission_half.hip -- the emission builders and the snippet hand-off of emission.hip with float16 storage on either side
// (vit_obs_build, vit_snippets_append_f16): float32 logits -> float16 emissions, float16 logits -> float32 emissions, float16 -> float16,
// for every geometry launch_obs serves, by the same form and under the same grid caps.  The kernels are obs_kernels.inc, the text
// emission.hip compiles for float32 -> float32; a translation unit of their own keeps that one's device code what it was.
//
// Contract (bitwise): float16 logits are widened exactly at the load, the frame is worked on in float32 by the
// statements of the float32 builder, and a float16 emission is the float32 one rounded to nearest even at the store (subnormals kept;
// the emission range [-87.34, ~+9] cannot overflow) -- what torch's .float() / .half() do around the float32 builder.
#include "device_common.hpp"
#include "obs_frame.hpp"

namespace vit {

#include "obs_kernels.inc"

namespace {

template <typename LT, typename ET>
hipError_t launch_obs_mode(int mode, const void* logits, int64_t n_frames, int U, int spw, double thr, double off, double sc,
                           const float* prior, void* out, hipStream_t st) {
    const LT* x = static_cast<const LT*>(logits);
    ET* o = static_cast<ET*>(out);
    if (mode == 0) return launch_obs<0>(x, n_frames, U, spw, thr, off, sc, nullptr, o, st);
    if (mode == 1) return launch_obs<1>(x, n_frames, U, spw, 0.0, 0.0, 0.0, nullptr, o, st);
    return launch_obs<2>(x, n_frames, U, spw, thr, 0.0, 0.0, prior, o, st);
}

}  // namespace

// mode 0 / 1 / 2 = launch_obs_shaun / _softmax / _softmax_scaled (thr: the threshold logit / unused / the unvoiced logit); at least one
// of l16 (float16 logits) and e16 (float16 emissions) is set -- float32 -> float32 is emission.hip's
hipError_t launch_obs_half(int mode, const void* logits, bool l16, int64_t n_frames, int U, int spw, double thr, double off, double sc,
                           const float* prior, void* out, bool e16, hipStream_t st) {
    if (mode < 0 || mode > 2 || (!l16 && !e16)) return hipErrorInvalidValue;
    if (l16 && e16) return launch_obs_mode<__half, __half>(mode, logits, n_frames, U, spw, thr, off, sc, prior, out, st);
    if (l16) return launch_obs_mode<__half, float>(mode, logits, n_frames, U, spw, thr, off, sc, prior, out, st);
    return launch_obs_mode<float, __half>(mode, logits, n_frames, U, spw, thr, off, sc, prior, out, st);
}

hipError_t launch_snippets_append_f16(const void* snips, int n, int C, int F, int mode, float* out, int64_t rows, hipStream_t st) {
    if (n <= 0 || rows <= 0) return hipSuccess;
    const int cols = mode == 0 ? C - 1 : C;
    hipLaunchKernelGGL(snippets_append_kernel<__half>, dim3((F + 63) / 64, (cols + 63) / 64, n), dim3(256), 0, st,
                       static_cast<const __half*>(snips), n, C, F, mode, out, rows);
    return hipGetLastError();
}

}  // namespace vit
