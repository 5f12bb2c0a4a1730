// banded_stream.hip -- the stream instantiations of the one-target floor kernel (banded_floor_forward_kernel<.., WgVariant::Stream>,
// vit_stream_append for banded plans): every (W, NWT) pair of the packed variant, float32 and float16 rows.  A translation unit of its
// own, like banded_pc.hip: banded.hip is the longest compile of the library, and these instantiations build beside it.
#include "device_common.hpp"

namespace vit {

#include "banded_floor.inc"

hipError_t floor_stream(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu) {
    return f16 ? floor_variant_e<__half, WgVariant::Stream>(a, st, per_cu) : floor_variant_e<float, WgVariant::Stream>(a, st, per_cu);
}

}  // namespace vit
