// banded_pc.hip -- the packed-checkpoint instantiations of the one-target floor kernel (banded_floor_forward_kernel<.., WgVariant::PackedCkpt>,
// vit_decode_packed_bounded for banded plans without the wave form).  A translation unit of its own: banded.hip is the longest compile
// of the library, and these instantiations build beside it.
#include "device_common.hpp"

namespace vit {

#include "banded_floor.inc"

hipError_t floor_pckpt(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu) {
    return f16 ? floor_variant_e<__half, WgVariant::PackedCkpt>(a, st, per_cu) : floor_variant_e<float, WgVariant::PackedCkpt>(a, st, per_cu);
}

}  // namespace vit
