// banded_stream_ring.hip -- the ring instantiations of the one-target floor kernel (banded_floor_forward_kernel<.., WgVariant::StreamRing>,
// vit_stream_append on a session of vit_stream_open_ring): the pairs of banded_stream.hip, float32 and float16 rows.  A translation unit of
// its own beside banded_stream.hip, whose kernels keep their code: a linear session never pays for the row cursor.
#include "device_common.hpp"

namespace vit {

#include "banded_floor.inc"

hipError_t floor_stream_ring(const FwdArgs& a, bool f16, hipStream_t st, int* per_cu) {
    return f16 ? floor_variant_e<__half, WgVariant::StreamRing>(a, st, per_cu) : floor_variant_e<float, WgVariant::StreamRing>(a, st, per_cu);
}

}  // namespace vit
