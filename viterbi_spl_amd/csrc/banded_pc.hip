// banded_pc.hip -- the packed-checkpoint instantiations of the one-target floor kernel (banded_floor_forward_kernel<.., PC = true>,
// vit_decode_packed_bounded for banded plans without the wave form).  A translation unit of its own: banded.hip is the longest compile
// of the library, and these instantiations build beside it.
#include "device_common.hpp"

namespace vit {

#include "banded_floor.inc"

// One workgroup per slot (pass 1, a.unit_song null) or per unit (a.unit_song set).  NXT, PF and the LDS size are those of the packed
// and checkpoint / resume variants.  With `per_cu` the launch is replaced by the occupancy query of that instantiation.
template <int W, int NWT, typename ET>
static hipError_t pckpt_floor_t(const FwdArgs& a, hipStream_t st, int* per_cu) {
    constexpr int NP = NWT * 64;
    constexpr int PF = W <= 32 ? 12 : 4;
    const size_t ldsf = sizeof(float) * (8 * (NP + 16) + kFmGroups * kFmGroupFloats) + sizeof(VI) * 16 +
                        ((W == 128 && NWT > 8) ? sizeof(f32x4) * 10 * NP : 0);      // (88 register-resident weights, 40 in LDS)
    const int groups = a.unit_song ? (int)a.B : a.n_slots;
    auto go = [&](auto kern) -> hipError_t {
        if (per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, NWT * 64, ldsf);
        hipLaunchKernelGGL(kern, dim3(groups), dim3(NWT * 64), ldsf, st, a);
        return hipGetLastError();
    };
    if ((W == 32 || W >= 84) && a.n_extras == 1)
        return go(banded_floor_forward_kernel<W, NWT, ((W == 32 || W >= 84) ? 1 : -1), PF, ET, false, false, false, true>);
    return go(banded_floor_forward_kernel<W, NWT, -1, PF, ET, false, false, false, true>);
}

template <int W, typename ET>
static hipError_t pckpt_floor_w(const FwdArgs& a, hipStream_t st, int* per_cu) {
    if (!floor_pckpt_applies(a.S, a.W, a.floor_ok != 0, a.n_dense)) return hipErrorInvalidConfiguration;
    switch (banded_waves_for(a.S)) {
        case 2: if constexpr (floor_ckpt_pair(W, 2)) return pckpt_floor_t<W, 2, ET>(a, st, per_cu); break;
        case 4: if constexpr (floor_ckpt_pair(W, 4)) return pckpt_floor_t<W, 4, ET>(a, st, per_cu); break;
        case 6: if constexpr (floor_ckpt_pair(W, 6)) return pckpt_floor_t<W, 6, ET>(a, st, per_cu); break;
        case 8: if constexpr (floor_ckpt_pair(W, 8)) return pckpt_floor_t<W, 8, ET>(a, st, per_cu); break;
        case 12: if constexpr (floor_ckpt_pair(W, 12)) return pckpt_floor_t<W, 12, ET>(a, st, per_cu); break;
        default: break;
    }
    return hipErrorInvalidConfiguration;
}

template <typename ET>
static hipError_t pckpt_floor_e(const FwdArgs& a, hipStream_t st, int* per_cu) {
    static_assert(sizeof(kBandedWidths) / sizeof(int) == 6, "one case per instantiated window width");
    switch (a.W) {
        case 16: return pckpt_floor_w<16, ET>(a, st, per_cu);
        case 32: return pckpt_floor_w<32, ET>(a, st, per_cu);
        case 64: return pckpt_floor_w<64, ET>(a, st, per_cu);
        case 84: return pckpt_floor_w<84, ET>(a, st, per_cu);
        case 96: return pckpt_floor_w<96, ET>(a, st, per_cu);
        case 128: return pckpt_floor_w<128, ET>(a, st, per_cu);
        default: return hipErrorInvalidConfiguration;
    }
}

hipError_t launch_banded_pckpt(const FwdArgs& a, bool f16, hipStream_t st) {
    if (!a.offsets || !a.ckpt_base || a.ckpt_every < 1 || a.hist_rows < 0) return hipErrorInvalidValue;
    if (a.unit_song ? (!a.unit_seg || !a.init_rows || a.B < 1 || a.hist_rows < (int64_t)a.ckpt_every + 2)
                    : (!a.slot_begin || !a.slot_songs || a.n_slots < 1))
        return hipErrorInvalidValue;
    return f16 ? pckpt_floor_e<__half>(a, st, nullptr) : pckpt_floor_e<float>(a, st, nullptr);
}

hipError_t banded_pckpt_resident(const FwdArgs& a, bool f16, int* per_cu) {
    return f16 ? pckpt_floor_e<__half>(a, nullptr, per_cu) : pckpt_floor_e<float>(a, nullptr, per_cu);
}

}  // namespace vit
