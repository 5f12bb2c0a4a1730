// wave_terminal.inc -- terminal state of the wave form: lowest-index argmax of delta over the wave, valid in lane 63 (bv, bi).
// Included as text by wave.hip and fused.hip (see wave_frame_body.inc).  In scope: NPL, d, j0.
        float bv = -INFINITY;
        int bi = kBig;
#pragma unroll
        for (int k = 0; k < NPL; ++k)
            if (j0 + k >= 0 && (d[k] > bv || bi == kBig)) { bv = d[k]; bi = j0 + k; }   // first state of the lane, then strictly greater
        // lanes ascend with the state index: an ordered (value, index) scan keeps the first maximum
#define VIT_WSTEP(CTRL, MASK)                                                                                      \
    {                                                                                                              \
        const float sv = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(bv), CTRL, MASK, 0xf, false)); \
        const int si = __builtin_amdgcn_update_dpp(kBig, bi, CTRL, MASK, 0xf, false);                               \
        const bool keep_earlier = !(bv > sv);   /* op_fwd: the later piece wins only if strictly greater */ \
        bv = keep_earlier ? sv : bv;                                                                               \
        bi = keep_earlier ? si : bi;                                                                               \
    }
        VIT_WSTEP(0x111, 0xf)
        VIT_WSTEP(0x112, 0xf)
        VIT_WSTEP(0x114, 0xf)
        VIT_WSTEP(0x118, 0xf)
        VIT_WSTEP(0x142, 0xa)
        VIT_WSTEP(0x143, 0xc)
#undef VIT_WSTEP
