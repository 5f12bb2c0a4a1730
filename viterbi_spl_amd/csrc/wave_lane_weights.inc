// wave_lane_weights.inc -- the window weights of the wave form, included as TEXT by wave_forward_kernel (wave.hip) and by the consumer
// waves of fused_logits_kernel (fused.hip): as an inlined helper the load changed the register allocation of the wave kernels
// (profiles/README.md).  In scope: NPL, NPM (constants), a (FwdArgs), lane.  Declares aw: NPM source pairs for each of the lane's NPL
// states.  The row constants and extra-column weights stay with each kernel: wave.hip loads NX columns and, in the same scope, the
// lanes and slots that own them; fused.hip loads one column and the prior.
    f32x2 aw[NPL][NPM];
    {
        const float* __restrict__ tv = reinterpret_cast<const float*>(a.image + a.off_tabV);
#pragma unroll
        for (int k = 0; k < NPL; ++k)
#pragma unroll
            for (int m = 0; m < NPM; ++m) {
                aw[k][m].x = tv[(((size_t)k * NPM + m) * 2 + 0) * 64 + lane];
                aw[k][m].y = tv[(((size_t)k * NPM + m) * 2 + 1) * 64 + lane];
            }
    }
