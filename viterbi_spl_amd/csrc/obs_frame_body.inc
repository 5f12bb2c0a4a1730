// obs_frame_body.inc -- one frame of the register-form emission builders, included as TEXT inside the frame lambda of
// observation_reg_kernel (emission.hip) and of fused_logits_kernel (fused.hip): the same statements, hence the same lane grouping of
// the sums and the same roundings, and emission.hip compiles to the code it compiled to before (DESIGN.md 4.8).  In scope at the
// point of inclusion: NPL, SPW, MODE, H, NA (constants); a[NA] with a[SPW + k] = this lane's logits; x0f (MODE 1: the row's unvoiced
// logit); real / never / first / rprior (per-lane geometry); threshold, offset, scale.  Leaves v[NPL] = the lane's log observation
// probabilities and `last` = the probability of the unvoiced state (before MODE 2's prior scaling).
        // ---- neighbours: a[SPW - d] = bin NPL*lane - d lives in lane - ceil(d / NPL); shifted copies chained; a lane without a source
        //      keeps -inf (the DPP `old` operand)
        {
            float sl[NPL], sr[NPL];
#pragma unroll
            for (int k = 0; k < NPL; ++k) { sl[k] = a[SPW + k]; sr[k] = a[SPW + k]; }
#pragma unroll
            for (int h = 1; h <= H; ++h) {
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const int dl = h * NPL - k;               // sl[k] after h shifts = bin NPL*(lane-h) + k = own start - dl
                    if (dl <= SPW) { sl[k] = wave_shift_up(sl[k], -INFINITY); a[SPW - dl] = sl[k]; }      // (a slot that is out of reach at h stays out of reach)
                    const int dr = (h - 1) * NPL + k;         // sr[k] after h shifts = bin NPL*(lane+h) + k = own end + 1 + dr
                    if (dr < SPW) { sr[k] = wave_shift_down(sr[k], -INFINITY); a[SPW + NPL + dr] = sr[k]; }
                }
            }
        }
        // ---- peaks: the FIRST maximum of its window: c > max(left SPW) and c >= max(right SPW)
        bool pk[NPL];
        float lmax = -INFINITY;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            float ml = a[k], mr = a[SPW + k + 1];
#pragma unroll
            for (int j = 1; j + 1 < SPW; j += 2) { ml = fmaxf(fmaxf(ml, a[k + j]), a[k + j + 1]); mr = fmaxf(fmaxf(mr, a[SPW + k + 1 + j]), a[SPW + k + 2 + j]); }
            if (SPW % 2 == 0) { ml = fmaxf(ml, a[k + SPW - 1]); mr = fmaxf(mr, a[2 * SPW + k]); }
            const float c = a[SPW + k];
            const bool std_pk = c > ml && c >= mr, first_pk = c > mr;
            pk[k] = real[k] && !never[k] && (first[k] ? first_pk : std_pk);
            lmax = pk[k] ? fmaxf(lmax, c) : lmax;
        }
        const float x0 = MODE == 1 ? x0f : (MODE == 2 ? (float)threshold : -INFINITY);     // the unvoiced logit (always in the peak set)
        float g = wave_max_all(lmax);
        const bool any_peak = g > -INFINITY;
        if (MODE >= 1) g = fmaxf(g, x0);
        float ex[NPL];
        float lsum = 0.f, e0 = 0.f;
        // (e^-1000 = 0: a select on the argument, no branch around the exp.)  A peak or unvoiced logit more than 80 nats below the top
        // may have a subnormal e^x (below -87.3, which v_exp_f32 flushes) or e^x / tot (tot <= U + 1 <= e^6.65): such a frame (rare on
        // real logits) takes ob_exp_far and true divisions, the branch is wave-uniform
        bool far = MODE >= 1 && x0 - g < -80.f;
#pragma unroll
        for (int k = 0; k < NPL; ++k) far = far || (pk[k] && a[SPW + k] - g < -80.f);
        const bool far_frame = __ballot(far) != 0;
        if (far_frame) {
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                ex[k] = ob_exp_far(pk[k] ? a[SPW + k] - g : -1000.f);
                lsum += ex[k];
            }
            if (MODE >= 1) e0 = ob_exp_far(x0 - g);
        } else {
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                ex[k] = ob_exp(pk[k] ? a[SPW + k] - g : -1000.f);
                lsum += ex[k];
            }
            if (MODE >= 1) e0 = ob_exp(x0 - g);
        }
        float tot = ob_wave_sum(lsum);
        float last;                                      // probability of the unvoiced state
        float v[NPL];
        if (MODE == 0) {
            // soft voicing on the strongest peak (tonet/for_paper.py:1703-1712, :1757-1764) in float64 exactly like the reference:
            // 1 - expit(s) is formed by subtraction there, so for s > ~37 the unvoiced probability is EXACTLY 0 (-> log tiny) and below
            // that it carries the float64 cancellation noise of the reference (2e-5 relative at 1 - pv = 6e-12); a float32 expit(-s)
            // would be more accurate and would not be the reference's number
            double pv = 0.0;
            if (any_peak) {
                const double gd = (double)g;
                const double s_ = gd >= threshold ? scale * (gd - threshold) + offset : scale * (gd - threshold) - offset;
                if (s_ > 0) pv = 1.0 / (1.0 + exp(-s_));
                else { const double q = exp(s_); pv = q / (1.0 + q); }
            }
            const double t = any_peak ? pv / (double)tot : 0.0;
            last = any_peak ? (float)(1.0 - pv) : 1.f;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                float lg = ob_log((float)((double)ex[k] * t) + kTiny);
                asm volatile("" : "+v"(lg));                          // (evaluate, then select: no branch per slot)
                v[k] = pk[k] ? lg : kLogTiny;
            }
        } else {
            tot += e0;
            auto emit = [&](const int k, float pr) {
                if (MODE == 2) pr *= rprior[k];
                float lg = ob_log(pr + kTiny);
                asm volatile("" : "+v"(lg));                          // (evaluate, then select: no branch per slot)
                v[k] = pk[k] ? lg : kLogTiny;
            };
            if (far_frame) {
                // e^x / tot may be subnormal, where a product with 1 / tot can round to a neighbouring multiple of 2^-149 (tens of %
                // at a few units) and MODE 2's prior scaling lifts that error into the normal range: divide, as the reference does
                last = any_peak ? e0 / tot : 1.f;
#pragma unroll
                for (int k = 0; k < NPL; ++k) emit(k, ex[k] / tot);
            } else {
                const float tf = 1.f / tot;
                last = any_peak ? e0 * tf : 1.f;
#pragma unroll
                for (int k = 0; k < NPL; ++k) emit(k, ex[k] * tf);
            }
        }
