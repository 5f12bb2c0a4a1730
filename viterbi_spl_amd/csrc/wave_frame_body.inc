// wave_frame_body.inc -- the arithmetic of one frame of the wave form (one song per wavefront), included as TEXT inside the frame
// lambda of wave_forward_kernel (wave.hip) and of fused_logits_kernel (fused.hip), so that both kernels hold the same statements
// and wave.hip compiles to the code it compiled to before the fused kernel existed (a __forceinline__ template gave the same values
// and different register allocation: DESIGN.md 4.8).  In scope at the point of inclusion: NPL, D, NX, H, NG, NPM, U5, U3 (constants);
// d (delta, replaced), M, xd (the previous frame's scalars), e (this frame's emission values), aw, cj, xa (per-lane weights).
        // ---- neighbourhood: group g holds delta of lane l - H + g.  The bound_ctrl shifts deliver 0 to the lane without a
        //      source -- any finite value would do: the sources that lane stands for do not exist (state < 0 or >= S) and
        //      their window weights are -inf (plan.cpp), so the candidate is -inf whatever the shift delivers.
        float nb[NG][NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) nb[H][k] = d[k];
#pragma unroll
        for (int s = 1; s <= H; ++s)
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                nb[H - s][k] = dpp_shr1(nb[H - s + 1][k]);
                nb[H + s][k] = dpp_shl1(nb[H + s - 1][k]);
            }
        auto NB = [&](const int p) -> float { return p < NG * NPL ? nb[p / NPL][p % NPL] : -INFINITY; };
        // ---- window candidates: D+1 packed adds and max3 per own state, walked source pair by source pair from the
        //      lane's own group outwards (the order the shifts deliver them) so that consecutive instructions belong to
        //      different states: independent chains, no wait state between a packed add and the max3 that reads it
        float acc[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) acc[k] = -INFINITY;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const int g = gi == 0 ? H : (gi & 1 ? H - (gi + 1) / 2 : H + gi / 2);
#pragma unroll
            for (int pp = (g * NPL) / 2; 2 * pp < (g + 1) * NPL + 1; ++pp) {
                const int p = 2 * pp;
                if (p / NPL != g && !(NPL % 2 && (p + 1) / NPL == g && p / NPL == g - 1 && false)) continue;
                f32x2 c[NPL];
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const int p0 = wave_p0e(NPL, D, k);
                    if (p >= p0 && p < p0 + 2 * NPM) c[k] = f32x2{NB(p), NB(p + 1)} + aw[k][(p - p0) / 2];
                }
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const int p0 = wave_p0e(NPL, D, k);
                    if (p >= p0 && p < p0 + 2 * NPM) acc[k] = fmaxf(fmaxf(acc[k], c[k].x), c[k].y);
                }
            }
        }
        // ---- floor term, extra columns, emission
        if (U5) {
            const float ya = fmaxf(M + cj[0], xd[0] + xa[0][0]), yb = fmaxf(M + cj[NPL - 1], xd[0] + xa[0][NPL - 1]);
#pragma unroll
            for (int k = 0; k < NPL; ++k) d[k] = fmaxf(acc[k], k < NPL - 1 ? ya : yb) + e[k];
        } else if (U3) {
            const float ya = fmaxf(M + cj[0], xd[0] + xa[0][0]), yb = fmaxf(M + cj[3], xd[0] + xa[0][3]);
            const float yc = fmaxf(M + cj[NPL - 1], xd[0] + xa[0][NPL - 1]);
#pragma unroll
            for (int k = 0; k < NPL; ++k) d[k] = fmaxf(acc[k], k < 3 ? ya : (k < NPL - 1 ? yb : yc)) + e[k];
        } else {
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                float m = fmaxf(acc[k], M + cj[k]);
#pragma unroll
                for (int x = 0; x < NX; ++x) m = fmaxf(m, xd[x] + xa[x][k]);
                d[k] = m + e[k];
            }
        }
