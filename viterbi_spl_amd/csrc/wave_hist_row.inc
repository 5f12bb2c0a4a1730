// wave_hist_row.inc -- history row t of the wave form in slot order, included as TEXT inside the store_hist lambdas of wave.hip and
// fused.hip (as an inlined helper it changed kernels: profiles/README.md).  In scope: NPL, NX, A3 (constants), d (delta_t), lane, l0a, M, xd
// (the scalars of frame t), Mp, xp (frame t-1), Mq, xq (frame t-2).  Declares v: delta, with lane 0's leading slots (always idle: o > NX is
// checked by the plan) carrying M_t and delta_t of the extra columns -- one cache line for the back-trace -- and A3: frames t-1, t-2.
        float v[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) v[k] = d[k];
        v[0] = lane == 0 ? M : v[0];
#pragma unroll
        for (int x = 0; x < NX; ++x) v[1 + x] = lane == 0 ? xd[x] : v[1 + x];
        if (A3) {
            v[2] = l0a ? Mp : v[2];
            v[3] = l0a ? xp[0] : v[3];
            v[4] = l0a ? Mq : v[4];
            v[5] = l0a ? xq : v[5];
        }
