// Micro-benchmark: what the full waves' copy writes cost at the end of a split floor frame (banded_floor_split_forward_kernel), and
// whether ds_write_addtid_b32 (address = M0[15:0] + 16-bit offset + 4 * lane, no address VGPR) shortens that stretch.
// One workgroup of eight waves per CU, no HBM traffic inside the loop.  Per iteration ("frame"):
//   waves 0-3: four dword stores of one VGPR into the four shifted copies of the frame's write buffer (the kernel's addresses:
//              copy 0 entry 4 + tid, copy c another c * DC - c floats on, buffers alternate), one ds_max_f32 into a slot,
//              s_waitcnt lgkmcnt(0), s_barrier
//   waves 4-7: straight to s_barrier
//   all waves: one ds_read_b128 behind the barrier, waited for, its first float folded into the VGPR the next frame stores
//              (so that a frame is one dependent chain, as in the kernel)
// Variants: A ds_write_b32 | B ds_write_addtid_b32, M0 set once in front of the loop | each again with the four stores removed.
// Reported: cycles per iteration (s_memtime around the loop, the slowest wave of all workgroups), five runs per variant, alternated.
// Build: hipcc --offload-arch=gfx950 -O3 -o lds_store_tail lds_store_tail.hip ; run: ./lds_store_tail [workgroups]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

// FloorSplitLds in floats: 384 state slots, copy stride DC, two buffers of four copies, four slot groups of 64 floats behind them
constexpr int DC = 384 + 16, BUF = 4 * DC, FMG = 2 * BUF, END = FMG + 4 * 64;
constexpr int copy_off(int c) { return c * DC - c; }
constexpr int kLdsBytes = 128 * 1024;   // more than half a CU's LDS: one workgroup per CU
static_assert(4 * (BUF + copy_off(3)) < 65536 && 4 * END < 65536, "16-bit offsets and bases");

#define STR_(x) #x
#define STR(x) STR_(x)
// byte offset of copy c in buffer b, as an assembler expression of constants
#define OFFB(b, c) "(4*(" STR(b) "*1600+" STR(c) "*400-" STR(c) "))"
static_assert(BUF == 1600 && DC == 400, "OFFB spells the layout out");

template <bool ADDTID, bool STORES>
__global__ void __launch_bounds__(512) k(float* out, unsigned long long* cyc, int iters) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* lds = reinterpret_cast<float*>(smem);
    for (int i = threadIdx.x; i < END; i += blockDim.x) lds[i] = 0.f;
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool full = wv < 4;
    const int j = full ? tid : 256 + 32 * (wv - 4) + (lane & 31);
    // 32-bit LDS addresses, taken from the shared pointer
    const unsigned lbase = (unsigned)(unsigned long)(__attribute__((address_space(3))) float*)lds;
    const unsigned waddr = lbase + 4u * (4 + j);                          // own entry of copy 0, buffer 0
    const unsigned m0base = lbase + 4u * (4 + 64 * wv);                   // the same without the lane
    const unsigned slot = lbase + 4u * (FMG + 4 * (lane & 3) + ((lane >> 2) & 3));
    const unsigned raddr = lbase + 4u * (4 + ((j & 3) * DC + (j & ~3)));  // an aligned window quad in copy j & 3
    float v = (float)tid;
    f32x4 r;
    if (ADDTID) asm volatile("s_mov_b32 m0, %0" ::"s"(m0base) : "memory");
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if (full) {
        for (int it = 0; it < iters; it += 2) {
#define FRAME(WB, RB)                                                                                                              \
    if (STORES && ADDTID)                                                                                                          \
        asm volatile("ds_write_addtid_b32 %0 offset:" OFFB(WB, 0) "\n\tds_write_addtid_b32 %0 offset:" OFFB(WB, 1) "\n\t"           \
                     "ds_write_addtid_b32 %0 offset:" OFFB(WB, 2) "\n\tds_write_addtid_b32 %0 offset:" OFFB(WB, 3)                 \
                     ::"v"(v) : "memory");                                                                                         \
    else if (STORES)                                                                                                               \
        asm volatile("ds_write_b32 %1, %0 offset:" OFFB(WB, 0) "\n\tds_write_b32 %1, %0 offset:" OFFB(WB, 1) "\n\t"               \
                     "ds_write_b32 %1, %0 offset:" OFFB(WB, 2) "\n\tds_write_b32 %1, %0 offset:" OFFB(WB, 3)                       \
                     ::"v"(v), "v"(waddr) : "memory");                                                                             \
    asm volatile("ds_max_f32 %2, %1\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n\t"                                                       \
                 "ds_read_b128 %0, %3 offset:" OFFB(RB, 0) "\n\ts_waitcnt lgkmcnt(0)"                                              \
                 : "=&v"(r) : "v"(v), "v"(slot), "v"(raddr) : "memory");                                                           \
    v = fmaxf(v, r.x);
            FRAME(1, 0)
            FRAME(0, 1)
        }
    } else {
        for (int it = 0; it < iters; it += 2) {
#define HFRAME(RB)                                                                                                                 \
    asm volatile("s_barrier\n\tds_read_b128 %0, %1 offset:" OFFB(RB, 0) "\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(raddr) : "memory"); \
    v = fmaxf(v, r.x);
            HFRAME(0)
            HFRAME(1)
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * blockDim.x + tid] = v;
    if (lane == 0) cyc[blockIdx.x * 8 + wv] = t1 - t0;
}

template <bool ADDTID, bool STORES>
double run(int wgs, int iters, float* out, unsigned long long* cyc) {
    static bool attr = (hipFuncSetAttribute(reinterpret_cast<const void*>(k<ADDTID, STORES>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes), true);
    (void)attr;
    hipLaunchKernelGGL((k<ADDTID, STORES>), dim3(wgs), dim3(512), kLdsBytes, 0, out, cyc, iters);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed: %s\n", hipGetErrorString(hipGetLastError())); exit(1); }
    std::vector<unsigned long long> h(8 * wgs);
    hipMemcpy(h.data(), cyc, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost);
    return (double)*std::max_element(h.begin(), h.end()) / iters;
}

int main(int argc, char** argv) {
    const int wgs = argc > 1 ? atoi(argv[1]) : 128, iters = 4000, runs = 5;
    float* out; unsigned long long* cyc;
    hipMalloc(&out, (size_t)wgs * 512 * sizeof(float));
    hipMalloc(&cyc, (size_t)wgs * 8 * sizeof(unsigned long long));
    const char* name[4] = {"A  ds_write_b32", "B  ds_write_addtid_b32", "A' no copy stores", "B' no copy stores, M0 set"};
    double c[4][runs];
    run<false, true>(wgs, iters, out, cyc);   // warm-up
    for (int r = 0; r < runs; ++r) {
        c[0][r] = run<false, true>(wgs, iters, out, cyc);
        c[1][r] = run<true, true>(wgs, iters, out, cyc);
        c[2][r] = run<false, false>(wgs, iters, out, cyc);
        c[3][r] = run<true, false>(wgs, iters, out, cyc);
    }
    printf("%d workgroups of 8 waves, %d iterations, cycles per iteration (slowest wave), %d runs alternated\n", wgs, iters, runs);
    for (int v = 0; v < 4; ++v) {
        printf("%-28s:", name[v]);
        for (int r = 0; r < runs; ++r) printf(" %7.2f", c[v][r]);
        printf("   min %7.2f max %7.2f spread %5.2f\n", *std::min_element(c[v], c[v] + runs), *std::max_element(c[v], c[v] + runs),
               *std::max_element(c[v], c[v] + runs) - *std::min_element(c[v], c[v] + runs));
    }
    const double amin = *std::min_element(c[0], c[0] + runs), amax = *std::max_element(c[0], c[0] + runs);
    const double bmax = *std::max_element(c[1], c[1] + runs);
    printf("A - B (ranges): %.2f .. ; B max %.2f %s A min %.2f, A spread %.2f\n", amin - bmax, bmax, bmax < amin ? "<" : ">=", amin, amax - amin);
    hipFree(out); hipFree(cyc);
    return 0;
}
