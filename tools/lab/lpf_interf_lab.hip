// Lab: what slows the low-pass loop when other waves of its workgroup work.  The product's low-pass loop
// (SDRG_LPF_LOOP_IL_ASM, csrc/ssb_lpf_asm.h) runs on wave 1 (SIMD 1) as in lpf_loop_lab.hip; the chosen other waves
// ("busy" mask) execute one kind of instruction per chunk between the same per-chunk barriers, ~384 per chunk (about
// what the DC / AGC waves issue):
//   valu  384 v_fma_f32 on four interleaved chains, straight-line     (VALU issue, 8-byte encodings)
//   pk    384 v_pk_fma_f32, straight-line                              (the low-pass loop's own op)
//   vloop the same 384 v_fma_f32 as a 96-iteration loop of 4           (same VALU, small code)
//   salu  384 s_add_u32, straight-line                                 (scalar issue, no VALU)
//   nop   384 s_nop 0, straight-line                                   (instruction fetch + issue only)
//   lds   96 ds_read_b32 + waits                                       (LDS only)
// If VALU forms slow the chain and salu / nop do not, the interference is in the VALU side; if nop does too, it is
// instruction fetch / issue arbitration; lds isolates the shared LDS.  s_memtime cycles per sample, the minimum of 5
// launches after a warm-up, one workgroup per CU (grid 256).
// Build: hipcc --offload-arch=gfx950 -O3 -I sdr-for-android-lib_amd/csrc -o tools/lab/lpf_interf_lab tools/lab/lpf_interf_lab.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "ssb_lpf_asm.h"

typedef float f2v __attribute__((ext_vector_type(2)));
constexpr int SLOT_F = 16 * 68;
constexpr int NCH = 256;
constexpr int CW = 1;  // the chain's wave (hardware wave w runs on SIMD w mod 4)

template <int B>
__device__ __forceinline__ void busy_body(float &a0, float &a1, float &a2, float &a3, f2v &p0, f2v &p1, uint32_t laddr) {
    const float c = 0.999f;
    if constexpr (B == 1) {
        asm volatile(".rept 96\n v_fma_f32 %0, %0, %4, %4\n v_fma_f32 %1, %1, %4, %4\n v_fma_f32 %2, %2, %4, %4\n"
                     " v_fma_f32 %3, %3, %4, %4\n.endr"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
                     : "v"(c));
    } else if constexpr (B == 2) {
        const f2v cc = {0.999f, 0.998f};
        asm volatile(".rept 192\n v_pk_fma_f32 %0, %0, %2, %2\n v_pk_fma_f32 %1, %1, %2, %2\n.endr"
                     : "+v"(p0), "+v"(p1)
                     : "v"(cc));
    } else if constexpr (B == 3) {
        for (int j = 0; j < 96; j++)
            asm volatile("v_fma_f32 %0, %0, %4, %4\n v_fma_f32 %1, %1, %4, %4\n v_fma_f32 %2, %2, %4, %4\n"
                         " v_fma_f32 %3, %3, %4, %4"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
                         : "v"(c));
    } else if constexpr (B == 4) {
        uint32_t s0 = 1, s1 = 2;
        asm volatile(".rept 192\n s_add_u32 %0, %0, 3\n s_add_u32 %1, %1, 5\n.endr" : "+s"(s0), "+s"(s1)::"scc");
        if (s0 == 7 && s1 == 9) a0 += 1.0f;
    } else if constexpr (B == 5) {
        asm volatile(".rept 384\n s_nop 0\n.endr" ::: "memory");
    } else if constexpr (B == 6) {
        float t;
        asm volatile(".rept 96\n ds_read_b32 %0, %1\n.endr\n s_waitcnt lgkmcnt(0)" : "=&v"(t) : "v"(laddr) : "memory");
        a0 += t;
    }
}

template <int B>
__global__ __launch_bounds__(768) void k(unsigned long long *out, int bmask) {
    __shared__ __attribute__((aligned(16))) float lds[7 * SLOT_F];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 7 * SLOT_F; i += 768) lds[i] = 1e-3f * (i % 97);
    __syncthreads();
    const int nit = NCH + 9;
    if (wave != CW) {
        const bool busy = (bmask >> wave) & 1;
        float a0 = lane, a1 = lane + 1, a2 = lane + 2, a3 = lane + 3;
        f2v p0 = {a0, a1}, p1 = {a2, a3};
        const uint32_t laddr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)&lds[6 * SLOT_F + lane];
        for (int r = 0; r < nit; r++) {
            if (busy) busy_body<B>(a0, a1, a2, a3, p0, p1, laddr);
            asm volatile("s_waitcnt lgkmcnt(0)\n s_barrier" ::: "memory");
        }
        if (a0 + a1 + a2 + a3 + p0.x + p1.y == 12345.0f) out[1] = 2;
        return;
    }
    __builtin_amdgcn_s_setprio(3);
    const int s = lane & 15;
    const uint32_t abase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)&lds[s * 68];
    const uint32_t ybase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)&lds[3 * SLOT_F + s * 68];
    const f2v c1 = {1.9f, -0.9f}, c2 = {0.01f, -0.005f};
    f2v z = {0.0f, 0.0f};
    unsigned long long sv;
    unsigned long long t_ret;
    int t_it, t_cc, t_yo;
    const int nch = NCH;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if (lane < 16) {
        asm volatile(SDRG_LPF_LOOP_IL_ASM
                     : [z] "+v"(z), [sv] "=&s"(sv), [it] "=&s"(t_it), [cc] "=&s"(t_cc), [ret] "=&s"(t_ret), [yo] "=&s"(t_yo)
                     : [abase] "v"(abase), [ybase] "v"(ybase), [c1] "s"(c1), [c2] "s"(c2), [nit] "s"(nit), [nch] "s"(nch)
                     : SDRG_CHUNK_CLOBBERS, "v54", "memory");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) out[blockIdx.x] = t1 - t0;
    if (lane == 0 && z.x == 12345.0f) out[1] = 1;
}

template <int B>
void run(const char *name, unsigned long long *d, int bmask, const char *set) {
    const int grid = 256;
    unsigned long long best = ~0ull;
    static unsigned long long h[256];
    for (int r = 0; r < 8; r++) {
        k<B><<<grid, 768>>>(d, bmask);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d, 8 * grid, hipMemcpyDeviceToHost) != hipSuccess) return;
        double mean = 0;
        for (int g = 0; g < grid; g++) mean += (double)h[g] / grid;
        if (r >= 3 && mean < best) best = (unsigned long long)mean;
    }
    printf("%-6s busy %-28s mask 0x%03x: %6.2f cyc/sample (%llu cycles per %d chunks)\n", name, set, bmask,
           best / (double)(NCH * 64), best, NCH);
    fflush(stdout);
}

__global__ void warm(float *x, int n) {  // a few ms of work so the clocks settle
    float a = x[threadIdx.x];
    for (int i = 0; i < n; i++) a = a * 1.0000001f + 1e-7f;
    x[threadIdx.x] = a;
}

template <int B>
void sets(const char *name, unsigned long long *d) {
    run<B>(name, d, 0x005, "waves 0,2 (SIMD 0,2)");
    run<B>(name, d, 0x220, "waves 5,9 (SIMD 1, chain's)");
    run<B>(name, d, 0xFFD, "all other 11");
}

int main() {
    unsigned long long *d;
    float *w;
    if (hipMalloc(&d, 8 * 256) != hipSuccess || hipMalloc(&w, 4096) != hipSuccess) return 2;
    hipLaunchKernelGGL(warm, dim3(1024), dim3(256), 0, 0, w, 1 << 18);
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    run<0>("none", d, 0, "-");
    sets<1>("valu", d);
    sets<2>("pk", d);
    sets<3>("vloop", d);
    sets<4>("salu", d);
    sets<5>("nop", d);
    sets<6>("lds", d);
    run<0>("none", d, 0, "-");
    return 0;
}
