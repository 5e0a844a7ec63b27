// quotient_probe.hip -- the two facts DevMathF's three-operation quotient (csrc/dev_math.inc) rests on, established on the
// device that runs it.  A stand-alone program (no libtrmc.so):
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/quotient_probe.hip -o tools/_bin/quotient_probe
//     tools/_bin/quotient_probe rcp          the significands whose refined reciprocal is not the correctly rounded one
//     tools/_bin/quotient_probe pairs [N]    quot(a, b, refined_rcp(b)) against a / b for ALL 2**23 x 2**23 pairs of
//                                            significands (a, b in [1, 2): every quotient of two normal floats whose
//                                            scaling helpers are the identity is one of these times a power of two);
//                                            N: only the first N of 64 slices of the numerators (default all)
// Both restate refined_rcp / quot as they stand in dev_math.inc; tests/test_gpu_quotient.py checks the library's own.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define TRY(x)                                                                                       \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) {                                                                      \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                             \
            return 2;                                                                                \
        }                                                                                            \
    } while (0)

constexpr int kCap = 4096; // mismatches kept (all are counted)

__device__ __forceinline__ float refined_rcp(float b)
{
    const float y0 = __builtin_amdgcn_rcpf(b);
    return __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0);
}
__device__ __forceinline__ float quot(float a, float b, float y1)
{
    const float q0 = a * y1;
    return __builtin_fmaf(__builtin_fmaf(-b, q0, a), y1, q0);
}

// one thread per significand of b at the biased exponent `ebits`
__global__ void __launch_bounds__(256) k_rcp(uint32_t ebits, unsigned long long *count, uint32_t *sig)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x; // grid = 2**23 / 256 blocks exactly
    const float b = __uint_as_float((ebits << 23) | s);
    const float want = (float)(1.0 / (double)b); // exact: fp64 carries more than 2*24 + 2 bits
    if (__float_as_uint(refined_rcp(b)) != __float_as_uint(want)) {
        const unsigned long long at = atomicAdd(count, 1ull);
        if (at < (unsigned long long)kCap) sig[at] = s;
    }
}

// one thread per significand of b; numerators a = 1.s_a for s_a in [a_lo, a_lo + a_n)
__global__ void __launch_bounds__(256) k_pairs(uint32_t a_lo, uint32_t a_n, unsigned long long *count, uint32_t *pair)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const float b = __uint_as_float(0x3f800000u | s);
    const float y1 = refined_rcp(b);
    unsigned long long bad = 0;
    for (uint32_t i = 0; i < a_n; ++i) {
        const float a = __uint_as_float(0x3f800000u | (a_lo + i));
        if (__float_as_uint(quot(a, b, y1)) != __float_as_uint(a / b)) {
            const unsigned long long at = atomicAdd(count + 1, 1ull);
            if (at < (unsigned long long)(kCap / 2)) {
                pair[2 * at] = a_lo + i;
                pair[2 * at + 1] = s;
            }
            ++bad;
        }
    }
    if (bad) atomicAdd(count, bad);
}

int main(int argc, char **argv)
{
    if (argc < 2 || (std::strcmp(argv[1], "rcp") && std::strcmp(argv[1], "pairs"))) {
        std::fprintf(stderr, "usage: quotient_probe rcp | pairs [slices]\n");
        return 2;
    }
    unsigned long long *d_count = nullptr, h_count[2];
    uint32_t *d_list = nullptr;
    static uint32_t h_list[kCap];
    TRY(hipMalloc((void **)&d_count, sizeof h_count));
    TRY(hipMalloc((void **)&d_list, sizeof h_list));
    const unsigned blocks = (1u << 23) / 256u;
    if (!std::strcmp(argv[1], "rcp")) {
        for (int e : {-14, 0, 35}) {
            TRY(hipMemset(d_count, 0, sizeof h_count));
            hipLaunchKernelGGL(k_rcp, dim3(blocks), dim3(256), 0, 0, (uint32_t)(e + 127), d_count, d_list);
            TRY(hipGetLastError());
            TRY(hipDeviceSynchronize());
            TRY(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
            TRY(hipMemcpy(h_list, d_list, sizeof h_list, hipMemcpyDeviceToHost));
            std::printf("rcp exponent %d: %llu of 8388608 significands differ from the correctly rounded reciprocal\n", e, h_count[0]);
            const unsigned long long n = h_count[0] < (unsigned long long)kCap ? h_count[0] : (unsigned long long)kCap;
            for (unsigned long long i = 0; i < n; ++i) std::printf("  0x%06x\n", h_list[i]);
            std::fflush(stdout);
        }
        return 0;
    }
    const int slices = argc > 2 ? std::atoi(argv[2]) : 64;
    const uint32_t per = (1u << 23) / 64u;
    TRY(hipMemset(d_count, 0, sizeof h_count));
    for (int k = 0; k < slices && k < 64; ++k) {
        hipLaunchKernelGGL(k_pairs, dim3(blocks), dim3(256), 0, 0, (uint32_t)k * per, per, d_count, d_list);
        TRY(hipGetLastError());
        TRY(hipDeviceSynchronize());
        TRY(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
        std::printf("pairs: numerators 0x%06x..0x%06x x all 8388608 divisors: %llu mismatches so far\n", (unsigned)k * per,
                    (unsigned)(k + 1) * per - 1u, h_count[0]);
        std::fflush(stdout);
    }
    TRY(hipMemcpy(h_list, d_list, sizeof h_list, hipMemcpyDeviceToHost));
    const unsigned long long n = h_count[1] < (unsigned long long)(kCap / 2) ? h_count[1] : (unsigned long long)(kCap / 2);
    for (unsigned long long i = 0; i < n && i < 64; ++i) std::printf("  a 0x%06x  b 0x%06x\n", h_list[2 * i], h_list[2 * i + 1]);
    std::printf("pairs: %llu mismatches in %d/64 of 2**46 pairs\n", h_count[0], slices < 64 ? slices : 64);
    return h_count[0] ? 1 : 0;
}
