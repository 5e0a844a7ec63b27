// quotient_host.cpp -- the three-operation quotient of csrc/dev_math.inc (DevMathF::quot) on the host, independent of any
// device's reciprocal: with fmaf and an EMULATED refined reciprocal.  y0 is the correctly rounded reciprocal of b moved by
// -1, 0 and +1 units in the last place (what a one-unit reciprocal instruction may return), y1 its Newton step; wherever y1 is
// the correctly rounded reciprocal -- the hypothesis the device's self-check establishes -- quot(a, b, y1) must have the bits
// of a / b.  Divisors and numerators as trmc_selfcheck_fast_arith(what = 3) draws them (include/trmc.h).  Exits non-zero on
// the first kind of failure; tests/test_quotient_host.py builds it with -ffp-contract=off and runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static float as_float(uint32_t u)
{
    float x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}
static uint32_t as_uint(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}
static uint64_t mix(uint64_t z) // splitmix64
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static float refined_rcp_from(float b, float y0) { return fmaf(fmaf(-b, y0, 1.0f), y0, y0); }
static float quot(float a, float b, float y1)
{
    const float q0 = a * y1;
    return fmaf(fmaf(-b, q0, a), y1, q0);
}

constexpr int64_t kDivisors = 65536 + 65 + 65;
static uint32_t divisor_sig(int64_t i)
{
    return i < 65536 ? (uint32_t)i * 128u : i < 65536 + 65 ? (uint32_t)(i - 65536) : 0x7fffffu - (uint32_t)(i - 65536 - 65);
}

int main(int argc, char **argv)
{
    const int64_t per = argc > 1 ? std::atoll(argv[1]) : 4096;
    const uint64_t seed = 1;
    uint64_t pairs = 0, bad = 0, inexact_y1 = 0, exact_y1 = 0;
    for (int64_t ib = 0; ib < kDivisors; ++ib) {
        const uint64_t rb = mix(seed ^ (0x5851f42d4c957f2dull * (uint64_t)(ib + 1)));
        const int eb = -14 + (int)((rb >> 32) % 50u);
        const float b = as_float(((uint32_t)(eb + 127) << 23) | divisor_sig(ib));
        const float y = (float)(1.0 / (double)b); // correctly rounded: fp64 carries more than 2*24 + 2 bits
        for (int d = -1; d <= 1; ++d) {
            const float y1 = refined_rcp_from(b, as_float(as_uint(y) + (uint32_t)d));
            if (as_uint(y1) != as_uint(y)) { // not a divisor the three operations are claimed for with this y0
                ++inexact_y1;
                continue;
            }
            ++exact_y1;
            if (as_uint(quot(0.0f, b, y1)) != 0u) {
                std::fprintf(stderr, "+0 / %a gave %a\n", b, quot(0.0f, b, y1));
                return 1;
            }
            for (int64_t j = 0; j < per; ++j) {
                const uint64_t r = mix(rb + (uint64_t)j);
                const int rel = -40 + (int)((j >> 1) % 91);
                float a;
                if ((j & 1) == 0) {
                    a = as_float(((uint32_t)(eb + rel + 127) << 23) | ((uint32_t)r & 0x7fffffu));
                } else {
                    const unsigned k = 2u + (unsigned)((r >> 24) % 23u), pick = (unsigned)(r >> 32) % 3u;
                    const double eps = std::ldexp(1.0, -(int)k);
                    const double t = pick == 0 ? 0.5 - eps : pick == 1 ? 0.5 + eps : 0.5;
                    const double q = ((double)(0x800000u | ((uint32_t)r & 0x7fffffu)) + t) * 0x1p-23;
                    const float a0 = (float)std::ldexp((double)b * q, rel);
                    a = as_float(as_uint(a0) + (uint32_t)(r >> 40) % 3u - 1u);
                }
                ++pairs;
                if (as_uint(quot(a, b, y1)) != as_uint(a / b)) {
                    if (bad++ < 8) std::fprintf(stderr, "%a / %a: %a, not %a (y0 off by %d)\n", a, b, quot(a, b, y1), a / b, d);
                }
            }
        }
    }
    std::printf("%llu pairs, %llu mismatches; refined reciprocal correctly rounded for %llu of %llu (divisor, y0) choices\n",
                (unsigned long long)pairs, (unsigned long long)bad, (unsigned long long)exact_y1,
                (unsigned long long)(exact_y1 + inexact_y1));
    // (a correctly rounded y0 always reproduces itself under the Newton step here, so every divisor is covered at least once)
    if (exact_y1 < (uint64_t)kDivisors) {
        std::fprintf(stderr, "some divisor was never covered\n");
        return 1;
    }
    return bad ? 1 : 0;
}
