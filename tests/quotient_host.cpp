// quotient_host.cpp -- the three-operation quotient of csrc/dev_math.inc (DevMathF::quot) on the host, independent of any
// device's reciprocal: with fmaf and an EMULATED refined reciprocal.  y0 is the correctly rounded reciprocal of b moved by
// -1, 0 and +1 units in the last place (what a one-unit reciprocal instruction may return), y1 its Newton step; wherever y1 is
// the correctly rounded reciprocal -- the hypothesis the device's self-check establishes -- quot(a, b, y1) must have the bits
// of a / b.  Divisors and numerators as trmc_selfcheck_fast_arith(what = 3) draws them (include/trmc.h).  Exits non-zero on
// A second pass draws them as what = 4 does: DevMathF::div4's own operand box -- divisor exponents in [-21, 52], numerators of
// both signs at absolute magnitudes in [2**-60, 2**60] (ql*dt), [2**-45, 2**52] (the two differences) and [2**-21, 2**52] (the
// sum), a = d*q +- 1 ulp with q of either sign, and the zeros: +0 must give +0, and -0 is shown to NEED coef_guard's bitwise
// test (the three operations turn it into +0 where the division gives -0).  Exits non-zero on
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

// a float with a uniform significand and an exponent uniform over [e_lo, e_hi], 2**e_hi itself as the top value
static float draw(uint64_t r, int e_lo, int e_hi)
{
    const uint32_t span = (uint32_t)(e_hi - e_lo);
    const uint32_t e = (uint32_t)((r >> 32) % (span + 1));
    const uint32_t frac = e == span ? 0u : (uint32_t)r & 0x7fffffu;
    return as_float(((uint32_t)(e_lo + (int)e + 127) << 23) | frac);
}
// coef_guard's test of the numerator n4 (csrc/dev_math.inc), restated
static bool n4_guard(float n4) { return as_uint(n4) == 0u || (std::fabs(n4) >= 0x1p-60f && std::fabs(n4) <= 0x1p60f); }

// the pass over div4's operand box (trmc_selfcheck_fast_arith, what = 4); returns non-zero on failure
static int box_pass(int64_t per, uint64_t seed)
{
    uint64_t pairs = 0, bad = 0, exact_y1 = 0, negative = 0;
    int rel_lo = 0, rel_hi = 0;
    for (int64_t ib = 0; ib < kDivisors; ++ib) {
        const uint64_t rb = mix(seed ^ (0x5851f42d4c957f2dull * (uint64_t)(ib + 1)));
        const int eb = -21 + (int)((rb >> 32) % 74u);
        const float b = as_float(((uint32_t)(eb + 127) << 23) | (eb == 52 ? 0u : divisor_sig(ib)));
        const float y = (float)(1.0 / (double)b);
        bool covered = false;
        for (int d = -1; d <= 1; ++d) {
            const float y1 = refined_rcp_from(b, as_float(as_uint(y) + (uint32_t)d));
            if (as_uint(y1) != as_uint(y)) continue;
            covered = true;
            if (!n4_guard(0.0f) || as_uint(quot(0.0f, b, y1)) != as_uint(0.0f / b) || as_uint(0.0f / b) != 0u) {
                std::fprintf(stderr, "box: +0 / %a gave %a\n", b, quot(0.0f, b, y1));
                return 1;
            }
            // -0: the division gives -0, the three operations +0 -- so the guard must send it to the division, and it does
            if (n4_guard(-0.0f) || as_uint(-0.0f / b) != 0x80000000u || as_uint(quot(-0.0f, b, y1)) != 0u) {
                std::fprintf(stderr, "box: -0 / %a: guard %d, division %a, three operations %a\n", b, (int)n4_guard(-0.0f), -0.0f / b,
                             quot(-0.0f, b, y1));
                return 1;
            }
            for (int64_t j = 0; j < per; ++j) {
                const uint64_t r = mix(rb + (uint64_t)j);
                const int cls = (int)(j & 3);
                const int lo = cls == 0 ? -60 : cls == 3 ? -21 : -45, hi = cls == 0 ? 60 : 52;
                const uint32_t sign = (cls != 3 && ((r >> 63) & 1u)) ? 0x80000000u : 0u;
                float a;
                if ((j & 4) == 0) {
                    a = as_float(as_uint(draw(r >> 1, lo, hi)) | sign);
                } else {
                    const unsigned k = 2u + (unsigned)((r >> 24) % 23u), pick = (unsigned)(r >> 32) % 3u;
                    const double eps = std::ldexp(1.0, -(int)k);
                    const double t = pick == 0 ? 0.5 - eps : pick == 1 ? 0.5 + eps : 0.5;
                    const double q = ((double)(0x800000u | ((uint32_t)r & 0x7fffffu)) + t) * 0x1p-23;
                    const int ea = lo + 1 + (int)((r >> 44) % (uint32_t)(hi - lo - 3));
                    const float a0 = (float)std::ldexp((double)b * q, ea - eb);
                    a = as_float((as_uint(a0) + (uint32_t)(r >> 40) % 3u - 1u) | sign);
                }
                const float mag = std::fabs(a);
                if (!(mag >= std::ldexp(1.0f, lo) && mag <= std::ldexp(1.0f, hi)) || (cls == 0 && !n4_guard(a))) {
                    std::fprintf(stderr, "box: numerator %a of class %d left its range\n", a, cls);
                    return 1;
                }
                int ex;
                std::frexp(mag, &ex);
                const int rel = ex - 1 - eb;
                rel_lo = rel < rel_lo ? rel : rel_lo;
                rel_hi = rel > rel_hi ? rel : rel_hi;
                negative += sign != 0u;
                ++pairs;
                if (as_uint(quot(a, b, y1)) != as_uint(a / b)) {
                    if (bad++ < 8) std::fprintf(stderr, "box: %a / %a: %a, not %a (y0 off by %d)\n", a, b, quot(a, b, y1), a / b, d);
                }
            }
        }
        exact_y1 += covered;
    }
    std::printf("box: %llu pairs (%llu negative, exponent distances %d .. %d), %llu mismatches\n", (unsigned long long)pairs,
                (unsigned long long)negative, rel_lo, rel_hi, (unsigned long long)bad);
    if (exact_y1 < (uint64_t)kDivisors) {
        std::fprintf(stderr, "box: some divisor was never covered\n");
        return 1;
    }
    // (the draws must really reach past the 2**96 of the compiler's unscaled division, on both signs)
    if (per >= 1024 && (rel_lo > -100 || rel_hi < 75 || negative * 4 < pairs)) {
        std::fprintf(stderr, "box: the draws do not span the operand box\n");
        return 1;
    }
    return bad ? 1 : 0;
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
    if (bad) return 1;
    return box_pass(per, seed);
}
