// dev_math.inc -- included by trmc.hip: the device arithmetic policies (DevMathF / DevMathTol / DevMathD).
// ---------------------------------------------------------------- device math
// fp32: the bit-reproducible power of det_pow.h (IEEE double + - * / fma only), so the
// whole fp32 path is bit-comparable with the host oracle; sqrtf and / are the
// correctly rounded forms (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt).
__device__ const uint64_t d_pow_tab[TRMC_POW_TAB_WORDS] = TRMC_POW_TAB_VALUES;

// fp32: the bit-reproducible powf of det_pow.h (tables staged in LDS by the kernel), so the whole
// fp32 path is bit-comparable with the host; sqrtf and / are the correctly rounded forms (hipcc
// default -fhip-fp32-correctly-rounded-divide-sqrt).
struct DevMathF {
    const uint64_t *tab; // LDS copy of d_pow_tab
    using Log = double;
    __device__ __forceinline__ Log log_of(float x) const { return trmc_det_log2(x, tab); }
    __device__ __forceinline__ float pow_l(Log l, float, float y) const { return trmc_det_powf_from_log(l, y, tab); }
    __device__ __forceinline__ float pow(float x, float y) const { return trmc_det_powf(x, y, tab); }
    // the hydraulic radius under fast_ok's ranges: the bound is derived at fast_ok
    __device__ __forceinline__ Log log_of_r(float x, bool ok) const { return ok ? trmc_det_log2_normal(x, tab) : trmc_det_log2(x, tab); }
    __device__ __forceinline__ float pow_l_r(Log l, float, float y, bool ok) const
    {
        return ok ? trmc_det_powf_from_log_inrange(l, y, tab) : trmc_det_powf_from_log(l, y, tab);
    }
    __device__ __forceinline__ float sqrt(float x) const { return ::sqrtf(x); }
    // wave-wide AND over the active lanes: a scalar, so the branch on it is a uniform one
    __device__ __forceinline__ bool all(bool p) const { return __all(p) != 0; }
    static constexpr bool kInbank = true;

    // The four Muskingum coefficients C1..C4 = n_i / D (f90:303-312) with ONE reciprocal.
    // hipcc expands an fp32 division into  v_div_scale x2, v_rcp, the refinement
    //     y1 = fma(fma(-b, y0, 1), y0, y0);  q0 = a*y1;  q1 = fma(fma(-b, q0, a), y1, q0);
    //     q  = div_fmas(fma(-b, q1, a), y1, q1)
    // and v_div_fixup.  v_div_scale / v_div_fmas / v_div_fixup only act on operands that are zero,
    // non-finite, subnormal or more than 2**96 apart, or on a subnormal quotient (CDNA3 ISA guide,
    // V_DIV_SCALE_F32 / V_DIV_FIXUP_F32); otherwise they are the identity and the division IS the
    // refinement above.  The kernel proves once per segment-step (`coef_ok`: dt in [2**-20, 2**40] and
    // n4 = ql*dt either +0 or 2**-60 <= |n4| <= 2**60) and once per coefficient set (D <= 2**52) that
    // all four divisions are of that kind: D >= dt/2 >= 2**-21; n1 = Km*X + dt/2 in [2**-21, 2**52];
    // n2, n3 are differences of two such floats, hence +0 or of magnitude >= 2**-45; so for n1, n2, n3 no
    // scaling, no fix-up, every quotient normal or +0 (for which the refinement returns +0 as IEEE does).  Then
    // the same instructions are issued, minus the three helpers, and y1 once instead of four times:
    // bit-identical by construction -- and of those, the second correction of each quotient is not
    // issued either (see quot).  n4 is the exception to "by construction": |n4| down to 2**-60 over D up to 2**52 is
    // 2**112 apart, more than the 2**96 inside which v_div_scale is the identity, so there the compiler's division DOES
    // scale.  The bits agree all the same, because both sides are the correctly rounded quotient: the division by IEEE,
    // quot by Markstein's theorem, whose side condition holds over the whole box -- q0 = n4*y1 >= 2**-113 and the quotient
    // <= 2**82 are normal, the residual is 0 or a multiple of 2**-47 |n4| >= 2**-107, normal too (checked over that box on
    // the device: trmc_selfcheck_fast_arith, what = 4).  A NEGATIVE zero n4 (ql = -0, or a negative product that underflows)
    // is NOT admitted: quot(-0, D, y1) is +0 where IEEE gives -0, which is why coef_guard tests the bits of n4 for +0.
    // Anything else takes the plain divisions.
    // The divisions of the hydraulic point (hydraulics_at: radius and composite n by the wetted perimeter, the top-width
    // term of the celerity, the reciprocal of the composite n) under the same argument.  `sane` is established once per
    // plan on the host (params_sane: bw, n, cs, twcc, ncc in [2**-14, 2**17], cs, twcc and ncc possibly 0; dt, dx, s0 as at k_of); with the in-bank and
    // over-bank depths in [2**-30, 2**17] the operands are: perimeter W = wp + wpc in [2**-14, 2**36]; area sum in
    // [2**-44, 2**51]; wp*n + wpc*ncc in [2**-28, 2**54]; the composite n in [2**-64, 2**18]; bw + 2hz in
    // [2**-14, 2**36] under 2*sqrt(1 + z*z) in [2, 2**19] -- all normal, no pair more than 2**80 apart, every quotient
    // normal: the scaling and fix-up instructions are the identity, and the refinement below IS the division.
    // The hydraulic radius under the same conditions (log_of_r / pow_l_r skip the power's special-value tests): R is
    // the mediant of the in-bank and the over-bank quotient area / wetted perimeter, so it lies between them.  In bank,
    // A/WP = (bw + h z) h / (bw + 2 h sq), sq = sqrt(1 + z*z) >= 1: since bw + 2 h sq <= 2 sq (bw + h) and
    // (bw + h z) / (bw + h) >= min(1, z), A/WP >= h min(1, z) / (2 sq) >= 2**-30 * 2**-17 / 2**15.1 > 2**-63, and
    // A/WP <= h (1 + h z / bw) <= 2**17 (1 + 2**17 2**14 2**14) < 2**63; over bank, twcc h / (twcc + 2 h) lies between
    // min(h, twcc) / 3 and h.  With one rounding of the quotient: 2**-64 < R < 2**63, a positive normal float whose
    // logarithm times 5/3 stays within +-107 -- inside the +-126 where glibc's powf takes its ordinary path.
    // The Muskingum K of an IN-BANK point (hydraulics_inbank: h <= bankfull depth, so area sum = A, perimeter = WP).
    // `sane` also bounds s0 in [2**-30, 2**10], dx in [2**-10, 2**19] and dt in [2**-20, 2**40] (params_sane).  The
    // celerity is ck = (sqrt(s0)/n) (5/3 r23 - 2/3 r53 q), r23 = R**(2/3), r53 = R**(5/3), q = 2 sq / twl.  In exact
    // arithmetic r53 q = r23 [A 2 sq / (WP twl)] and the bracket is the product of (bw + h z) / (bw + 2 h z) in [1/2, 1)
    // and 2 h sq / (bw + 2 h sq) in (0, 1): below one.  Each of the dozen roundings on the way (A, WP, twl, the two
    // quotients, the powers -- glibc's powf is within one unit in the last place --, the products) moves a term by at
    // most 2**-23 of itself, so the computed bracket is at least r23 (5/3 (1 - 2**-21) - 2/3 (1 + 2**-20)) > 0.99 r23 and at
    // most 5/3 r23 (1 + 2**-21): with r23 in [2**-43, 2**42] and sqrt(s0)/n in [2**-32, 2**19] the celerity is a positive
    // normal number in [2**-76, 2**62].  Hence max(0, ck) = ck, the guard `ck > 0` holds, and dx / ck divides a number of
    // exponent <= 18 by one of exponent >= -76: exponents less than 96 apart, numerator above 2**-103, quotient in
    // [2**-72, 2**95] -- none of the cases in which v_div_scale / v_div_fmas / v_div_fixup act (see div4), so the
    // division IS the refinement below; max(dt, K) with both operands ordinary numbers is v_max.
    bool sane;
    __device__ __forceinline__ float k_of(float dx, float ck) const { return quot(dx, ck, refined_rcp(ck)); }
    __device__ __forceinline__ float max_num(float a, float b) const { return __builtin_fmaxf(a, b); }
    // sqrt(x), correctly rounded.  hipcc expands sqrtf into: scale x by 2**32 if x < 2**-96, v_sqrt_f32 (one unit in the
    // last place), the two neighbours s-, s+ of that result with the residuals x - s- s and x - s+ s (one fma each) choosing
    // among the three, unscale, and pass zeros / infinities / NaNs through.  For an ordinary x >= 2**-96 the scaling and
    // the pass-through are the identity; what is left is issued here -- the same instructions, eight fewer.
    __device__ __forceinline__ float sqrt_r(float x, bool ok) const
    {
        if (!ok) return ::sqrtf(x);
        const float s = __builtin_amdgcn_sqrtf(x);
        const float s_dn = __uint_as_float(__float_as_uint(s) - 1u), s_up = __uint_as_float(__float_as_uint(s) + 1u);
        const float r_dn = __builtin_fmaf(-s_dn, s, x), r_up = __builtin_fmaf(-s_up, s, x);
        float r = (r_dn <= 0.0f) ? s_dn : s;
        r = (r_up > 0.0f) ? s_up : r;
        return r;
    }
    __device__ __forceinline__ bool fast_ok(float h, float h_in, float h_over) const
    {
        return sane && h_in >= 0x1p-30f && h <= 0x1p17f && (h_over == 0.0f || h_over >= 0x1p-30f);
    }
    __device__ __forceinline__ static float refined_rcp(float b)
    {
        const float y0 = __builtin_amdgcn_rcpf(b);
        return __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0);
    }
    __device__ __forceinline__ void div2(float a1, float a2, float b, bool ok, float &q1, float &q2) const
    {
        if (ok) {
            const float y1 = refined_rcp(b);
            q1 = quot(a1, b, y1);
            q2 = quot(a2, b, y1);
        } else {
            q1 = a1 / b;
            q2 = a2 / b;
        }
    }
    __device__ __forceinline__ float div1(float a, float b, bool ok) const
    {
        if (ok) return quot(a, b, refined_rcp(b));
        return a / b;
    }
    // the remaining divisions of a secant iteration (weighting factor, K = dx / celerity, secant update): IEEE
    __device__ __forceinline__ float divx(float a, float b) const
    {
        return a / b;
    }
    // a / b in THREE operations, y1 = refined_rcp(b).  The compiler's expansion (above) corrects q0 = a*y1 twice; the second
    // correction never changes a bit, so it is not issued.  Why:
    //   Markstein's theorem (P. Markstein, "Computation of elementary functions on the IBM RISC System/6000 processor", IBM
    //   J. Res. Dev. 34, 1990; Muller et al., Handbook of Floating-Point Arithmetic, section 4.7): in radix 2, if y = RN(1/b)
    //   and q0 is within one unit in the last place of a/b, then r = fma(-b, q0, a) is exact and fma(r, y, q0) = RN(a/b),
    //   provided nothing overflows, underflows or is subnormal on the way.
    //   (1) y1 = RN(1/b).  v_rcp_f32 is within one unit in the last place and one Newton step follows; whether that lands on
    //       the correctly rounded reciprocal is a property of the hardware's table (the classical failure is a significand
    //       of all ones).  Both operations commute with scaling by a power of two for a normal b with a normal reciprocal, so
    //       the 2**23 significands of one binade decide it: on gfx950 (MI355X) ALL of them give RN(1/b), against
    //       (float)(1.0 / (double)b), exact because fp64 carries more than 2*24 + 2 bits -- the compiled-in set of
    //       exceptions is EMPTY (profiles/r21_quotient_exhaustive.txt; tests/test_gpu_quotient.py at 2**-14, 2**0, 2**35).
    //       A device is not taken on trust: the first plan created on it runs k_selfcheck_rcp over the 2**23 significands
    //       (quot_selfcheck, host_misc.inc), and ONE mismatch clears `sane` for every plan there and c_quot_ok for
    //       coef_guard, i.e. selects the plain divisions everywhere: slower, never other bits.
    //   (2) q0 = a*y1 against a/b: |y1 - 1/b| <= ulp(1/b)/2 and one rounding.  With a, b scaled into [1, 2) that is
    //       |q0 - a/b| <= a 2**-25 + ulp(q0)/2: below one unit in the last place when a >= b (quotient in [1, 2)), and below
    //       (a + 1)/2 < 3/2 units when a < b (quotient in (1/2, 1)).  So the hypothesis holds in the looser sense only -- a
    //       host count finds q0 more than one unit of the quotient's binade away for about one pair in a hundred when a is
    //       close below b, and r then needs 25 bits now and then -- and the theorem alone does not close the case a < b.
    //       What closes it is exhaustion: for normal operands and results quot(a, b, y1) commutes with scaling a and b by
    //       powers of two, so the 2**23 x 2**23 pairs of significands decide every pair, and tools/quotient_probe.hip
    //       compares quot(a, b, refined_rcp(b)) with a / b for ALL 2**46 of them on the device: no mismatch (20 s of one
    //       MI355X; same file).  Given (1), every operation involved is an IEEE one, so the result holds for any device
    //       that passes the self-check.
    //   (3) no overflow, underflow or subnormal: the ranges proved at div4, fast_ok and k_of (every divisor, numerator and
    //       quotient normal, numerators at least 2**-64, so r -- a multiple of 2**-47 a -- is normal or zero).  A numerator
    //       +0 (div4's n4) gives q0 = +0, r = fma(-b, +0, +0) = +0 and fma(+0, y1, +0) = +0, as IEEE does.
    //   IEEE division has one correctly rounded result, so these are the bits of the five operations, two fewer issued.
    __device__ __forceinline__ static float quot(float a, float b, float y1)
    {
        const float q0 = a * y1;
        return __builtin_fmaf(__builtin_fmaf(-b, q0, a), y1, q0);
    }
    bool coef_ok;
    __device__ __forceinline__ void div4(float n1, float n2, float n3, float n4, float d, float &q1, float &q2,
                                         float &q3, float &q4) const
    {
        if (coef_ok && d <= 0x1p52f) {
            const float y1 = refined_rcp(d);
            q1 = quot(n1, d, y1);
            q2 = quot(n2, d, y1);
            q3 = quot(n3, d, y1);
            q4 = quot(n4, d, y1);
        } else {
            q1 = n1 / d;
            q2 = n2 / d;
            q3 = n3 / d;
            q4 = n4 / d;
        }
    }
};
// The same arithmetic for the dataflow kernels, without the in-bank body: there a wavefront steps through time by itself
// and what counts is the latency of ITS step -- registers and code size -- not the instruction count of a full device
// (measured: a lone 4 096-row chain 6.6 us per step against 7.3 with the in-bank body, the general-mode CONUS day the same).
#ifndef TRMC_FLOW_INBANK
#define TRMC_FLOW_INBANK 0
#endif
struct DevMathFlow : DevMathF {
    static constexpr bool kInbank = TRMC_FLOW_INBANK != 0;
};
// fp32, TOLERANCE arithmetic (a plan created with trmc_plan_options.arithmetic = TRMC_ARITH_TOLERANCE): the power as
// exp2(y * log2(x)) on the hardware's v_log_f32 / v_exp_f32, every division as a * v_rcp_f32(b), the square root as
// v_sqrt_f32 -- each within one unit in the last place of its exact result, the power within |y log2 x| 2**-23 (some 1e-6 for
// a hydraulic radius between a millimetre and a hundred metres).  NOT bit-comparable with the reference: its results are
// stated and tested against a tolerance (include/trmc.h, tests/test_gpu_tolerance.py), and the 1 % exit of the secant
// iteration (MCsingleSegStime_f2py_NOLOOP.f90:83) turns a last-place difference into a different iteration count now and
// then.  The special values the step relies on keep their meaning: log2(0) = -inf and exp2(-inf) = 0 (a dry point's
// power is 0), a quotient by zero is inf or NaN and is discarded by the selects that guard it (mc_segment.hpp).
struct DevMathTol {
    const uint64_t *tab; // unused (no tables)
    bool sane;
    bool coef_ok;        // unused
    using Log = float;
    __device__ __forceinline__ Log log_of(float x) const { return __builtin_amdgcn_logf(x); }
    __device__ __forceinline__ float pow_l(Log l, float, float y) const { return __builtin_amdgcn_exp2f(y * l); }
    __device__ __forceinline__ float pow(float x, float y) const { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
    __device__ __forceinline__ Log log_of_r(float x, bool) const { return __builtin_amdgcn_logf(x); }
    __device__ __forceinline__ float pow_l_r(Log l, float, float y, bool) const { return __builtin_amdgcn_exp2f(y * l); }
    __device__ __forceinline__ float sqrt(float x) const { return __builtin_amdgcn_sqrtf(x); }
    __device__ __forceinline__ float sqrt_r(float x, bool) const { return __builtin_amdgcn_sqrtf(x); }
    __device__ __forceinline__ bool all(bool p) const { return __all(p) != 0; }
    static constexpr bool kInbank = true;
    // (the ranges under which the in-bank body of the hydraulic point stands for the general one are DevMathF's: its argument
    // leaves a margin of 1 % on the sign of the celerity, far more than these operations give away)
    __device__ __forceinline__ bool fast_ok(float h, float h_in, float h_over) const
    {
        return sane && h_in >= 0x1p-30f && h <= 0x1p17f && (h_over == 0.0f || h_over >= 0x1p-30f);
    }
    __device__ __forceinline__ float k_of(float dx, float ck) const { return dx * __builtin_amdgcn_rcpf(ck); }
    __device__ __forceinline__ float max_num(float a, float b) const { return __builtin_fmaxf(a, b); }
    __device__ __forceinline__ void div2(float a1, float a2, float b, bool, float &q1, float &q2) const
    {
        const float y = __builtin_amdgcn_rcpf(b);
        q1 = a1 * y;
        q2 = a2 * y;
    }
    __device__ __forceinline__ float div1(float a, float b, bool) const { return a * __builtin_amdgcn_rcpf(b); }
    __device__ __forceinline__ float divx(float a, float b) const { return a * __builtin_amdgcn_rcpf(b); }
    __device__ __forceinline__ void div4(float n1, float n2, float n3, float n4, float d, float &q1, float &q2, float &q3,
                                         float &q4) const
    {
        const float y = __builtin_amdgcn_rcpf(d);
        q1 = n1 * y;
        q2 = n2 * y;
        q3 = n3 * y;
        q4 = n4 * y;
    }
};
struct DevMathTolFlow : DevMathTol {
    static constexpr bool kInbank = TRMC_FLOW_INBANK != 0;
};
// fp64: the bit-reproducible double power of det_pow64.h (glibc 2.35 pow restated, the one the reference links when it
// is built with -fdefault-real-8: oracle/_ref/libmc_ref_qj0_f64.so), so that the fp64 path -- BASELINE configs[1] -- is
// bit-comparable with the reference too, not merely close; / and sqrt are the correctly rounded forms.
struct DevMathD {
    const uint64_t *tab; // unused
    using Log = double;
    __device__ __forceinline__ Log log_of(double x) const { return x; }
    __device__ __forceinline__ double pow_l(Log, double x, double y) const { return det_pow64(x, y); }
    __device__ __forceinline__ double pow(double x, double y) const { return det_pow64(x, y); }
    __device__ __forceinline__ Log log_of_r(double x, bool) const { return x; }
    __device__ __forceinline__ double pow_l_r(Log, double x, double y, bool) const { return det_pow64(x, y); }
    __device__ __forceinline__ double sqrt(double x) const { return ::sqrt(x); }
    __device__ __forceinline__ bool all(bool p) const { return __all(p) != 0; }
    static constexpr bool kInbank = false;
    bool coef_ok; // unused
    bool sane;    // unused
    __device__ __forceinline__ bool fast_ok(double, double, double) const { return false; }
    __device__ __forceinline__ void div2(double a1, double a2, double b, bool, double &q1, double &q2) const
    {
        q1 = a1 / b;
        q2 = a2 / b;
    }
    __device__ __forceinline__ double div1(double a, double b, bool) const { return a / b; }
    __device__ __forceinline__ double divx(double a, double b) const { return a / b; }
    // (only the in-bank body uses these, which this policy never takes: kInbank = false)
    __device__ __forceinline__ double k_of(double dx, double ck) const { return dx / ck; }
    __device__ __forceinline__ double max_num(double a, double b) const { return a > b ? a : b; }
    __device__ __forceinline__ double sqrt_r(double x, bool) const { return ::sqrt(x); }
    __device__ __forceinline__ void div4(double n1, double n2, double n3, double n4, double d, double &q1, double &q2,
                                         double &q3, double &q4) const
    {
        q1 = n1 / d;
        q2 = n2 / d;
        q3 = n3 / d;
        q4 = n4 / d;
    }
};
// every kernel that evaluates segment steps stages the 512-byte power tables into LDS first
__device__ __forceinline__ const uint64_t *stage_pow_tables(uint64_t *s_tab)
{
    if (threadIdx.x < TRMC_POW_TAB_WORDS) s_tab[threadIdx.x] = d_pow_tab[threadIdx.x];
    __syncthreads();
    return s_tab;
}
// 1 unless this device's refined reciprocal failed the self-check (quot_selfcheck, host_misc.inc; see DevMathF::quot)
__constant__ int32_t c_quot_ok = 1;
// the once-per-segment-step part of DevMathF::div4's proof obligation (see there)
__device__ __forceinline__ bool coef_guard(float dt, float ql)
{
    const float n4 = ql * dt, an4 = __builtin_fabsf(n4);
    return (c_quot_ok != 0) && (dt >= 0x1p-20f) && (dt <= 0x1p40f)
           && ((__float_as_uint(n4) == 0u) || (an4 >= 0x1p-60f && an4 <= 0x1p60f));
}
__device__ __forceinline__ bool coef_guard(double, double) { return false; }
// TOL: the plan's arithmetic is TRMC_ARITH_TOLERANCE (fp32 plans only)
template <class T, bool TOL = false> struct DevMath;
template <> struct DevMath<float, false> { using type = DevMathF; };
template <> struct DevMath<float, true> { using type = DevMathTol; };
template <> struct DevMath<double, false> { using type = DevMathD; };

constexpr int kBlock = 256;

// The threads of a block take the block's NB positions by DESCENDING cost class (cls: one byte per position; 8 = no row): a count
// per class in LDS, a prefix over the classes, a scatter of lane numbers.  Returns the lane whose position this thread takes.
// Every thread of the block must call it (three barriers).  Order inside a class is whatever the atomics give; results do not
// depend on which thread routes a row.  `none`: the position this thread takes is one of key 8 (no row there).
template <int NB> __device__ __forceinline__ int32_t block_partition_by_class(int32_t key, bool &none)
{
    __shared__ int32_t s_cnt[9], s_base[9];
    __shared__ int16_t s_lane[NB];
    if (threadIdx.x < 9) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int32_t rank = atomicAdd(&s_cnt[key], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t acc = 0;
        for (int b = 0; b < 9; ++b) {
            s_base[b] = acc;
            acc += s_cnt[b];
        }
    }
    __syncthreads();
    s_lane[s_base[key] + rank] = (int16_t)threadIdx.x;
    __syncthreads();
    none = (int32_t)threadIdx.x >= s_base[8];
    return (int32_t)s_lane[threadIdx.x];
}

// element of a column at a 32-bit BYTE offset from a (wave-uniform) base pointer
template <class T> __device__ __forceinline__ T &at(T *base, uint32_t byte_off)
{
    return *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off);
}
template <class T> __device__ __forceinline__ const T &at(const T *base, uint32_t byte_off)
{
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}

