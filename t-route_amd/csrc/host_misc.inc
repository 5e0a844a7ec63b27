// host_misc.inc -- included by trmc.hip: batch of single segment steps, state hand-over between plans, arithmetic self-checks.
template <class T> int segments_t(int64_t n, const void *in, void *out, bool tol, int32_t *iters_out)
{
    DevBuf din, dout, dit;
    int rc = din.ensure((size_t)n * 15 * sizeof(T));
    if (!rc) rc = dout.ensure((size_t)n * 6 * sizeof(T));
    if (!rc && iters_out) rc = dit.ensure((size_t)n * sizeof(int32_t));
    if (!rc) {
        hipError_t e = hipMemcpy(din.p, in, (size_t)n * 15 * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            bool launched = false;
            if constexpr (sizeof(T) == 4) {
                if (tol) {
                    hipLaunchKernelGGL((k_segments<T, true>), dim3(blocks_for(n)), dim3(kBlock), 0, 0, (const T *)din.p, (T *)dout.p,
                                       (int32_t *)dit.p, n);
                    launched = true;
                }
            }
            if (!launched)
                hipLaunchKernelGGL((k_segments<T, false>), dim3(blocks_for(n)), dim3(kBlock), 0, 0, (const T *)din.p, (T *)dout.p,
                                   (int32_t *)dit.p, n);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 6 * sizeof(T), hipMemcpyDeviceToHost);
        if (e == hipSuccess && iters_out) e = hipMemcpy(iters_out, dit.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(TRMC_EHIP, std::string("trmc_segments: ") + hipGetErrorString(e));
    }
    return rc;
}

// trmc_reservoir_da_steps: n independent data-assimilation steps, one thread each, through the device functions the step
// kernels call (reservoir_da.hpp); `hybrid` picks the step kind.  Row layouts: HybridIn / HybridOut, RfcIn / RfcOut.
__global__ void __launch_bounds__(kBlock)
k_reservoir_da_steps(bool hybrid, int64_t n, int32_t ncol, const float *obs, const float *time, const float *fin, const int32_t *iin,
                     float *fout, int32_t *iout)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (hybrid) {
        const float *p = fin + i * 12;
        const trmc::HybridIn in{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]};
        const trmc::HybridOut o = trmc::hybrid_da_step(obs + i * ncol, time + i * ncol, ncol, in);
        float *q = fout + i * 6;
        q[0] = o.outflow;
        q[1] = o.persisted_outflow;
        q[2] = o.water_elevation;
        q[3] = o.update_time;
        q[4] = o.persistence_index;
        q[5] = o.persistence_update_time;
    } else {
        const float *p = fin + i * 9;
        const int32_t *k = iin + i * 6;
        const trmc::RfcIn in{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], k[0], k[1], k[2], k[3], k[4], k[5]};
        const trmc::RfcOut o = trmc::rfc_da_step(obs + i * ncol, ncol, in);
        float *q = fout + i * 3;
        q[0] = o.outflow;
        q[1] = o.water_elevation;
        q[2] = o.update_time;
        iout[i] = o.timeseries_idx;
    }
}

int reservoir_da_steps(bool hybrid, int64_t n, int32_t ncol, const float *obs, const float *time, const float *fin, const int32_t *iin,
                       float *fout, int32_t *iout)
{
    const size_t nin = hybrid ? 12 : 9, nout = hybrid ? 6 : 3, row = (size_t)n * (size_t)ncol * sizeof(float);
    DevBuf dobs, dtime, dfin, diin, dfout, diout;
    int rc = dobs.ensure(row);
    if (!rc && hybrid) rc = dtime.ensure(row);
    if (!rc) rc = dfin.ensure((size_t)n * nin * sizeof(float));
    if (!rc) rc = dfout.ensure((size_t)n * nout * sizeof(float));
    if (!rc && !hybrid) rc = diin.ensure((size_t)n * 6 * sizeof(int32_t));
    if (!rc && !hybrid) rc = diout.ensure((size_t)n * sizeof(int32_t));
    if (!rc) {
        hipError_t e = hipMemcpy(dobs.p, obs, row, hipMemcpyHostToDevice);
        if (e == hipSuccess && hybrid) e = hipMemcpy(dtime.p, time, row, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dfin.p, fin, (size_t)n * nin * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess && !hybrid) e = hipMemcpy(diin.p, iin, (size_t)n * 6 * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_reservoir_da_steps, dim3(blocks_for(n)), dim3(kBlock), 0, 0, hybrid, n, ncol, (const float *)dobs.p,
                               (const float *)dtime.p, (const float *)dfin.p, (const int32_t *)diin.p, (float *)dfout.p, (int32_t *)diout.p);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(fout, dfout.p, (size_t)n * nout * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess && !hybrid) e = hipMemcpy(iout, diout.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(TRMC_EHIP, std::string("trmc_reservoir_da_steps: ") + hipGetErrorString(e));
    }
    return rc;
}

// trmc_plan_chain_from: time row `src_row` of one plan's planes -> time row 0 of another's, positions [lo, hi) (same order)
template <class T>
__global__ void __launch_bounds__(kBlock)
k_chain_state(const T *__restrict__ sq, const T *__restrict__ sv, const T *__restrict__ sd, T *__restrict__ dq,
              T *__restrict__ dv, T *__restrict__ dd, int32_t lo, int32_t hi)
{
    const int32_t p = lo + (int32_t)blockIdx.x * kBlock + (int32_t)threadIdx.x;
    if (p >= hi) return;
    dq[p] = sq[p];
    dv[p] = sv[p];
    dd[p] = sd[p];
}
template <class T> int chain_from_t(trmc_plan *dst, trmc_plan *src, int nsteps_dst)
{
    const trmc::Topology &tp = src->sh->topo;
    const int64_t np = src->nseg_pad;
    const int32_t ns = src->run.nsteps;
    const size_t plane_s = (size_t)(ns + 1) * np, plane_d = (size_t)(nsteps_dst + 1) * np;
    if (int rc = dst->tm.ensure(3 * plane_d * sizeof(T))) return rc;
    const T *sq = (const T *)src->tm.p + (size_t)ns * np, *sv = sq + plane_s, *sd = sv + plane_s;
    T *dq = (T *)dst->tm.p, *dv = dq + plane_d, *dd = dv + plane_d;
    for (DevEvent &e : dst->ev_chain)
        if (int rc = e.ensure(false)) return rc;
    if (int rc = ensure_tile_stream(dst)) return rc;
    // the rows of the source's wide levels are final when its last tile is (they never wrote a velocity row: the velocity
    // of the initial state is not an input of the step); the other rows when its tail is
    const int32_t W = src->run.short_ts ? src->run.wide : 0, M = W > 0 ? src->run.mid : 0;
    const int32_t b0 = 0, w1 = tp.lvl_ptr[W], s1 = (int32_t)src->nseg; // (boundary rows, if any, go with the tail's part)
    const int32_t w0 = W > 0 ? tp.lvl_ptr[0] : w1;
    const int32_t m1 = tp.lvl_ptr[W + M]; // (the second tier's rows, [w1, m1): routed on the source's own stream, no velocity row either)
    if (W > 0 && src->wstream) {
        HIP_TRY(hipEventRecord(dst->ev_chain[0], src->wstream));
        HIP_TRY(hipStreamWaitEvent(dst->wstream, dst->ev_chain[0], 0));
        hipLaunchKernelGGL((k_chain_state<T>), dim3(blocks_for(w1 - w0)), dim3(kBlock), 0, dst->wstream, sq, sq, sd, dq, dv, dd, w0, w1);
        HIP_TRY(hipEventRecord(dst->ev_chain[2], dst->wstream));
        // The source's NEXT window must not overwrite what is being read here.  Not as waits queued on the source's streams
        // now: with one hardware queue per stream priority the two plans' tile streams share an in-order queue, and a wait
        // placed there at this point -- behind the source's tiles, ahead of everything this plan is about to queue -- holds
        // THIS plan's set-up and tiles back until the event fires: the second one below only does when the source's tail
        // has ended, so the receiver's leading levels started after the source's whole window instead of behind its last
        // tile (the timeline of bench.py's sequence showed exactly that).  The source takes the events (its own objects)
        // and waits for them at its next trmc_route_begin -- a window later, when they have long fired.
        if (int rc = src->mk_released[0].record(dst->wstream)) return rc;
        // ... and the receiver's own stream does not read time row 0 of the wide rows before this copy has written it: its
        // tail's first launch (step 1) takes no tile wait and reads q_tm[0] of its upstream wide rows
        HIP_TRY(hipStreamWaitEvent(dst->stream, dst->ev_chain[2], 0));
    }
    HIP_TRY(hipEventRecord(dst->ev_chain[1], src->stream));
    HIP_TRY(hipStreamWaitEvent(dst->stream, dst->ev_chain[1], 0));
    if (w0 > b0) hipLaunchKernelGGL((k_chain_state<T>), dim3(blocks_for(w0 - b0)), dim3(kBlock), 0, dst->stream, sq, sv, sd, dq, dv, dd, b0, w0);
    if (m1 > w1) hipLaunchKernelGGL((k_chain_state<T>), dim3(blocks_for(m1 - w1)), dim3(kBlock), 0, dst->stream, sq, sq, sd, dq, dv, dd, w1, m1);
    // (rows routed by cluster tiles wrote no velocity row either)
    if (s1 > m1) hipLaunchKernelGGL((k_chain_state<T>), dim3(blocks_for(s1 - m1)), dim3(kBlock), 0, dst->stream, sq, src->run.cl ? sq : sv, sd, dq, dv, dd, m1, s1);
    HIP_TRY(hipEventRecord(dst->ev_chain[3], dst->stream));
    if (int rc = src->mk_released[1].record(dst->stream)) return rc;
    HIP_TRY(hipGetLastError());
    dst->chain_staged = true;
    return 0;
}

// trmc_selfcheck_fast_arith: the short forms of DevMathF against the operations they stand for (see trmc.h)
__global__ void __launch_bounds__(kBlock)
k_selfcheck_sqrt(uint32_t lo_bits, uint32_t hi_bits, unsigned long long *mismatches)
{
    DevMathF m{nullptr, false};
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t b = (uint64_t)lo_bits + (uint64_t)blockIdx.x * kBlock + threadIdx.x; b <= hi_bits; b += stride) {
        const float x = __uint_as_float((uint32_t)b);
        bad += __float_as_uint(m.sqrt_r(x, true)) != __float_as_uint(::sqrtf(x));
    }
    if (bad) atomicAdd(mismatches, bad);
}
__device__ __forceinline__ uint64_t selfcheck_mix(uint64_t z) // splitmix64
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// a float with a uniform significand and an exponent uniform over [e_lo, e_hi] (2**e_hi itself included as the top value)
__device__ __forceinline__ float selfcheck_draw(uint64_t r, int e_lo, int e_hi)
{
    const uint32_t span = (uint32_t)(e_hi - e_lo);
    const uint32_t e = (uint32_t)((r >> 32) % (span + 1));
    const uint32_t frac = e == span ? 0u : (uint32_t)r & 0x7fffffu;
    return __uint_as_float(((uint32_t)(e_lo + (int)e + 127) << 23) | frac);
}
__global__ void __launch_bounds__(kBlock)
k_selfcheck_div(int64_t n, uint64_t seed, unsigned long long *mismatches)
{
    DevMathF m{nullptr, false};
    unsigned long long bad = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint64_t r0 = selfcheck_mix(seed + 3 * (uint64_t)i), r1 = selfcheck_mix(seed + 3 * (uint64_t)i + 1),
                       r2 = selfcheck_mix(seed + 3 * (uint64_t)i + 2);
        float a = selfcheck_draw(r0, -10, 19), b = selfcheck_draw(r1, -76, 62);
        const float c = selfcheck_draw(r2, -20, 40);
        // one draw in eight: a divisor (and in half of those a dividend too) with a significand of all ones, all ones but the
        // last bit, or all zeros -- the hard cases of reciprocal-based division
        if (((r2 >> 40) & 7u) == 0u) {
            const uint32_t pick = (uint32_t)(r2 >> 43) & 3u, frac = pick == 0 ? 0x7fffffu : pick == 1 ? 0x7ffffeu : pick == 2 ? 0u : 1u;
            b = __uint_as_float((__float_as_uint(b) & 0xff800000u) | frac);
            if ((r2 >> 45) & 1u) a = __uint_as_float((__float_as_uint(a) & 0xff800000u) | (0x7fffffu - frac));
        }
        const float q_fast = m.k_of(a, b), q = a / b;
        const float k_fast = m.max_num(c, q_fast), k = c > q ? c : q;
        bad += (__float_as_uint(q_fast) != __float_as_uint(q)) || (__float_as_uint(k_fast) != __float_as_uint(k));
    }
    if (bad) atomicAdd(mismatches, bad);
}
// refined_rcp(b) against the correctly rounded reciprocal for all 2**23 significands of the binade 2**(ebits - 127): hypothesis
// (1) of DevMathF::quot.  (float)(1.0 / (double)b) is exact: fp64 carries more than 2*24 + 2 bits.  Grid: 2**23 / kBlock blocks.
__global__ void __launch_bounds__(kBlock)
k_selfcheck_rcp(uint32_t ebits, unsigned long long *mismatches)
{
    const float b = __uint_as_float((ebits << 23) | (blockIdx.x * (uint32_t)kBlock + threadIdx.x));
    if (__float_as_uint(DevMathF::refined_rcp(b)) != __float_as_uint((float)(1.0 / (double)b))) atomicAdd(mismatches, 1ull);
}
// ... and the values themselves, for a host that forms the correctly rounded reciprocals itself (trmc_selfcheck_rcp_values):
// y[s] = refined_rcp of significand s in the binade 2**(ebits - 127); y holds 2**23 floats, the grid is 2**23 / kBlock blocks
__global__ void __launch_bounds__(kBlock)
k_rcp_values(uint32_t ebits, float *__restrict__ y)
{
    const uint32_t s = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    y[s] = DevMathF::refined_rcp(__uint_as_float((ebits << 23) | s));
}
// the divisors of k_selfcheck_quot: 2**16 significands at a stride of 128, then those within 64 of 0 and of 2**23 - 1 (the
// compiled-in set of reciprocal exceptions is empty, or their neighbourhoods would follow here)
constexpr int64_t kQuotDivisors = 65536 + 65 + 65;
__device__ __forceinline__ uint32_t selfcheck_divisor_sig(int64_t i)
{
    return i < 65536 ? (uint32_t)i * 128u : i < 65536 + 65 ? (uint32_t)(i - 65536) : 0x7fffffu - (uint32_t)(i - 65536 - 65);
}
// DevMathF::quot(a, b, refined_rcp(b)) against a / b, bit for bit: per divisor (exponent drawn from [-14, 35]) `per` numerators --
//   even j   a random significand at the exponent of b plus -40 + (j/2) % 91: every exponent distance in [-40, 50]
//   odd j    a = RN(b * q) moved by -1, 0 or +1 units in its last place, q = (m + t) 2**(e - 23) for a random 24-bit m and
//            t = 1/2 - 2**-k (a quotient whose bits go on ...0111...) or t = 1/2 + 2**-k, k in [2, 24], or t = 1/2 (...1000...):
//            quotients next to the boundary between two floats, the hard cases of a rounded division
// and the numerator +0, whose quotient must be +0.  One thread per (divisor, 64 numerators).
__global__ void __launch_bounds__(kBlock)
k_selfcheck_quot(int64_t per, uint64_t seed, unsigned long long *mismatches)
{
    const int64_t chunks = (per + 63) / 64, total = kQuotDivisors * chunks;
    unsigned long long bad = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < total; w += stride) {
        const int64_t ib = w / chunks, c = w - ib * chunks;
        const uint64_t rb = selfcheck_mix(seed ^ (0x5851f42d4c957f2dull * (uint64_t)(ib + 1)));
        const int eb = -14 + (int)((rb >> 32) % 50u);
        const float b = __uint_as_float(((uint32_t)(eb + 127) << 23) | selfcheck_divisor_sig(ib));
        const float y1 = DevMathF::refined_rcp(b);
        if (c == 0) bad += __float_as_uint(DevMathF::quot(0.0f, b, y1)) != 0u || __float_as_uint(0.0f / b) != 0u;
        const int64_t j1 = (c + 1) * 64 < per ? (c + 1) * 64 : per;
        for (int64_t j = c * 64; j < j1; ++j) {
            const uint64_t r = selfcheck_mix(rb + (uint64_t)j);
            const int rel = -40 + (int)((j >> 1) % 91);
            float a;
            if ((j & 1) == 0) {
                a = __uint_as_float(((uint32_t)(eb + rel + 127) << 23) | ((uint32_t)r & 0x7fffffu));
            } else {
                const uint32_t k = 2u + (uint32_t)((r >> 24) % 23u), pick = (uint32_t)(r >> 32) % 3u;
                const double eps = __longlong_as_double((long long)(1023u - k) << 52); // 2**-k
                const double t = pick == 0 ? 0.5 - eps : pick == 1 ? 0.5 + eps : 0.5;
                const double q = ((double)(0x800000u | ((uint32_t)r & 0x7fffffu)) + t) * 0x1p-23; // in [1, 2)
                const double scale = __longlong_as_double((long long)(1023 + rel) << 52);         // 2**rel
                const float a0 = (float)((double)b * q * scale); // normal: exponent within [-55, 87]
                a = __uint_as_float(__float_as_uint(a0) + (uint32_t)(r >> 40) % 3u - 1u);
            }
            bad += __float_as_uint(DevMathF::quot(a, b, y1)) != __float_as_uint(a / b);
        }
    }
    if (bad) atomicAdd(mismatches, bad);
}
// The same over DevMathF::div4's OWN operand box (what = 4): the divisor's exponent drawn from [-21, 52], the numerators
// SIGNED and at absolute magnitudes, by j % 4 the class of
//   n4 = ql*dt   2**-60 <= |a| <= 2**60      n2, n3   2**-45 <= |a| <= 2**52      n1   2**-21 <= a <= 2**52 (positive)
// -- exponent distances from -112 to +81, beyond the 2**96 within which the compiler's own division needs no scaling:
//   j % 8 < 4    a random significand at an exponent uniform over the class's range, 2**hi itself as the top value
//   else         a = RN(d * q) moved by -1, 0, +1 units in its last place for q next to a rounding boundary (as at what = 3),
//                of either sign, at an exponent that keeps a two binades inside the class's range
// and, through div4 itself under the verdict of coef_guard (dt = 1, ql = the numerator, so n4 = ql*dt is the numerator), the
// numerators +0 and -0: +0 passes the guard and takes the three operations, -0 -- what a negative n4 that underflows is --
// must fail it and get the -0 of the IEEE division.  One thread per (divisor, 64 numerators).
struct QuotBox {
    int lo, hi;
    bool is_signed;
};
__device__ __forceinline__ QuotBox selfcheck_box(int64_t j)
{
    const int cls = (int)(j & 3);
    return cls == 0 ? QuotBox{-60, 60, true} : cls == 3 ? QuotBox{-21, 52, false} : QuotBox{-45, 52, true};
}
__global__ void __launch_bounds__(kBlock)
k_selfcheck_quot_box(int64_t per, uint64_t seed, unsigned long long *mismatches)
{
    const int64_t nchunk = per > 0 ? (per + 63) / 64 : 1, total = kQuotDivisors * nchunk; // (per = 0: the zeros alone)
    unsigned long long bad = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < total; w += stride) {
        const int64_t ib = w / nchunk, c = w - ib * nchunk;
        const uint64_t rb = selfcheck_mix(seed ^ (0x5851f42d4c957f2dull * (uint64_t)(ib + 1)));
        const int eb = -21 + (int)((rb >> 32) % 74u);                                         // [-21, 52]
        const uint32_t sig = eb == 52 ? 0u : selfcheck_divisor_sig(ib);                      // (d <= 2**52: the top value itself)
        const float b = __uint_as_float(((uint32_t)(eb + 127) << 23) | sig);
        const float y1 = DevMathF::refined_rcp(b);
        if (c == 0) {
            for (int neg = 0; neg < 2; ++neg) {
                const uint32_t sign = neg ? 0x80000000u : 0u;
                const float z = __uint_as_float(sign);
                DevMathF m{nullptr, false};
                m.coef_ok = coef_guard(1.0f, z);
                float q1, q2, q3, q4;
                m.div4(b, z, z, z, b, q1, q2, q3, q4);
                bad += __float_as_uint(q4) != __float_as_uint(z / b) || __float_as_uint(q4) != sign;
            }
        }
        const int64_t j1 = (c + 1) * 64 < per ? (c + 1) * 64 : per;
        for (int64_t j = c * 64; j < j1; ++j) {
            const uint64_t r = selfcheck_mix(rb + (uint64_t)j);
            const QuotBox box = selfcheck_box(j);
            const uint32_t sign = (box.is_signed && ((r >> 63) & 1u)) ? 0x80000000u : 0u;
            float a;
            if ((j & 4) == 0) {
                a = __uint_as_float(__float_as_uint(selfcheck_draw(r >> 1, box.lo, box.hi)) | sign);
            } else {
                const uint32_t k = 2u + (uint32_t)((r >> 24) % 23u), pick = (uint32_t)(r >> 32) % 3u;
                const double eps = __longlong_as_double((long long)(1023u - k) << 52); // 2**-k
                const double t = pick == 0 ? 0.5 - eps : pick == 1 ? 0.5 + eps : 0.5;
                const double q = ((double)(0x800000u | ((uint32_t)r & 0x7fffffu)) + t) * 0x1p-23; // in [1, 2)
                const int ea = box.lo + 1 + (int)((r >> 44) % (uint32_t)(box.hi - box.lo - 3));   // [lo + 1, hi - 3]
                const double scale = __longlong_as_double((long long)(1023 + ea - eb) << 52);     // |ea - eb| <= 112
                const float a0 = (float)((double)b * q * scale);                                  // in [2**ea, 2**(ea + 2))
                a = __uint_as_float((__float_as_uint(a0) + (uint32_t)(r >> 40) % 3u - 1u) | sign);
            }
            bad += __float_as_uint(DevMathF::quot(a, b, y1)) != __float_as_uint(a / b);
        }
    }
    if (bad) atomicAdd(mismatches, bad);
}

// Hypothesis (1) of DevMathF::quot on the device a plan is about to use, once per device and process: all 2**23 significands.
// A device that fails it gets c_quot_ok = 0 (coef_guard) and `ok` = false (the plan's `sane`): plain divisions everywhere.
int quot_selfcheck(int device, bool *ok)
{
    static std::mutex mu;
    static std::vector<int8_t> known; // per device ordinal: 0 not checked yet, 1 passed, -1 failed
    std::lock_guard<std::mutex> lock(mu);
    if ((size_t)device >= known.size()) known.resize((size_t)device + 1, 0);
    if (known[(size_t)device] == 0) {
        HIP_TRY(hipSetDevice(device));
        DevBuf cnt;
        if (int rc = cnt.ensure(sizeof(unsigned long long))) return rc;
        HIP_TRY(hipMemset(cnt.p, 0, sizeof(unsigned long long)));
        hipLaunchKernelGGL(k_selfcheck_rcp, dim3((1u << 23) / kBlock), dim3(kBlock), 0, 0, 127u, (unsigned long long *)cnt.p);
        HIP_TRY(hipGetLastError());
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, cnt.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad) {
            const int32_t zero = 0;
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_quot_ok), &zero, sizeof zero));
        }
        known[(size_t)device] = bad ? -1 : 1;
    }
    *ok = known[(size_t)device] > 0;
    return 0;
}

int check_device(int device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(TRMC_ENODEVICE, std::string("no HIP device available (") + hipGetErrorString(e)
                                        + "); this library has no CPU fallback");
    if (device < 0 || device >= count)
        return fail(TRMC_EINVAL, "device ordinal " + std::to_string(device) + " out of range [0," + std::to_string(count) + ")");
    return 0;
}

// trmc_window_summary / _courant_summary / _exceedance (abi.inc): the optional per-row columns of a window's product.  lay() puts
// those with a host destination into the plan's scratch block, each on a 256-byte boundary; dev<U>(k) is column k's place on the
// device (NULL for one not asked for); fetch() queues their copies to the host behind whatever wrote them.
struct WindowColumns {
    struct Col {
        void *host;
        size_t row_bytes;
    };
    Col col[7];
    size_t off[7];
    int n = 0;
    int64_t nrows = 0;
    char *base = nullptr;
    int lay(trmc_plan *pl, int64_t rows, std::initializer_list<Col> cols)
    {
        nrows = rows;
        size_t total = 0;
        for (const Col &c : cols) {
            col[n] = c;
            off[n++] = total;
            if (c.host) total += ((size_t)nrows * c.row_bytes + 255) / 256 * 256;
        }
        if (int rc = pl->scratch.ensure(total)) return rc;
        base = (char *)pl->scratch.p;
        return 0;
    }
    template <class U> U *dev(int k) const { return col[k].host ? (U *)(base + off[k]) : nullptr; }
    int fetch(hipStream_t st) const
    {
        for (int k = 0; k < n; ++k)
            if (col[k].host) HIP_TRY(hipMemcpyAsync(col[k].host, base + off[k], (size_t)nrows * col[k].row_bytes, hipMemcpyDeviceToHost, st));
        return 0;
    }
};
// ... and the end of such a call, behind its launch: the timer's second event, the columns' way to the host, the wait for both
int window_product_finish(trmc_plan *pl, KernelTimer &timer, const WindowColumns &cols)
{
    if (int rc = timer.end(pl->stream)) return rc;
    if (int rc = cols.fetch(pl->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(pl->stream));
    return timer.read();
}

// trmc_window_courant / trmc_window_courant_summary (abi.inc): k_window_courant's arguments up to its destinations ...
template <class T> int window_courant_args(trmc_plan *pl, int32_t rowset, CourantArgs<T> &a)
{
    a.par = (const T *)pl->sh->params.p;
    a.nseg_pad = pl->nseg_pad;
    a.up_ptr = (const int32_t *)pl->sh->up_ptr.p;
    a.up_idx = (const int32_t *)pl->sh->up_idx.p;
    a.row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
    a.pos_of_row = (const int32_t *)pl->sh->pos_of_row.p;
    a.res_of_pos = pl->nres > 0 ? (const int32_t *)pl->res_of_pos.p : nullptr;
    const bool raw = pl->ngage > 0 && pl->nraw > 0 && !pl->run.short_ts;
    a.raw_of_pos = raw ? (const int32_t *)pl->raw_of_pos.p : nullptr;
    a.da_raw = raw ? (const T *)pl->da_raw.p : nullptr;
    a.qlat_tm = (const T *)pl->qlat_tm.p;
    a.out = (const T *)pl->out.p;
    if (pl->flow) { // the dataflow engine keeps no time row 0: the state the window began from is still the staged one
        a.s0q = (const T *)pl->in_q0.p;
        a.s0d = a.s0q + 2;
        a.s0_stride = 3;
        a.s0_by_row = 1;
    } else {        // the level engine: time row 0 of the flow and depth planes, which no step of a window writes
        a.s0q = (const T *)pl->tm.p;
        a.s0d = a.s0q + 2 * (size_t)(pl->routed_nsteps + 1) * (size_t)pl->nseg_pad;
        a.s0_stride = 1;
        a.s0_by_row = 0;
    }
    a.rowset_pos = rowset < 0 ? nullptr : (const int32_t *)pl->rowsets[(size_t)rowset].p;
    a.nrows = rowset < 0 ? pl->nseg : pl->rowset_n[(size_t)rowset];
    a.nboundary = (int32_t)pl->sh->topo.nboundary;
    a.nsteps = pl->routed_nsteps;
    a.qts = pl->run.qts;
    a.short_ts = pl->run.short_ts;
    a.stride = 1;
    a.nkeep = pl->routed_nsteps;
    a.sane = pl->params_sane ? 1 : 0;
    a.dst = nullptr;
    a.peak_cn = nullptr;
    a.peak_step = a.steps_over = nullptr;
    a.limit = T(0);
    return 0;
}
// ... and its launch in the plan's arithmetic
template <class T, bool SUMMARY> void window_courant_launch(trmc_plan *pl, const CourantArgs<T> &a)
{
    const dim3 grid((unsigned)((a.nrows + kCourantRows - 1) / kCourantRows)), block(kCourantRows * 64);
    if constexpr (std::is_same<T, float>::value) {
        if (pl->opt.tol) {
            hipLaunchKernelGGL((k_window_courant<float, true, SUMMARY>), grid, block, 0, pl->stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((k_window_courant<T, false, SUMMARY>), grid, block, 0, pl->stream, a);
}

// trmc_window_exceedance (abi.inc): k_window_exceed's instance for the plan's precision, the alignment of the rows' records, the
// column of (q, v, d) and the width of the threshold table's rows, on the plan's stream
template <class T, bool VEC, int COL> int window_exceed_launch_kp(trmc_plan *pl, const int32_t *rp, const WexcOut &o, int64_t nrows, int32_t nsteps)
{
    const dim3 grid((unsigned)((nrows + kRecRows - 1) / kRecRows)), block(kRecRows);
    const T *const out = (const T *)pl->out.p, *const th = (const T *)pl->thresholds.p;
    const int32_t *const row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
    switch (pl->th_pad) {
    case 1: hipLaunchKernelGGL((k_window_exceed<T, VEC, COL, 1>), grid, block, 0, pl->stream, out, rp, row_of_pos, th, o, nrows, nsteps, pl->th_levels); break;
    case 2: hipLaunchKernelGGL((k_window_exceed<T, VEC, COL, 2>), grid, block, 0, pl->stream, out, rp, row_of_pos, th, o, nrows, nsteps, pl->th_levels); break;
    case 4: hipLaunchKernelGGL((k_window_exceed<T, VEC, COL, 4>), grid, block, 0, pl->stream, out, rp, row_of_pos, th, o, nrows, nsteps, pl->th_levels); break;
    default: return fail(TRMC_ESTATE, "no thresholds set on this plan (trmc_plan_set_thresholds)");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
template <class T, bool VEC> int window_exceed_launch_col(trmc_plan *pl, const int32_t *rp, int column, const WexcOut &o, int64_t nrows, int32_t nsteps)
{
    switch (column) {
    case 0: return window_exceed_launch_kp<T, VEC, 0>(pl, rp, o, nrows, nsteps);
    case 1: return window_exceed_launch_kp<T, VEC, 1>(pl, rp, o, nrows, nsteps);
    case 2: return window_exceed_launch_kp<T, VEC, 2>(pl, rp, o, nrows, nsteps);
    }
    return fail(TRMC_EINVAL, "unknown quantity");
}
int window_exceed_launch(trmc_plan *pl, int32_t rowset, int column, const WexcOut &o, int64_t nrows, int32_t nsteps)
{
    const int32_t *const rp = rowset < 0 ? nullptr : (const int32_t *)pl->rowsets[(size_t)rowset].p;
    return by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        // (16-byte loads where every row's record starts on a 16-byte boundary: k_window_exceed's head)
        if (nsteps % (16 / (int)sizeof(T)) == 0) return window_exceed_launch_col<T, true>(pl, rp, column, o, nrows, nsteps);
        return window_exceed_launch_col<T, false>(pl, rp, column, o, nrows, nsteps);
    });
}
