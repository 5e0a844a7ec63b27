// k_stream_velocity -- PEAK VELOCITY AND VELOCITY-THRESHOLD EXCEEDANCE OF EVERY ROW OVER A WHOLE STREAM OF DAYS
// (trmc_stream_set_velocity, trmc_stream_velocity; launched by stream_complete_day, stream.inc, beside k_stream_exceed,
// k_stream_courant and k_stream_exceed_depth).  v[t] is column 1 of the same days routed as a window on the same plan, in the
// plan's precision and arithmetic, and per row
//   peak_velocity       pk = v[1]; t = 2..: if (v[t] > pk) -- the first of equal peaks wins, a NaN never replaces a number, a NaN at
//                       the stream's step 1 stays (the window summary's rule, k_window_summary.inc)
//   peak_velocity_step  the step the peak was first reached at
// and, against a threshold table of KP > 0 levels (m/s), k_stream_exceed's four figures on velocity: over(t) := v[t] > th[row][k],
// compared in T -- false when either side is a NaN, equality is not over -- steps_over, first_step, last_step, longest_run; a run
// that is open at a day's last step goes on at the next day's first.  t is counted on over the days, 1-based from the stream's
// first step.  Not a product of the day: the state lives in an accumulator outside the ring and this kernel folds one day into it,
// in day order.
//
// NO SECANT SOLVE, AND NO VELOCITY IN THE TILE KERNELS.  A products-only stream forms no velocity in its step loop (LAZYV).  The
// velocity of a step is step_velocity at the depth the step ended on, and 0 where the step had no flow (mc_segment_step); the depth
// is the row's stored depth of step t, and whether the step had flow is step_has_flow of (ql, qup, quc = qup, qdp): the forcing and
// the flows of step t - 1, all in the day's slot -- what the LAZYV instances do out of line for a kept step (it_last > 0).  A gage's
// stored flow is the nudged one -- what the next step and the rows below were fed -- and nudging changes the flow only, so v is the
// un-nudged step's, as the window's is.
// ROWS THAT ROUTE NO MUSKINGUM-CUNGE STEP: a reservoir row of every type hands out v = 0 at every step (reservoir_row,
// k_tile_row.inc: v_new = 0; its depth slot is the pool's elevation and is not read here); a boundary row is routed by nobody in a
// stream (its flows are prescribed, its velocity and depth are the zeros of the planes and of the full result).  Both: v[t] = 0, so
// (0, 1) for the peak, and every step is over a NEGATIVE threshold, as the rule says.
// TWO BODIES OF step_velocity: it takes one of two straight-line bodies by the wavefront-uniform m.all(fast_ok).  A wavefront here
// holds other rows than a tile kernel's, so the verdict may differ for the same row-step; the bodies agree bit for bit wherever the
// fast one is allowed -- sqrt_r is the correctly rounded root sqrtf is, div1's quot the correctly rounded quotient the division is
// (DevMathF::quot), the in-range logarithm and power the general ones without their special-value tests (det_pow.h) -- the tolerance
// policy's two bodies are the same instructions and fp64 has one.  tests/test_gpu_guard_edges.py pins the agreement.
//
// WALK: k_stream_courant's.  One thread per plan position, time runs in the thread over the slot's time-major planes, so a
// wavefront's load of a time row is 64 consecutive elements; kStreamVelocityUnroll steps' loads -- the row's flow and depth, the
// forcing column, every upstream row's flow -- are issued before the first step_velocity that depends on them.  Once per thread: the
// nine parameters from the plan's columns, make_const in the exact policy (as a plan's constants: k_make_const), the CSR range.
// qup is summed in T in CSR order from 0, as mc_step_rows and the tile kernels do.
// STEP 0 OF A DAY -- the flows of the day before's last step, or the stream's initial state -- is time row 0 of the day's slot in
// the flow plane.  The rows that end the day slots - 1 days later write that row again: the launches of a push go behind the last
// fold queued (stream.inc, ORDER).
// DEPTH OF STEPS 1..nsteps: the slot's depth plane where the tile launches write it at every step (k_mc_tile_dpl, k_mc_ctile_dpl),
// or, in a stream with full_output, the day's out[row][step][2] -- the same bits; one kernel, two addressings: the depth of step
// t of position p is d1[x * d_row + (t - 1) * d_step] with (x, d_row, d_step) = (p, 1, nseg_pad) or (row_of_pos[p], 3 nsteps, 3).
// The velocity is recomputed from the depth in both, one code path; it equals out[row][step][1] where the full result exists.
// THRESHOLDS: [nseg][KP] in ROW order, KP in {1, 2, 4}, +inf -- never over -- behind the K levels asked for, ONE vector load per row
// through row_of_pos from a 256-byte-aligned base (k_stream_exceed_depth's table).  KP = 0: peak and step only.
// STATE in PLAN order, read once and written once per row and day: peak T [nseg_pad], step int32 [nseg_pad], and with KP > 0
// int32 acc[5][KP][nseg_pad] -- count, first, last, longest, current run; trmc_stream_push_day refuses the day that would take the
// stream's step count past INT32_MAX; k_stream_velocity_rows brings the peak into row order and widens the step to int64,
// k_stream_exceed_depth_rows (the same layout) the four figures.  Resource usage: profiles/r30_resource_usage.txt.
constexpr int kStreamVelocityUnroll = 8;

template <class T> struct StreamVelocityArgs {
    const T *par;               // the plan's parameter columns [TRMC_NPARAM][nseg_pad], plan order
    int64_t nseg_pad;
    const int32_t *up_ptr, *up_idx;
    const int32_t *res_of_pos;  // nullptr: no reservoirs
    const int32_t *row_of_pos;
    const T *q_tm;              // the slot's flow plane [nsteps + 1][nseg_pad]
    const T *d1;                // depth of step 1 of x = 0 (see the head)
    int64_t d_row, d_step;
    const T *qlat;              // the slot's forcing [nq][nseg_pad]
    const T *th;                // the threshold table (KP > 0)
    T *peak;                    // the accumulator
    int32_t *step, *acc;
    int32_t nseg, nboundary, nsteps, qts, t0, sane, by_row;
};

template <class T, bool TOL, int KP>
__global__ void __launch_bounds__(kBlock)
k_stream_velocity(const StreamVelocityArgs<T> a)
{
    static_assert(KP == 0 || KP == 1 || KP == 2 || KP == 4, "no table, or 1, 2 or 4 padded levels");
    constexpr int KN = KP > 0 ? KP : 1; // (arrays of KP = 0 levels: one unused element)
    using M = typename DevMath<T, TOL>::type;
    using MX = typename DevMath<T, false>::type; // (the segment-invariant constants are exact in either arithmetic: k_make_const)
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    M m{stage_pow_tables(s_tab), false};
    const MX mx{s_tab, false};
    m.sane = a.sane != 0;
    const int32_t pos = blockIdx.x * kBlock + threadIdx.x;
    if (pos >= a.nseg) return;
    const size_t np = (size_t)a.nseg_pad;
    const size_t row = (size_t)a.row_of_pos[pos];
    T lim[KN];
    int32_t cnt[KN], first[KN], last[KN], best[KN], run[KN];
    int32_t *const ac = KP > 0 ? a.acc + pos : nullptr;
    auto at = [&](int f, int k) -> int32_t & { return ac[(size_t)(f * KP + k) * np]; };
    if constexpr (KP == 1) {
        lim[0] = a.th[row];
    } else if constexpr (KP > 1) { // (the table's rows are KP * sizeof(T) apart from a 256-byte-aligned base)
        typedef T TV __attribute__((ext_vector_type(KN)));
        const TV x = *reinterpret_cast<const TV *>(a.th + row * KP);
#pragma unroll
        for (int k = 0; k < KP; ++k) lim[k] = x[k];
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        cnt[k] = at(0, k);
        first[k] = at(1, k);
        last[k] = at(2, k);
        best[k] = at(3, k);
        run[k] = at(4, k);
    }
    int32_t tg = a.t0 + 1; // the step's number in the stream
    auto exceed = [&](T v) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool over = v > lim[k]; // (ordered compare: false when either side is a NaN)
            cnt[k] += over ? 1 : 0;
            first[k] = (over && first[k] == 0) ? tg : first[k];
            last[k] = over ? tg : last[k];
            run[k] = over ? run[k] + 1 : 0;
            best[k] = max(best[k], run[k]);
        }
    };
    auto store_levels = [&]() {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            at(0, k) = cnt[k];
            at(1, k) = first[k];
            at(2, k) = last[k];
            at(3, k) = best[k];
            at(4, k) = run[k];
        }
    };
    if (pos < a.nboundary || (a.res_of_pos && a.res_of_pos[pos] >= 0)) { // (no Muskingum-Cunge step is routed here: v = 0)
        a.peak[pos] = T(0);
        a.step[pos] = 1;
        if constexpr (KP > 0) {
            for (int32_t t = 1; t <= a.nsteps; ++t, ++tg) exceed(T(0));
            store_levels();
        }
        return;
    }
    trmc::ChannelParams<T> p;
    {
        const T *c = a.par + pos;
        p.dt = c[(size_t)TRMC_P_DT * np];
        p.dx = c[(size_t)TRMC_P_DX * np];
        p.bw = c[(size_t)TRMC_P_BW * np];
        p.tw = c[(size_t)TRMC_P_TW * np];
        p.twcc = c[(size_t)TRMC_P_TWCC * np];
        p.n = c[(size_t)TRMC_P_N * np];
        p.ncc = c[(size_t)TRMC_P_NCC * np];
        p.cs = c[(size_t)TRMC_P_CS * np];
        p.s0 = c[(size_t)TRMC_P_S0 * np];
    }
    const trmc::ChannelConst<T> c = trmc::make_const<T, MX>(p, mx);
    const int32_t k0 = a.up_ptr[pos], k1 = a.up_ptr[pos + 1];
    T pk = a.peak[pos];
    int32_t pk_at = a.step[pos];
    const T *const q = a.q_tm + pos;                                  // (time row 0)
    const T *const d = a.d1 + (a.by_row ? row : (size_t)pos) * (size_t)a.d_row;
    const size_t ds = (size_t)a.d_step;
    const T *const ql = a.qlat + pos;
    int32_t ql_col = 0, ql_left = a.qts; // the forcing column of step t is (t - 1) / qts: by a counter
    // step t from: the flows of step t - 1 (own, upstream sum), the forcing, the depth of step t
    auto step = [&](T qdp, T qup, T qlv, T d_new) {
        trmc::Inflow<T> f;
        f.qup = qup;
        f.quc = qup; // (assume_short_ts: a stream's rows read flows of step t - 1 only)
        f.qdp = qdp;
        f.ql = qlv;
        T v = T(0);
        if (trmc::step_has_flow(f)) v = trmc::step_velocity<T, M>(p, c, d_new, m);
        if (tg == 1 || v > pk) { // (the first of equal peaks wins; a NaN never replaces a number; the stream's step 1 stands)
            pk = v;
            pk_at = tg;
        }
        exceed(v);
        ++tg;
    };
    int32_t t = 1;
    for (; t + kStreamVelocityUnroll - 1 <= a.nsteps; t += kStreamVelocityUnroll) {
        T qv[kStreamVelocityUnroll], dv[kStreamVelocityUnroll], lv[kStreamVelocityUnroll], uv[kStreamVelocityUnroll];
#pragma unroll
        for (int j = 0; j < kStreamVelocityUnroll; ++j) {
            qv[j] = q[(size_t)(t - 1 + j) * np];
            dv[j] = d[(size_t)(t - 1 + j) * ds];
            if (ql_left == 0) {
                ++ql_col;
                ql_left = a.qts;
            }
            --ql_left;
            lv[j] = ql[(size_t)ql_col * np];
            uv[j] = T(0);
        }
        for (int32_t e = k0; e < k1; ++e) {
            const T *const qu = a.q_tm + a.up_idx[e];
            T w[kStreamVelocityUnroll];
#pragma unroll
            for (int j = 0; j < kStreamVelocityUnroll; ++j) w[j] = qu[(size_t)(t - 1 + j) * np];
#pragma unroll
            for (int j = 0; j < kStreamVelocityUnroll; ++j) uv[j] += w[j];
        }
#pragma unroll
        for (int j = 0; j < kStreamVelocityUnroll; ++j) step(qv[j], uv[j], lv[j], dv[j]);
    }
    for (; t <= a.nsteps; ++t) {
        if (ql_left == 0) {
            ++ql_col;
            ql_left = a.qts;
        }
        --ql_left;
        T qup = T(0);
        for (int32_t e = k0; e < k1; ++e) qup += a.q_tm[(size_t)(t - 1) * np + (size_t)a.up_idx[e]];
        step(q[(size_t)(t - 1) * np], qup, ql[(size_t)ql_col * np], d[(size_t)(t - 1) * ds]);
    }
    a.peak[pos] = pk;
    a.step[pos] = pk_at;
    store_levels();
}

// the peak for the host: [nseg] arrays in ROW order, the step widened to int64 (either may be nullptr), one thread per row
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_velocity_rows(const T *__restrict__ peak, const int32_t *__restrict__ step, const int32_t *__restrict__ pos_of_row,
                       T *__restrict__ out_peak, int64_t *__restrict__ out_step, int32_t nseg)
{
    const int32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nseg) return;
    const size_t p = (size_t)pos_of_row[r];
    if (out_peak) out_peak[r] = peak[p];
    if (out_step) out_step[r] = step[p];
}
