// k_stream_courant -- THE COURANT NUMBER OF EVERY ROW OVER A WHOLE STREAM OF DAYS (trmc_stream_set_courant, trmc_stream_courant;
// launched by stream_complete_day, stream.inc, beside k_stream_summary and k_stream_exceed).  The definition is the window
// summary's (k_window_courant.inc, SUMMARY): cn[t] = courant_at(h[t]) in the plan's precision and arithmetic, and per row
//   peak_cn       pk = cn[1]; t = 2..: if (cn[t] > pk) -- the first of equal peaks wins, a NaN never replaces a number, a NaN at the
//                 stream's step 1 stays
//   peak_cn_step  the step the peak was first reached at
//   steps_over    number of steps t with cn[t] > limit, compared in T (a NaN is not counted)
// with t counted on over the days, 1-based from the stream's first step.  Reservoir rows of every type and boundary rows route no
// Muskingum-Cunge step: (0, 1, 0).  Not a product of the day: the state lives in an accumulator outside the ring, as the
// exceedance's does, and this kernel folds one day into it, in day order.
//
// NO SECANT SOLVE.  The window kernel re-runs mc_segment_step for every row-step because it also hands out X; cn needs only the
// depth h that courant_at is evaluated at, and that depth is already in the ring: where the step had flow it is the depth the step
// ended on (mc_segment_step: out.h = out.depthc = s.h) -- the row's stored depth of step t -- and where it had none it is
// step_bracket(depthp), depthp the row's stored depth of step t - 1.  Which of the two is step_has_flow of (ql, qup, quc = qup,
// qdp): the forcing and flows of step t - 1, all in the day's slot.  A gage's stored flow is the nudged one -- what the next step
// and the rows below were fed -- and nudging changes the flow only, so the triple is the un-nudged step's, as the window's is.
// One courant_at and a few loads per row-step.
//
// WALK: k_stream_exceed's.  One thread per plan position, time runs in the thread over the slot's time-major planes, so a
// wavefront's load of a time row is 64 consecutive elements; kStreamCourantUnroll steps' loads -- the row's flow and depth, the
// forcing column, every upstream row's flow -- are issued before the first courant_at that depends on them.  Once per thread: the
// nine parameters from the plan's columns, make_const in the exact policy (as a plan's constants: k_make_const), the CSR range.
// qup is summed in T in CSR order from 0, as mc_step_rows and the tile kernels do.
// STEP 0 OF A DAY -- flow and depth of the day before's last step, or the stream's initial state -- is time row 0 of the day's
// slot in both planes: where the tile launches start the day from (hand_on_row writes both at a day's end under every instance,
// k_init_state for day 0, k_stream_first_obs a gage's first observation).  The rows that end the day slots - 1 days later write that
// row again: the launches of a push go behind the last fold queued (stream.inc, ORDER).
// DEPTH OF STEPS 1..nsteps: the slot's depth plane where the tile launches write it at every step (k_mc_tile_dpl, k_mc_ctile_dpl),
// or, in a stream with full_output, the day's out[row][step][2] -- the same bits; one kernel, two addressings: the depth of step
// t of position p is d1[x * d_row + (t - 1) * d_step] with (x, d_row, d_step) = (p, 1, nseg_pad) or (row_of_pos[p], 3 nsteps, 3).
// STATE: peak T [nseg_pad], step int32 [nseg_pad], count int32 [nseg_pad] in PLAN order, read once and written once per row and
// day; trmc_stream_push_day refuses the day that would take the stream's step count past INT32_MAX; k_stream_courant_rows brings
// it into row order and widens to int64 on the way to the host.  Resource usage: profiles/r27_resource_usage.txt.
constexpr int kStreamCourantUnroll = 8;

template <class T> struct StreamCourantArgs {
    const T *par;               // the plan's parameter columns [TRMC_NPARAM][nseg_pad], plan order
    int64_t nseg_pad;
    const int32_t *up_ptr, *up_idx;
    const int32_t *res_of_pos;  // nullptr: no reservoirs
    const int32_t *row_of_pos;  // nullptr: the depths come from the plane (x = p); else from the full result (x = row)
    const T *q_tm;              // the slot's flow plane [nsteps + 1][nseg_pad]
    const T *d0;                // time row 0 of the slot's depth plane
    const T *d1;                // depth of step 1 of x = 0 (see the head)
    int64_t d_row, d_step;
    const T *qlat;              // the slot's forcing [nq][nseg_pad]
    T *peak;                    // the accumulator
    int32_t *step, *count;
    int32_t nseg, nboundary, nsteps, qts, t0, sane;
    T limit;
};

template <class T, bool TOL>
__global__ void __launch_bounds__(kBlock)
k_stream_courant(const StreamCourantArgs<T> a)
{
    using M = typename DevMath<T, TOL>::type;
    using MX = typename DevMath<T, false>::type; // (the segment-invariant constants are exact in either arithmetic: k_make_const)
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    M m{stage_pow_tables(s_tab), false};
    const MX mx{s_tab, false};
    m.sane = a.sane != 0;
    const int32_t pos = blockIdx.x * kBlock + threadIdx.x;
    if (pos >= a.nseg) return;
    if (pos < a.nboundary || (a.res_of_pos && a.res_of_pos[pos] >= 0)) { // (no Muskingum-Cunge step is routed here)
        a.peak[pos] = T(0);
        a.step[pos] = 1;
        a.count[pos] = 0;
        return;
    }
    const size_t np = (size_t)a.nseg_pad;
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
    int32_t at = a.step[pos], over = a.count[pos];
    int32_t tg = a.t0 + 1; // the step's number in the stream
    const T *const q = a.q_tm + pos;                                  // (time row 0)
    const T *const d = a.d1 + (size_t)(a.row_of_pos ? a.row_of_pos[pos] : pos) * (size_t)a.d_row;
    const size_t ds = (size_t)a.d_step;
    const T *const ql = a.qlat + pos;
    T d_prev = a.d0[pos];
    int32_t ql_col = 0, ql_left = a.qts; // the forcing column of step t is (t - 1) / qts: by a counter
    // step t from: the flows of step t - 1 (own, upstream sum), the forcing, the depths of steps t - 1 and t
    auto step = [&](T qdp, T qup, T qlv, T d_new) {
        trmc::Inflow<T> f;
        f.qup = qup;
        f.quc = qup; // (assume_short_ts: a stream's rows read flows of step t - 1 only)
        f.qdp = qdp;
        f.ql = qlv;
        T h = d_new, h_0;
        if (!trmc::step_has_flow(f)) trmc::step_bracket(d_prev, h, h_0);
        T ck, cn;
        trmc::courant_at<T, M>(h, p, c, ck, cn, m);
        if (tg == 1 || cn > pk) { // (the first of equal peaks wins; a NaN never replaces a number; the stream's step 1 stands)
            pk = cn;
            at = tg;
        }
        over += cn > a.limit ? 1 : 0; // (ordered compare: a NaN is not counted)
        d_prev = d_new;
        ++tg;
    };
    int32_t t = 1;
    for (; t + kStreamCourantUnroll - 1 <= a.nsteps; t += kStreamCourantUnroll) {
        T qv[kStreamCourantUnroll], dv[kStreamCourantUnroll], lv[kStreamCourantUnroll], uv[kStreamCourantUnroll];
#pragma unroll
        for (int j = 0; j < kStreamCourantUnroll; ++j) {
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
            T w[kStreamCourantUnroll];
#pragma unroll
            for (int j = 0; j < kStreamCourantUnroll; ++j) w[j] = qu[(size_t)(t - 1 + j) * np];
#pragma unroll
            for (int j = 0; j < kStreamCourantUnroll; ++j) uv[j] += w[j];
        }
#pragma unroll
        for (int j = 0; j < kStreamCourantUnroll; ++j) step(qv[j], uv[j], lv[j], dv[j]);
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
    a.step[pos] = at;
    a.count[pos] = over;
}

// the accumulator for the host: [nseg] arrays in ROW order, the steps and the counts widened to int64 (any may be nullptr), one
// thread per row
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_courant_rows(const T *__restrict__ peak, const int32_t *__restrict__ step, const int32_t *__restrict__ count,
                      const int32_t *__restrict__ pos_of_row, T *__restrict__ out_peak, int64_t *__restrict__ out_step,
                      int64_t *__restrict__ out_count, int32_t nseg)
{
    const int32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nseg) return;
    const size_t p = (size_t)pos_of_row[r];
    if (out_peak) out_peak[r] = peak[p];
    if (out_step) out_step[r] = step[p];
    if (out_count) out_count[r] = count[p];
}
