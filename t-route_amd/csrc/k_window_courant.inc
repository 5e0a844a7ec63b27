// k_window_courant -- the Courant metrics (cn, ck, X) of every row-step of the LAST routed window, recomputed from what the plan
// still holds after it (trmc_window_courant / trmc_window_courant_summary, abi.inc).  The reference can leave the triple beside a
// step's (q, v, d) (mc_reach.pyx:128-131: output_buf[3:6] = cn, ck, X); here no routing kernel forms it.  It need not: the triple of
// row r at step t is a pure function of
//     the row's channel parameters and dt;   ql = qlat[r, (t - 1) / qts];   qdp = q[r, t-1], depthp = d[r, t-1];
//     qup = sum of q[u, t-1] over the upstream rows u, quc = sum of q[u, t] (assume_short_ts: quc = qup, mc_reach.pyx:504-505)
// -- the inputs the routing kernels fed the same mc_segment_step with -- and all of them are still on the device: q and d of
// steps 1..nsteps in the assembled result out[row][step][3], step 0 in the window's initial state, the forcing in qlat_tm.  Same
// function, same inputs, same bits; and since no step waits for another one, all row-steps of a window are independent.
//
// LAYOUT.  A WAVEFRONT takes one row and walks its kept steps 64 at a time, lane = step.  Everything that belongs to the row is
// then wave-uniform and lives in scalar registers (the index of the row is made uniform with readfirstlane, so the nine
// parameters, the CSR range and the upstream rows are scalar loads): the constants of make_const are formed once per row, not
// once per step.  What a lane loads is q and d of ITS step of the row and q of its step of every upstream row: consecutive lanes
// 12 B (3 elements) apart, a wave-load 768 contiguous bytes of `out` (fp32, stride 1), and q and d of a step share a sector.
// The forcing column (t - 1) / qts changes once in qts lanes.  Neighbouring steps of a row take alike numbers of secant
// iterations, so the lanes of a wavefront mostly leave the loop together.  A block is kCourantRows = 4 wavefronts on four
// consecutive rows of the output, sharing the staged power tables; the tile is 4 rows x 64 steps in either precision.
//
// Sums over the upstream rows are taken in T in CSR order starting from 0, as mc_step_rows does (the reference's order,
// mc_reach.pyx:499-502); a headwater gets qup = quc = 0.  A gage's stored flow is the nudged one, which is what the next step and
// the rows below were fed (mc_reach.pyx:733); the segment below a gage INSIDE a reach (general mode, trmc_set_nudging_successors)
// was fed the gage row's flow before the nudge, which the window left in da_raw: it is read from there.  The triple itself is that
// of the un-nudged step.  Reservoir rows of any type route no Muskingum-Cunge step and boundary rows are inputs only: (0, 0, 0).
//
// SUMMARY = false: dst[i][k][3] = (cn, ck, X) of step (k + 1) * stride, k < nkeep -- only the kept steps are computed.
// SUMMARY = true (stride 1): per row the highest cn, the 1-based step it was FIRST reached at and the number of steps with
// cn > limit, the compare in T.  Across the lanes: a butterfly of (value, step) pairs under k_window_summary's rule -- a later
// step replaces an earlier one only if its cn is greater, an earlier one a later one unless that is greater, and the cn of
// step 1 stands whatever it is (pk = cn[1]; t = 2..: if (cn[t] > pk)): the first of equal peaks wins, a NaN never replaces a
// number and a NaN at step 1 stays.  Chunk after chunk the same rule folds the wavefront's pair into the row's.
// Resource usage: profiles/r19_resource_usage.txt.
constexpr int kCourantRows = 4, kCourantSteps = 64;

template <class T> struct CourantArgs {
    const T *par;                 // the plan's parameter columns [TRMC_NPARAM][nseg_pad], plan order
    int64_t nseg_pad;
    const int32_t *up_ptr, *up_idx, *row_of_pos, *pos_of_row;
    const int32_t *res_of_pos;    // nullptr: no reservoirs
    const int32_t *raw_of_pos;    // nullptr, or (general mode): gage whose un-nudged flow of the step a position reads as quc
    const T *da_raw;              // [gage][nsteps]
    const T *qlat_tm;             // [nq][nseg_pad]
    const T *out;                 // [nseg][nsteps][3]
    // step 0 of index x (a plan position, or a row if s0_by_row): flow s0q[x * s0_stride], depth s0d[x * s0_stride]
    const T *s0q, *s0d;
    int32_t s0_stride, s0_by_row;
    const int32_t *rowset_pos;    // nullptr: output i = row i
    int64_t nrows;
    int32_t nboundary, nsteps, qts, short_ts, stride, nkeep, sane;
    T *dst;                       // block
    T *peak_cn;                   // summary (any may be nullptr)
    int32_t *peak_step, *steps_over;
    T limit;
};

// (a, ta) <- the winner of (a, ta) and (b, tb), ta != tb, under an ORDER that gives what the walk in step order gives: a NaN at
// step 1 beats everything (the walk starts at it and no compare against it holds), a NaN at any other step loses to everything
// (no compare of it holds), numbers by value and, equal, the earlier step.  An order, so the fold is associative and symmetric:
// a butterfly may take the pairs in any grouping, and both partners of an exchange keep the same winner.
template <class T> __device__ __forceinline__ void courant_fold(T &a, int32_t &ta, T b, int32_t tb)
{
    const bool a_nan = a != a, b_nan = b != b;
    const bool a_first = a_nan && ta == 1, b_first = b_nan && tb == 1;
    const bool b_better = a_nan || b > a || (b == a && tb < ta); // (a NaN b against a number a: none of the three holds)
    if (b_first || (!a_first && b_better)) {
        a = b;
        ta = tb;
    }
}

template <class T, bool TOL, bool SUMMARY>
__global__ void __launch_bounds__(kCourantRows * 64)
k_window_courant(const CourantArgs<T> a)
{
    using M = typename DevMath<T, TOL>::type;
    using MX = typename DevMath<T, false>::type; // (the segment-invariant constants are exact in either arithmetic, as in a plan: k_make_const)
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    M m{stage_pow_tables(s_tab), false};
    const MX mx{s_tab, false};
    m.sane = a.sane != 0;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kCourantRows + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= a.nrows) return;
    const int32_t pos = a.rowset_pos ? a.rowset_pos[i] : a.pos_of_row[i];
    const int64_t row = a.row_of_pos[pos];
    const bool routed = pos >= a.nboundary && !(a.res_of_pos && a.res_of_pos[pos] >= 0);

    T pk = T(0);
    int32_t at = 1, over = 0;
    if (routed) {
        trmc::ChannelParams<T> p;
        {
            const T *c = a.par + pos;
            p.dt = c[(size_t)TRMC_P_DT * a.nseg_pad];
            p.dx = c[(size_t)TRMC_P_DX * a.nseg_pad];
            p.bw = c[(size_t)TRMC_P_BW * a.nseg_pad];
            p.tw = c[(size_t)TRMC_P_TW * a.nseg_pad];
            p.twcc = c[(size_t)TRMC_P_TWCC * a.nseg_pad];
            p.n = c[(size_t)TRMC_P_N * a.nseg_pad];
            p.ncc = c[(size_t)TRMC_P_NCC * a.nseg_pad];
            p.cs = c[(size_t)TRMC_P_CS * a.nseg_pad];
            p.s0 = c[(size_t)TRMC_P_S0 * a.nseg_pad];
        }
        const trmc::ChannelConst<T> c = trmc::make_const<T, MX>(p, mx);
        const int32_t k0 = a.up_ptr[pos], k1 = a.up_ptr[pos + 1];
        const int32_t graw = (!a.short_ts && a.raw_of_pos) ? a.raw_of_pos[pos] : -1;
        const T *const own = a.out + row * (int64_t)a.nsteps * 3;
        const int64_t own0 = (a.s0_by_row ? row : (int64_t)pos) * a.s0_stride;

        for (int32_t kb = 0; kb < a.nkeep; kb += kCourantSteps) {
            const int32_t k = kb + lane;
            const bool live = k < a.nkeep;
            T cn = T(0), ck = T(0), X = T(0);
            const int32_t t = live ? (k + 1) * a.stride : 0; // 1-based step, <= nsteps
            if (live) {
                trmc::Inflow<T> f;
                T depthp;
                if (t == 1) {
                    f.qdp = a.s0q[own0];
                    depthp = a.s0d[own0];
                } else {
                    f.qdp = own[(int64_t)(t - 2) * 3];
                    depthp = own[(int64_t)(t - 2) * 3 + 2];
                }
                f.ql = a.qlat_tm[(size_t)((t - 1) / a.qts) * (size_t)a.nseg_pad + (size_t)pos];
                T qup = T(0), quc = T(0);
                for (int32_t e = k0; e < k1; ++e) {
                    const int32_t u = a.up_idx[e];
                    const int64_t urow = a.row_of_pos[u];
                    const T *const uo = a.out + urow * (int64_t)a.nsteps * 3;
                    qup += (t == 1) ? a.s0q[(a.s0_by_row ? urow : (int64_t)u) * a.s0_stride] : uo[(int64_t)(t - 2) * 3];
                    if (!a.short_ts) quc += uo[(int64_t)(t - 1) * 3];
                }
                if (graw >= 0) quc = a.da_raw[(size_t)graw * (size_t)a.nsteps + (size_t)(t - 1)]; // (its one upstream row is that gage)
                f.qup = qup;
                f.quc = a.short_ts ? qup : quc;
                m.coef_ok = coef_guard(p.dt, f.ql);
                const trmc::StepResult<T> r = trmc::mc_segment_step<T, M>(p, c, f, depthp, m, false);
                trmc::courant_at<T, M>(r.h, p, c, ck, cn, m);
                X = r.X;
            }
            if constexpr (!SUMMARY) {
                if (live) {
                    T *const o = a.dst + ((int64_t)i * a.nkeep + k) * 3;
                    o[0] = cn;
                    o[1] = ck;
                    o[2] = X;
                }
            } else {
                // lanes beyond the chunk's end take part with the chunk's first step (a copy never wins against its original)
                const T first = __shfl(cn, 0);
                const int32_t first_t = __shfl(t, 0);
                T v = live ? cn : first;
                int32_t vt = live ? t : first_t;
                over += __popcll(__ballot(live && cn > a.limit));
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const T w = __shfl_xor(v, d);
                    const int32_t wt = __shfl_xor(vt, d);
                    if (wt != vt) courant_fold(v, vt, w, wt);
                }
                if (kb == 0) {
                    pk = v;
                    at = vt;
                } else
                    courant_fold(pk, at, v, vt);
            }
        }
    } else if constexpr (!SUMMARY) {
        for (int64_t e = lane; e < (int64_t)a.nkeep * 3; e += 64) a.dst[i * a.nkeep * 3 + e] = T(0);
    }
    if constexpr (SUMMARY) {
        if (lane == 0) {
            if (a.peak_cn) a.peak_cn[i] = pk;
            if (a.peak_step) a.peak_step[i] = at;
            if (a.steps_over) a.steps_over[i] = over;
        }
    }
}
