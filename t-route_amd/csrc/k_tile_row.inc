// k_tile_row.inc -- included by kernels_levels.inc in front of mc_step_rows (same namespace, same StepArgs).
//
// What a thread does with ITS ROW in the same way whichever kernel it runs in: the parameter and constant loads of mc_step_rows,
// mc_tile_rows and mc_ctile_rows, and, of the time loop of the two tile kernels (k_mc_tile: the slices, k_mc_ctile: the cluster
// tiles), the branches that read tables -- the level-pool reservoir row with its data assimilation, the nudged gage -- and the
// stores that hand a row's state on at the end of a tile and of a day.  Each is inlined into the loops with the loops' own
// locals, and COLD arguments (see cold_args) are read through `cold` at their use.
//
// The rest of the step still stands in both loops, because the kernels did not come out register for register the same with
// it here (make resource-usage, spill counts included; k_mc_step* did not move in any of these builds):
//   the segment step with its cost bookkeeping (mc_segment_step, it_last / over_last / it_acc), as one function: other VGPR
//     counts, scratch sizes and spill counts in 26 of the 28 tile instances -- k_mc_tile<double, 0, 0, 0> 171 -> 175 VGPRs,
//     k_mc_tile<float, 0, 0, 1> 20 -> 12 B of scratch, k_mc_ctile<float, 0, 0, 1> 30 -> 26 spilled SGPRs -- by reference and
//     by value alike;
//   staging, the runs and the kept steps, as one function: k_mc_ctile_rda<true> 126 -> 128 VGPRs, k_mc_tile<float, 0, 1, 0>
//     44 -> 52 B of scratch, k_mc_tile<float, 1, 1, 0> 11 -> 15 spilled VGPRs;
//   the counters of the forcing column (ql_col, ql_left, coef_guard) and of the kept velocities (v_every, v_left, want_v):
//     each alone changes nothing, either of them TOGETHER with the reservoir and gage branches below moves the spilled SGPRs
//     of eight k_mc_ctile instances by one or two (k_mc_ctile<float, 0, 0, 1> 30 -> 32); the branches are the text every
//     feature of the last rounds edited twice, so they are what is shared.

// the row's seven raw parameters and seven plan-time constants, by ONE shared 32-bit byte offset: with uniform (SGPR) array
// bases every load is `global_load v, v_off, s[base]` instead of a 64-bit add per array
template <class T>
__device__ __forceinline__ void load_row_params(const StepArgs<T> &a, uint32_t &ob, trmc::ChannelParams<T> &p, trmc::ChannelConst<T> &c)
{
    p.dt = a.dt_col ? at(a.dt_col, ob) : a.dt;
    // (the zero-extension of the offset has to be visible in the basic block of the loads for the
    // SGPR-base addressing form to be selected: re-introduce it after every branch)
    asm volatile("" : "+v"(ob));
    p.dx = at(a.dx, ob);
    p.bw = at(a.bw, ob);
    p.twcc = at(a.twcc, ob);
    p.n = at(a.n, ob);
    p.ncc = at(a.ncc, ob);
    p.s0 = at(a.s0, ob);
    p.tw = p.cs = T(0); // only enter the constants below
    c.z = at(a.z, ob);
    c.bfd = at(a.bfd, ob);
    c.sqrt_s0 = at(a.sqrt_s0, ob);
    c.sq1pz2 = at(a.sq1pz2, ob);
    c.s0_n = at(a.s0_n, ob);
    c.s0_ncc = at(a.s0_ncc, ob);
    c.inv_n = at(a.inv_n, ob);
    trmc::derive_const(c, p);
}

// Step t of a level-pool reservoir row (see k_mc_step; RDA: with its data-assimilation tables) whose upstream flows of step
// t - 1 sum to qup; the row keeps its water elevation in the depth slot.  In a stream of days the tables and the inflow record
// are those of the row's own day: its slot's.
template <class T, class M, bool RDA>
__device__ __forceinline__ void reservoir_row(ColdArgs<StepArgs<T>> cold, const M &m, int32_t slot, int32_t ri, int32_t t, T qup, T d_prev, T &q_new, T &v_new, T &d_new)
{
    const T *rp = cold->res_par + (size_t)ri * 9;
    const trmc::LevelPoolParams<T> lp{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8]};
    T H = d_prev;
    q_new = trmc::levelpool_step<T, M>(qup, T(0), cold->res_dt, H, lp, m);
    if constexpr (RDA) {
        void *const da = cold->res_da;
        trmc::ResDaState *const carry = (trmc::ResDaState *)cold->res_da_carry;
        const trmc::ResDaResult r =
            carry ? trmc::reservoir_da_row_day((char *)da + (size_t)slot * (size_t)cold->slot_rda, carry, ri, t, cold->nsteps, cold->res_t_end,
                                               qup, d_prev, cold->res_dt, rp, q_new, H)
                  : trmc::reservoir_da_row(da, ri, t, qup, d_prev, cold->res_dt, rp, q_new, H);
        q_new = r.outflow;
        H = r.water_elevation;
    }
    v_new = T(0);
    d_new = H;
    cold->res_inflow[(size_t)slot * (size_t)cold->slot_res + (size_t)ri * (size_t)cold->nsteps + (size_t)(t - 1)] = qup; // (the day's own record)
}

// streamflow nudging of step t at gage gi (see k_mc_step); in a stream: the tables of the row's own day
template <class T>
__device__ __forceinline__ void nudge_row(ColdArgs<StepArgs<T>> cold, int32_t slot, int32_t gi, int32_t t, T &q_new)
{
    const size_t e = (size_t)slot * (size_t)cold->slot_da + (size_t)gi * (size_t)cold->nsteps + (size_t)(t - 1);
    const T *const da_a = cold->da_a;
    const uint8_t mode = cold->da_mode[e];
    T nudge = T(0);
    if (mode == 1) {
        nudge = da_a[e] - q_new;
        q_new = da_a[e];
    } else if (mode == 2) {
        nudge = (da_a[e] - q_new) * cold->da_w[e];
        q_new = q_new + nudge;
    }
    cold->da_nudge[e] = nudge;
}

// Of the time-major planes a tile kernel writes the flow row of every step (its own store) and, here, the depth row of a tile's
// last step: where the row's next tile, or the final state, picks it up.
template <class T>
__device__ __forceinline__ void hand_on_row(ColdArgs<StepArgs<T>> cold, int32_t slot, int32_t slot_next, uint32_t ob, size_t np, int32_t t, int32_t t_hi, T q_new, T d_new)
{
    if (t == t_hi) {
        at(cold->d_tm + (size_t)slot * (size_t)cold->slot_tm + (size_t)t * np, ob) = d_new;
        if (cold->seq_slots > 1 && t == cold->nsteps) { // the day ends: the next one starts from here (its slot's time row 0)
            at(cold->q_tm + (size_t)slot_next * (size_t)cold->slot_tm, ob) = q_new;
            at(cold->d_tm + (size_t)slot_next * (size_t)cold->slot_tm, ob) = d_new;
        }
    }
}
