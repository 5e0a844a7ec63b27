// kernels_flow.inc -- included by trmc.hip: the dataflow engine's kernels (k_mc_flow, k_mc_flow_lean).
// ---------------------------------------------------------------- dataflow engine (fp32)
// The level engine above makes a kernel boundary of every dependence: one launch per timestep (or per
// wavefront diagonal), 12 parameter loads and 3 state loads per segment-step, and between launches the whole
// device drains.  The dataflow engine keeps a row in ONE thread for a whole routing window instead:
//   * rows are laid out in BLOCK ORDER (topology.hpp): depth-first post-order cut into blocks of kFlowBlock rows, rows
//     of a block grouped by cost.  A block is a workgroup; it takes a ticket when it starts, so block k only ever
//     needs flows of blocks <= k, all of which are running or done: no deadlock whatever the dispatch order;
//   * a thread loads its row's parameters, constants and state ONCE, then steps through time in registers;
//   * the only thing rows exchange is the flow they pass downstream.  Every row publishes it per step as an 8-byte
//     GRANULE {flow bits, tag = tag_base + step} with one agent-scope store into gran[step][position]; a row reads its
//     upstream rows' granules of the step it needs and, where the tag is not there yet, waits for it (relaxed
//     agent-scope polls, MI355X_MICROARCH.md "handoff-1to1": a self-validating word needs no fence and no flag).
//     A kernel boundary is never needed: producers run ahead of consumers, a consumer that catches up sleeps;
//   * results go straight into the caller's layout out[row][step][q,v,d]: a thread stages 8 steps in LDS and writes
//     them as one 96-byte run (whole 32-byte sectors) -- no time-major planes, no transposing pass.
// Timestep modes: with assume_short_ts a row at step t needs its upstream rows at step t-1; without, also at step t
// (mc_reach.pyx:499-505) -- then rows of one wavefront that feed each other cannot be at the same step, and every
// row trails by its level rank inside the block (lane i works on step t0 + k - rank_i in round k).
// HBM traffic per segment-step: 8 B granule + 12 B result written, <= 16 B of upstream granules read (L2), the
// forcing every qts-th step -- against 64 B algorithmic; what bounds the engine is VALU issue.
#ifndef TRMC_FLOW_BLOCK
#define TRMC_FLOW_BLOCK 256
#endif
#ifndef TRMC_FLOW_WAVES // minimum waves per SIMD the register allocation must allow (workgroups per CU = this * 256 / block)
#define TRMC_FLOW_WAVES 4
#endif
constexpr int kFlowBlock = TRMC_FLOW_BLOCK;
#ifndef TRMC_FLOW_STAGE
#define TRMC_FLOW_STAGE 8
#endif
constexpr int kFlowStage = TRMC_FLOW_STAGE; // steps staged per thread before they are written to `out`

struct FlowArgs {
    const float *dx, *bw, *twcc, *n, *ncc, *s0;
    const float *z, *bfd, *sqrt_s0, *sq1pz2, *s0_n, *s0_ncc, *inv_n;
    const float *dt_col;
    float dt;
    const int32_t *up_ptr, *up_idx;
    const int2 *up2;
    const int32_t *lag;            // short-timestep mode: steps a row trails by (trmc_plan_set_lag); general mode: its
                                   // level rank inside the block; nullptr = none
    const float *qlat_tm;
    unsigned long long *gran;      // [nsteps + 1][nseg_pad] granules
    float *d_state;                // [nseg_pad] depth at the last step each row has completed
    unsigned long long *d_gran;    // [nseg_pad] the same as a granule {depth bits, tag of that step}: hand-over between
                                   // consecutive launches of one window that overlap in time (k_mc_flow_lean)
    float *out;                    // [nseg][nsteps][3]
    const int32_t *row_of_pos;
    uint8_t *it_prev;
    uint16_t *it_sum;
    bool sane, out_vec;            // out_vec: the 8-step runs of `out` are 16-byte aligned (nsteps % 4 == 0)
    const int32_t *res_of_pos;
    const float *res_par;
    float *res_inflow;
    float res_dt;
    void *res_da;                  // nullptr, or the data-assimilation tables of the reservoirs (reservoir_da.hpp)
    const int32_t *gage_of_pos;
    const uint8_t *da_mode;
    const float *da_a, *da_w;
    float *da_nudge;
    int64_t nseg_pad;
    int32_t nsteps, qts, nseg, first; // first: position of the first routed row (= number of boundary rows)
    uint32_t tag_base;
    int32_t *ticket;               // [0] block tickets of this launch, [1] abort flag of the window
    uint64_t watchdog_ticks;       // wall_clock64 ticks (100 MHz) a row may wait for one granule
    const uint8_t *prio;           // issue priority 0..3 of every wavefront of the block order (topology.cpp)
    // blocks dealt to compute units by cost (lean kernels, see flow_place_blocks): queue q holds cuq_blk[cuq_ptr[q] ..
    // cuq_ptr[q + 1]), cuq_head[q] counts what has been taken, cu_index maps hw_cu_key() to a queue; nullptr = block tickets
    const int32_t *cuq_ptr, *cuq_blk, *cu_index;
    const uint8_t *cuq_perm;       // [nblocks] row group of the block for SIMD s: bits 2s+1..2s
    int32_t *cuq_head;
    int32_t ncuq;
    unsigned long long *dbg;       // nullptr, or [nblocks][2]: wall clock at the start and the end of every block (TRMC_FLOW_DEBUG)
    int32_t nblocks_dbg;
    const int32_t *ticket_map;     // general mode: ticket -> block, the blocks of the long main stems first (topology.hpp,
                                   // stem_min_rows); nullptr = block tickets in order
};

using FlowCold = ColdArgs<FlowArgs>;

// which compute unit a wavefront runs on: XCC_ID[3:0] | HW_ID {se_id[15:13], sh_id[12], cu_id[11:8]} -> 12 bits
__device__ __forceinline__ uint32_t hw_cu_key()
{
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);   // HW_REG_HW_ID
    const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);  // HW_REG_XCC_ID
    return ((xcc & 15u) << 8) | ((hw >> 8) & 0xffu);
}
__device__ __forceinline__ unsigned long long gran_load(const unsigned long long *g)
{
    return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// flow of position `u` at the step whose tag is `want`; waits until it has been published.  A waiting row costs
// the others as little as possible: long sleeps, and a poll counter for a watchdog instead of a clock read per poll
// (the clock is only consulted every 1024th poll).
#ifndef TRMC_FLOW_SLEEP
#define TRMC_FLOW_SLEEP 16 // x 64 clocks between two polls of a granule that is not there yet
#endif
__device__ __forceinline__ bool flow_watchdog(uint32_t &polls, uint64_t &t_start, FlowCold a)
{
    if ((++polls & 1023u) != 0u) return false;
    if (t_start == 0) {
        t_start = wall_clock64();
        return false;
    }
    if (wall_clock64() - t_start > a->watchdog_ticks
        || __hip_atomic_load(a->ticket + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        __hip_atomic_store(a->ticket + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    }
    return false;
}
// what the first row to give up was waiting for, for the host's error message: ticket[2..5] = {granule index in the
// plane (low, high word), wanted tag, tag found}
__device__ __forceinline__ void flow_report(FlowCold a, const unsigned long long *g, uint32_t want, unsigned long long v)
{
    if (atomicCAS(a->ticket + 6, 0, 1) == 0) {
        const unsigned long long idx = (unsigned long long)(g - a->gran);
        a->ticket[2] = (int32_t)(idx & 0xffffffffull);
        a->ticket[3] = (int32_t)(idx >> 32);
        a->ticket[4] = (int32_t)want;
        a->ticket[5] = (int32_t)(v >> 32);
    }
}
__device__ __forceinline__ float flow_wait(const unsigned long long *g, uint32_t want, FlowCold a, bool &dead)
{
    unsigned long long v = gran_load(g);
    if ((uint32_t)(v >> 32) != want) {
        uint32_t polls = 0;
        uint64_t t_start = 0;
        do {
            __builtin_amdgcn_s_sleep(TRMC_FLOW_SLEEP);
            v = gran_load(g);
            if (flow_watchdog(polls, t_start, a)) {
                dead = true;
                flow_report(a, g, want, v);
            }
        } while ((uint32_t)(v >> 32) != want && !dead);
    }
    return __uint_as_float((uint32_t)v);
}

// One upstream edge of a row.  In-block edges are read from the block's LDS ring while producer and consumer run in
// step; an edge whose producer runs well ahead (its ring slot is already overwritten: a cheap row feeding a costly one)
// or lives in another block is read from the granule plane, one step ahead of its use (the load is in flight during the
// arithmetic of the current step).
struct FlowEdge {
    int32_t u;                // plan position of the upstream row, -1 = none
    int32_t l;                // its index in the block's LDS ring, -1 = not eligible (other block, other lag)
    bool ahead;               // read through the granule plane, prefetched
    bool pre_ok;
    unsigned long long pre;   // the prefetched granule
};
#ifndef TRMC_FLOW_RING
#define TRMC_FLOW_RING 4
#endif
constexpr int kFlowRing = TRMC_FLOW_RING;  // steps the LDS ring of a block holds (a power of two)

__device__ __forceinline__ float flow_edge_get(FlowEdge &e, const unsigned long long *plane_row, unsigned long long *ring,
                                               int32_t ws, uint32_t want, FlowCold a, bool &dead)
{
    unsigned long long v = e.pre;
    if (!(e.ahead && e.pre_ok && (uint32_t)(v >> 32) == want)) {
        bool got = false;
        if (e.l >= 0) {
            const unsigned long long *slot = ring + (size_t)(ws & (kFlowRing - 1)) * kFlowBlock + e.l;
            v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if ((int32_t)((uint32_t)(v >> 32) - want) < 0) { // not produced yet: the producer is a wave of this block
                uint32_t polls = 0;
                uint64_t t_start = 0;
                do {
                    __builtin_amdgcn_s_sleep(TRMC_FLOW_SLEEP);
                    v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (flow_watchdog(polls, t_start, a)) dead = true;
                } while ((int32_t)((uint32_t)(v >> 32) - want) < 0 && !dead);
            }
            got = (uint32_t)(v >> 32) == want;
            e.ahead = !got; // overwritten: the producer is ahead by more than the ring holds
        }
        if (!got) {
            const float q = flow_wait(plane_row + e.u, want, a, dead);
            return q;
        }
    }
    return __uint_as_float((uint32_t)v);
}

template <bool SHORT, bool TOL, bool RDA> // (RDA: reservoir data-assimilation tables, kernels of their own -- see mc_step_rows)
__device__ __forceinline__ void mc_flow_rows(const FlowArgs &a, int32_t t0, int32_t t1);
template <bool SHORT, bool TOL = false>
__global__ void __launch_bounds__(kFlowBlock, TRMC_FLOW_WAVES)
k_mc_flow(const FlowArgs a, const int32_t t0, const int32_t t1) // routes the launches / steps (t0, t1] of the window
{
    mc_flow_rows<SHORT, TOL, false>(a, t0, t1);
}
template <bool SHORT>
__global__ void __launch_bounds__(kFlowBlock, TRMC_FLOW_WAVES)
k_mc_flow_rda(const FlowArgs a, const int32_t t0, const int32_t t1)
{
    mc_flow_rows<SHORT, false, true>(a, t0, t1);
}
template <bool SHORT, bool TOL, bool RDA>
__device__ __forceinline__ void mc_flow_rows(const FlowArgs &a, const int32_t t0, const int32_t t1)
{
    using M = std::conditional_t<TOL, DevMathTolFlow, DevMathFlow>;
    const FlowCold cold = cold_args<FlowArgs>(); // (see cold_args: what the loop rarely needs is not kept in registers)
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    __shared__ float s_out[3 * kFlowStage * kFlowBlock];             // [step slot * 3 + c][thread]
    __shared__ unsigned long long s_ring[kFlowRing * kFlowBlock];    // [step % kFlowRing][thread] granules
    __shared__ int32_t s_blk;
    if (threadIdx.x == 0) {
        // General mode on a plan laid out for it: the first tickets go to the blocks of the long main stems.  They wait for
        // their inflows in place -- a stem then advances behind the sweep over its basin instead of after it -- and every
        // other block still only needs blocks that took their tickets before it or are among those few, all resident.
        const int32_t tk = atomicAdd(a.ticket, 1);
        s_blk = (!SHORT && cold->ticket_map) ? cold->ticket_map[tk] : tk;
    }
#pragma unroll
    for (int j = 0; j < kFlowRing; ++j) s_ring[j * kFlowBlock + threadIdx.x] = 0ull; // tag 0: older than any live tag
    M m{stage_pow_tables(s_tab), false}; // (its barrier also publishes s_blk and the cleared ring)
    m.sane = a.sane;

    const int32_t blk_base = a.first + s_blk * kFlowBlock;
    const int32_t pos = blk_base + (int32_t)threadIdx.x;
    const bool valid = pos < a.nseg;
    const uint32_t su = valid ? (uint32_t)pos : (uint32_t)a.first;
    const uint32_t ob = su * 4u;
    const int32_t lag = a.lag ? a.lag[su] : 0;
    if (cold->dbg && threadIdx.x == 0) cold->dbg[2 * s_blk] = ((unsigned long long)hw_cu_key() << 48) | (wall_clock64() & 0xffffffffffffull);
    // the steps [t_lo, t_hi] this row covers in this launch, and the round it starts in
    const int32_t t_lo = SHORT ? max(t0 - lag, 0) + 1 : t0 + 1;
    const int32_t t_hi = valid ? (SHORT ? min(t1 - lag, a.nsteps) : min(t1, a.nsteps)) : 0;
    const int32_t delay = SHORT ? 0 : lag;
    // General mode: a wavefront whose rows trail each other deeply sits on a long chain of the network -- the critical
    // path of the window (a row at level l cannot finish step t before l rows have, one after the other).  It gets
    // issue priority over the wavefronts it shares its SIMD with, so that the chain advances at the pace of one
    // wavefront alone while the bulk of the network fills the remaining issue slots.
    if (!SHORT && __any(delay >= 16)) __builtin_amdgcn_s_setprio(3);

    trmc::ChannelParams<float> p;
    p.dt = a.dt_col ? at(a.dt_col, ob) : a.dt;
    p.dx = at(a.dx, ob);
    p.bw = at(a.bw, ob);
    p.twcc = at(a.twcc, ob);
    p.n = at(a.n, ob);
    p.ncc = at(a.ncc, ob);
    p.s0 = at(a.s0, ob);
    p.tw = p.cs = 0.0f; // only enter the constants below
    trmc::ChannelConst<float> c;
    c.z = at(a.z, ob);
    c.bfd = at(a.bfd, ob);
    c.sqrt_s0 = at(a.sqrt_s0, ob);
    c.sq1pz2 = at(a.sq1pz2, ob);
    c.s0_n = at(a.s0_n, ob);
    c.s0_ncc = at(a.s0_ncc, ob);
    c.inv_n = at(a.inv_n, ob);
    trmc::derive_const(c, p);
    const int2 up = a.up2[su];
    const bool more = up.y >= 0 && (up.y & 0x40000000);
    FlowEdge e0, e1;
    {
        auto init = [&](FlowEdge &e, int32_t u) {
            e.u = valid ? u : -1;
            e.l = -1;
            e.pre = 0ull;
            e.pre_ok = false;
            if (e.u >= 0) {
                const bool inb = u >= blk_base && u < blk_base + kFlowBlock;
                // (a skewed row and a row in step never share the ring: their step windows differ)
                const bool same = !SHORT || !a.lag || a.lag[u] == lag;
                if (inb && same) e.l = u - blk_base;
            }
            e.ahead = e.l < 0;
        };
        init(e0, up.x);
        init(e1, up.y >= 0 ? (up.y & 0x3fffffff) : -1);
    }
    const int32_t ri = a.res_of_pos ? a.res_of_pos[su] : -1;
    const int32_t gi = a.gage_of_pos ? a.gage_of_pos[su] : -1;
    const size_t np = (size_t)a.nseg_pad;
    float *const out_row = a.out + (size_t)a.row_of_pos[su] * (size_t)a.nsteps * 3;

    float q_prev = 0.0f, d_prev = 0.0f, ql = 0.0f, xp0 = 0.0f, xp1 = 0.0f;
    int32_t ql_col = -1, ql_left = 0, staged = 0, it_acc = 0, it_last = 0;
    bool have_state = false, dead = false;

    for (int32_t k = 0;; ++k) {
        const int32_t t = t_lo + k - delay;
        if (!__any(t <= t_hi) || __any(dead)) break;
        if (t < t_lo || t > t_hi) continue;
        const uint32_t tag_p = a.tag_base + (uint32_t)(t - 1);
        const unsigned long long *g_prev = a.gran + (size_t)(t - 1) * np;
        unsigned long long *g_curr = a.gran + (size_t)t * np;
        if (!have_state) { // the state this row was left in: its own granule of step t - 1, its depth column
            q_prev = flow_wait(g_prev + su, tag_p, cold, dead);
            d_prev = cold->d_state[su];
            __hip_atomic_store(s_ring + (size_t)((t - 1) & (kFlowRing - 1)) * kFlowBlock + threadIdx.x,
                               ((unsigned long long)tag_p << 32) | (unsigned long long)__float_as_uint(q_prev),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (!SHORT) { // the general mode also needs its upstream rows at the step before its first one
                if (e0.u >= 0) xp0 = flow_wait(g_prev + e0.u, tag_p, cold, dead);
                if (e1.u >= 0) xp1 = flow_wait(g_prev + e1.u, tag_p, cold, dead);
            }
            // the lateral-inflow column of step t is (t - 1) / qts: found by division once, by a counter from then on
            const int32_t qts = cold->qts;
            ql_col = (t - 1) / qts;
            ql_left = qts - (t - 1) % qts;
            ql = cold->qlat_tm[(size_t)ql_col * np + su];
            have_state = true;
        }
        if (ql_left == 0) {
            ++ql_col;
            ql = cold->qlat_tm[(size_t)ql_col * np + su];
            ql_left = cold->qts;
        }
        --ql_left;
        // (Evaluating the part of the step that needs the row's OWN state only -- step_pre: the bracket and its two hydraulic
        // points -- BEFORE the look-up below, off the dependence chain, was built and measured: the general-mode CONUS day
        // 55 ms instead of 38, a lone chain 8.3 us per row instead of 7.4.  The chain mostly runs through the lanes of ONE
        // wavefront, which advance a row per round whatever the order inside the round, and the two points held across the
        // look-up cost registers the kernel does not have.  What stayed: the flow is published before the velocity is formed.)
        trmc::StepPre<float> pre;
        pre.have = false;
        // junction sums in the reference's order (mc_reach.pyx:499-502): with assume_short_ts the upstream flows of
        // step t - 1 (they are also `quc`, :504-505), without it those of step t and -- kept from the round before --
        // of step t - 1
        const int32_t ws = SHORT ? t - 1 : t;
        const uint32_t want = SHORT ? tag_p : tag_p + 1u;
        const unsigned long long *g_want = SHORT ? g_prev : g_curr;
        float x0 = 0.0f, x1 = 0.0f;
        if (e0.u >= 0) x0 = flow_edge_get(e0, g_want, s_ring, ws, want, cold, dead);
        if (e1.u >= 0) x1 = flow_edge_get(e1, g_want, s_ring, ws, want, cold, dead);
        // edges read through the granule plane: next step's granule starts its way here now
        if (t < t_hi) {
            if (e0.u >= 0 && e0.ahead) e0.pre = gran_load(g_want + np + e0.u);
            if (e1.u >= 0 && e1.ahead) e1.pre = gran_load(g_want + np + e1.u);
        }
        e0.pre_ok = e1.pre_ok = t < t_hi;
        float qup = 0.0f, quc = 0.0f;
        if (e0.u >= 0) {
            qup += SHORT ? x0 : xp0;
            quc += x0;
        }
        if (e1.u >= 0) {
            qup += SHORT ? x1 : xp1;
            quc += x1;
        }
        if (more) { // fan-in above two (0.2 % of junctions): straight from the granule plane
            const int32_t *const up_ptr = cold->up_ptr, *const up_idx = cold->up_idx;
            const int32_t k1 = up_ptr[su + 1];
            for (int32_t e = up_ptr[su] + 2; e < k1; ++e) {
                const int32_t ue = up_idx[e];
                qup += flow_wait(g_prev + ue, tag_p, cold, dead);
                if (!SHORT) quc += flow_wait(g_curr + ue, tag_p + 1u, cold, dead);
            }
        }
        xp0 = x0;
        xp1 = x1;
        trmc::Inflow<float> f;
        f.qup = qup;
        f.quc = SHORT ? qup : quc;
        f.qdp = q_prev;
        f.ql = ql;

        float q_new, v_new = 0.0f, d_new;
        bool routed = false;
        if (ri >= 0) { // level-pool reservoir row, mc_reach.pyx:507-510,:551-553,:706-710 (see k_mc_step)
            const float *rp = cold->res_par + (size_t)ri * 9;
            const trmc::LevelPoolParams<float> lp{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8]};
            float H = d_prev;
            q_new = trmc::levelpool_step<float, M>(f.quc, 0.0f, cold->res_dt, H, lp, m);
            if constexpr (RDA) { // hybrid persistence / RFC series, mc_reach.pyx:555-703
                void *const da = cold->res_da;
                const trmc::ResDaResult r = trmc::reservoir_da_row(da, ri, t, f.quc, d_prev, cold->res_dt, rp, q_new, H);
                q_new = r.outflow;
                H = r.water_elevation;
            }
            d_new = H;
            cold->res_inflow[(size_t)ri * (size_t)cold->nsteps + (size_t)(t - 1)] = f.quc;
            it_last = 0;
        } else {
            q_new = 0.0f;
            d_new = 0.0f;
            it_last = 0;
            if (trmc::step_has_flow(f)) {
                m.coef_ok = coef_guard(p.dt, f.ql);
                const trmc::StepSolve<float> r = trmc::step_solve<float, M>(p, c, f, d_prev, pre, m);
                q_new = r.qdc;
                d_new = r.h;
                routed = true;
                it_last = min(r.iters, 255);
                it_acc += min(r.iters, 3) + (r.over ? 4 : 0);
            }
            if (gi >= 0) { // streamflow nudging, mc_reach.pyx:761-796 / simple_da.pyx:47-76 (see k_mc_step)
                const size_t e = (size_t)gi * (size_t)cold->nsteps + (size_t)(t - 1);
                const float *const da_a = cold->da_a;
                const uint8_t mode = cold->da_mode[e];
                float nudge = 0.0f;
                if (mode == 1) {
                    nudge = da_a[e] - q_new;
                    q_new = da_a[e];
                } else if (mode == 2) {
                    nudge = (da_a[e] - q_new) * cold->da_w[e];
                    q_new = q_new + nudge;
                }
                cold->da_nudge[e] = nudge;
            }
        }
        // publish the flow as soon as it exists -- the block's ring, and one 8-byte agent-scope store into the plane; tag
        // in the high word -- and only then form the velocity (a power, a square root, a division: f90:163-169), which no
        // other row reads
        {
            const unsigned long long g = ((unsigned long long)(tag_p + 1u) << 32) | (unsigned long long)__float_as_uint(q_new);
            __hip_atomic_store(s_ring + (size_t)(t & (kFlowRing - 1)) * kFlowBlock + threadIdx.x, g, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(g_curr + su, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (routed) v_new = trmc::step_velocity<float, M>(p, c, d_new, m);
        q_prev = q_new;
        d_prev = d_new;
        // stage (q, v, d) of step t; a run ends at every 8th step of the window and at the last step of the launch
        {
            const int32_t slot = (t - 1) & (kFlowStage - 1);
            float *so = s_out + (size_t)(slot * 3) * kFlowBlock + threadIdx.x;
            so[0] = q_new;
            so[kFlowBlock] = v_new;
            so[2 * kFlowBlock] = d_new;
            ++staged;
            if (slot == kFlowStage - 1 || t == t_hi) {
                const int32_t s_first = slot + 1 - staged; // first staged slot
                float *dst = out_row + (size_t)(t - staged) * 3;
                const float *si = s_out + (size_t)(s_first * 3) * kFlowBlock + threadIdx.x;
                if (staged == kFlowStage && a.out_vec) {
#pragma unroll
                    for (int j = 0; j < 3 * kFlowStage / 4; ++j) {
                        float4 v;
                        v.x = si[(4 * j + 0) * kFlowBlock];
                        v.y = si[(4 * j + 1) * kFlowBlock];
                        v.z = si[(4 * j + 2) * kFlowBlock];
                        v.w = si[(4 * j + 3) * kFlowBlock];
                        reinterpret_cast<float4 *>(dst)[j] = v;
                    }
                } else {
                    for (int32_t e = 0; e < 3 * staged; ++e) dst[e] = si[e * kFlowBlock];
                }
                staged = 0;
            }
        }
    }
    if (cold->dbg) atomicMax(cold->dbg + 2 * s_blk + 1, (unsigned long long)wall_clock64());
    if (valid && have_state) {
        cold->d_state[su] = d_prev;
        if (t_hi == cold->nsteps) cold->it_prev[su] = (uint8_t)it_last;
        if (uint16_t *const it_sum = cold->it_sum) it_sum[su] = (uint16_t)min(65535, (int)it_sum[su] + it_acc);
    }
}

// The short-timestep form of the engine, written for occupancy: with assume_short_ts a row only ever needs flows of the
// step before, all rows of a block advance together, and the whole window is VALU-bound -- what decides the pace of a
// partly filled device (one rank of a multi-GPU job: 340 k rows are 5 455 wavefronts against 4 096 slots at four per
// SIMD) is whether every wavefront of the job is resident at once.  So a thread keeps only what it must in registers
// (its flow, its depth, its forcing, two upstream positions, one result offset): the twelve parameter and constant
// columns of its row wait in LDS (48 B per row, read back at every step), results are stored step by step (12 B;
// neighbouring steps of a row merge in the L2 / Infinity Cache), the LDS ring holds two steps.  LAG: rows with a skew
// (trmc_plan_set_lag) -- then the step is a per-lane quantity; without, it is wave-uniform and lives in SGPRs.
#ifndef TRMC_LEAN_WAVES
#define TRMC_LEAN_WAVES 6
#endif
#ifndef TRMC_LEAN_RING_SLEEP // x 64 clocks between two polls of the block's LDS ring
#define TRMC_LEAN_RING_SLEEP 2
#endif
constexpr int kLeanRing = 2;
constexpr int kLeanCols = 13;

__device__ __forceinline__ float lean_edge_get(int32_t u, int32_t l, uint32_t &flags, uint32_t ahead_bit, uint32_t never_bit,
                                               const unsigned long long *plane_row, const unsigned long long *ring, int32_t ws,
                                               uint32_t want, FlowCold a, bool &dead)
{
    if (!(flags & (ahead_bit | never_bit))) {
        const unsigned long long *slot = ring + (size_t)(ws & (kLeanRing - 1)) * kFlowBlock + l;
        unsigned long long v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((int32_t)((uint32_t)(v >> 32) - want) < 0) { // not produced yet: the producer is a wave of this block
            uint32_t polls = 0;
            uint64_t t_start = 0;
            do {
                __builtin_amdgcn_s_sleep(TRMC_LEAN_RING_SLEEP);
                v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (flow_watchdog(polls, t_start, a)) dead = true;
            } while ((int32_t)((uint32_t)(v >> 32) - want) < 0 && !dead);
        }
        if ((uint32_t)(v >> 32) == want) return __uint_as_float((uint32_t)v);
        flags |= ahead_bit; // overwritten: the producer runs ahead of what the ring holds
    }
    return flow_wait(plane_row + u, want, a, dead);
}

// Which block a workgroup of a lean launch routes.  Every block of such a launch is resident at once (flow_lean), each
// stays on its compute unit for the whole launch, and a SIMD issues for its wavefronts one instruction at a time: the launch
// lasts as long as the most heavily loaded compute unit needs.  The hardware deals workgroups out by COUNT (5 or 6 per
// unit for a 340 k-row rank); by block tickets the costliest unit of such a rank carried 1.5 times the mean (measured
// per-unit end times 0.8 .. 4.5 ms, correlation with the modelled load 0.8).  So the host deals the blocks to per-unit queues
// by cost (flow_place_blocks), a workgroup finds out where it runs (hw_cu_key) and takes the next block of that unit's
// queue -- or, when the hardware sent the unit more workgroups than its queue holds, of the nearest queue that has one left.
// Any assignment is correct: nothing depends on the order blocks start in while all of them are resident.
__device__ __forceinline__ int32_t lean_pick_block(const FlowArgs &a)
{
    if (!a.cuq_blk) return atomicAdd(a.ticket, 1);
    const int32_t Q = a.ncuq;
    const uint32_t key = hw_cu_key();
    int32_t q = a.cu_index[key];
    if (q < 0) q = (int32_t)(key % (uint32_t)Q);
    // cuq_head[q]: low half = blocks taken from the front (by workgroups of the unit itself: its costliest first), high half =
    // blocks taken from the back (by workgroups of other units whose own queue had run out: the cheapest); both only grow,
    // and a take counts if front + back was below the queue length before it
    for (int32_t k = 0; k < Q; ++k) {
        const int32_t qq = q + k < Q ? q + k : q + k - Q;
        const int32_t lo = a.cuq_ptr[qq], n = a.cuq_ptr[qq + 1] - lo;
        const uint32_t seen = (uint32_t)__hip_atomic_load(a.cuq_head + qq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int32_t)((seen & 0xffffu) + (seen >> 16)) >= n) continue;
        const uint32_t was = (uint32_t)atomicAdd(a.cuq_head + qq, k == 0 ? 1 : 0x10000);
        const int32_t front = (int32_t)(was & 0xffffu), back = (int32_t)(was >> 16);
        if (front + back < n) return a.cuq_blk[lo + (k == 0 ? front : n - 1 - back)];
    }
    return -1; // (cannot happen: as many workgroups as blocks)
}

template <bool LAG, bool TOL, bool RDA> // (see mc_flow_rows)
__device__ __forceinline__ void mc_flow_lean_rows(const FlowArgs &a, int32_t t0, int32_t t1);
template <bool LAG, bool TOL = false>
__global__ void __launch_bounds__(kFlowBlock, TRMC_LEAN_WAVES)
k_mc_flow_lean(const FlowArgs a, const int32_t t0, const int32_t t1)
{
    mc_flow_lean_rows<LAG, TOL, false>(a, t0, t1);
}
template <bool LAG>
__global__ void __launch_bounds__(kFlowBlock, TRMC_LEAN_WAVES)
k_mc_flow_lean_rda(const FlowArgs a, const int32_t t0, const int32_t t1)
{
    mc_flow_lean_rows<LAG, false, true>(a, t0, t1);
}
template <bool LAG, bool TOL, bool RDA>
__device__ __forceinline__ void mc_flow_lean_rows(const FlowArgs &a, const int32_t t0, const int32_t t1)
{
    using M = std::conditional_t<TOL, DevMathTolFlow, DevMathFlow>;
    const FlowCold cold = cold_args<FlowArgs>(); // (see cold_args: what the loop rarely needs is not kept in registers)
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    __shared__ float s_par[kLeanCols * kFlowBlock];                 // [column][thread]
    __shared__ unsigned long long s_ring[kLeanRing * kFlowBlock];   // [step % 2][thread] granules
    __shared__ int32_t s_blk;
    __shared__ int32_t s_grp[kFlowBlock / 64];
    if (threadIdx.x == 0) s_blk = lean_pick_block(a);
    if (threadIdx.x < kFlowBlock / 64) s_grp[threadIdx.x] = -1;
#pragma unroll
    for (int j = 0; j < kLeanRing; ++j) s_ring[j * kFlowBlock + threadIdx.x] = 0ull;
    M m{stage_pow_tables(s_tab), false}; // (its barrier also publishes s_blk and the cleared ring)
    m.sane = a.sane;
    if (s_blk < 0) return;
    // Which 64 rows of the block this wavefront takes.  A block's rows are grouped by descending cost, so its first
    // wavefront is its costliest (1 010 instructions per step against 730 for the others, 8-way CONUS rank) -- and if that
    // always lands on the same SIMD of its unit, that SIMD carries 1.3 times the others' load.  The host has matched the
    // block's four row groups with the four SIMDs of the unit it dealt the block to (costliest group to the SIMD carrying
    // least, flow_place_blocks); a wavefront reads which SIMD it is on and takes that SIMD's group.  Should two wavefronts
    // of the workgroup share a SIMD, everybody keeps the plain order.
    int32_t grp = (int32_t)(threadIdx.x >> 6);
    uint32_t my_simd = 0;
    if (a.cuq_perm) {
        my_simd = (__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4) >> 4) & 3u; // HW_REG_HW_ID.simd_id
        const int32_t g = (int32_t)((a.cuq_perm[s_blk] >> (2u * my_simd)) & 3u);
        if ((threadIdx.x & 63u) == 0) s_grp[g] = (int32_t)(threadIdx.x >> 6);
        __syncthreads();
        bool all_taken = true;
#pragma unroll
        for (int j = 0; j < kFlowBlock / 64; ++j) all_taken = all_taken && s_grp[j] >= 0;
        if (all_taken) grp = g;
    }
    const int32_t tix = grp * 64 + (int32_t)(threadIdx.x & 63u); // the row of the block this thread routes
    const int32_t blk_base = a.first + s_blk * kFlowBlock;
    if (cold->dbg && tix == 0) cold->dbg[2 * s_blk] = ((unsigned long long)hw_cu_key() << 48) | (wall_clock64() & 0xffffffffffffull);
    if (cold->dbg && (threadIdx.x & 63u) == 0) // which SIMD every row group ran on
        cold->dbg[2 * (size_t)(cold->nblocks_dbg + 1) + 4 * (size_t)s_blk + grp] = 1ull + my_simd + ((unsigned long long)(threadIdx.x >> 6) << 8);
    if (a.prio) { // the costlier a wavefront, the higher its issue priority (topology.cpp)
        const int pr = __builtin_amdgcn_readfirstlane((int)a.prio[(s_blk * kFlowBlock + tix) >> 6]);
        if (pr == 1) __builtin_amdgcn_s_setprio(1);
        else if (pr == 2) __builtin_amdgcn_s_setprio(2);
        else if (pr == 3) __builtin_amdgcn_s_setprio(3);
    }
    if (blk_base + tix >= a.nseg) return; // (no block-wide barrier below)
    const uint32_t su = (uint32_t)(blk_base + tix);
    {
        const uint32_t ob = su * 4u;
        float *sp = s_par + tix;
        sp[0 * kFlowBlock] = at(a.dx, ob);
        sp[1 * kFlowBlock] = at(a.bw, ob);
        sp[2 * kFlowBlock] = at(a.twcc, ob);
        sp[3 * kFlowBlock] = at(a.n, ob);
        sp[4 * kFlowBlock] = at(a.ncc, ob);
        sp[5 * kFlowBlock] = at(a.s0, ob);
        sp[6 * kFlowBlock] = at(a.z, ob);
        sp[7 * kFlowBlock] = at(a.bfd, ob);
        sp[8 * kFlowBlock] = at(a.sqrt_s0, ob);
        sp[9 * kFlowBlock] = at(a.sq1pz2, ob);
        sp[10 * kFlowBlock] = at(a.s0_n, ob);
        sp[11 * kFlowBlock] = at(a.s0_ncc, ob);
        sp[12 * kFlowBlock] = at(a.inv_n, ob);
    }
    const float dt = a.dt_col ? a.dt_col[su] : a.dt;
    const int32_t lag = LAG ? a.lag[su] : 0;
    const int32_t t_lo = LAG ? max(t0 - lag, 0) + 1 : t0 + 1;
    const int32_t t_hi = LAG ? min(t1 - lag, a.nsteps) : min(t1, a.nsteps);
    // flag bits: 0 edge 0 ahead, 1 edge 0 never through the ring, 2 / 3 the same for edge 1, 4 more than two upstream
    // rows, 5 reservoir row, 6 gage row
    uint32_t flags = 0;
    int32_t u0, u1;
    {
        const int2 up = a.up2[su];
        u0 = up.x;
        u1 = up.y >= 0 ? (up.y & 0x3fffffff) : -1;
        if (up.y >= 0 && (up.y & 0x40000000)) flags |= 16u;
        auto ring_ok = [&](int32_t u) { return u >= blk_base && u < blk_base + kFlowBlock && (!LAG || a.lag[u] == lag); };
        if (u0 >= 0 && !ring_ok(u0)) flags |= 2u;
        if (u1 >= 0 && !ring_ok(u1)) flags |= 8u;
        if (a.res_of_pos && a.res_of_pos[su] >= 0) flags |= 32u;
        if (a.gage_of_pos && a.gage_of_pos[su] >= 0) flags |= 64u;
    }
    const size_t np = (size_t)a.nseg_pad;
    const uint32_t out_idx = (uint32_t)a.row_of_pos[su] * (uint32_t)a.nsteps * 3u; // (the host checks nseg * nsteps * 3 < 2**32)
    bool dead = false;
    if (t_lo > t_hi) return;
    // the state this row was left in -- possibly by a launch that is still running (consecutive time chunks of a window
    // overlap on two streams): its own flow granule of step t_lo - 1 and the depth granule tagged with the same step
    float q_prev = flow_wait(a.gran + (size_t)(t_lo - 1) * np + su, a.tag_base + (uint32_t)(t_lo - 1), cold, dead);
    float d_prev = flow_wait(cold->d_gran + su, a.tag_base + (uint32_t)(t_lo - 1), cold, dead);
    __hip_atomic_store(s_ring + (size_t)((t_lo - 1) & (kLeanRing - 1)) * kFlowBlock + tix,
                       ((unsigned long long)(a.tag_base + (uint32_t)(t_lo - 1)) << 32) | (unsigned long long)__float_as_uint(q_prev),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    // the lateral-inflow column of step t is (t - 1) / qts: the first one is read now, the next ones as the counter runs out
    int32_t ql_col = (t_lo - 1) / a.qts;
    int32_t ql_left = a.qts - (t_lo - 1) % a.qts;
    float ql = a.qlat_tm[(size_t)ql_col * np + su];
    ++ql_col;
    uint32_t its = 0; // iterations: low 24 bits the sum of min(iterations, 3), high 8 bits those of the last step
    for (int32_t t = t_lo; t <= t_hi && !dead; ++t) {
        const uint32_t tag_p = a.tag_base + (uint32_t)(t - 1);
        const unsigned long long *g_prev = a.gran + (size_t)(t - 1) * np;
        if (ql_left == 0) { // (a counter, not (t - 1) % qts and (t - 1) / qts: two integer divisions per step otherwise)
            ql = cold->qlat_tm[(size_t)ql_col * np + su];
            ql_left = cold->qts;
            ++ql_col;
        }
        --ql_left;
        if ((t & 15) == 0) flags &= ~5u; // a producer that ran ahead may have been caught up with: try the ring again
        // junction sum in the reference's order (mc_reach.pyx:499-505)
        float qup = 0.0f;
        if (u0 >= 0) qup += lean_edge_get(u0, u0 - blk_base, flags, 1u, 2u, g_prev, s_ring, t - 1, tag_p, cold, dead);
        if (u1 >= 0) qup += lean_edge_get(u1, u1 - blk_base, flags, 4u, 8u, g_prev, s_ring, t - 1, tag_p, cold, dead);
        if (flags & 16u) {
            const int32_t *const up_ptr = cold->up_ptr, *const up_idx = cold->up_idx;
            const int32_t k1 = up_ptr[su + 1];
            for (int32_t e = up_ptr[su] + 2; e < k1; ++e) qup += flow_wait(g_prev + up_idx[e], tag_p, cold, dead);
        }
        float q_new = 0.0f, v_new = 0.0f, d_new = 0.0f;
        bool routed = false;
        trmc::ChannelParams<float> p;
        trmc::ChannelConst<float> c;
        if (flags & 32u) { // level-pool reservoir row (see k_mc_step)
            const int32_t ri = cold->res_of_pos[su];
            const int32_t nsteps = cold->nsteps;
            const float *rp = cold->res_par + (size_t)ri * 9;
            const trmc::LevelPoolParams<float> lp{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8]};
            float H = d_prev;
            q_new = trmc::levelpool_step<float, M>(qup, 0.0f, cold->res_dt, H, lp, m);
            if constexpr (RDA) { // (see k_mc_flow)
                void *const da = cold->res_da;
                const trmc::ResDaResult r = trmc::reservoir_da_row(da, ri, t, qup, d_prev, cold->res_dt, rp, q_new, H);
                q_new = r.outflow;
                H = r.water_elevation;
            }
            d_new = H;
            cold->res_inflow[(size_t)ri * (size_t)nsteps + (size_t)(t - 1)] = qup;
            its &= 0x00ffffffu;
        } else {
            trmc::Inflow<float> f;
            f.qup = qup;
            f.quc = qup;
            f.qdp = q_prev;
            f.ql = ql;
            uint32_t it_now = 0, it_cost = 0;
            if (trmc::step_has_flow(f)) {
                // (with assume_short_ts a row reads flows its upstream rows published a step ago: no dependence chain runs
                // through the step, so nothing of it is hoisted above the look-up -- see k_mc_flow -- and the two points of
                // the bracket are formed inside step_solve)
                const float *sp = s_par + tix;
                p.dt = dt;
                p.dx = sp[0 * kFlowBlock];
                p.bw = sp[1 * kFlowBlock];
                p.twcc = sp[2 * kFlowBlock];
                p.n = sp[3 * kFlowBlock];
                p.ncc = sp[4 * kFlowBlock];
                p.s0 = sp[5 * kFlowBlock];
                p.tw = p.cs = 0.0f;
                c.z = sp[6 * kFlowBlock];
                c.bfd = sp[7 * kFlowBlock];
                c.sqrt_s0 = sp[8 * kFlowBlock];
                c.sq1pz2 = sp[9 * kFlowBlock];
                c.s0_n = sp[10 * kFlowBlock];
                c.s0_ncc = sp[11 * kFlowBlock];
                c.inv_n = sp[12 * kFlowBlock];
                trmc::derive_const(c, p);
                trmc::StepPre<float> pre;
                pre.have = false;
                m.coef_ok = coef_guard(p.dt, f.ql);
                const trmc::StepSolve<float> r = trmc::step_solve<float, M>(p, c, f, d_prev, pre, m);
                q_new = r.qdc;
                d_new = r.h;
                routed = true;
                it_now = (uint32_t)min(r.iters, 255);
                it_cost = (uint32_t)min(r.iters, 3) + (r.over ? 4u : 0u);
            }
            its = ((its + it_cost) & 0x00ffffffu) | (it_now << 24);
            if (flags & 64u) { // streamflow nudging (see k_mc_step)
                const size_t e = (size_t)cold->gage_of_pos[su] * (size_t)cold->nsteps + (size_t)(t - 1);
                const float *const da_a = cold->da_a;
                const uint8_t mode = cold->da_mode[e];
                float nudge = 0.0f;
                if (mode == 1) {
                    nudge = da_a[e] - q_new;
                    q_new = da_a[e];
                } else if (mode == 2) {
                    nudge = (da_a[e] - q_new) * cold->da_w[e];
                    q_new = q_new + nudge;
                }
                cold->da_nudge[e] = nudge;
            }
        }
        // the flow goes out as soon as it exists; the velocity (a power, a square root, a division no other row waits for)
        // is formed after the granule is on its way
        {
            const unsigned long long g = ((unsigned long long)(tag_p + 1u) << 32) | (unsigned long long)__float_as_uint(q_new);
            __hip_atomic_store(s_ring + (size_t)(t & (kLeanRing - 1)) * kFlowBlock + tix, g, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(a.gran + (size_t)t * np + su, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (routed) v_new = trmc::step_velocity<float, M>(p, c, d_new, m);
        q_prev = q_new;
        d_prev = d_new;
        if (t == t_hi) // hand the depth over to the next launch of the window
            __hip_atomic_store(cold->d_gran + su, ((unsigned long long)(tag_p + 1u) << 32) | (unsigned long long)__float_as_uint(d_new),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        {
            float *o = a.out + (size_t)(out_idx + (uint32_t)(t - 1) * 3u);
            o[0] = q_new;
            o[1] = v_new;
            o[2] = d_new;
        }
    }
    if (cold->dbg) atomicMax(cold->dbg + 2 * s_blk + 1, (unsigned long long)wall_clock64());
    cold->d_state[su] = d_prev;
    if (t_hi == cold->nsteps) cold->it_prev[su] = (uint8_t)(its >> 24);
    if (uint16_t *const it_sum = cold->it_sum) it_sum[su] = (uint16_t)min(65535u, (uint32_t)it_sum[su] + (its & 0x00ffffffu));
}

// which compute units exist: every workgroup marks the key of the unit it runs on
__global__ void __launch_bounds__(64) k_cu_probe(uint8_t *seen)
{
    if (threadIdx.x == 0) seen[hw_cu_key()] = 1;
}
// initial state of the dataflow engine: granule row 0 <- qu0 (mc_reach.pyx:361), depth column <- h0
__global__ void __launch_bounds__(kBlock)
k_flow_init(const float *__restrict__ q0, const int32_t *__restrict__ row_of_pos, unsigned long long *gran, float *d_state,
            unsigned long long *d_gran, int32_t nseg, uint32_t tag_base)
{
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const size_t r = (size_t)row_of_pos[p] * 3;
    gran[p] = ((unsigned long long)tag_base << 32) | (unsigned long long)__float_as_uint(q0[r + 0]);
    d_state[p] = q0[r + 2];
    d_gran[p] = ((unsigned long long)tag_base << 32) | (unsigned long long)__float_as_uint(q0[r + 2]);
}
// boundary rows of the dataflow engine: hydrographs -> granules of the steps (t_begin, t_end] and the rows' result.
// src[b * stride_b + (t - 1 - t_begin) * stride_t + c]: bfvd[b][t-1][c] (stride_t = 3, ncomp = 3) or a flow block
// [b][t - 1 - t_begin] (stride_t = 1, ncomp = 1: velocity and depth of a boundary row are not inputs of anything, 0)
__global__ void __launch_bounds__(kBlock)
k_flow_boundary(const float *__restrict__ src, unsigned long long *gran, float *__restrict__ out,
                const int32_t *__restrict__ row_of_pos, int32_t nboundary, int32_t nsteps, int64_t nseg_pad, int32_t t_begin,
                int32_t t_end, int64_t stride_b, int32_t stride_t, int32_t ncomp, uint32_t tag_base,
                const int64_t *__restrict__ src_index)
{
    const int32_t w = t_end - t_begin;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)nboundary * w) return;
    const int32_t b = (int32_t)(i / w), k = (int32_t)(i % w), t = t_begin + 1 + k;
    const float *v = src + (size_t)(src_index ? src_index[b] : b) * stride_b + (size_t)k * stride_t;
    const float q = v[0];
    gran[(size_t)t * nseg_pad + b] = ((unsigned long long)(tag_base + (uint32_t)t) << 32) | (unsigned long long)__float_as_uint(q);
    float *o = out + ((size_t)row_of_pos[b] * nsteps + (t - 1)) * 3;
    o[0] = q;
    o[1] = ncomp > 1 ? v[1] : 0.0f;
    o[2] = ncomp > 2 ? v[2] : 0.0f;
}

// trmc_plan_set_stamps: the device's constant-rate clock (100 MHz) at four points of a window, written straight into
// page-locked host memory -- a timeline of consecutive windows of several plans without a profiler attached
__global__ void k_stamp(unsigned long long *slot) { *slot = wall_clock64(); }

// Every `stride`-th step of the result, out[row][t][3] -> dec[row][k][3] with t = stride (k + 1) - 1 (0-based): what the
// reference's writers consume of a window (nwm_routing/output.py:209-216 and :232-240 keep the steps whose END falls on a
// multiple of dt * qts_subdivisions).  One thread per (row, kept step): a 12-byte triple read at a stride of 12 * stride
// bytes, written densely.
template <class T>
__global__ void __launch_bounds__(kBlock)
k_decimate(const T *__restrict__ out, T *__restrict__ dec, int64_t nseg, int32_t nsteps, int32_t stride, int32_t nkeep)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nseg * nkeep) return;
    const int64_t row = i / nkeep;
    const int32_t k = (int32_t)(i - row * nkeep);
    const T *src = out + ((size_t)row * (size_t)nsteps + (size_t)(stride * (k + 1) - 1)) * 3;
    T *dst = dec + (size_t)i * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}

// NaN -> 0 in a freshly uploaded block (trmc_plan_set_nan_is_zero: the rows a caller's frame does not hold -- waterbody rows of the
// reference's reindexed q0 / qlat tables, compute.py:1466-1467 -- arrive as NaN; nothing routed reads them, and a plan that is
// told so spares its caller a pass over 260 MB of forcing on the host)
template <class T>
__global__ void __launch_bounds__(kBlock)
k_nan_to_zero(T *__restrict__ x, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const T v = x[i];
    if (v != v) x[i] = T(0);
}

// The same for a registered set of rows, in the set's order: dec[i][k][3] = the kept steps of row i of the set (rowset_pos holds
// plan positions, row_of_pos takes them to the rows of `out`) -- the result already grouped the way the caller hands it on
// (compute_nhd_routing_v02's per-tailwater list), without a gather of the whole block on the host.
template <class T>
__global__ void __launch_bounds__(kBlock)
k_decimate_rows(const T *__restrict__ out, T *__restrict__ dec, const int32_t *__restrict__ rowset_pos, const int32_t *__restrict__ row_of_pos,
                int64_t nrows, int32_t nsteps, int32_t stride, int32_t nkeep)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nrows * nkeep) return;
    const int64_t r = i / nkeep;
    const int32_t k = (int32_t)(i - r * nkeep);
    const int64_t row = row_of_pos[rowset_pos[r]];
    const T *src = out + ((size_t)row * (size_t)nsteps + (size_t)(stride * (k + 1) - 1)) * 3;
    T *dst = dec + (size_t)i * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}

// The rows a window's tiles did NOT decimate as they went (k_mc_tile<.., DEC>): their kept steps from the time-major planes --
// coalesced by position -- into dec[row][k][3]; positions [skip_lo, skip_hi) are the tiles'.
template <class T>
__global__ void __launch_bounds__(kBlock)
k_decimate_planes(const T *__restrict__ q_tm, const T *__restrict__ v_tm, const T *__restrict__ d_tm, const int32_t *__restrict__ row_of_pos,
                  T *__restrict__ dec, int32_t nseg, int64_t nseg_pad, int32_t stride, int32_t nkeep, int32_t skip_lo, int32_t skip_hi)
{
    const int32_t p = (int32_t)blockIdx.x * kBlock + (int32_t)threadIdx.x;
    if (p >= nseg || (p >= skip_lo && p < skip_hi)) return;
    T *dst = dec + (size_t)row_of_pos[p] * (size_t)nkeep * 3;
    size_t src = (size_t)stride * (size_t)nseg_pad + (size_t)p;
    for (int32_t k = 0; k < nkeep; ++k, src += (size_t)stride * (size_t)nseg_pad, dst += 3) {
        dst[0] = q_tm[src];
        dst[1] = v_tm[src];
        dst[2] = d_tm[src];
    }
}

