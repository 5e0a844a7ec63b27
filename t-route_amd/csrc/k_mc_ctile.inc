// k_mc_ctile.inc -- included by trmc.hip right behind k_mc_tile (same namespace, same StepArgs).
//
// The rows BELOW the wide levels of a short-timestep window, K timesteps per launch as well: CLUSTER TILES.
//
// k_mc_tile needs every flow a row reads during a tile to have been written by an earlier launch, so a level trails the one
// above it by a whole tile -- affordable for the six levels that hold three quarters of the CONUS network, not for the 3 532
// narrow ones below them, which until round 6 took one launch per timestep (k_mc_step: 288 launches that wait for each other,
// thirteen columns re-read at every step, a transposing pass for their results).  The plan now lays those rows out in
// CLUSTERS (topology.hpp, cluster_rows): connected pieces of the network of at most 128 rows.  The rows of a cluster sit
// in ONE block and advance together: a flow that stays inside the cluster goes from thread to thread through LDS (two step
// slots, one barrier per step), only a flow that ENTERS the cluster is read from the time-major plane -- and its row belongs to
// a cluster level (or a slice) that runs at least one tile ahead, exactly k_mc_tile's argument.  A chain of the network climbs a
// cluster level per 128 rows it collects instead of a level per row: 29 cluster levels under CONUS's six slices, so a window is
// 18 + 6 + 29 - 1 launches of this kind instead of 23 + 288, and all of a row's work is k_mc_tile's: parameters and state in
// registers, the forcing once per column, results staged in LDS and written as 96-byte runs of out[row][step][q,v,d].
//
// One block = one cluster block of the plan (cblk_ptr): whole clusters of ONE cluster level, up to kCtileBlock rows of them -- a
// block's rows share their lag, hence their steps: the barriers inside the time loop are uniform.  Threads take the block's rows
// by descending cost class like k_mc_tile's (the LDS slots are indexed by POSITION, so it does not matter which thread routes a
// row); there are no hot rows here -- a row routed by another block could not hand its flow over.
// Same bits as every other path: the same segment steps on the same inputs (tests run all of them against the oracle).
//
// kCtileBlock, the threads of a block, is the number of rows the class partition deals over wavefronts -- NOT the size of a
// cluster (cluster_rows, at most kClusterRowsMax: what decides how many cluster levels a chain climbs).  A wavefront's step costs
// what its costliest lane's does, and these rows are the big rivers: the partition puts a block's costly rows into its first
// wavefronts, so the wider the block, the smaller the share of its wavefronts that a handful of costly rows spoil (the slices
// have the hot list for that).  The plan packs whole clusters into blocks of this capacity (topology.hpp, cluster_block_rows).
// Measured on the CONUS stream, ms per day, one run each on one box: 128: 13.42, 256: 12.88, 512: 12.75, 1024: 12.99 (the parent
// commit beside them: 13.44); DESIGN.md section 7 has the interleaved A/B -- and what the counters say: the clusters issue 8 % fewer
// instructions at 512, but most of the gain is k_mc_tile's, whose launches no longer share their first third with all of the
// clusters' wavefronts (a launch of this kernel now lasts as long as the slices' beside it).  -DTRMC_CTILE_BLOCK=<width> builds another.
#ifndef TRMC_CTILE_BLOCK
#define TRMC_CTILE_BLOCK 512
#endif
constexpr int kCtileBlock = TRMC_CTILE_BLOCK;
constexpr int kClusterRowsMax = 128; // the most rows of a cluster (trmc_plan_options.cluster_rows)
static_assert(kCtileBlock % 64 == 0 && kCtileBlock >= kClusterRowsMax && kCtileBlock <= 1024,
              "TRMC_CTILE_BLOCK: whole wavefronts, at least one cluster, at most one workgroup");
constexpr int kCtileStage = kCtileBlock > 512 ? kTileStage / 2 : kTileStage; // (steps staged per run: fp64 rows of 1024 threads within a CU's LDS)
template <class T, bool TOL, bool DEC, bool LAZYV, bool RDA, bool PKD = false, bool DPL = false> // (see mc_step_rows; PKD: see k_mc_tile_pkd; DPL: k_mc_tile_dpl)
__device__ __forceinline__ void mc_ctile_rows(const StepArgs<T> &a, const int32_t *__restrict__ cblk_ptr, int32_t cb0, int32_t tile, int32_t K,
                                              T *pk_d = nullptr, int32_t *pk_at = nullptr);
template <class T, bool TOL = false, bool DEC = false, bool LAZYV = false>
__global__ void __launch_bounds__(kCtileBlock, sizeof(T) == 4 ? (LAZYV ? TRMC_TILE_WAVES_LAZY : TRMC_TILE_WAVES) : 1)
k_mc_ctile(const StepArgs<T> a, const int32_t *__restrict__ cblk_ptr, const int32_t cb0, const int32_t tile, const int32_t K)
{
    mc_ctile_rows<T, TOL, DEC, LAZYV, false>(a, cblk_ptr, cb0, tile, K);
}
template <bool DEC>
__global__ void __launch_bounds__(kCtileBlock, TRMC_TILE_WAVES)
k_mc_ctile_rda(const StepArgs<float> a, const int32_t *__restrict__ cblk_ptr, const int32_t cb0, const int32_t tile, const int32_t K)
{
    mc_ctile_rows<float, false, DEC, false, true>(a, cblk_ptr, cb0, tile, K);
}
// (the cluster rows' peak depth of the day: k_mc_tile_pkd)
template <class T, bool TOL = false, bool DEC = false>
__global__ void __launch_bounds__(kCtileBlock, sizeof(T) == 4 ? TRMC_TILE_WAVES_LAZY : 1)
k_mc_ctile_pkd(const StepArgs<T> a, const int32_t *__restrict__ cblk_ptr, const int32_t cb0, const int32_t tile, const int32_t K,
               T *const pk_d, int32_t *const pk_at)
{
    mc_ctile_rows<T, TOL, DEC, true, false, true>(a, cblk_ptr, cb0, tile, K, pk_d, pk_at);
}
// (the cluster rows' depth of every step into the slot's depth plane: k_mc_tile_dpl)
template <class T, bool TOL = false, bool DEC = false, bool PKD = false>
__global__ void __launch_bounds__(kCtileBlock, sizeof(T) == 4 ? TRMC_TILE_WAVES_LAZY : 1)
k_mc_ctile_dpl(const StepArgs<T> a, const int32_t *__restrict__ cblk_ptr, const int32_t cb0, const int32_t tile, const int32_t K,
               T *const pk_d, int32_t *const pk_at)
{
    mc_ctile_rows<T, TOL, DEC, true, false, PKD, true>(a, cblk_ptr, cb0, tile, K, pk_d, pk_at);
}
template <class T, bool TOL, bool DEC, bool LAZYV, bool RDA, bool PKD, bool DPL>
__device__ __forceinline__ void mc_ctile_rows(const StepArgs<T> &a, const int32_t *__restrict__ cblk_ptr, const int32_t cb0,
                                              const int32_t tile, const int32_t K, T *const pk_d, int32_t *const pk_at)
{
    using M = typename DevMath<T, TOL>::type;
    const ColdArgs<StepArgs<T>> cold = cold_args<StepArgs<T>>();
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    // (an instance that stages nothing -- LAZYV without DEC: a stream whose callers take products only -- declares one element)
    __shared__ T s_out[(DEC || !LAZYV) ? 3 * kCtileStage * kCtileBlock : 1]; // [step slot * 3 + c][thread]
    __shared__ T s_x[2 * kCtileBlock];                // [step & 1][position in the block]: the flows the cluster hands on
    M m{stage_pow_tables(s_tab), false};
    m.sane = a.sane;

    const int32_t cb = cb0 + (int32_t)blockIdx.x;
    const int32_t lo = cblk_ptr[cb], hi = cblk_ptr[cb + 1];
    int32_t behind, slot, slot_next; // (one cluster level per block: block-uniform)
    const bool in_range = seq_locate(a, tile, a.level[lo], behind, slot, slot_next);
    const int32_t t_lo = behind * K + 1, t_hi = min(behind * K + K, a.nsteps);
    if (!in_range || t_lo > t_hi) return;

    int32_t s = lo + (int32_t)threadIdx.x;
    bool active = s < hi;
    if (a.cls_last) {
        const int32_t c = active ? (int32_t)(a.cls_last[s] & 0x7f) : 0x80;
        const int32_t key = (c & 0x80) ? 8 : 7 - min(c, 7);
        bool none;
        s = lo + block_partition_by_class<kCtileBlock>(key, none);
        active = !none;
    }
    // issue priority by cost, as in k_mc_tile -- and never below 1: a cluster's rows wait for each other at every step
    if (a.cls_last) {
        const int32_t cp = active ? (int32_t)(a.cls_last[s] & 0x7f) : 0;
        if (__any(cp >= 3)) __builtin_amdgcn_s_setprio(3);
        else if (__any(cp == 2)) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(1);
    } else
        __builtin_amdgcn_s_setprio(2);
    const uint32_t su = (uint32_t)(active ? s : lo);
    const uint32_t sl = su - (uint32_t)lo; // the row's slot in s_x
    uint32_t ob = su * (uint32_t)sizeof(T);
    const size_t np = (size_t)a.nseg_pad;
    trmc::ChannelParams<T> p;
    trmc::ChannelConst<T> c;
    load_row_params(a, ob, p, c);
    int2 u = a.up2[su];
    if (!active) u.x = u.y = -1;
    // an upstream row inside the block's range is a row of the same cluster: its flow comes through LDS.  in0 / in1 hold the
    // BYTE offset of its slot, -1 = read the plane
    const int32_t uy = u.y >= 0 ? (u.y & 0x3fffffff) : -1;
    const int32_t in0 = (u.x >= lo && u.x < hi) ? (u.x - lo) * (int32_t)sizeof(T) : -1;
    const int32_t in1 = (uy >= lo && uy < hi) ? (uy - lo) * (int32_t)sizeof(T) : -1;
    const int32_t ri = (active && a.res_of_pos) ? a.res_of_pos[su] : -1;
    const int32_t gi = (active && a.gage_of_pos) ? a.gage_of_pos[su] : -1;

    T *const q_tm = a.q_tm + (size_t)slot * (size_t)a.slot_tm; // (a stream of windows: the block's day lives in its slot of the ring)
    const size_t ql_base = (size_t)slot * (size_t)a.slot_qlat;
    T q_prev = at(q_tm + (size_t)(t_lo - 1) * np, ob);
    T d_prev = at(a.d_tm + (size_t)slot * (size_t)a.slot_tm + (size_t)(t_lo - 1) * np, ob);
    T *const out_row = a.out + (size_t)slot * (size_t)a.slot_out + (size_t)a.row_of_pos[su] * (size_t)a.nsteps * 3;
    int32_t ql_col = (t_lo - 1) / a.qts, ql_left = a.qts - (t_lo - 1) % a.qts;
    T ql = at(a.qlat_tm + ql_base + (size_t)ql_col * np, ob);
    m.coef_ok = coef_guard(p.dt, ql);
    const bool count_cost = a.it_sum != nullptr;
    int32_t it_acc = 0, it_last = 0, staged = 0;
    bool over_last = false;
    if (active) s_x[(size_t)((t_lo - 1) & 1) * kCtileBlock + sl] = q_prev;
    __syncthreads();
    T *q_up = q_tm + (size_t)(t_lo - 1) * np;
    const ptrdiff_t d_of_q = DPL ? a.d_tm - a.q_tm : 0; // (as k_mc_tile)
    const int32_t v_every = (LAZYV && DEC) ? cold->v_every : 0; // (see StepArgs and k_mc_tile)
    int32_t v_left = v_every > 0 ? (v_every - 1) - ((t_lo - 1) % v_every) : 0;
    T dmax = T(0);
    int32_t dmax_at = 1;
    if constexpr (PKD) {
        if (t_lo != 1) { // (as k_mc_tile; a lane without a row reads the block's first row's and writes nothing)
            const size_t col = (size_t)slot * np + (size_t)su;
            dmax = pk_d[col];
            dmax_at = pk_at[col];
        }
    }
    for (int32_t t = t_lo; t <= t_hi; ++t, q_up += np) {
        bool want_v = false;
        if constexpr (LAZYV && DEC) {
            want_v = v_every > 0 && v_left == 0;
            if (v_every > 0) v_left = v_left == 0 ? v_every - 1 : v_left - 1;
        }
        if (active) {
            if (ql_left == 0) {
                ++ql_col;
                ql = at(cold->qlat_tm + ql_base + (size_t)ql_col * np, ob);
                m.coef_ok = coef_guard(p.dt, ql);
                ql_left = cold->qts;
            }
            --ql_left;
            // junction sum in the reference's order (mc_reach.pyx:499-502), every term from where it lives
            const T *const sx = s_x + (size_t)((t - 1) & 1) * kCtileBlock;
            T qup = T(0);
            if (u.x >= 0) qup += in0 >= 0 ? at(sx, (uint32_t)in0) : at(q_up, (uint32_t)u.x * (uint32_t)sizeof(T));
            if (uy >= 0) qup += in1 >= 0 ? at(sx, (uint32_t)in1) : at(q_up, (uint32_t)uy * (uint32_t)sizeof(T));
            if (uy >= 0) {
                if (u.y & 0x40000000) {
                    const int32_t *const up_ptr = cold->up_ptr, *const up_idx = cold->up_idx;
                    const int32_t k1 = up_ptr[su + 1];
                    for (int32_t k = up_ptr[su] + 2; k < k1; ++k) {
                        const int32_t uk = up_idx[k];
                        qup += (uk >= lo && uk < hi) ? sx[uk - lo] : at(q_up, (uint32_t)uk * (uint32_t)sizeof(T));
                    }
                }
            }
            T q_new, v_new, d_new;
            if (ri >= 0) { // level-pool reservoir row (see k_mc_step)
                reservoir_row<T, M, RDA>(cold, m, slot, ri, t, qup, d_prev, q_new, v_new, d_new);
                it_last = 0;
            } else {
                trmc::Inflow<T> f;
                f.qup = qup;
                f.quc = qup;
                f.qdp = q_prev;
                f.ql = ql;
                const trmc::StepResult<T> r = trmc::mc_segment_step<T, M>(p, c, f, d_prev, m, !LAZYV);
                q_new = r.qdc;
                v_new = r.velc;
                d_new = r.depthc;
                it_last = r.iters;
                over_last = r.over;
                if (count_cost) it_acc += min(r.iters, 3) + (r.over ? 4 : 0);
                if (gi >= 0) nudge_row<T>(cold, slot, gi, t, q_new);
            }
            asm volatile("" : "+v"(ob));
            at(q_up + np, ob) = q_new;
            if constexpr (DPL) {
                if (t != t_hi) at(q_up + np + d_of_q, ob) = d_new; // (the tile's last step: hand_on_row)
            }
            s_x[(size_t)(t & 1) * kCtileBlock + sl] = q_new;
            hand_on_row<T>(cold, slot, slot_next, ob, np, t, t_hi, q_new, d_new);
            q_prev = q_new;
            d_prev = d_new;
            if constexpr (PKD) {
                if (t == 1 || d_new > dmax) {
                    dmax = d_new;
                    dmax_at = t;
                }
            }
            if (LAZYV && want_v && it_last > 0) v_new = trmc::step_velocity<T, M>(p, c, d_new, m); // (as k_mc_tile)
            if (DEC || (!LAZYV && a.out)) { // stage (q, v, d) of step t; a run ends when kCtileStage steps are staged and at the tile's last step
                // (a.out == nullptr: a stream of windows whose callers take products only -- nothing of the full result is assembled)
                T *so = s_out + (size_t)(staged * 3) * kCtileBlock + threadIdx.x;
                so[0] = q_new;
                so[kCtileBlock] = v_new;
                so[2 * kCtileBlock] = d_new;
                ++staged;
                if (staged == kCtileStage || t == t_hi) {
                    T *dst = out_row + (size_t)(t - staged) * 3;
                    const T *si = s_out + threadIdx.x;
                    if (LAZYV || !a.out) {
                    } else if (a.out_vec && (staged & 3) == 0) {
                        for (int j = 0; j < 3 * staged / 4; ++j) {
                            float4 v;
                            v.x = (float)si[(4 * j + 0) * kCtileBlock];
                            v.y = (float)si[(4 * j + 1) * kCtileBlock];
                            v.z = (float)si[(4 * j + 2) * kCtileBlock];
                            v.w = (float)si[(4 * j + 3) * kCtileBlock];
                            reinterpret_cast<float4 *>(dst)[j] = v;
                        }
                    } else {
                        for (int32_t e = 0; e < 3 * staged; ++e) dst[e] = si[e * kCtileBlock];
                    }
                    if constexpr (DEC) {
                        const int32_t ds = cold->dec_stride;
                        for (int32_t k = t / ds; k >= 1 && k * ds > t - staged; --k) {
                            if (k > cold->dec_keep) continue;
                            const int32_t kslot = k * ds - (t - staged) - 1;
                            T *dd = cold->dec + (size_t)slot * (size_t)cold->slot_dec + ((size_t)cold->row_of_pos[su] * (size_t)cold->dec_keep + (size_t)(k - 1)) * 3;
                            dd[0] = si[(kslot * 3 + 0) * kCtileBlock];
                            dd[1] = si[(kslot * 3 + 1) * kCtileBlock];
                            dd[2] = si[(kslot * 3 + 2) * kCtileBlock];
                        }
                    }
                    staged = 0;
                }
            }
        }
        __syncthreads(); // step t's flows are in s_x[t & 1] for step t + 1; slot (t - 1) & 1 is free again
    }
    if (!active) return;
    if constexpr (PKD) {
        const size_t col = (size_t)slot * np + (size_t)su;
        pk_d[col] = dmax;
        pk_at[col] = dmax_at;
    }
    if (t_hi == cold->nsteps) cold->it_prev[su] = (uint8_t)min(it_last, 255);
    if (uint8_t *const cls = cold->cls_last) cls[su] = (uint8_t)(min(it_last, 3) + (over_last ? 4 : 0));
    if (uint16_t *const it_sum = cold->it_sum) it_sum[su] = (uint16_t)min(65535, (int)it_sum[su] + it_acc);
}
