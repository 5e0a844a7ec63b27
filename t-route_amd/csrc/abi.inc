// abi.inc -- included by trmc.hip inside extern "C": the entry points of include/trmc.h (the stream of windows: stream.inc).

static bool stream_active(const trmc_plan *pl);

const char *trmc_last_error(void) { return g_err.c_str(); }
int trmc_abi_version(void) { return TRMC_ABI_VERSION; }

int trmc_device_count(int *count)
{
    if (!count) return fail(TRMC_EINVAL, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *count = 0;
        return fail(TRMC_ENODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = c;
    return 0;
}

int trmc_topology_levels(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const uint8_t *boundary,
                         int32_t *level_of_row, int64_t *plan_pos_of_row, int32_t *nlevels)
{
    return trmc_topology_levels_hinted(nseg, up_ptr, up_idx, boundary, nullptr, level_of_row, plan_pos_of_row, nlevels);
}

int trmc_topology_levels_hinted(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const uint8_t *boundary,
                                const uint8_t *cost_hint, int32_t *level_of_row, int64_t *plan_pos_of_row, int32_t *nlevels)
{
    trmc::Topology t;
    std::string err;
    const int rc = trmc::build_topology(nseg, up_ptr, up_idx, boundary, t, err, cost_hint);
    if (rc) return fail(rc == -2 ? TRMC_ECYCLE : TRMC_EINVAL, err);
    for (int64_t r = 0; r < nseg; ++r) {
        if (level_of_row) level_of_row[r] = t.level_of_row[r];
        if (plan_pos_of_row) plan_pos_of_row[r] = t.pos_of_row[r];
    }
    if (nlevels) *nlevels = t.nlevels;
    return 0;
}

int trmc_topology_clusters(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const uint8_t *boundary,
                           const uint8_t *cost_hint, int64_t wide_min_rows, int32_t wide_max_levels, int32_t cluster_rows,
                           int64_t *plan_pos_of_row, int32_t *lag_of_row, int32_t *block_of_row, int32_t *wide_levels,
                           int32_t *cluster_levels, int32_t *cluster_blocks)
{
    if (cluster_rows <= 0 || cluster_rows > kClusterRowsMax) return fail(TRMC_EINVAL, "cluster_rows must be in [1, 128]");
    trmc::Topology t;
    std::string err;
    const int rc = trmc::build_topology(nseg, up_ptr, up_idx, boundary, t, err, cost_hint, 0, true, kWideMaxLevels, wide_min_rows,
                                        std::min<int32_t>(wide_max_levels, kWideMaxLevels), 0, 0, 0, cluster_rows);
    if (rc) return fail(rc == -2 ? TRMC_ECYCLE : TRMC_EINVAL, err);
    const int32_t nb = t.ncl > 0 ? (int32_t)t.cblk_ptr.size() - 1 : 0;
    std::vector<int32_t> blk_of_pos((size_t)nseg, -1);
    for (int32_t b = 0; b < nb; ++b)
        for (int32_t p = t.cblk_ptr[(size_t)b]; p < t.cblk_ptr[(size_t)b + 1]; ++p) blk_of_pos[(size_t)p] = b;
    for (int64_t r = 0; r < nseg; ++r) {
        const int32_t p = t.pos_of_row[r];
        if (plan_pos_of_row) plan_pos_of_row[r] = p;
        if (lag_of_row) lag_of_row[r] = t.level_of_row[r] < 0 ? -1 : t.lagk_of_pos[(size_t)p];
        if (block_of_row) block_of_row[r] = blk_of_pos[(size_t)p];
    }
    if (wide_levels) *wide_levels = t.cl_from_level;
    if (cluster_levels) *cluster_levels = t.ncl;
    if (cluster_blocks) *cluster_blocks = nb;
    return 0;
}

int trmc_topology_blocks(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const uint8_t *boundary,
                         const uint8_t *cost_hint, int cost_tiers, int64_t *plan_pos_of_row, int32_t *rank_of_row,
                         int32_t *block_rows, int32_t *nblocks)
{
    trmc::Topology t;
    std::string err;
    const int rc = trmc::build_topology(nseg, up_ptr, up_idx, boundary, t, err, cost_hint, kFlowBlock, cost_tiers != 0);
    if (rc) return fail(rc == -2 ? TRMC_ECYCLE : TRMC_EINVAL, err);
    for (int64_t r = 0; r < nseg; ++r) {
        if (plan_pos_of_row) plan_pos_of_row[r] = t.pos_of_row[r];
        if (rank_of_row) rank_of_row[r] = t.rank_of_pos[t.pos_of_row[r]];
    }
    if (block_rows) *block_rows = t.block_rows;
    if (nblocks) *nblocks = t.nblocks;
    return 0;
}

int trmc_topology_blocks_general(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const uint8_t *boundary,
                                 int32_t stem_min_rows, int64_t *plan_pos_of_row, int32_t *rank_of_row, int32_t *block_rows,
                                 int32_t *nblocks, int32_t *early_blocks, int32_t early_cap, int32_t *nearly)
{
    trmc::Topology t;
    std::string err;
    const int rc = trmc::build_topology(nseg, up_ptr, up_idx, boundary, t, err, nullptr, kFlowBlock, false, 0, 0, 0,
                                        std::max<int32_t>(0, stem_min_rows));
    if (rc) return fail(rc == -2 ? TRMC_ECYCLE : TRMC_EINVAL, err);
    for (int64_t r = 0; r < nseg; ++r) {
        if (plan_pos_of_row) plan_pos_of_row[r] = t.pos_of_row[r];
        if (rank_of_row) rank_of_row[r] = t.rank_of_pos[t.pos_of_row[r]];
    }
    if (block_rows) *block_rows = t.block_rows;
    if (nblocks) *nblocks = t.nblocks;
    if (nearly) *nearly = (int32_t)t.early_blocks.size();
    for (int32_t i = 0; early_blocks && i < early_cap && i < (int32_t)t.early_blocks.size(); ++i) early_blocks[i] = t.early_blocks[(size_t)i];
    return 0;
}

int trmc_plan_create(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const float *params,
                     const uint8_t *boundary, int precision, int device, trmc_plan **out)
{
    return trmc_plan_create_hinted(nseg, up_ptr, up_idx, params, boundary, nullptr, precision, device, out);
}

int trmc_plan_create_hinted(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const float *params,
                            const uint8_t *boundary, const uint8_t *cost_hint, int precision, int device, trmc_plan **out)
{
    return trmc_plan_create_ex(nseg, up_ptr, up_idx, params, boundary, cost_hint, precision, device, TRMC_ENGINE_AUTO, out);
}

int trmc_plan_engine(const trmc_plan *pl, int32_t *is_flow)
{
    if (!pl || !is_flow) return fail(TRMC_EINVAL, "plan/is_flow is NULL");
    *is_flow = pl->flow ? 1 : 0;
    return 0;
}

int trmc_plan_set_sequence_mode(trmc_plan *pl, int on)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is in progress");
    pl->opt.sequence = on != 0;
    return 0;
}

int trmc_plan_hot_rows(trmc_plan *pl, int64_t *rows_out)
{
    if (!pl || !rows_out) return fail(TRMC_EINVAL, "plan/rows_out is NULL");
    *rows_out = 0;
    if (!pl->hot_cnt.p) return 0;
    if (int rc = use_device(pl)) return rc;
    int32_t n = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&n, (const int32_t *)pl->hot_cnt.p + 3, sizeof n, hipMemcpyDeviceToHost));
    *rows_out = n;
    return 0;
}

// (host only: no launch, no buffer of its own -- what tile_setup / tile_args / tile_turn hold, and the three lengths as the last
// launch left them: an append past hot_cap is counted and not stored, so a length above hot_cap says the list overflowed)
int trmc_plan_hot_state(trmc_plan *pl, int32_t *cap, int32_t *hot_home, int32_t counts[3], int32_t *cur_next, int32_t *tile_block,
                        int32_t *wave_max)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (tile_block) *tile_block = kTileBlock;
    if (wave_max) *wave_max = TRMC_HOT_WAVE_MAX;
    if (cur_next) *cur_next = (int32_t)(pl->tile_seq % 3);
    if (cap) *cap = 0;
    if (hot_home) *hot_home = 0;
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    if (!pl->hot_cnt.p || !pl->hot_list.p || pl->hot_cap <= 0) return 0;
    if (cap) *cap = pl->hot_cap;
    if (hot_home) {
        const int32_t per_block = hot_wave_rows_of(pl) * (kTileBlock / 64);
        *hot_home = (pl->hot_cap + per_block - 1) / per_block;
    }
    if (!counts) return 0;
    if (int rc = use_device(pl)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, pl->hot_cnt.p, 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int trmc_plan_set_output_stride(trmc_plan *pl, int32_t stride)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is open");
    if (stride < 0) return fail(TRMC_EINVAL, "stride must be >= 0");
    pl->out_stride = stride;
    return 0;
}

int trmc_plan_set_stamps(trmc_plan *pl, void *host_ring, int32_t nwindows)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is open");
    if (host_ring && nwindows < 1) return fail(TRMC_EINVAL, "nwindows must be >= 1");
    pl->stamps = (unsigned long long *)host_ring;
    pl->nstamp_windows = host_ring ? nwindows : 0;
    pl->stamp_seq = -1;
    return 0;
}

int trmc_plan_arithmetic(const trmc_plan *pl, int32_t *arithmetic)
{
    if (!pl || !arithmetic) return fail(TRMC_EINVAL, "plan/arithmetic is NULL");
    *arithmetic = pl->opt.tol ? TRMC_ARITH_TOLERANCE : TRMC_ARITH_EXACT;
    return 0;
}

int trmc_plan_create_ex(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const float *params,
                        const uint8_t *boundary, const uint8_t *cost_hint, int precision, int device, int flags,
                        trmc_plan **out)
{
    return trmc_plan_create_opt(nseg, up_ptr, up_idx, params, boundary, cost_hint, precision, device, flags, nullptr, out);
}

// the streams and events every plan has from the start (the others are made where they are first needed)
static int plan_streams(trmc_plan *pl)
{
    HIP_TRY(hipSetDevice(pl->device));
    // step launches on a high-priority stream, the overlapped transpose on a low-priority one:
    // the transpose should fill gaps, not displace the VALU-bound step kernel
    int prio_lo = 0, prio_hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    if (int rc = pl->stream.ensure(hipStreamNonBlocking, prio_hi)) return rc;
    if (int rc = pl->stream2.ensure(hipStreamNonBlocking, prio_lo)) return rc;
    if (int rc = pl->ev_emit.ensure(false)) return rc;
    if (pl->flow) {
        if (int rc = pl->fstream.ensure(hipStreamNonBlocking, prio_hi)) return rc;
        for (DevEvent &e : pl->ev_chunk)
            if (int rc = e.ensure(false)) return rc;
        if (int rc = pl->ev_ctl.ensure(false)) return rc;
    }
    for (DevEvent &e : pl->ev)
        if (int rc = e.ensure(true)) return rc;
    return 0;
}

int trmc_plan_create_opt(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const float *params,
                         const uint8_t *boundary, const uint8_t *cost_hint, int precision, int device, int flags,
                         const trmc_plan_options *options, trmc_plan **out)
{
    if (!out) return fail(TRMC_EINVAL, "out is NULL");
    trmc_plan_options o{};
    if (options) {
        if (options->struct_size < 8 || options->struct_size > (int32_t)sizeof(trmc_plan_options))
            return fail(TRMC_EINVAL, "trmc_plan_options.struct_size is not the size of a trmc_plan_options this library knows");
        std::memcpy(&o, options, (size_t)options->struct_size);
    }
    if (o.arithmetic != TRMC_ARITH_EXACT && o.arithmetic != TRMC_ARITH_TOLERANCE) return fail(TRMC_EINVAL, "bad trmc_plan_options.arithmetic");
    if (o.arithmetic == TRMC_ARITH_TOLERANCE && precision != 32)
        return fail(TRMC_EINVAL, "TRMC_ARITH_TOLERANCE is an arithmetic of precision-32 plans");
    *out = nullptr;
    if (precision != 32 && precision != 64) return fail(TRMC_EINVAL, "precision must be 32 or 64");
    if (nseg > 0 && !params) return fail(TRMC_EINVAL, "params is NULL");
    if ((flags & ~(TRMC_ENGINE_MASK | TRMC_PLAN_SHORT_TS | TRMC_PLAN_FULL_TS)) || (flags & TRMC_ENGINE_MASK) == 3
        || ((flags & TRMC_PLAN_SHORT_TS) && (flags & TRMC_PLAN_FULL_TS)))
        return fail(TRMC_EINVAL, "bad plan flags");
    int engine = flags & TRMC_ENGINE_MASK;
    if (engine == TRMC_ENGINE_FLOW && precision != 32) return fail(TRMC_EINVAL, "the dataflow engine runs precision-32 plans only");
    if (int rc = check_device(device)) return rc;

    trmc_plan *pl = new (std::nothrow) trmc_plan();
    if (!pl) return fail(TRMC_ENOMEM, "out of host memory");
    pl->sh = std::make_shared<PlanShared>();
    if (engine == TRMC_ENGINE_AUTO) {
        if (precision != 32)
            engine = TRMC_ENGINE_LEVELS;
        else {
            int64_t nb = 0;
            for (int64_t r = 0; boundary && r < nseg; ++r) nb += boundary[r] == 1;
            engine = ((flags & TRMC_PLAN_SHORT_TS) && nseg - nb >= 1000000) ? TRMC_ENGINE_LEVELS : TRMC_ENGINE_FLOW;
        }
    }
    pl->flow = engine == TRMC_ENGINE_FLOW;
    pl->watchdog_ticks = (uint64_t)(o.flow_watchdog_ms > 0 ? o.flow_watchdog_ms : 30000) * 100000ull;
    {   // the options, resolved once (see trmc.h)
        int ncu = 256;
        if (hipSetDevice(device) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        trmc_plan::Opt &po = pl->opt;
        po.tol = o.arithmetic == TRMC_ARITH_TOLERANCE;
        // (default threshold of the wide tier, until round 5: 384 rows per compute unit -- five levels of the CONUS network -- in exact arithmetic,
        // where the tiles are what the device is busy with and the ramps of the skew cost; 256 -- seven levels -- in tolerance
        // arithmetic, where a tile's arithmetic is a quarter cheaper and the window waits for the tail's chain of launches:
        // 12.8 ms per CONUS day against 14.0, measured on the sequence of bench.py; 192: 13.0, 128: 13.4)
        // Round 5, with the partition of a tile's rows inside the launch (no launch between tiles any more): exact arithmetic
        // 288 rows per compute unit -- six levels of CONUS -- 16.7 ms per day against 17.2 with five, 16.85 with seven or eight
        // (three runs each on one box).
        po.wide_min_rows = o.wide_min_rows < 0 ? 0 : (o.wide_min_rows > 0 ? o.wide_min_rows : (po.tol ? 256L : 288L) * ncu);
        po.wide_levels = (int32_t)std::min<long>(o.wide_levels > 0 ? o.wide_levels : 16, kWideMaxLevels);
        po.wide_k = o.wide_k > 0 ? o.wide_k : 0; // (0: 16, or an eighth of a short window -- route_begin_t)
        po.mid_min_rows = o.mid_min_rows < 0 ? 0 : (o.mid_min_rows > 0 ? o.mid_min_rows : kMidDefaultRowsPerCu * (int64_t)ncu);
        po.mid_levels = (int32_t)std::min<long>(o.mid_levels > 0 ? o.mid_levels : 12, kMidMaxLevels);
        po.mid_k = o.mid_k > 0 ? o.mid_k : 4;
        po.tile_perm_group = o.tile_perm_group < 0 ? 0 : (o.tile_perm_group > 0 ? 1 : -1); // off / on / by the plan (default)
        po.hot_rows = o.hot_rows < 0 ? 0 : (o.hot_rows > 0 ? 1 : -1);
        // (the cluster order is for plans whose windows follow each other as a stream, trmc_stream_*: a single window pays for the
        // clusters' skew with some thirty small launches at its end -- CONUS: 20.7 ms alone against 16.8 with one launch per
        // step -- so a plan only gets it when asked)
        po.cluster_rows = o.cluster_rows > 0 ? std::min<int32_t>(o.cluster_rows, kClusterRowsMax) : 0;
        po.cluster_late_lag = std::max(0, o.cluster_late_lag);
        po.stream_split = std::max(0, o.stream_split);
        po.hot_wave_rows = std::max(0, std::min(64, o.hot_wave_rows));
        po.velocity_on_demand = o.velocity_on_demand;
        po.sequence = o.sequence_mode != 0;
        po.flow_overlap = o.flow_overlap != 0;
        po.flow_lean = o.flow_lean;
        po.flow_debug = o.flow_debug != 0;
    }
    const bool tiers = (flags & TRMC_PLAN_SHORT_TS) != 0;
    std::string err;
    // (plans meant for assume_short_ts on the level engine: rows fed by boundary rows stay below the levels that may be routed
    // several timesteps per launch -- topology.hpp, boundary_floor; wide_levels never asks for more than kWideMaxLevels, and the
    // second tier only takes levels none of whose rows reads a boundary row: route_begin_t)
    // ... and (a hinted short-timestep plan of the level engine) the rows below the levels that can be routed several timesteps
    // per launch are ordered by cost across levels: the same rule picks those levels here as in route_begin_t, which never
    // takes more of them than the plan was ordered for.  tail_sort < 0 keeps the per-level order (A/B).
    int64_t wide_min_rows = 0, mid_min_rows = 0;
    int32_t wide_max_levels = 0, mid_max_levels = 0;
    if (tiers && !pl->flow && cost_hint && o.tail_sort >= 0) {
        wide_min_rows = pl->opt.wide_min_rows;
        wide_max_levels = pl->opt.wide_levels;
        mid_min_rows = pl->opt.mid_min_rows;
        mid_max_levels = pl->opt.mid_levels;
    }
    // ... or, if asked for, laid out in CLUSTERS (topology.hpp, cluster_rows): then they are routed several timesteps per launch
    // as well (k_mc_ctile) -- what a stream of windows needs (trmc_stream_*); the second tier has no part in that
    int32_t cluster_rows = 0;
    if (tiers && !pl->flow && pl->opt.cluster_rows > 0) {
        cluster_rows = pl->opt.cluster_rows;
        wide_min_rows = pl->opt.wide_min_rows;
        wide_max_levels = pl->opt.wide_levels;
        mid_min_rows = 0;
        mid_max_levels = 0;
        pl->opt.mid_min_rows = 0;
    }
    // (a dataflow plan built for the general mode: basins with a main stem of at least stem_min_rows rows -- default 1 024,
    // < 0 = off -- are laid out stem-last with the side tributaries from the top of the stem down, and their stems' blocks take
    // the first tickets: topology.hpp, stem_min_rows)
    int32_t stem_min_rows = 0;
    if (pl->flow && (flags & TRMC_PLAN_FULL_TS)) stem_min_rows = o.stem_min_rows < 0 ? 0 : (o.stem_min_rows > 0 ? o.stem_min_rows : 1024);
    const int trc = trmc::build_topology(nseg, up_ptr, up_idx, boundary, pl->sh->topo, err, cost_hint, pl->flow ? kFlowBlock : 0, tiers,
                                         (tiers && !pl->flow) ? kWideMaxLevels : 0, wide_min_rows, wide_max_levels, stem_min_rows,
                                         mid_min_rows, mid_max_levels, cluster_rows, pl->opt.cluster_late_lag, kCtileBlock);
    if (trc) {
        delete pl;
        return fail(trc == -2 ? TRMC_ECYCLE : TRMC_EINVAL, err);
    }
    pl->device = device;
    pl->hinted = cost_hint != nullptr && (!pl->flow || tiers);
    pl->precision = precision;
    pl->esz = precision == 32 ? 4 : 8;
    pl->nseg = nseg;
    pl->nseg_pad = (nseg + 63) / 64 * 64;
    if (pl->nseg_pad == 0) pl->nseg_pad = 64;
    pl->nrouted = nseg - pl->sh->topo.nboundary;
    pl->dt_uniform = true;
    pl->dt = nseg ? params[TRMC_P_DT] : 0.0;
    for (int64_t r = 1; r < nseg; ++r)
        if (params[(size_t)r * TRMC_NPARAM + TRMC_P_DT] != params[TRMC_P_DT]) {
            pl->dt_uniform = false;
            break;
        }

    auto bail = [&](int rc) {
        trmc_plan_destroy(pl);
        return rc;
    };
    int rc = plan_streams(pl);
    if (rc) return bail(rc);
    rc = by_precision(pl, [&](auto t) { return upload_params<decltype(t)>(pl, params); });
    if (rc) return bail(rc);
    std::vector<int32_t> level_plan((size_t)pl->nseg_pad, 0);
    for (int64_t p = 0; p < nseg; ++p) level_plan[p] = pl->sh->topo.level_of_row[pl->sh->topo.row_of_pos[p]];
    if ((rc = upload_i32(pl->sh->level, level_plan, 1))) return bail(rc);
    if (pl->sh->topo.ncl > 0) {
        std::vector<int32_t> lagk(pl->sh->topo.lagk_of_pos);
        lagk.resize((size_t)pl->nseg_pad, 0);
        if ((rc = upload_i32(pl->sh->lagk, lagk, 1))) return bail(rc);
        if ((rc = upload_i32(pl->sh->cblk_ptr, pl->sh->topo.cblk_ptr, 1))) return bail(rc);
    }
    if ((rc = upload_i32(pl->sh->up_ptr, pl->sh->topo.up_ptr, 1))) return bail(rc);
    if ((rc = upload_i32(pl->sh->up_idx, pl->sh->topo.up_idx, 1))) return bail(rc);
    {
        if (nseg >= (int64_t)1 << 30) return bail(fail(TRMC_EINVAL, "more than 2**30 segments in one plan"));
        // (the step kernels address a column with a 32-bit BYTE offset: position * element size)
        if ((uint64_t)pl->nseg_pad * pl->esz >= (1ull << 32))
            return bail(fail(TRMC_EINVAL, "too many segments for one plan at this precision (column size reaches 4 GiB)"));
        std::vector<int32_t> up2((size_t)pl->nseg_pad * 2, -1);
        for (int64_t p = 0; p < nseg; ++p) {
            const int32_t k0 = pl->sh->topo.up_ptr[p], k1 = pl->sh->topo.up_ptr[p + 1];
            if (k1 - k0 >= 1) up2[2 * p] = pl->sh->topo.up_idx[k0];
            if (k1 - k0 >= 2) up2[2 * p + 1] = pl->sh->topo.up_idx[k0 + 1] | (k1 - k0 > 2 ? 0x40000000 : 0);
        }
        if ((rc = upload_i32(pl->sh->up2, up2, 2))) return bail(rc);
    }
    if (pl->flow && (rc = upload_i32(pl->sh->rank, pl->sh->topo.rank_of_pos, 1))) return bail(rc);
    if (pl->flow) {
        if ((rc = pl->sh->prio.ensure(pl->sh->topo.prio_of_wave.size() + 1))) return bail(rc);
        if (!pl->sh->topo.prio_of_wave.empty()
            && hipMemcpy(pl->sh->prio.p, pl->sh->topo.prio_of_wave.data(), pl->sh->topo.prio_of_wave.size(), hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(TRMC_EHIP, "uploading the wavefront priorities failed"));
        if ((rc = flow_place_blocks(pl))) return bail(rc);
        // The stems' blocks take the first tickets and wait IN PLACE for their inflows: nothing deadlocks as long as the device
        // holds more workgroups of the kernel at once than there are such blocks -- the others then still find slots.  Asked
        // of the runtime for THIS device (occupancy x compute units; a smaller part, a masked one); a plan whose stems would
        // take more than half of the slots routes in the plain ticket order instead.
        if (!pl->sh->topo.early_blocks.empty()) {
            int per_cu = 0, ncu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_mc_flow<false, false>, kFlowBlock, 0) != hipSuccess) per_cu = 0;
            (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device);
            if ((int64_t)pl->sh->topo.early_blocks.size() * 2 > (int64_t)per_cu * ncu) pl->sh->topo.early_blocks.clear();
        }
        if (!pl->sh->topo.early_blocks.empty()) { // ticket -> block: the stems' blocks, then everybody else in order
            const int32_t nb = pl->sh->topo.nblocks;
            std::vector<int32_t> map;
            map.reserve((size_t)nb);
            std::vector<uint8_t> early((size_t)nb, 0);
            for (const int32_t b : pl->sh->topo.early_blocks) {
                early[(size_t)b] = 1;
                map.push_back(b);
            }
            for (int32_t b = 0; b < nb; ++b)
                if (!early[(size_t)b]) map.push_back(b);
            if ((rc = upload_i32(pl->sh->ticket_map, map, 1))) return bail(rc);
        }
    }
    if ((rc = upload_i32(pl->sh->row_of_pos, pl->sh->topo.row_of_pos, 1))) return bail(rc);
    if ((rc = upload_i32(pl->sh->pos_of_row, pl->sh->topo.pos_of_row, 1))) return bail(rc);
    if ((rc = pl->it_prev.ensure((size_t)pl->nseg_pad))) return bail(rc);
    *out = pl;
    return 0;
}

void trmc_plan_destroy(trmc_plan *pl)
{
    if (!pl) return;
    (void)hipSetDevice(pl->device);
    delete pl; // (the members release themselves, in the order the head of trmc_plan describes)
}

static int final_state_into(trmc_plan *pl, void *dst, int32_t nsteps_of_window = -1);
static int ensure_copy_stream(trmc_plan *pl);

int trmc_plan_clone(trmc_plan *src, trmc_plan **out)
{
    if (!out) return fail(TRMC_EINVAL, "out is NULL");
    *out = nullptr;
    if (!src) return fail(TRMC_EINVAL, "plan is NULL");
    if (int rc = use_device(src)) return rc;
    trmc_plan *pl = new (std::nothrow) trmc_plan();
    if (!pl) return fail(TRMC_ENOMEM, "out of host memory");
    pl->device = src->device;
    pl->precision = src->precision;
    pl->esz = src->esz;
    pl->nseg = src->nseg;
    pl->nseg_pad = src->nseg_pad;
    pl->nrouted = src->nrouted;
    pl->dt_uniform = src->dt_uniform;
    pl->dt = src->dt;
    pl->hinted = src->hinted;
    pl->params_sane = src->params_sane;
    pl->flow = src->flow;
    pl->watchdog_ticks = src->watchdog_ticks;
    pl->opt = src->opt;
    pl->ncuq = src->ncuq;
    // static data: the original's (plan order, parameters and constants, the dataflow engine's placement tables), shared with
    // it and with every other clone of it -- a clone of a clone holds the same block
    pl->sh = src->sh;
    pl->is_clone = true;
    auto bail = [&](int rc) {
        trmc_plan_destroy(pl);
        return rc;
    };
    if (int rc = plan_streams(pl)) return bail(rc);
    // the lag of its rows (trmc_plan_set_lag: the trunk of a cut basin riding behind its owner's sub-basins) is part of how
    // the plan routes: the clone routes the same way (row sets and the cost collection are per plan and start empty)
    if (src->maxlag > 0) {
        pl->lag_of_row = src->lag_of_row;
        pl->maxlag = src->maxlag;
    }
    if (int rc = pl->it_prev.ensure((size_t)pl->nseg_pad)) return bail(rc);
    if (pl->ncuq > 0)
        if (int rc = pl->cuq_head.ensure((size_t)pl->ncuq * 2 * sizeof(int32_t))) return bail(rc);
    *out = pl;
    return 0;
}

// The next window's forcing on its way to the device WHILE another plan's window (or this plan's copy of results) runs:
// the host-to-device copy is queued on the plan's copy stream and nothing is waited for; the next trmc_route_begin orders
// the window's set-up behind it.  The initial state is not touched: it is what trmc_plan_chain_from hands over, or (q0 =
// NULL semantics of trmc_upload_forcing) the state this plan's last window left.
int trmc_stage_forcing(trmc_plan *pl, int nsteps, const void *qlat, int64_t nq)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    // Also WHILE the plan routes a window that has been queued to its end: the staging area is only read by the window's
    // set-up (the transposing pass at its start), so the next window's forcing may land in it behind that -- a sequence that
    // alternates between a plan and its clone stages a day's forcing two days ahead, right after it has queued the plan's
    // current day, and the copy is through long before the plan's next set-up asks for it.  (Then there is no state of
    // "the plan's last window" yet: trmc_plan_chain_from must supply one.)
    const bool busy = pl->run.active;
    if (busy && pl->run.t_done < pl->run.nsteps + (pl->run.short_ts ? pl->maxlag : 0))
        return fail(TRMC_ESTATE, "the window in progress has not been queued to its end (trmc_route_advance)");
    if (busy && (pl->ngage > 0 || pl->nres > 0))
        return fail(TRMC_ESTATE, "a window with nudging tables or reservoirs is in progress: its series are read after trmc_route_end; "
                                 "stage the next forcing then");
    if (nsteps < 1) return fail(TRMC_EINVAL, "nsteps must be >= 1");
    if (nq < 1) return fail(TRMC_EINVAL, "qlat needs at least one column");
    if (pl->nseg > 0 && !qlat) return fail(TRMC_EINVAL, "qlat is NULL");
    if (int rc = use_device(pl)) return rc;
    if (int rc = ensure_copy_stream(pl)) return rc;
    const size_t bytes = (size_t)pl->nseg * nq * pl->esz;
    if (busy && bytes > pl->in_qlat.bytes)
        return fail(TRMC_ESTATE, "the staging area would have to grow while the window in progress may still read it");
    if (int rc = pl->in_qlat.ensure(bytes)) return rc;
    // the initial state unless trmc_plan_chain_from replaces it: what this plan's last window left (gathered now, on the
    // plan's stream, before anything overwrites the planes); a plan that has routed nothing must be chained to
    if (int rc = pl->in_q0.ensure((size_t)pl->nseg * 3 * pl->esz)) return rc;
    // (a second staging before the window is routed -- a corrected forcing -- finds routed_nsteps < 0 but the state the first
    // one gathered still in in_q0: q0_staged)
    pl->state_missing = busy || (pl->routed_nsteps < 0 && !pl->q0_staged);
    if (pl->nseg > 0 && !pl->state_missing && pl->routed_nsteps >= 0)
        if (int rc = final_state_into(pl, pl->in_q0.p)) return rc;
    pl->q0_staged = !pl->state_missing;
    // (a forcing staged earlier and not routed yet is still on its way on the same stream: the new copy lands behind it)
    // (behind the set-up of the window in progress, which reads the staging area)
    if (busy) HIP_TRY(hipStreamWaitEvent(pl->hstream, pl->ev[1], 0));
    if (pl->nseg > 0) HIP_TRY(hipMemcpyAsync(pl->in_qlat.p, qlat, bytes, hipMemcpyHostToDevice, pl->hstream));
    // Sequence mode, level engine: the transpose into plan order right behind the copy, into the forcing buffer the window in
    // progress does not read -- 0.27 ms of a CONUS day that the next window's set-up, which sits in the tile queue between
    // one day's last tile and the next day's first, no longer has to do
    pl->qlat_alt_ready = false;
    if (pl->opt.sequence && !pl->flow && pl->nseg > 0) {
        if (int rc = pl->qlat_alt.ensure((size_t)nq * pl->nseg_pad * pl->esz)) return rc;
        const int32_t n = (int32_t)pl->nseg;
        const dim3 grid((n + 63) / 64, (unsigned)((nq + 31) / 32));
        const int rc = by_precision(pl, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((k_prep_qlat<T>), grid, dim3(kBlock), 0, pl->hstream, (const T *)pl->in_qlat.p,
                               (const int32_t *)pl->sh->row_of_pos.p, (T *)pl->qlat_alt.p, n, pl->nseg_pad, (int32_t)nq);
            return launched();
        });
        if (rc) return rc;
        pl->qlat_alt_ready = true;
    }
    if (int rc = pl->mk_forcing.record(pl->hstream)) return rc;
    pl->qlat_direct = false;
    pl->nq = nq;
    // (a plan with boundary rows: their hydrographs of the staged window arrive in ranges while it runs --
    // trmc_set_boundary_flow_range, the multi-GPU hand-off -- or with trmc_set_boundary_flow_device before it begins)
    pl->have_boundary = pl->sh->topo.nboundary == 0;
    pl->ngage = 0; // nudging tables belong to one window (the launches of a window in progress carry their own copy of the pointers)
    pl->nraw = 0;
    pl->staged_nsteps = nsteps;
    if (!busy) pl->routed_nsteps = -1; // (a window in progress sets it when it ends)
    return 0;
}

int trmc_plan_info(const trmc_plan *pl, int64_t *nseg, int64_t *nseg_routed, int32_t *nlevels, int32_t *precision,
                   int32_t *device)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (nseg) *nseg = pl->nseg;
    if (nseg_routed) *nseg_routed = pl->nrouted;
    if (nlevels) *nlevels = pl->sh->topo.nlevels;
    if (precision) *precision = pl->precision;
    if (device) *device = pl->device;
    return 0;
}

int trmc_plan_lags(const trmc_plan *pl, int32_t *lag_of_row, int32_t *wide_levels, int32_t *cluster_levels)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    const trmc::Topology &t = pl->sh->topo;
    if (t.cl_rows <= 0) return fail(TRMC_EINVAL, "the plan is not in cluster order (trmc_plan_options.cluster_rows)");
    for (int64_t r = 0; lag_of_row && r < pl->nseg; ++r)
        lag_of_row[r] = t.level_of_row[r] < 0 ? -1 : t.lagk_of_pos[(size_t)t.pos_of_row[r]];
    if (wide_levels) *wide_levels = t.cl_from_level;
    if (cluster_levels) *cluster_levels = t.ncl;
    return 0;
}

int trmc_plan_cluster_blocks(const trmc_plan *pl, int32_t *block_of_row, int32_t *block_width, int32_t *cluster_blocks)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    const trmc::Topology &t = pl->sh->topo;
    if (t.cl_rows <= 0) return fail(TRMC_EINVAL, "the plan is not in cluster order (trmc_plan_options.cluster_rows)");
    const int32_t nb = t.ncl > 0 ? (int32_t)t.cblk_ptr.size() - 1 : 0;
    if (block_of_row) {
        for (int64_t r = 0; r < pl->nseg; ++r) block_of_row[r] = -1;
        for (int32_t b = 0; b < nb; ++b)
            for (int32_t p = t.cblk_ptr[(size_t)b]; p < t.cblk_ptr[(size_t)b + 1]; ++p) block_of_row[t.row_of_pos[(size_t)p]] = b;
    }
    if (block_width) *block_width = kCtileBlock;
    if (cluster_blocks) *cluster_blocks = nb;
    return 0;
}

int trmc_plan_levels(const trmc_plan *pl, int32_t *level_of_row, int64_t *plan_pos_of_row)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    for (int64_t r = 0; r < pl->nseg; ++r) {
        if (level_of_row) level_of_row[r] = pl->sh->topo.level_of_row[r];
        if (plan_pos_of_row) plan_pos_of_row[r] = pl->sh->topo.pos_of_row[r];
    }
    return 0;
}

// (q_T, q_T, depth_T) of the last routed window, row order, into device memory `dst` [nseg][3]; queued on the plan stream
static int final_state_into(trmc_plan *pl, void *dst, int32_t nsteps_of_window)
{
    const int32_t n = (int32_t)pl->nseg, T_ = nsteps_of_window >= 0 ? nsteps_of_window : pl->routed_nsteps;
    const size_t plane = (size_t)(T_ + 1) * pl->nseg_pad;
    const int32_t *rop = (const int32_t *)pl->sh->row_of_pos.p;
    int rc;
    if (pl->flow) { // (precision 32 only; the depths in a column of their own)
        hipLaunchKernelGGL((k_final_state<float>), dim3(blocks_for(n)), dim3(kBlock), 0, pl->stream, (const float *)pl->tm.p,
                           (const float *)pl->d_state.p, rop, (float *)dst, n, pl->nseg_pad, T_, 2, 0);
        rc = launched();
    } else {
        rc = by_precision(pl, [&](auto t) {
            using T = decltype(t);
            const T *q = (const T *)pl->tm.p;
            hipLaunchKernelGGL((k_final_state<T>), dim3(blocks_for(n)), dim3(kBlock), 0, pl->stream, q, q + 2 * plane, rop, (T *)dst, n,
                               pl->nseg_pad, T_, 1, T_);
            return launched();
        });
    }
    return rc ? rc : note_gather(pl, nsteps_of_window >= 0);
}

// initial state (or warm start), boundary hydrographs, and the bookkeeping common to every forcing upload
static int stage_state(trmc_plan *pl, int nsteps, int64_t nq, const void *q0, const void *boundary_fvd)
{
    const size_t e = pl->esz;
    if (int rc = pl->in_q0.ensure((size_t)pl->nseg * 3 * e)) return rc;
    if (pl->nseg > 0) {
        if (q0) {
            HIP_TRY(hipMemcpyAsync(pl->in_q0.p, q0, (size_t)pl->nseg * 3 * e, hipMemcpyHostToDevice, pl->stream));
            if (pl->nan_is_zero)
                if (int rc = nan_to_zero(pl, pl->in_q0.p, pl->nseg * 3)) return rc;
        } else if (pl->routed_nsteps >= 0) { // warm start in HBM: (q_T, q_T, depth_T) of the previous window, AbstractNetwork.py:182-190
            if (int rc = final_state_into(pl, pl->in_q0.p)) return rc;
        } // (else: q0_staged -- the state an earlier staging of this window put into in_q0 stands, upload_check)
    }
    if (pl->sh->topo.nboundary > 0 && boundary_fvd) {
        const size_t b = (size_t)pl->sh->topo.nboundary * nsteps * 3 * e;
        if (int rc = pl->in_bfvd.ensure(b)) return rc;
        HIP_TRY(hipMemcpyAsync(pl->in_bfvd.p, boundary_fvd, b, hipMemcpyHostToDevice, pl->stream));
    }
    HIP_TRY(hipStreamSynchronize(pl->stream));
    pl->nq = nq;
    pl->have_boundary = pl->sh->topo.nboundary == 0 || boundary_fvd != nullptr;
    pl->ngage = 0; // nudging tables belong to one window: trmc_set_nudging() after each upload
    pl->nraw = 0;
    pl->staged_nsteps = nsteps;
    pl->routed_nsteps = -1;
    pl->state_missing = false;
    pl->q0_staged = true;
    return 0;
}

static int upload_check(trmc_plan *pl, int nsteps, int64_t nq, const void *q0)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is in progress");
    if (stream_active(pl)) return fail(TRMC_ESTATE, "a stream of windows is in progress (trmc_stream_end it first)");
    if (nsteps < 1) return fail(TRMC_EINVAL, "nsteps must be >= 1");
    if (nq < 1) return fail(TRMC_EINVAL, "qlat needs at least one column");
    if (pl->nseg > 0 && !q0 && pl->routed_nsteps < 0 && !pl->q0_staged)
        return fail(TRMC_ESTATE, "q0 is NULL (continue from the resident state) but nothing has been routed yet");
    if (int rc = use_device(pl)) return rc;
    // a forcing staged with trmc_stage_forcing is (or may still be) on its way into in_qlat on the copy stream: this upload
    // replaces it, and its own copy must not be overtaken by the older one
    return pl->mk_forcing.sync();
}

int trmc_upload_forcing(trmc_plan *pl, int nsteps, const void *qlat, int64_t nq, const void *q0,
                        const void *boundary_fvd)
{
    if (int rc = upload_check(pl, nsteps, nq, q0)) return rc;
    if (pl->nseg > 0 && !qlat) return fail(TRMC_EINVAL, "qlat is NULL");
    // boundary_fvd may be NULL here when trmc_set_boundary_flow_device() supplies the hydrographs later
    const size_t e = pl->esz;
    if (int rc = pl->in_qlat.ensure((size_t)pl->nseg * nq * e)) return rc;
    if (pl->nseg > 0) {
        HIP_TRY(hipMemcpyAsync(pl->in_qlat.p, qlat, (size_t)pl->nseg * nq * e, hipMemcpyHostToDevice, pl->stream));
        if (pl->nan_is_zero)
            if (int rc = nan_to_zero(pl, pl->in_qlat.p, pl->nseg * nq)) return rc;
    }
    pl->qlat_direct = false;
    pl->qlat_alt_ready = false; // (a staged forcing, transposed already, is replaced by this one)
    return stage_state(pl, nsteps, nq, q0, boundary_fvd);
}

// the packing facts of one variable as the ingest kernels take them: pack = (scale_factor, add_offset, _FillValue, missing_value,
// valid_min, valid_max), NaN where the file defines none; NULL: the variable that is not there (never read)
static PackSpec pack_spec(const double *k)
{
    if (!k) return PackSpec{1.0, 0.0, 0, 0, INT32_MIN, INT32_MAX, 0, 0};
    PackSpec s;
    s.scale = k[0];
    s.offset = k[1];
    s.use1 = k[2] == k[2];
    s.use2 = k[3] == k[3];
    s.fill1 = s.use1 ? (int32_t)k[2] : 0;
    s.fill2 = s.use2 ? (int32_t)k[3] : 0;
    s.vmin = k[4] == k[4] ? (int32_t)k[4] : INT32_MIN; // NaN: no lower / upper bound in the file
    s.vmax = k[5] == k[5] ? (int32_t)k[5] : INT32_MAX;
    return s;
}

int trmc_upload_forcing_packed(trmc_plan *pl, int nsteps, int64_t nq, int64_t nfeat, const int32_t *raw_a,
                               const int32_t *raw_b, const double *pack_a, const double *pack_b,
                               const int64_t *feat_of_row, const void *q0, const void *boundary_fvd)
{
    if (int rc = upload_check(pl, nsteps, nq, q0)) return rc;
    if (nfeat < 0 || (pl->nseg > 0 && (!raw_a || !pack_a || !feat_of_row))) return fail(TRMC_EINVAL, "raw_a/pack_a/feat_of_row is NULL");
    if (raw_b && !pack_b) return fail(TRMC_EINVAL, "pack_b is NULL");
    if (nfeat > INT32_MAX) return fail(TRMC_EINVAL, "feature axis too long");
    const PackSpec ka = pack_spec(pack_a), kb = pack_spec(raw_b ? pack_b : nullptr);
    const int64_t n = pl->nseg;
    std::vector<int32_t> feat_of_pos((size_t)(n > 0 ? n : 1), -1);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t f = feat_of_row[pl->sh->topo.row_of_pos[p]];
        if (f >= nfeat) return fail(TRMC_EINVAL, "feat_of_row entry outside the feature axis");
        feat_of_pos[(size_t)p] = f < 0 ? -1 : (int32_t)f;
    }
    const size_t raw_bytes = (size_t)nq * (size_t)nfeat * sizeof(int32_t);
    const size_t pbytes = ((size_t)(n > 0 ? n : 1) * sizeof(int32_t) + 255) / 256 * 256;
    if (int rc = pl->in_qlat.ensure((raw_b ? 2 : 1) * raw_bytes)) return rc; // staging for the raw columns
    if (int rc = pl->scratch.ensure(pbytes)) return rc;
    if (int rc = pl->qlat_tm.ensure((size_t)nq * pl->nseg_pad * pl->esz)) return rc;
    if (n > 0) {
        int32_t *da = (int32_t *)pl->in_qlat.p, *db = raw_b ? da + (size_t)nq * nfeat : nullptr;
        HIP_TRY(hipMemcpyAsync(da, raw_a, raw_bytes, hipMemcpyHostToDevice, pl->stream));
        if (raw_b) HIP_TRY(hipMemcpyAsync(db, raw_b, raw_bytes, hipMemcpyHostToDevice, pl->stream));
        HIP_TRY(hipMemcpyAsync(pl->scratch.p, feat_of_pos.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, pl->stream));
        const int rc = by_precision(pl, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((k_ingest_packed<T>), dim3(blocks_for(n)), dim3(kBlock), 0, pl->stream, da, db, ka, kb,
                               (const int32_t *)pl->scratch.p, (T *)pl->qlat_tm.p, (int32_t)n, pl->nseg_pad, (int32_t)nq, nfeat);
            return launched();
        });
        if (rc) return rc;
    }
    pl->qlat_direct = true;
    pl->qlat_alt_ready = false;
    // (feat_of_pos is pageable host memory: the copy above must have been consumed before it goes out of scope;
    // stage_state ends with a stream synchronisation)
    return stage_state(pl, nsteps, nq, q0, boundary_fvd);
}

int trmc_set_boundary_flow_device(trmc_plan *pl, int nsteps, const void *q_dev)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->staged_nsteps < 0) return fail(TRMC_ESTATE, "trmc_upload_forcing must precede trmc_set_boundary_flow_device");
    if (nsteps != pl->staged_nsteps) return fail(TRMC_EINVAL, "nsteps differs from the staged forcing");
    const int64_t nb = pl->sh->topo.nboundary;
    if (nb == 0) return 0;
    if (!q_dev) return fail(TRMC_EINVAL, "q_dev is NULL");
    if (int rc = use_device(pl)) return rc;
    const size_t e = pl->esz;
    if (int rc = pl->in_bfvd.ensure((size_t)nb * nsteps * 3 * e)) return rc;
    // expand [b][t] -> [b][t][q,0,0] on the device (velocity and depth of a boundary row are never read)
    HIP_TRY(hipMemsetAsync(pl->in_bfvd.p, 0, (size_t)nb * nsteps * 3 * e, pl->stream));
    HIP_TRY(hipMemcpy2DAsync(pl->in_bfvd.p, 3 * e, q_dev, e, e, (size_t)nb * nsteps, hipMemcpyDeviceToDevice, pl->stream));
    HIP_TRY(hipStreamSynchronize(pl->stream));
    pl->have_boundary = true;
    pl->routed_nsteps = -1;
    return 0;
}

int trmc_set_reservoirs(trmc_plan *pl, int64_t nres, const int64_t *res_rows, const void *par, double routing_period)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (nres < 0) return fail(TRMC_EINVAL, "nres < 0");
    if (stream_active(pl)) return fail(TRMC_ESTATE, "a stream of windows is in progress: its reservoirs are set before trmc_stream_begin");
    pl->nres = 0;
    pl->res_da_on = false; // (the tables of trmc_set_reservoir_da belong to the reservoirs they were set for)
    if (nres == 0) return 0;
    if (!res_rows || !par) return fail(TRMC_EINVAL, "res_rows/par is NULL");
    if (int rc = use_device(pl)) return rc;
    std::vector<int32_t> r_of_pos((size_t)pl->nseg_pad, -1);
    for (int64_t i = 0; i < nres; ++i) {
        const int64_t r = res_rows[i];
        if (r < 0 || r >= pl->nseg) return fail(TRMC_EINVAL, "reservoir row out of range");
        if (pl->sh->topo.level_of_row[r] < 0) return fail(TRMC_EINVAL, "reservoir on a boundary row");
        if (r_of_pos[pl->sh->topo.pos_of_row[r]] >= 0) return fail(TRMC_EINVAL, "two reservoirs on one row");
        r_of_pos[pl->sh->topo.pos_of_row[r]] = (int32_t)i;
    }
    if (int rc = upload_i32(pl->res_of_pos, r_of_pos, 1)) return rc;
    const size_t bytes = (size_t)nres * 9 * pl->esz;
    if (int rc = pl->res_par.ensure(bytes)) return rc;
    HIP_TRY(hipMemcpy(pl->res_par.p, par, bytes, hipMemcpyHostToDevice));
    pl->nres = nres;
    pl->res_dt = routing_period;
    pl->res_rows.assign(res_rows, res_rows + nres);
    pl->routed_nsteps = -1;
    return 0;
}

int trmc_download_reservoir_inflow(trmc_plan *pl, void *inflow_out)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (pl->nres == 0) return 0;
    if (!inflow_out) return fail(TRMC_EINVAL, "inflow_out is NULL");
    if (int rc = use_device(pl)) return rc;
    HIP_TRY(hipMemcpy(inflow_out, pl->res_inflow.p, (size_t)pl->nres * pl->routed_nsteps * pl->esz, hipMemcpyDeviceToHost));
    return 0;
}

// the plans that can have reservoir data-assimilation tables at all (trmc_set_reservoir_da; trmc_stream_set_reservoir_da, trmc_stream_begin)
static int reservoir_da_plan_check(const trmc_plan *pl)
{
    if (pl->precision != 32 || pl->opt.tol)
        return fail(TRMC_EINVAL, "reservoir data assimilation needs a precision 32 plan in the exact arithmetic");
    return 0;
}

int trmc_set_reservoir_da(trmc_plan *pl, int64_t nres, const int32_t *kind, const int32_t *table_row,
                          const trmc_reservoir_da_table *usgs, const trmc_reservoir_da_table *usace, const trmc_reservoir_da_table *rfc)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (stream_active(pl)) return fail(TRMC_ESTATE, "a stream of windows is in progress: its reservoir tables arrive with every day (trmc_stream_push_day)");
    pl->res_da_on = false;
    if (nres == 0) return 0;
    if (nres != pl->nres) return fail(TRMC_ESTATE, "trmc_set_reservoirs (same nres) must precede trmc_set_reservoir_da");
    if (!kind || !table_row) return fail(TRMC_EINVAL, "kind/table_row is NULL");
    if (int rc = reservoir_da_plan_check(pl)) return rc;
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is in progress");
    const trmc_reservoir_da_table none{};
    const trmc_reservoir_da_table *tab[3] = {usgs ? usgs : &none, usace ? usace : &none, rfc ? rfc : &none};
    const char *const tname[3] = {"usgs", "usace", "rfc"};
    int64_t off[3], time_off[3] = {0, 0, 0};
    int64_t floats = nres * (int64_t)(sizeof(trmc::ResDaRec) / sizeof(float)); // the float rows begin behind the records
    for (int k = 0; k < 3; ++k) {
        const trmc_reservoir_da_table &t = *tab[k];
        if (t.n < 0 || t.ncol < 0) return fail(TRMC_EINVAL, std::string(tname[k]) + " table: n/ncol < 0");
        if (t.n > 0 && (t.ncol < 1 || t.ncol > INT32_MAX)) return fail(TRMC_EINVAL, std::string(tname[k]) + " table: rows without columns");
        if (t.n > 0 && (!t.obs || !t.state || (k < 2 && !t.time) || (k == 2 && !t.ipar)))
            return fail(TRMC_EINVAL, std::string(tname[k]) + " table: a pointer is NULL");
        off[k] = floats;
        floats += t.n * t.ncol;
        if (k < 2) {
            time_off[k] = floats;
            floats += t.n > 0 ? t.ncol : 0;
        }
    }
    std::vector<float> host((size_t)floats, 0.0f);
    trmc::ResDaRec *rec = reinterpret_cast<trmc::ResDaRec *>(host.data());
    std::vector<uint8_t> used[3];
    for (int k = 0; k < 3; ++k) {
        used[k].assign((size_t)tab[k]->n, 0);
        if (tab[k]->n > 0) std::memcpy(host.data() + off[k], tab[k]->obs, (size_t)(tab[k]->n * tab[k]->ncol) * sizeof(float));
        if (k < 2 && tab[k]->n > 0) std::memcpy(host.data() + time_off[k], tab[k]->time, (size_t)tab[k]->ncol * sizeof(float));
    }
    bool any = false;
    for (int64_t i = 0; i < nres; ++i) {
        trmc::ResDaRec r{};
        r.kind = kind[i];
        if (r.kind == 0) {
            rec[i] = r;
            continue;
        }
        if (r.kind < 2 || r.kind > 5) return fail(TRMC_EINVAL, "reservoir " + std::to_string(i) + ": kind must be 0 or 2..5");
        const int k = r.kind == 2 ? 0 : (r.kind == 3 ? 1 : 2);
        const trmc_reservoir_da_table &t = *tab[k];
        const int64_t j = table_row[i];
        if (j < 0 || j >= t.n)
            return fail(TRMC_EINVAL, "reservoir " + std::to_string(i) + ": no row " + std::to_string(j) + " in the " + tname[k] + " table");
        if (used[k][(size_t)j]) return fail(TRMC_EINVAL, std::string("two reservoirs on one row of the ") + tname[k] + " table");
        used[k][(size_t)j] = 1;
        r.ncol = (int32_t)t.ncol;
        r.obs_off = off[k] + j * t.ncol;
        r.time_off = time_off[k];
        if (k < 2) {
            const float *s = t.state + 4 * j;
            r.st.update_time = s[0];
            r.st.prev_persisted = s[1];
            r.st.persistence_index = s[2];
            r.st.persistence_update_time = s[3];
        } else {
            const int32_t *p = t.ipar + 5 * j;
            r.st.update_time = t.state[j];
            r.st.timeseries_idx = p[0];
            r.total_counts = p[1];
            r.use_forecast = p[2];
            r.da_timestep = p[3];
            r.persist_days = p[4];
            if (r.st.timeseries_idx < 0 || r.st.timeseries_idx >= r.ncol)
                return fail(TRMC_EINVAL, "rfc table row " + std::to_string(j) + ": timeseries_idx outside the series");
        }
        rec[i] = r;
        any = true;
    }
    if (!any) return 0;
    if (int rc = use_device(pl)) return rc;
    if (int rc = pl->res_da.ensure(host.size() * sizeof(float))) return rc;
    HIP_TRY(hipMemcpy(pl->res_da.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    pl->res_da_on = true;
    pl->res_da_kind.assign(kind, kind + nres);
    pl->res_da_trow.assign(table_row, table_row + nres);
    for (int k = 0; k < 3; ++k) {
        pl->res_da_n[k] = tab[k]->n;
        pl->res_da_ncol[k] = tab[k]->n > 0 ? tab[k]->ncol : 0;
    }
    pl->routed_nsteps = -1;
    return 0;
}

int trmc_download_reservoir_da(trmc_plan *pl, float *state_out, int32_t *timeseries_idx_out)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (pl->nres == 0 || !pl->res_da_on) return fail(TRMC_ESTATE, "the routed window had no reservoir data-assimilation tables");
    if (!state_out || !timeseries_idx_out) return fail(TRMC_EINVAL, "state_out/timeseries_idx_out is NULL");
    if (int rc = use_device(pl)) return rc;
    std::vector<trmc::ResDaRec> rec((size_t)pl->nres);
    HIP_TRY(hipMemcpy(rec.data(), pl->res_da.p, rec.size() * sizeof(trmc::ResDaRec), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < rec.size(); ++i) {
        state_out[4 * i + 0] = rec[i].st.update_time;
        state_out[4 * i + 1] = rec[i].st.prev_persisted;
        state_out[4 * i + 2] = rec[i].st.persistence_index;
        state_out[4 * i + 3] = rec[i].st.persistence_update_time;
        timeseries_idx_out[i] = rec[i].st.timeseries_idx;
    }
    return 0;
}

int trmc_reservoir_da_steps(int device, int kind, int64_t n, int64_t ncol, const float *obs, const float *time, const float *fin,
                            const int32_t *iin, float *fout, int32_t *iout)
{
    if (kind != TRMC_RESERVOIR_DA_HYBRID && kind != TRMC_RESERVOIR_DA_RFC) return fail(TRMC_EINVAL, "bad kind");
    if (n < 0) return fail(TRMC_EINVAL, "n < 0");
    if (n == 0) return 0;
    if (ncol < 1 || ncol > INT32_MAX) return fail(TRMC_EINVAL, "ncol must be >= 1");
    const bool hybrid = kind == TRMC_RESERVOIR_DA_HYBRID;
    if (!obs || !fin || !fout || (hybrid && !time) || (!hybrid && (!iin || !iout))) return fail(TRMC_EINVAL, "an array pointer is NULL");
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    return reservoir_da_steps(hybrid, n, (int32_t)ncol, obs, time, fin, iin, fout, iout);
}

int trmc_set_nudging(trmc_plan *pl, int nsteps, int64_t ngage, const int64_t *gage_rows, const uint8_t *mode,
                     const void *a, const void *w)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->staged_nsteps < 0) return fail(TRMC_ESTATE, "trmc_upload_forcing must precede trmc_set_nudging");
    if (ngage < 0 || nsteps < 1) return fail(TRMC_EINVAL, "bad ngage/nsteps");
    pl->ngage = 0;
    if (ngage == 0) return 0;
    if (!gage_rows || !mode || !a || !w) return fail(TRMC_EINVAL, "nudging table pointer is NULL");
    if (int rc = use_device(pl)) return rc;
    std::vector<int32_t> g_of_pos((size_t)pl->nseg_pad, -1);
    std::vector<int32_t> res_of_pos;
    if (pl->nres > 0) {
        res_of_pos.resize((size_t)pl->nseg_pad);
        HIP_TRY(hipMemcpy(res_of_pos.data(), pl->res_of_pos.p, (size_t)pl->nseg_pad * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    for (int64_t g = 0; g < ngage; ++g) {
        const int64_t r = gage_rows[g];
        if (r < 0 || r >= pl->nseg) return fail(TRMC_EINVAL, "gage row out of range");
        if (pl->sh->topo.level_of_row[r] < 0) return fail(TRMC_EINVAL, "gage on a boundary row");
        // (the reservoir branch of the kernels ends a row's step before the nudging hook)
        if (!res_of_pos.empty() && res_of_pos[(size_t)pl->sh->topo.pos_of_row[r]] >= 0)
            return fail(TRMC_EINVAL, "a gage on a reservoir row is not supported (row " + std::to_string(r) + ")");
        g_of_pos[pl->sh->topo.pos_of_row[r]] = (int32_t)g; // one gage per segment: the last listed wins, as reach_has_gage does
    }
    const size_t n = (size_t)ngage * nsteps, e = pl->esz;
    if (int rc = upload_i32(pl->gage_of_pos, g_of_pos, 1)) return rc;
    if (int rc = pl->da_mode.ensure(n)) return rc;
    if (int rc = pl->da_a.ensure(n * e)) return rc;
    if (int rc = pl->da_w.ensure(n * e)) return rc;
    if (int rc = pl->da_nudge.ensure(n * e)) return rc;
    HIP_TRY(hipMemcpy(pl->da_mode.p, mode, n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pl->da_a.p, a, n * e, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pl->da_w.p, w, n * e, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(pl->da_nudge.p, 0, n * e, pl->stream)); // (on the plan's stream: ordered before its kernels)
    pl->ngage = ngage;
    pl->nraw = 0;
    pl->da_nsteps = nsteps;
    pl->routed_nsteps = -1;
    return 0;
}

int trmc_set_nudging_successors(trmc_plan *pl, int64_t ngage, const int64_t *successor_rows)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->ngage == 0 || ngage != pl->ngage) return fail(TRMC_ESTATE, "trmc_set_nudging (same ngage) must precede trmc_set_nudging_successors");
    if (!successor_rows) return fail(TRMC_EINVAL, "successor_rows is NULL");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is in progress");
    pl->nraw = 0;
    int64_t n = 0;
    for (int64_t g = 0; g < ngage; ++g) n += successor_rows[g] >= 0;
    if (n == 0) return 0;
    if (pl->flow)
        return fail(TRMC_ESTATE, "gages inside a reach without assume_short_ts need the level engine (create the plan with "
                                       "TRMC_ENGINE_LEVELS)");
    if (int rc = use_device(pl)) return rc;
    std::vector<int32_t> g_of_pos((size_t)pl->nseg_pad, -1), raw((size_t)pl->nseg_pad, -1);
    HIP_TRY(hipMemcpy(g_of_pos.data(), pl->gage_of_pos.p, (size_t)pl->nseg_pad * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < ngage; ++g) {
        const int64_t r = successor_rows[g];
        if (r < 0) continue;
        if (r >= pl->nseg || pl->sh->topo.level_of_row[r] < 0) return fail(TRMC_EINVAL, "successor row out of range or a boundary row");
        const int32_t p = pl->sh->topo.pos_of_row[r];
        // the segment below a gage inside a reach has exactly one upstream row: that gage's segment
        if (pl->sh->topo.up_ptr[p + 1] - pl->sh->topo.up_ptr[p] != 1 || g_of_pos[(size_t)pl->sh->topo.up_idx[pl->sh->topo.up_ptr[p]]] != (int32_t)g)
            return fail(TRMC_EINVAL, "successor row " + std::to_string(r) + " is not the segment directly below gage " + std::to_string(g));
        raw[(size_t)p] = (int32_t)g;
    }
    if (int rc = upload_i32(pl->raw_of_pos, raw, 1)) return rc;
    if (int rc = pl->da_raw.ensure((size_t)ngage * pl->da_nsteps * pl->esz)) return rc;
    HIP_TRY(hipMemsetAsync(pl->da_raw.p, 0, (size_t)ngage * pl->da_nsteps * pl->esz, pl->stream));
    pl->nraw = n;
    return 0;
}

int trmc_download_nudge(trmc_plan *pl, void *nudge_out)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (pl->ngage == 0) return 0;
    if (!nudge_out) return fail(TRMC_EINVAL, "nudge_out is NULL");
    if (int rc = use_device(pl)) return rc;
    HIP_TRY(hipMemcpy(nudge_out, pl->da_nudge.p, (size_t)pl->ngage * pl->da_nsteps * pl->esz, hipMemcpyDeviceToHost));
    return 0;
}

static int route_check(trmc_plan *pl, int nsteps, int qts_subdivisions, bool boundary_later)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->staged_nsteps < 0) return fail(TRMC_ESTATE, "trmc_upload_forcing must precede routing");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is already in progress (trmc_route_end it first)");
    if (stream_active(pl)) return fail(TRMC_ESTATE, "a stream of windows is in progress (trmc_stream_end it first)");
    if (nsteps < 1) return fail(TRMC_EINVAL, "nsteps must be >= 1");
    if (qts_subdivisions < 1) return fail(TRMC_EINVAL, "qts_subdivisions must be >= 1");
    if (pl->sh->topo.nboundary > 0 && nsteps != pl->staged_nsteps)
        return fail(TRMC_EINVAL, "nsteps differs from the staged boundary hydrographs");
    if (!pl->have_boundary && !boundary_later)
        return fail(TRMC_ESTATE, "plan has boundary rows but no boundary hydrographs were supplied");
    if (pl->ngage > 0 && pl->da_nsteps != nsteps) return fail(TRMC_EINVAL, "nudging tables were set for a different nsteps");
    if (pl->state_missing && !pl->chain_staged)
        return fail(TRMC_ESTATE, "the forcing was staged on a plan that has routed nothing (or whose window has not ended yet): "
                                 "trmc_plan_chain_from must hand it a state, or trmc_route_end the window first");
    // the reference's precondition, mc_reach.pyx:246-247
    if ((int64_t)(nsteps - 1) / qts_subdivisions >= pl->nq)
        return fail(TRMC_EINVAL, "Number of columns (timesteps) in Qlat is incorrect: need "
                                     + std::to_string((nsteps - 1) / qts_subdivisions + 1) + ", got " + std::to_string(pl->nq));
    return use_device(pl);
}

static int lag_check(trmc_plan *pl, int assume_short_ts)
{
    if ((pl->sh->topo.tail_from_level > 0 || pl->sh->topo.ncl > 0) && !assume_short_ts)
        return fail(TRMC_EINVAL, "this plan was created for assume_short_ts (TRMC_PLAN_SHORT_TS on the level engine: its deeper rows are "
                                 "ordered in clusters or by cost, not by level); create a plan for the general mode");
    if (pl->maxlag > 0 && !assume_short_ts)
        return fail(TRMC_EINVAL, "a plan with lagged rows (trmc_plan_set_lag) routes with assume_short_ts only");
    return 0;
}

// A forcing staged WHILE the plan's own window was in flight (trmc_stage_forcing on a busy plan) had no state to take then; if
// that window has ended since and nobody has handed a state over (trmc_plan_chain_from), the window continues from it: the
// gather of (q_T, q_T, depth_T) that an idle staging does at once is done here, at the head of the new window's queue.
static int settle_deferred_state(trmc_plan *pl)
{
    if (!pl || !pl->state_missing || pl->chain_staged || pl->run.active || pl->routed_nsteps < 0) return 0;
    if (int rc = use_device(pl)) return rc;
    if (pl->nseg > 0)
        if (int rc = final_state_into(pl, pl->in_q0.p)) return rc;
    pl->state_missing = false;
    pl->q0_staged = true;
    return 0;
}

int trmc_route_device(trmc_plan *pl, int nsteps, int qts_subdivisions, int assume_short_ts)
{
    if (int rc = settle_deferred_state(pl)) return rc;
    if (int rc = route_check(pl, nsteps, qts_subdivisions, false)) return rc;
    if (int rc = lag_check(pl, assume_short_ts)) return rc;
    const int t_last = nsteps + (assume_short_ts ? pl->maxlag : 0);
    int rc;
    if (pl->flow) {
        rc = flow_route_begin(pl, nsteps, qts_subdivisions, assume_short_ts);
        if (!rc) rc = flow_route_advance(pl, t_last);
        if (!rc) rc = flow_route_end(pl);
    } else {
        rc = by_precision(pl, [&](auto t) {
            using T = decltype(t);
            int rc = route_begin_t<T>(pl, nsteps, qts_subdivisions, assume_short_ts);
            if (!rc) rc = route_advance_t<T>(pl, t_last);
            return rc ? rc : route_end_t<T>(pl);
        });
    }
    if (rc) pl->run.active = false;
    return rc;
}

int trmc_route_begin(trmc_plan *pl, int nsteps, int qts_subdivisions, int assume_short_ts)
{
    if (int rc = settle_deferred_state(pl)) return rc;
    if (int rc = route_check(pl, nsteps, qts_subdivisions, true)) return rc;
    if (int rc = lag_check(pl, assume_short_ts)) return rc;
    const int rc = pl->flow ? flow_route_begin(pl, nsteps, qts_subdivisions, assume_short_ts)
                         : by_precision(pl, [&](auto t) { return route_begin_t<decltype(t)>(pl, nsteps, qts_subdivisions, assume_short_ts); });
    if (rc) pl->run.active = false;
    return rc;
}

int trmc_route_advance(trmc_plan *pl, int t_end)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (!pl->run.active) return fail(TRMC_ESTATE, "trmc_route_begin must precede trmc_route_advance");
    const int32_t lagmax = pl->run.short_ts ? pl->maxlag : 0;
    if (t_end < pl->run.t_done || t_end > pl->run.nsteps + lagmax)
        return fail(TRMC_EINVAL, "t_end outside [launches done, nsteps + lag]");
    // boundary rows feed the lagged rows when the plan has a lag (trmc_plan_set_lag), all rows otherwise
    const int32_t need = t_end - lagmax < pl->run.nsteps ? t_end - lagmax : pl->run.nsteps;
    if (need > pl->run.boundary_through)
        return fail(TRMC_ESTATE, "boundary hydrographs are staged through step " + std::to_string(pl->run.boundary_through)
                                     + " only (trmc_set_boundary_flow_range)");
    if (t_end == pl->run.t_done) return 0;
    if (int rc = use_device(pl)) return rc;
    if (pl->flow) return flow_route_advance(pl, t_end);
    return by_precision(pl, [&](auto t) { return route_advance_t<decltype(t)>(pl, t_end); });
}

int trmc_route_end(trmc_plan *pl)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (!pl->run.active) return fail(TRMC_ESTATE, "no routing window in progress");
    if (pl->run.t_done != pl->run.nsteps + (pl->run.short_ts ? pl->maxlag : 0)) {
        // abandon the window: drain the queue so the plan can be reused
        (void)hipStreamSynchronize(pl->stream);
        (void)hipStreamSynchronize(pl->stream2);
        if (pl->fstream) (void)hipStreamSynchronize(pl->fstream);
        pl->run.active = false;
        return fail(TRMC_ESTATE, "trmc_route_end before every timestep was queued; window abandoned");
    }
    if (int rc = use_device(pl)) return rc;
    const int rc = pl->flow ? flow_route_end(pl) : by_precision(pl, [&](auto t) { return route_end_t<decltype(t)>(pl); });
    if (rc) pl->run.active = false;
    return rc;
}

int trmc_plan_stream(trmc_plan *pl, void **stream_out)
{
    if (!pl || !stream_out) return fail(TRMC_EINVAL, "plan/stream_out is NULL");
    // inside a window of the dataflow engine whose launches alternate between two compute streams: the stream the NEXT
    // trmc_route_advance uses (afterwards: the one it used, on which trmc_gather_flow_range is queued as well)
    *stream_out = (void *)((pl->flow && pl->run.active && flow_overlap(pl)) ? flow_stream(pl, pl->flow_next) : pl->stream);
    return 0;
}

int trmc_plan_set_lag(trmc_plan *pl, const int32_t *lag_of_row)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is in progress");
    if (!pl->rowsets.empty()) return fail(TRMC_ESTATE, "set the lag before registering row sets");
    // (a clone for its whole life; an original while anybody else holds the shared block, that is while a clone of it lives)
    if (pl->is_clone || pl->sh.use_count() > 1) return fail(TRMC_ESTATE, "set the lag before cloning the plan (a clone shares the lag table)");
    pl->maxlag = 0;
    pl->lag_of_row.clear();
    pl->wide_safe_pos = -1;
    if (!lag_of_row) return 0;
    int32_t mx = 0;
    for (int64_t r = 0; r < pl->nseg; ++r) {
        if (lag_of_row[r] < 0) return fail(TRMC_EINVAL, "negative lag");
        mx = std::max(mx, lag_of_row[r]);
    }
    if (mx == 0) return 0;
    // two classes only: in step, or `mx` launches behind; an upstream neighbour is never behind its consumer
    std::vector<int32_t> by_pos((size_t)pl->nseg_pad, 0);
    for (int64_t r = 0; r < pl->nseg; ++r) {
        if (lag_of_row[r] != 0 && lag_of_row[r] != mx) return fail(TRMC_EINVAL, "lag must be 0 or one common value");
        by_pos[(size_t)pl->sh->topo.pos_of_row[r]] = lag_of_row[r];
    }
    for (int64_t p = pl->sh->topo.nboundary; p < pl->nseg; ++p)
        for (int32_t k = pl->sh->topo.up_ptr[p]; k < pl->sh->topo.up_ptr[p + 1]; ++k) {
            const int32_t u = pl->sh->topo.up_idx[k];
            if (u >= pl->sh->topo.nboundary && by_pos[(size_t)u] > by_pos[(size_t)p])
                return fail(TRMC_EINVAL, "a lagged row feeds a row that is not lagged");
            if (u < pl->sh->topo.nboundary && by_pos[(size_t)p] != mx)
                return fail(TRMC_EINVAL, "with a lag, boundary rows may only feed lagged rows");
        }
    if (int rc = use_device(pl)) return rc;
    if (int rc = pl->sh->lag.ensure((size_t)pl->nseg_pad * sizeof(int32_t))) return rc;
    HIP_TRY(hipMemcpy(pl->sh->lag.p, by_pos.data(), (size_t)pl->nseg_pad * sizeof(int32_t), hipMemcpyHostToDevice));
    pl->lag_of_row.assign(lag_of_row, lag_of_row + pl->nseg);
    pl->maxlag = mx;
    return 0;
}

int trmc_rowset_create(trmc_plan *pl, const int64_t *rows, int64_t nrows, int32_t *id_out)
{
    if (!pl || !id_out) return fail(TRMC_EINVAL, "plan/id_out is NULL");
    if (nrows < 0 || (nrows > 0 && !rows)) return fail(TRMC_EINVAL, "rows is NULL");
    if (int rc = use_device(pl)) return rc;
    std::vector<int32_t> pos((size_t)nrows);
    for (int64_t i = 0; i < nrows; ++i) {
        if (rows[i] < 0 || rows[i] >= pl->nseg) return fail(TRMC_EINVAL, "row out of range");
        pos[i] = pl->sh->topo.pos_of_row[rows[i]];
    }
    DevBuf b;
    if (int rc = b.ensure((size_t)(nrows > 0 ? nrows : 1) * sizeof(int32_t))) return rc;
    if (nrows > 0) HIP_TRY(hipMemcpy(b.p, pos.data(), (size_t)nrows * sizeof(int32_t), hipMemcpyHostToDevice));
    int32_t rs_lag = 0; // a set with lagged rows is complete `maxlag` launches later
    if (pl->maxlag > 0)
        for (int64_t i = 0; i < nrows; ++i) rs_lag = std::max(rs_lag, pl->lag_of_row[(size_t)rows[i]]);
    pl->rowsets.push_back(std::move(b));
    pl->rowset_n.push_back(nrows);
    pl->rowset_lag.push_back(rs_lag);
    int32_t lk = 0;
    if (!pl->sh->topo.lagk_of_pos.empty())
        for (int64_t i = 0; i < nrows; ++i) lk = std::max(lk, pl->sh->topo.lagk_of_pos[(size_t)pos[i]]);
    pl->rowset_lagk.push_back(lk);
    *id_out = (int32_t)pl->rowsets.size() - 1;
    return 0;
}

int trmc_gather_flow_range(trmc_plan *pl, int32_t rowset, int t_begin, int t_end, void *dst_dev, int64_t dst_stride)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (rowset < 0 || rowset >= (int32_t)pl->rowsets.size()) return fail(TRMC_EINVAL, "unknown row set");
    const int32_t through = pl->run.active ? std::min(pl->run.nsteps, pl->run.t_done - (pl->run.short_ts ? pl->rowset_lag[rowset] : 0))
                                           : pl->routed_nsteps;
    if (t_begin < 0 || t_end < t_begin || t_end > through)
        return fail(TRMC_ESTATE, "steps (t_begin, t_end] are not all routed yet");
    const int64_t nrows = pl->rowset_n[rowset];
    if (nrows == 0 || t_end == t_begin) return 0;
    if (!dst_dev || dst_stride < t_end - t_begin) return fail(TRMC_EINVAL, "dst_dev is NULL or dst_stride too small");
    if (int rc = use_device(pl)) return rc;
    const int64_t work = nrows * (t_end - t_begin);
    hipStream_t gst = pl->stream;
    if (pl->flow && pl->run.active && flow_overlap(pl) && pl->run.launches > 0) {
        // on the stream of the last launch, and behind the last launch of the other one (which holds the steps before)
        gst = flow_stream(pl, pl->flow_last);
        if (pl->run.launches > 1) HIP_TRY(hipStreamWaitEvent(gst, pl->ev_chunk[1 - pl->flow_last], 0));
    }
    const int rc = by_precision(pl, [&](auto t) { // (precision 64 is the level engine's: gst is the plan's stream, the planes hold numbers)
        using T = decltype(t);
        hipLaunchKernelGGL((k_gather_range<T>), dim3(blocks_for(work)), dim3(kBlock), 0, gst, (const T *)pl->tm.p,
                           (const int32_t *)pl->rowsets[rowset].p, (T *)dst_dev, nrows, pl->nseg_pad, t_begin, t_end, dst_stride,
                           pl->flow ? 2 : 1);
        return launched();
    });
    if (rc) return rc;
    return gst == pl->stream ? note_gather(pl) : 0;
}

int trmc_set_boundary_flow_range(trmc_plan *pl, int t_begin, int t_end, const void *q_dev, int64_t src_stride,
                                 void *stream)
{
    return trmc_set_boundary_flow_range_indexed(pl, t_begin, t_end, q_dev, src_stride, nullptr, stream);
}

int trmc_set_boundary_flow_range_indexed(trmc_plan *pl, int t_begin, int t_end, const void *q_dev, int64_t src_stride,
                                         const int64_t *src_index_dev, void *stream)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (!pl->run.active) return fail(TRMC_ESTATE, "trmc_route_begin must precede trmc_set_boundary_flow_range");
    RouteRun &r = pl->run;
    if (t_begin != r.boundary_through || t_end < t_begin || t_end > r.nsteps)
        return fail(TRMC_EINVAL, "ranges must continue where the staged boundary hydrographs end (step "
                                     + std::to_string(r.boundary_through) + ")");
    const int64_t nb = pl->sh->topo.nboundary;
    if (nb == 0 || t_end == t_begin) {
        r.boundary_through = t_end;
        return 0;
    }
    if (!q_dev || src_stride < t_end - t_begin) return fail(TRMC_EINVAL, "q_dev is NULL or src_stride too small");
    if (int rc = use_device(pl)) return rc;
    const size_t plane = (size_t)(r.nsteps + 1) * pl->nseg_pad;
    const int64_t work = nb * (t_end - t_begin);
    hipStream_t st = stream ? (hipStream_t)stream : pl->stream;
    if (!stream && pl->flow && flow_overlap(pl)) {
        // no stream given: before the next launch, and behind whatever was queued after the last one (a gather that
        // produced q_dev, typically)
        st = flow_stream(pl, pl->flow_next);
        if (r.launches > 0 && pl->flow_next != pl->flow_last) {
            HIP_TRY(hipEventRecord(pl->ev_ctl, flow_stream(pl, pl->flow_last)));
            HIP_TRY(hipStreamWaitEvent(st, pl->ev_ctl, 0));
        }
    }
    int rc;
    if (pl->flow) {
        hipLaunchKernelGGL(k_flow_boundary, dim3(blocks_for(work)), dim3(kBlock), 0, st, (const float *)q_dev,
                           (unsigned long long *)pl->tm.p, (float *)pl->out.p, (const int32_t *)pl->sh->row_of_pos.p, (int32_t)nb,
                           r.nsteps, pl->nseg_pad, t_begin, t_end, src_stride, 1, 1, pl->tag_base, src_index_dev);
        rc = launched();
    } else {
        rc = by_precision(pl, [&](auto t) {
            using T = decltype(t);
            T *q = (T *)pl->tm.p;
            hipLaunchKernelGGL((k_fill_boundary_range<T>), dim3(blocks_for(work)), dim3(kBlock), 0, st, (const T *)q_dev, q, q + plane,
                               q + 2 * plane, (int32_t)nb, pl->nseg_pad, t_begin, t_end, src_stride, src_index_dev);
            return launched();
        });
    }
    if (rc) return rc;
    r.boundary_through = t_end;
    return 0;
}

int trmc_download_fvd(trmc_plan *pl, void *fvd_out)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (pl->nseg == 0) return 0;
    if (!fvd_out) return fail(TRMC_EINVAL, "fvd_out is NULL");
    if (int rc = use_device(pl)) return rc;
    HIP_TRY(hipMemcpy(fvd_out, pl->out.p, (size_t)pl->nseg * pl->routed_nsteps * 3 * pl->esz, hipMemcpyDeviceToHost));
    return 0;
}

// the common end of the two strided downloads: `nkeep` steps of `nrows` rows (the set's, or every row: rowset < 0), decimated into
// the plan's scratch block for gathers of its result and copied to the host
static int download_decimated(trmc_plan *pl, int stride, int32_t nkeep, int32_t rowset, int64_t nrows, void *fvd_out)
{
    if (!fvd_out) return fail(TRMC_EINVAL, "fvd_out is NULL");
    if (int rc = use_device(pl)) return rc;
    const size_t bytes = (size_t)nrows * nkeep * 3 * pl->esz;
    if (int rc = pl->gathered.ensure(bytes)) return rc;
    pl->gathered_bytes = 0;
    if (int rc = decimate_out(pl, pl->gathered.p, pl->routed_nsteps, stride, nkeep, rowset)) return rc;
    HIP_TRY(hipMemcpyAsync(fvd_out, pl->gathered.p, bytes, hipMemcpyDeviceToHost, pl->stream));
    HIP_TRY(hipStreamSynchronize(pl->stream));
    return 0;
}

int trmc_download_fvd_strided(trmc_plan *pl, int stride, void *fvd_out)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (stride < 1) return fail(TRMC_EINVAL, "stride must be >= 1");
    if (stride == 1) return trmc_download_fvd(pl, fvd_out);
    const int32_t nkeep = pl->routed_nsteps / stride;
    if (pl->nseg == 0 || nkeep == 0) return 0;
    return download_decimated(pl, stride, nkeep, -1, pl->nseg, fvd_out);
}

int trmc_download_fvd_rowset(trmc_plan *pl, int stride, int32_t rowset, void *fvd_out)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (stride < 1) return fail(TRMC_EINVAL, "stride must be >= 1");
    if (rowset < 0 || rowset >= (int32_t)pl->rowsets.size()) return fail(TRMC_EINVAL, "unknown row set");
    const int64_t nrows = pl->rowset_n[(size_t)rowset];
    const int32_t nkeep = pl->routed_nsteps / stride;
    if (nrows == 0 || nkeep == 0) return 0;
    return download_decimated(pl, stride, nkeep, rowset, nrows, fvd_out);
}

// ---- the per-row products of a FINISHED window: trmc_window_summary, _courant, _courant_summary, _exceedance

// (rows, steps) of a product kernel's tile
static int window_tile(int precision, int32_t *rows, int32_t *steps, int32_t tile_rows, int32_t steps32, int32_t steps64)
{
    if (precision != 32 && precision != 64) return fail(TRMC_EINVAL, "precision must be 32 or 64");
    if (rows) *rows = tile_rows;
    if (steps) *steps = precision == 32 ? steps32 : steps64;
    return 0;
}

// device time of a product's last kernel (`none`: the refusal while none has been timed)
static int window_kernel_ms(const trmc_plan *pl, KernelTimer trmc_plan::*timer, double *ms_out, const char *none)
{
    if (!pl || !ms_out) return fail(TRMC_EINVAL, "plan/ms_out is NULL");
    if ((pl->*timer).ms < 0) return fail(TRMC_ESTATE, none);
    *ms_out = (pl->*timer).ms;
    return 0;
}

// "The last finished window's result is there."  The products read `out` (the Courant metrics its forcing and initial state too),
// which windows alone assemble and which is whole only once the window has ended: a stream of days leaves its own products and,
// without full_output, assembles no result at all; it recycles the buffers day by day, and trmc_stream_begin forgets the last
// window.  `formed`: the product, as the stream's refusal names it; `stream_own`: what a stream has in its place, if anything.
// The row set is checked by the caller, BEHIND the product's own refusals: the order a caller sees them in is part of the ABI.
static int window_result_check(const trmc_plan *pl, const char *formed, const char *stream_own = "")
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (stream_active(pl))
        return fail(TRMC_ESTATE, std::string("a stream of windows is in progress: ") + formed
                                     + " from the result the plan assembles for a window, which a stream does not fill" + stream_own);
    if (pl->run.active)
        return fail(TRMC_ESTATE, "a routing window is in progress: its result is not assembled before trmc_route_end");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    return 0;
}

int trmc_window_summary_tile(int precision, int32_t *rows, int32_t *steps)
{
    return window_tile(precision, rows, steps, kRecRows, kRecSteps<float>, kRecSteps<double>);
}

int trmc_window_summary(trmc_plan *pl, int32_t rowset, void *peak_flow, int32_t *peak_step, void *mean_flow, void *peak_depth,
                        int32_t *peak_depth_step, void *peak_velocity, int32_t *peak_velocity_step)
{
    if (int rc = window_result_check(pl, "a window's summary is formed", " (trmc_stream_set_summary is the stream's own)")) return rc;
    if (!peak_flow && !peak_step && !mean_flow && !peak_depth && !peak_depth_step && !peak_velocity && !peak_velocity_step)
        return fail(TRMC_EINVAL, "every destination is NULL: nothing to summarise");
    if ((peak_step && !peak_flow) || (peak_depth_step && !peak_depth) || (peak_velocity_step && !peak_velocity))
        return fail(TRMC_EINVAL, "the step of a peak comes with the peak: its value destination is NULL");
    if (rowset < -1 || rowset >= (int32_t)pl->rowsets.size()) return fail(TRMC_EINVAL, "unknown row set");
    const int64_t nrows = rowset < 0 ? pl->nseg : pl->rowset_n[(size_t)rowset];
    if (pl->nseg == 0 || nrows == 0) return 0;
    const int32_t nsteps = pl->routed_nsteps;
    if (nsteps < 1) return fail(TRMC_ESTATE, "the last window had no timesteps");
    if (int rc = use_device(pl)) return rc;
    WindowColumns cols; // seven, [nrows] each
    if (int rc = cols.lay(pl, nrows, {{peak_flow, pl->esz}, {peak_step, 4}, {mean_flow, pl->esz}, {peak_depth, pl->esz}, {peak_depth_step, 4},
                                      {peak_velocity, pl->esz}, {peak_velocity_step, 4}}))
        return rc;
    const int32_t *rp = rowset < 0 ? nullptr : (const int32_t *)pl->rowsets[(size_t)rowset].p;
    if (int rc = pl->t_wsum.begin(pl->stream)) return rc;
    const int rc = by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        const WsumOut<T> o{cols.dev<T>(0), cols.dev<int32_t>(1), cols.dev<T>(2), cols.dev<T>(3), cols.dev<int32_t>(4), cols.dev<T>(5),
                           cols.dev<int32_t>(6)};
        const dim3 grid((unsigned)((nrows + kRecRows - 1) / kRecRows)), block(kRecRows);
        // (16-byte loads where every row's record starts on a 16-byte boundary: k_window_summary's head)
        if (nsteps % (16 / (int)sizeof(T)) == 0)
            hipLaunchKernelGGL((k_window_summary<T, true>), grid, block, 0, pl->stream, (const T *)pl->out.p, rp, (const int32_t *)pl->sh->row_of_pos.p,
                               o, nrows, nsteps);
        else
            hipLaunchKernelGGL((k_window_summary<T, false>), grid, block, 0, pl->stream, (const T *)pl->out.p, rp, (const int32_t *)pl->sh->row_of_pos.p,
                               o, nrows, nsteps);
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    return window_product_finish(pl, pl->t_wsum, cols);
}

int trmc_window_summary_kernel_ms(const trmc_plan *pl, double *ms_out)
{
    return window_kernel_ms(pl, &trmc_plan::t_wsum, ms_out, "no window summary has been formed on this plan");
}

int trmc_window_courant_tile(int precision, int32_t *rows, int32_t *steps)
{
    return window_tile(precision, rows, steps, kCourantRows, kCourantSteps, kCourantSteps);
}

static int window_courant_check(trmc_plan *pl, int32_t rowset)
{
    // (the triples are recomputed from the result AND from the window's forcing and initial state: k_window_courant)
    if (int rc = window_result_check(pl, "the Courant metrics are recomputed")) return rc;
    if (pl->maxlag > 0)
        return fail(TRMC_EUNSUPPORTED, "a plan with lagged rows (trmc_plan_set_lag) routes rows of other ranks' trunks at shifted steps: the "
                                       "Courant metrics of such a window are not built");
    if (pl->row0_replaced)
        return fail(TRMC_ESTATE, "trmc_plan_chain_from has replaced the initial state of the plan's last window since it ended");
    if (rowset < -1 || rowset >= (int32_t)pl->rowsets.size()) return fail(TRMC_EINVAL, "unknown row set");
    return 0;
}
int trmc_window_courant(trmc_plan *pl, int32_t rowset, int stride, void *dst)
{
    if (int rc = window_courant_check(pl, rowset)) return rc;
    if (stride < 1) return fail(TRMC_EINVAL, "stride must be >= 1");
    const int64_t nrows = rowset < 0 ? pl->nseg : pl->rowset_n[(size_t)rowset];
    const int32_t nkeep = pl->routed_nsteps / stride;
    if (pl->nseg == 0 || nrows == 0 || nkeep == 0) return 0;
    if (!dst) return fail(TRMC_EINVAL, "dst is NULL");
    if (int rc = use_device(pl)) return rc;
    const size_t bytes = (size_t)nrows * nkeep * 3 * pl->esz;
    if (int rc = pl->gathered.ensure(bytes)) return rc; // (the plan's scratch block for gathers of its result)
    pl->gathered_bytes = 0;
    if (int rc = pl->t_cour.begin(pl->stream)) return rc;
    const int rc = by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        CourantArgs<T> a;
        window_courant_args<T>(pl, rowset, a);
        a.stride = stride;
        a.nkeep = nkeep;
        a.dst = (T *)pl->gathered.p;
        window_courant_launch<T, false>(pl, a);
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    if (int rc = pl->t_cour.end(pl->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(dst, pl->gathered.p, bytes, hipMemcpyDeviceToHost, pl->stream));
    HIP_TRY(hipStreamSynchronize(pl->stream));
    return pl->t_cour.read();
}

int trmc_window_courant_summary(trmc_plan *pl, int32_t rowset, double limit, void *peak_cn, int32_t *peak_cn_step, int32_t *steps_over)
{
    if (int rc = window_courant_check(pl, rowset)) return rc;
    if (!peak_cn && !peak_cn_step && !steps_over) return fail(TRMC_EINVAL, "every destination is NULL: nothing to summarise");
    if (peak_cn_step && !peak_cn) return fail(TRMC_EINVAL, "the step of a peak comes with the peak: its value destination is NULL");
    const int64_t nrows = rowset < 0 ? pl->nseg : pl->rowset_n[(size_t)rowset];
    if (pl->nseg == 0 || nrows == 0) return 0;
    if (pl->routed_nsteps < 1) return fail(TRMC_ESTATE, "the last window had no timesteps");
    if (int rc = use_device(pl)) return rc;
    WindowColumns cols; // three, [nrows] each
    if (int rc = cols.lay(pl, nrows, {{peak_cn, pl->esz}, {peak_cn_step, 4}, {steps_over, 4}})) return rc;
    if (int rc = pl->t_cour.begin(pl->stream)) return rc;
    const int rc = by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        CourantArgs<T> a;
        window_courant_args<T>(pl, rowset, a);
        a.peak_cn = cols.dev<T>(0);
        a.peak_step = cols.dev<int32_t>(1);
        a.steps_over = cols.dev<int32_t>(2);
        a.limit = (T)limit;
        window_courant_launch<T, true>(pl, a);
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    return window_product_finish(pl, pl->t_cour, cols);
}

int trmc_window_courant_kernel_ms(const trmc_plan *pl, double *ms_out)
{
    return window_kernel_ms(pl, &trmc_plan::t_cour, ms_out, "no Courant metrics have been formed on this plan");
}

int trmc_plan_set_thresholds(trmc_plan *pl, int32_t nlevels, const void *th)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (nlevels < 0 || nlevels > 4) return fail(TRMC_EINVAL, "nlevels must be 0..4");
    if (stream_active(pl)) return fail(TRMC_ESTATE, "a stream of windows is in progress (trmc_stream_end it first)");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is in progress");
    if (nlevels == 0 || !th) {
        if (pl->thresholds.p) {
            if (int rc = use_device(pl)) return rc;
            pl->thresholds.release();
        }
        pl->th_levels = pl->th_pad = 0;
        return 0;
    }
    // the device table's rows are 1, 2 or 4 wide (k_window_exceed's KP), +inf -- never over -- behind the caller's levels
    const int32_t pad = nlevels == 3 ? 4 : nlevels;
    pl->th_levels = pl->th_pad = 0; // (nothing half-set if the copy fails)
    if (pl->nseg > 0) {
        if (int rc = use_device(pl)) return rc;
        const int rc = by_precision(pl, [&](auto t) -> int {
            using T = decltype(t);
            const T *const src = (const T *)th;
            std::vector<T> host((size_t)pl->nseg * pad, std::numeric_limits<T>::infinity());
            for (int64_t r = 0; r < pl->nseg; ++r)
                for (int32_t k = 0; k < nlevels; ++k) host[(size_t)r * pad + k] = src[(size_t)r * nlevels + k];
            if (int rc = pl->thresholds.ensure(host.size() * sizeof(T))) return rc;
            // (synchronous: the table is whole before the call returns, whichever stream reads it)
            HIP_TRY(hipMemcpy(pl->thresholds.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
            return 0;
        });
        if (rc) return rc;
    }
    pl->th_levels = nlevels;
    pl->th_pad = pad;
    return 0;
}

int trmc_window_exceedance_tile(int precision, int32_t *rows, int32_t *steps)
{
    return window_tile(precision, rows, steps, kRecRows, kRecSteps<float>, kRecSteps<double>);
}

int trmc_window_exceedance(trmc_plan *pl, int32_t rowset, int quantity, int32_t *steps_over, int32_t *first_step, int32_t *last_step,
                           int32_t *longest_run)
{
    if (int rc = window_result_check(pl, "a window's exceedance is formed")) return rc;
    if (pl->th_levels < 1) return fail(TRMC_ESTATE, "no thresholds set on this plan (trmc_plan_set_thresholds)");
    if (!steps_over && !first_step && !last_step && !longest_run) return fail(TRMC_EINVAL, "every destination is NULL: nothing to form");
    if (quantity != TRMC_X_FLOW && quantity != TRMC_X_VELOCITY && quantity != TRMC_X_DEPTH)
        return fail(TRMC_EINVAL, "quantity must be TRMC_X_FLOW, TRMC_X_VELOCITY or TRMC_X_DEPTH");
    if (rowset < -1 || rowset >= (int32_t)pl->rowsets.size()) return fail(TRMC_EINVAL, "unknown row set");
    const int64_t nrows = rowset < 0 ? pl->nseg : pl->rowset_n[(size_t)rowset];
    if (pl->nseg == 0 || nrows == 0) return 0;
    const int32_t nsteps = pl->routed_nsteps;
    if (nsteps < 1) return fail(TRMC_ESTATE, "the last window had no timesteps");
    if (int rc = use_device(pl)) return rc;
    WindowColumns cols; // the four asked for, [nrows][K] int32 each
    const size_t row_bytes = (size_t)pl->th_levels * sizeof(int32_t);
    if (int rc = cols.lay(pl, nrows, {{steps_over, row_bytes}, {first_step, row_bytes}, {last_step, row_bytes}, {longest_run, row_bytes}}))
        return rc;
    if (int rc = pl->t_wexc.begin(pl->stream)) return rc;
    const WexcOut o{cols.dev<int32_t>(0), cols.dev<int32_t>(1), cols.dev<int32_t>(2), cols.dev<int32_t>(3)};
    if (int rc = window_exceed_launch(pl, rowset, quantity, o, nrows, nsteps)) return rc;
    return window_product_finish(pl, pl->t_wexc, cols);
}

int trmc_window_exceedance_kernel_ms(const trmc_plan *pl, double *ms_out)
{
    return window_kernel_ms(pl, &trmc_plan::t_wexc, ms_out, "no window exceedance has been formed on this plan");
}

int trmc_plan_bankfull_depth(trmc_plan *pl, void *dst)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->nseg == 0) return 0;
    if (!dst) return fail(TRMC_EINVAL, "dst is NULL");
    if (int rc = use_device(pl)) return rc;
    return by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        // the plan's own column (k_make_const: make_const's bfd), plan order -> row order
        std::vector<T> by_pos((size_t)pl->nseg);
        HIP_TRY(hipMemcpy(by_pos.data(), col<T>(pl, TRMC_NPARAM + 1), by_pos.size() * sizeof(T), hipMemcpyDeviceToHost));
        T *const out = (T *)dst;
        const trmc::Topology &topo = pl->sh->topo;
        // rows that route no Muskingum-Cunge step have no bankfull: boundary rows, and a pool's elevation is not a channel's depth
        for (int64_t r = 0; r < pl->nseg; ++r)
            out[r] = topo.level_of_row[r] < 0 ? std::numeric_limits<T>::infinity() : by_pos[(size_t)topo.pos_of_row[r]];
        if (pl->nres > 0)
            for (int64_t r : pl->res_rows) out[r] = std::numeric_limits<T>::infinity();
        return 0;
    });
}

int trmc_plan_set_nan_is_zero(trmc_plan *pl, int on)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    pl->nan_is_zero = on != 0;
    return 0;
}

int trmc_host_alloc(size_t bytes, void **ptr_out)
{
    if (!ptr_out) return fail(TRMC_EINVAL, "ptr_out is NULL");
    *ptr_out = nullptr;
    if (bytes == 0) return 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(TRMC_ENODEVICE, "no HIP device available");
    const hipError_t e = hipHostMalloc(ptr_out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        *ptr_out = nullptr;
        (void)hipGetLastError();
        return fail(TRMC_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    return 0;
}

int trmc_host_free(void *ptr)
{
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return 0;
}

int trmc_plan_collect_cost(trmc_plan *pl, int enable)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is open");
    pl->collect_cost = enable != 0;
    if (!pl->collect_cost) pl->cost_nsteps = -1;
    return 0;
}

int trmc_download_cost(trmc_plan *pl, uint16_t *cost_out, int32_t *nsteps_out)
{
    if (!pl || !cost_out) return fail(TRMC_EINVAL, "plan/cost_out is NULL");
    if (!pl->collect_cost || pl->cost_nsteps < 0 || pl->routed_nsteps != pl->cost_nsteps)
        return fail(TRMC_ESTATE, "no window has been routed with cost collection on");
    if (int rc = use_device(pl)) return rc;
    std::vector<uint16_t> by_pos((size_t)pl->nseg_pad);
    HIP_TRY(hipMemcpy(by_pos.data(), pl->it_sum.p, (size_t)pl->nseg_pad * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < pl->nseg; ++p) cost_out[pl->sh->topo.row_of_pos[p]] = by_pos[(size_t)p];
    if (nsteps_out) *nsteps_out = pl->cost_nsteps;
    return 0;
}

int trmc_download_iterations(trmc_plan *pl, uint8_t *iters_out)
{
    if (!pl || !iters_out) return fail(TRMC_EINVAL, "plan/iters_out is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (int rc = use_device(pl)) return rc;
    std::vector<uint8_t> by_pos((size_t)pl->nseg_pad);
    HIP_TRY(hipMemcpy(by_pos.data(), pl->it_prev.p, (size_t)pl->nseg_pad, hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < pl->nseg; ++p) iters_out[pl->sh->topo.row_of_pos[p]] = by_pos[(size_t)p];
    return 0;
}

int trmc_download_final_state(trmc_plan *pl, void *q0_out)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (pl->nseg == 0) return 0;
    if (!q0_out) return fail(TRMC_EINVAL, "q0_out is NULL");
    if (int rc = use_device(pl)) return rc;
    const size_t bytes = (size_t)pl->nseg * 3 * pl->esz;
    if (int rc = pl->scratch.ensure(bytes)) return rc;
    if (int rc = final_state_into(pl, pl->scratch.p)) return rc;
    HIP_TRY(hipMemcpyAsync(q0_out, pl->scratch.p, bytes, hipMemcpyDeviceToHost, pl->stream));
    HIP_TRY(hipStreamSynchronize(pl->stream));
    return 0;
}

// the plan's copy stream (results to the host beside the next window; the next window's forcing to the device beside this one)
static int ensure_copy_stream(trmc_plan *pl)
{
    if (pl->cstream) return 0;
    // LOW priority: with one hardware queue per priority (GPU_MAX_HW_QUEUES=1, DESIGN.md 7b) a copy on a stream of ordinary
    // priority shares the queue of the tile stream, and the barrier packet that orders the copy holds the window's tile
    // launches back for as long as the copy runs (CONUS: 50 MB, 0.9 ms of an 18 ms window).  The low-priority queue only
    // carries the result transposes.
    int prio_lo = 0, prio_hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    if (int rc = pl->cstream.ensure(hipStreamNonBlocking, prio_lo)) return rc;
    // (a stream per direction: a day's decimated result on its way out -- 0.8 GB for a CONUS day, most of a window -- does not
    // hold the next day's forcing back, which the plan's next set-up waits for)
    if (int rc = pl->hstream.ensure(hipStreamNonBlocking, prio_lo)) return rc;
    return pl->ev_fetch_ready.ensure(false);
}

int trmc_fetch_begin(trmc_plan *pl, int32_t rowset, void *hyd_host, void *q0_host)
{
    return trmc_fetch_begin_fvd(pl, rowset, hyd_host, q0_host, 0, nullptr);
}

int trmc_fetch_begin_fvd(trmc_plan *pl, int32_t rowset, void *hyd_host, void *q0_host, int stride, void *fvd_host)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (fvd_host && stride < 1) return fail(TRMC_EINVAL, "stride must be >= 1");
    // After a window (trmc_route_end), or -- level engine -- WITH a window that has been queued to its end: the gathers then go
    // right behind the window's last launch on the plan's stream.  That is where a sequence alternating between two plans
    // wants them: queued after the window has been waited for, they would sit in the shared high-priority hardware queue
    // behind the OTHER plan's 288 tail launches, run a whole window late, and this plan's next window -- which overwrites
    // the planes they read -- could not start before (the timeline of bench.py's sequence showed exactly that).
    const bool in_window = pl->run.active;
    if (in_window) {
        if (pl->flow) return fail(TRMC_ESTATE, "a fetch queued with the window needs the level engine");
        if (pl->run.t_done < pl->run.nsteps + (pl->run.short_ts ? pl->maxlag : 0))
            return fail(TRMC_ESTATE, "the window in progress has not been queued to its end (trmc_route_advance)");
    } else if (pl->routed_nsteps < 0) {
        return fail(TRMC_ESTATE, "nothing routed yet");
    }
    if (pl->mk_fetch_done.pending()) return fail(TRMC_ESTATE, "a fetch is in flight (trmc_fetch_wait it first)");
    if (hyd_host && (rowset < 0 || rowset >= (int32_t)pl->rowsets.size())) return fail(TRMC_EINVAL, "unknown row set");
    if (int rc = use_device(pl)) return rc;
    if (int rc = ensure_copy_stream(pl)) return rc;
    if (in_window) { // (the window's own end -- transposing launches, the clock's events -- first)
        if (int rc = by_precision(pl, [&](auto t) { return route_end_queue<decltype(t)>(pl); })) return rc;
    }
    const int32_t T_ = in_window ? pl->run.nsteps : pl->routed_nsteps;
    const int64_t nrows = hyd_host ? pl->rowset_n[rowset] : 0;
    const size_t hb = (size_t)nrows * T_ * pl->esz, qb = q0_host ? (size_t)pl->nseg * 3 * pl->esz : 0;
    if (hb) {
        if (int rc = pl->fetch_hyd.ensure(hb)) return rc;
        if (int rc = gather_rows(pl, (const int32_t *)pl->rowsets[rowset].p, pl->fetch_hyd.p, nrows, T_)) return rc;
        if (int rc = note_gather(pl, in_window)) return rc;
    }
    if (qb) {
        if (int rc = pl->fetch_q0.ensure(qb)) return rc;
        if (int rc = final_state_into(pl, pl->fetch_q0.p, in_window ? T_ : -1)) return rc;
    }
    // Every stride-th step of (q, v, d) of every row: decimated on the plan's stream, which at this point follows everything
    // that writes `out` (the tiles and the transposes: route_end_queue).  The kernel reads the whole result once (12 bytes of
    // every 144 at stride 12: every cache line) -- about 2 ms of a CONUS day's period wherever it runs; measured on the sequence
    // with hourly output (ms per day; 17.3 with neither kernel nor copy): here 19.4; on the transpose stream (low priority) 19.3
    // with the copy on a stream of its own and 28 with the copy on the copy stream (the in-order hardware queue of that
    // priority then also holds the next day's transposes and forcing behind the 14-ms copy); without the kernel 17.5.  The copy
    // on a stream of its own with no event behind it (its end polled with hipStreamQuery): days of 24.7 and 15 ms in turn,
    // 20.7 on average -- the copies of consecutive days overlap on the one PCIe direction.
    const int32_t nkeep = fvd_host ? T_ / stride : 0;
    const size_t fb = (size_t)pl->nseg * nkeep * 3 * pl->esz;
    const void *fvd_src = pl->out.p;
    // ... unless the window decimated as it went (trmc_plan_set_output_stride): the tiled rows' kept steps are in `dec` already,
    // the others are gathered from the time-major planes (coalesced; 0.2 GB of a CONUS day instead of 9.4)
    const bool have_dec = fb && !pl->flow && pl->dec.p
                          && (in_window ? pl->run.dec_stride == stride && pl->run.dec_keep == nkeep
                                        : pl->dec_stride_done == stride && pl->dec_keep_done == nkeep && pl->dec_nsteps_done == T_);
    bool from_dec = false;
    if (have_dec) {
        const int32_t lo = in_window ? pl->run.dec_lo : pl->dec_lo_done, hi = in_window ? pl->run.dec_hi : pl->dec_hi_done;
        const size_t plane = (size_t)(T_ + 1) * pl->nseg_pad;
        const int rc = by_precision(pl, [&](auto t) {
            using T = decltype(t);
            const T *q = (const T *)pl->tm.p;
            hipLaunchKernelGGL((k_decimate_planes<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pl->stream, q, q + plane, q + 2 * plane,
                               (const int32_t *)pl->sh->row_of_pos.p, (T *)pl->dec.p, (int32_t)pl->nseg, pl->nseg_pad, stride, nkeep, lo, hi);
            return launched();
        });
        if (rc) return rc;
        if (int rc = note_gather(pl, in_window)) return rc;
        fvd_src = pl->dec.p;
        from_dec = true;
    } else if (fb && stride > 1) {
        if (int rc = pl->fetch_fvd.ensure(fb)) return rc;
        if (int rc = decimate_out(pl, pl->fetch_fvd.p, T_, stride, nkeep, -1)) return rc;
        if (int rc = note_gather(pl, in_window)) return rc; // (the next window's set-up, wherever it is queued, goes behind it)
        fvd_src = pl->fetch_fvd.p;
    }
    HIP_TRY(hipEventRecord(pl->ev_fetch_ready, pl->stream));
    HIP_TRY(hipStreamWaitEvent(pl->cstream, pl->ev_fetch_ready, 0));
    // (Queued WITH the window the copies have a dependence that is still pending, and hipMemcpyAsync device-to-host then keeps
    // the calling thread until it is resolved: trmc_fetch_begin returns when the window ends.  A copy by a kernel that writes
    // the page-locked arrays through the device's mapping never waits on the host, but was no gain on the CONUS sequence --
    // 17.1 ms per day against 16.7: a day's narrow levels can only start when the day before has ended -- and is gone.)
    auto to_host = [&](void *dst_host, const void *src_dev, size_t bytes) -> int {
        HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, pl->cstream));
        return 0;
    };
    if (hb)
        if (int rc = to_host(hyd_host, pl->fetch_hyd.p, hb)) return rc;
    if (qb)
        if (int rc = to_host(q0_host, pl->fetch_q0.p, qb)) return rc;
    if (fb) {
        if (int rc = to_host(fvd_host, fvd_src, fb)) return rc;
        if (stride == 1 || from_dec) // (copied from `out` / `dec` themselves: the plan's next window, which writes them, starts behind the copy)
            if (int rc = pl->mk_dec.record(pl->cstream)) return rc;
    }
    return pl->mk_fetch_done.record(pl->cstream);
}

int trmc_fetch_wait(trmc_plan *pl)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (!pl->mk_fetch_done.pending()) return 0;
    if (int rc = use_device(pl)) return rc;
    return pl->mk_fetch_done.sync();
}

int trmc_gather_flow_rows(trmc_plan *pl, const int64_t *rows, int64_t nrows, void *out, int dst_is_device)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    if (pl->routed_nsteps < 0) return fail(TRMC_ESTATE, "nothing routed yet");
    if (nrows == 0) return 0;
    if (!rows || (!out && !dst_is_device)) return fail(TRMC_EINVAL, "rows/out is NULL");
    if (int rc = use_device(pl)) return rc;
    std::vector<int32_t> pos((size_t)nrows);
    for (int64_t i = 0; i < nrows; ++i) {
        if (rows[i] < 0 || rows[i] >= pl->nseg) return fail(TRMC_EINVAL, "row out of range");
        pos[i] = pl->sh->topo.pos_of_row[rows[i]];
    }
    const int32_t T_ = pl->routed_nsteps;
    const size_t obytes = (size_t)nrows * T_ * pl->esz;
    const size_t pbytes = ((size_t)nrows * sizeof(int32_t) + 255) / 256 * 256;
    if (int rc = pl->scratch.ensure(pbytes + (dst_is_device ? 0 : obytes))) return rc;
    HIP_TRY(hipMemcpyAsync(pl->scratch.p, pos.data(), (size_t)nrows * sizeof(int32_t), hipMemcpyHostToDevice, pl->stream));
    if (dst_is_device && !out) { // keep the block in plan-owned HBM; fetch with trmc_download_gathered()
        if (int rc = pl->gathered.ensure(obytes)) return rc;
        out = pl->gathered.p;
        pl->gathered_bytes = obytes;
    }
    void *dst = dst_is_device ? out : (void *)((char *)pl->scratch.p + pbytes);
    if (int rc = gather_rows(pl, (const int32_t *)pl->scratch.p, dst, nrows, T_)) return rc;
    if (!dst_is_device) HIP_TRY(hipMemcpyAsync(out, dst, obytes, hipMemcpyDeviceToHost, pl->stream));
    HIP_TRY(hipStreamSynchronize(pl->stream));
    return 0;
}

int trmc_download_gathered(trmc_plan *pl, void *out)
{
    if (!pl || !out) return fail(TRMC_EINVAL, "plan/out is NULL");
    if (pl->gathered_bytes == 0) return fail(TRMC_ESTATE, "no device-resident gather to download");
    if (int rc = use_device(pl)) return rc;
    HIP_TRY(hipMemcpy(out, pl->gathered.p, pl->gathered_bytes, hipMemcpyDeviceToHost));
    return 0;
}

int trmc_get_stats(const trmc_plan *pl, trmc_stats *stats)
{
    if (!pl || !stats) return fail(TRMC_EINVAL, "plan/stats is NULL");
    *stats = pl->stats;
    return 0;
}

int trmc_route(trmc_plan *pl, int nsteps, int qts_subdivisions, int assume_short_ts, const void *qlat, int64_t nq,
               const void *q0, const void *boundary_fvd, void *fvd_out)
{
    if (int rc = trmc_upload_forcing(pl, nsteps, qlat, nq, q0, boundary_fvd)) return rc;
    if (int rc = trmc_route_device(pl, nsteps, qts_subdivisions, assume_short_ts)) return rc;
    return trmc_download_fvd(pl, fvd_out);
}

int trmc_segments(int device, int precision, int64_t n, const void *in, void *out)
{
    return trmc_segments_ex(device, precision, TRMC_ARITH_EXACT, n, in, out, nullptr);
}

int trmc_segments_ex(int device, int precision, int arithmetic, int64_t n, const void *in, void *out, int32_t *iters_out)
{
    if (arithmetic != TRMC_ARITH_EXACT && arithmetic != TRMC_ARITH_TOLERANCE) return fail(TRMC_EINVAL, "bad arithmetic");
    if (arithmetic == TRMC_ARITH_TOLERANCE && precision != 32)
        return fail(TRMC_EINVAL, "TRMC_ARITH_TOLERANCE is an arithmetic of precision 32");
    if (precision != 32 && precision != 64) return fail(TRMC_EINVAL, "precision must be 32 or 64");
    if (n < 0) return fail(TRMC_EINVAL, "n < 0");
    if (n == 0) return 0;
    if (!in || !out) return fail(TRMC_EINVAL, "in/out is NULL");
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const bool tol = arithmetic == TRMC_ARITH_TOLERANCE;
    return precision == 32 ? segments_t<float>(n, in, out, tol, iters_out) : segments_t<double>(n, in, out, false, iters_out);
}

// The reference's own C binding of one segment-step -- c_muskingcungenwm, src/kernel/muskingum/pyMCsingleSegStime_NoLoop.f90:8-21
// (header src/troute-routing/troute/routing/fast_reach/pyMCsingleSegStime_NoLoop.h:1-21, declared to Cython at
// fast_reach/fortran_wrappers.pxd:19-40): 21 float pointers, 15 in, 6 out, no return value.  One step on the device per call
// (trmc_segments with n = 1): the drop-in for reach.pyx:37-94's call site, not a fast path -- the fast paths are the batch
// form and the plans.  Like the Fortran it cannot signal: on failure the six outputs are NaN and trmc_last_error() says why.
// qdc is taken as 0 on entry (reach.pyx:55 passes 0; f90:74 reads it).  Device: TRMC_DEVICE (default 0).
void trmc_muskingcungenwm(float *dt, float *qup, float *quc, float *qdp, float *ql, float *dx, float *bw, float *tw,
                          float *twcc, float *n, float *ncc, float *cs, float *s0, float *velp, float *depthp, float *qdc,
                          float *velc, float *depthc, float *ck, float *cn, float *X)
{
    float *outs[6] = {qdc, velc, depthc, ck, cn, X};
    const float *ins[15] = {dt, qup, quc, qdp, ql, dx, bw, tw, twcc, n, ncc, cs, s0, velp, depthp};
    bool ok = true;
    for (const float *p : ins) ok = ok && p != nullptr;
    for (float *p : outs) ok = ok && p != nullptr;
    float in[15], out[6];
    int rc = TRMC_EINVAL;
    if (ok) {
        for (int i = 0; i < 15; ++i) in[i] = *ins[i];
        const char *d = std::getenv("TRMC_DEVICE");
        rc = trmc_segments(d ? std::atoi(d) : 0, 32, 1, in, out);
    } else {
        (void)fail(TRMC_EINVAL, "trmc_muskingcungenwm: an argument is NULL");
    }
    for (int i = 0; i < 6; ++i)
        if (outs[i]) *outs[i] = rc == 0 ? out[i] : std::nanf("");
}

int trmc_plan_chain_from(trmc_plan *dst, trmc_plan *src)
{
    if (!dst || !src || dst == src) return fail(TRMC_EINVAL, "two different plans are needed");
    if (dst->flow || src->flow) return fail(TRMC_EINVAL, "plans of the level engine only");
    if (dst->run.active) return fail(TRMC_ESTATE, "a routing window of the receiving plan is in progress");
    if (dst->staged_nsteps < 1) return fail(TRMC_ESTATE, "the receiving plan has no forcing staged (trmc_upload_forcing)");
    if (src->run.nsteps < 1 || (!src->run.active && src->routed_nsteps < 0))
        return fail(TRMC_ESTATE, "the source plan has routed nothing");
    if (src->run.active && src->run.t_done < src->run.nsteps + (src->run.short_ts ? src->maxlag : 0))
        return fail(TRMC_ESTATE, "the source plan's window has not been queued to its end (trmc_route_advance)");
    if (dst->nseg != src->nseg || dst->precision != src->precision || dst->device != src->device
        || dst->sh->topo.row_of_pos != src->sh->topo.row_of_pos)
        return fail(TRMC_EINVAL, "the two plans must hold the same network in the same order (same inputs, same cost hint)");
    if (int rc = use_device(dst)) return rc;
    dst->row0_replaced = true; // (what trmc_window_courant reads as the last window's initial state; the next window clears it)
    return by_precision(dst, [&](auto t) { return chain_from_t<decltype(t)>(dst, src, dst->staged_nsteps); });
}

int trmc_selfcheck_fast_arith(int device, int what, int64_t n, uint64_t seed, int64_t *checked_out, int64_t *mismatches_out)
{
    if (!checked_out || !mismatches_out) return fail(TRMC_EINVAL, "checked_out/mismatches_out is NULL");
    if (what < 0 || what > 4)
        return fail(TRMC_EINVAL, "what must be 0 (square root), 1 (division, maximum), 2 (refined reciprocal), 3 (three-operation quotient) "
                                 "or 4 (that quotient over the operands of the Muskingum coefficients)");
    if ((what == 1 || what == 3 || what == 4) && n < 0) return fail(TRMC_EINVAL, "n < 0");
    if (what == 2 && (n < -126 || n > 126)) return fail(TRMC_EINVAL, "n (the binade's exponent) outside [-126, 126]");
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    DevBuf cnt;
    if (int rc = cnt.ensure(sizeof(unsigned long long))) return rc;
    hipError_t e = hipMemset(cnt.p, 0, sizeof(unsigned long long));
    int64_t checked = 0;
    if (e == hipSuccess) {
        if (what == 0) {
            const uint32_t lo = (uint32_t)(127 - 60) << 23, hi = (uint32_t)(127 + 63) << 23; // 2**-60 .. 2**63 inclusive
            checked = (int64_t)hi - (int64_t)lo + 1;
            hipLaunchKernelGGL(k_selfcheck_sqrt, dim3(8192), dim3(kBlock), 0, 0, lo, hi, (unsigned long long *)cnt.p);
        } else if (what == 1) {
            checked = n;
            if (n > 0) hipLaunchKernelGGL(k_selfcheck_div, dim3(8192), dim3(kBlock), 0, 0, n, seed, (unsigned long long *)cnt.p);
        } else if (what == 2) {
            checked = (int64_t)1 << 23;
            hipLaunchKernelGGL(k_selfcheck_rcp, dim3((1u << 23) / kBlock), dim3(kBlock), 0, 0, (uint32_t)(n + 127), (unsigned long long *)cnt.p);
        } else if (what == 3) {
            checked = kQuotDivisors * (n + 1); // (+1: the numerator +0 of every divisor)
            hipLaunchKernelGGL(k_selfcheck_quot, dim3(8192), dim3(kBlock), 0, 0, n, seed, (unsigned long long *)cnt.p);
        } else {
            checked = kQuotDivisors * (n + 2); // (+2: the numerators +0 and -0 of every divisor, through coef_guard and div4)
            hipLaunchKernelGGL(k_selfcheck_quot_box, dim3(8192), dim3(kBlock), 0, 0, n, seed, (unsigned long long *)cnt.p);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, cnt.p, sizeof bad, hipMemcpyDeviceToHost);
    cnt.release();
    if (e != hipSuccess) return fail(TRMC_EHIP, std::string("trmc_selfcheck_fast_arith: ") + hipGetErrorString(e));
    *checked_out = checked;
    *mismatches_out = (int64_t)bad;
    return 0;
}

int trmc_selfcheck_rcp_values(int device, int exponent, float *out)
{
    if (!out) return fail(TRMC_EINVAL, "out is NULL");
    if (exponent < -126 || exponent > 126) return fail(TRMC_EINVAL, "exponent outside [-126, 126]");
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)1 << 23;
    DevBuf y;
    if (int rc = y.ensure(n * sizeof(float))) return rc;
    hipLaunchKernelGGL(k_rcp_values, dim3((unsigned)(n / kBlock)), dim3(kBlock), 0, 0, (uint32_t)(exponent + 127), (float *)y.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, y.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
