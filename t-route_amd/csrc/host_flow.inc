// host_flow.inc -- included by trmc.hip: a routing window on the dataflow engine.
// ---- dataflow engine, host side (fp32 plans in block order) ------------------------------------------------------
// Deal the blocks of a dataflow plan to the compute units by cost (see lean_pick_block).  Cost of a wavefront: the
// instructions of one of its steps by the hint of its costliest row (counters of the lean kernel by iteration class: dry
// 130, one iteration 600, two 890, three 1 150, over-bank rows about twice that) -- a hint is either the iteration class
// 0..3 (+ 4 over bank) or its window mean in sixteenths (ShardedRouter.iteration_hint); without one it is the drainage
// class 0..3, the same scale.  Blocks go out in rounds of one per unit, costliest first, each to the unit that carries least
// so far: every unit gets as many blocks as the hardware will send it workgroups (it deals those out by count).
int flow_place_blocks(trmc_plan *pl)
{
    pl->ncuq = 0;
    const int32_t nb = pl->sh->topo.nblocks;
    if (nb <= 0) return 0;
    constexpr int kKeys = 4096;
    // which compute units are there?
    DevBuf seen;
    if (int rc = seen.ensure(kKeys)) return rc;
    HIP_TRY(hipMemset(seen.p, 0, kKeys));
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device);
    hipLaunchKernelGGL(k_cu_probe, dim3((unsigned)(64 * ncu)), dim3(64), 0, nullptr, (uint8_t *)seen.p);
    std::vector<uint8_t> hs(kKeys);
    hipError_t e = hipMemcpy(hs.data(), seen.p, kKeys, hipMemcpyDeviceToHost);
    seen.release();
    if (e != hipSuccess) return fail(TRMC_EHIP, std::string("compute-unit probe: ") + hipGetErrorString(e));
    std::vector<int32_t> cu_index(kKeys, -1);
    int32_t Q = 0;
    for (int k = 0; k < kKeys; ++k)
        if (hs[k]) cu_index[k] = Q++;
    if (Q < 2) return 0;
    // cost of every block
    const std::vector<uint8_t> &wc = pl->sh->topo.cost_of_wave;
    int hi = 0;
    for (const uint8_t c : wc) hi = std::max(hi, (int)c);
    const bool sixteenths = hi > 7;
    auto units = [&](int hint) {
        const double c = sixteenths ? hint / 16.0 : (double)hint;
        static const double x[5] = {0, 1, 2, 3, 7}, y[5] = {130, 600, 890, 1150, 2200};
        for (int i = 1; i < 5; ++i)
            if (c <= x[i]) return y[i - 1] + (y[i] - y[i - 1]) * (c - x[i - 1]) / (x[i] - x[i - 1]);
        return y[4];
    };
    constexpr int wpb = kFlowBlock / 64;
    std::vector<double> cost((size_t)nb, 0.0), wcost((size_t)nb * wpb, 0.0);
    for (int32_t b = 0; b < nb; ++b)
        for (int q = 0; q < wpb; ++q) {
            const size_t w = (size_t)b * wpb + q;
            if (w < wc.size()) wcost[w] = units(wc[w]);
            cost[(size_t)b] += wcost[w];
        }
    std::vector<int32_t> order((size_t)nb);
    for (int32_t b = 0; b < nb; ++b) order[(size_t)b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return cost[(size_t)x] > cost[(size_t)y]; });
    std::vector<double> load((size_t)Q, 0.0), sload((size_t)Q * 4, 0.0); // per unit; per SIMD of a unit
    std::vector<std::vector<int32_t>> queue((size_t)Q);
    std::vector<int32_t> cus((size_t)Q);
    std::vector<uint8_t> perm((size_t)nb + 4, 0xe4); // identity: group s for SIMD s
    for (int32_t r = 0; r < nb; r += Q) {
        for (int32_t c = 0; c < Q; ++c) cus[(size_t)c] = c;
        std::stable_sort(cus.begin(), cus.end(), [&](int32_t x, int32_t y) { return load[(size_t)x] < load[(size_t)y]; });
        for (int32_t j = 0; j < std::min(Q, nb - r); ++j) {
            const int32_t b = order[(size_t)(r + j)], c = cus[(size_t)j];
            queue[(size_t)c].push_back(b);
            load[(size_t)c] += cost[(size_t)b];
            if (wpb == 4) { // the block's row groups by descending cost meet the unit's SIMDs by ascending load
                int g[4] = {0, 1, 2, 3}, sd[4] = {0, 1, 2, 3};
                std::stable_sort(g, g + 4, [&](int x, int y) { return wcost[(size_t)b * 4 + x] > wcost[(size_t)b * 4 + y]; });
                std::stable_sort(sd, sd + 4, [&](int x, int y) { return sload[(size_t)c * 4 + x] < sload[(size_t)c * 4 + y]; });
                uint8_t pm = 0;
                for (int i = 0; i < 4; ++i) {
                    pm |= (uint8_t)(g[i] << (2 * sd[i]));
                    sload[(size_t)c * 4 + sd[i]] += wcost[(size_t)b * 4 + g[i]];
                }
                perm[(size_t)b] = pm;
            }
        }
    }
    std::vector<int32_t> ptr((size_t)Q + 1, 0), blk;
    blk.reserve((size_t)nb);
    for (int32_t c = 0; c < Q; ++c) {
        // (in the order they were dealt: by descending cost -- a unit's own workgroups take from the front, thieves from the back)
        for (const int32_t b : queue[(size_t)c]) blk.push_back(b);
        ptr[(size_t)c + 1] = (int32_t)blk.size();
    }
    if (int rc = pl->sh->cuq_perm.ensure(perm.size())) return rc;
    HIP_TRY(hipMemcpy(pl->sh->cuq_perm.p, perm.data(), perm.size(), hipMemcpyHostToDevice));
    if (int rc = upload_i32(pl->sh->cuq_ptr, ptr, 1)) return rc;
    if (int rc = upload_i32(pl->sh->cuq_blk, blk, 1)) return rc;
    if (int rc = upload_i32(pl->sh->cu_index, cu_index, 1)) return rc;
    if (int rc = pl->cuq_head.ensure((size_t)Q * 2 * sizeof(int32_t))) return rc;
    pl->ncuq = Q;
    return 0;
}

FlowArgs flow_args(trmc_plan *pl, int nsteps, int qts, bool short_ts)
{
    FlowArgs a;
    a.dt_col = pl->dt_uniform ? nullptr : col<float>(pl, TRMC_P_DT);
    a.dt = (float)pl->dt;
    a.dx = col<float>(pl, TRMC_P_DX);
    a.bw = col<float>(pl, TRMC_P_BW);
    a.twcc = col<float>(pl, TRMC_P_TWCC);
    a.n = col<float>(pl, TRMC_P_N);
    a.ncc = col<float>(pl, TRMC_P_NCC);
    a.s0 = col<float>(pl, TRMC_P_S0);
    a.z = col<float>(pl, TRMC_NPARAM + 0);
    a.bfd = col<float>(pl, TRMC_NPARAM + 1);
    a.sqrt_s0 = col<float>(pl, TRMC_NPARAM + 2);
    a.sq1pz2 = col<float>(pl, TRMC_NPARAM + 3);
    a.s0_n = col<float>(pl, TRMC_NPARAM + 4);
    a.s0_ncc = col<float>(pl, TRMC_NPARAM + 5);
    a.inv_n = col<float>(pl, TRMC_NPARAM + 6);
    a.up_ptr = (const int32_t *)pl->sh->up_ptr.p;
    a.up_idx = (const int32_t *)pl->sh->up_idx.p;
    a.up2 = (const int2 *)pl->sh->up2.p;
    // short-timestep mode: the skew of trmc_plan_set_lag; general mode: the level rank inside the block
    a.lag = short_ts ? (pl->maxlag > 0 ? (const int32_t *)pl->sh->lag.p : nullptr)
                     : (pl->sh->topo.maxrank > 0 ? (const int32_t *)pl->sh->rank.p : nullptr);
    a.ticket_map = short_ts ? nullptr : (const int32_t *)pl->sh->ticket_map.p;
    a.qlat_tm = (const float *)pl->qlat_tm.p;
    a.gran = (unsigned long long *)pl->tm.p;
    a.d_state = (float *)pl->d_state.p;
    a.d_gran = (unsigned long long *)pl->d_gran.p;
    a.out = (float *)pl->out.p;
    a.row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
    a.it_prev = (uint8_t *)pl->it_prev.p;
    a.it_sum = pl->collect_cost ? (uint16_t *)pl->it_sum.p : nullptr;
    a.sane = pl->params_sane;
    a.out_vec = nsteps % 4 == 0;
    a.res_of_pos = pl->nres > 0 ? (const int32_t *)pl->res_of_pos.p : nullptr;
    a.res_par = (const float *)pl->res_par.p;
    a.res_inflow = (float *)pl->res_inflow.p;
    a.res_dt = (float)pl->res_dt;
    a.res_da = (pl->nres > 0 && pl->res_da_on) ? pl->res_da.p : nullptr;
    const bool da = pl->ngage > 0;
    a.gage_of_pos = da ? (const int32_t *)pl->gage_of_pos.p : nullptr;
    a.da_mode = (const uint8_t *)pl->da_mode.p;
    a.da_a = (const float *)pl->da_a.p;
    a.da_w = (const float *)pl->da_w.p;
    a.da_nudge = (float *)pl->da_nudge.p;
    a.nseg_pad = pl->nseg_pad;
    a.nsteps = nsteps;
    a.qts = qts;
    a.nseg = (int32_t)pl->nseg;
    a.first = (int32_t)pl->sh->topo.nboundary;
    a.tag_base = pl->tag_base;
    a.ticket = (int32_t *)pl->ticket.p;
    a.watchdog_ticks = pl->watchdog_ticks;
    a.dbg = pl->opt.flow_debug ? (unsigned long long *)pl->dbg.p : nullptr; // (trmc_plan_options.flow_debug: when did every block run?)
    a.nblocks_dbg = pl->sh->topo.nblocks;
    a.prio = (const uint8_t *)pl->sh->prio.p;
    a.cuq_ptr = a.cuq_blk = a.cu_index = nullptr; // (flow_route_advance switches the queues on for lean launches)
    a.cuq_perm = nullptr;
    a.cuq_head = nullptr;
    a.ncuq = 0;
    return a;
}

int flow_route_begin(trmc_plan *pl, int nsteps, int qts, int short_ts)
{
    const trmc::Topology &tp = pl->sh->topo;
    const int32_t n = (int32_t)pl->nseg;
    const int64_t np = pl->nseg_pad;
    hipStream_t st = pl->stream;
    if (int rc = pl->tm.ensure((size_t)(nsteps + 1) * np * sizeof(unsigned long long), true)) return rc;
    if (int rc = pl->d_state.ensure((size_t)np * sizeof(float))) return rc;
    if (int rc = pl->d_gran.ensure((size_t)np * sizeof(unsigned long long), true)) return rc;
    if (int rc = pl->ticket.ensure(16 * sizeof(int32_t))) return rc; // one set of 8 per compute stream
    if (pl->opt.flow_debug) {
        if (int rc = pl->dbg.ensure((size_t)(tp.nblocks + 1) * 6 * sizeof(unsigned long long))) return rc;
        HIP_TRY(hipMemsetAsync(pl->dbg.p, 0, pl->dbg.bytes, st));
    }
    if (int rc = pl->qlat_tm.ensure((size_t)pl->nq * np * sizeof(float))) return rc;
    if (int rc = pl->out.ensure((size_t)pl->nseg * nsteps * 3 * sizeof(float))) return rc;
    if (pl->nres > 0)
        if (int rc = pl->res_inflow.ensure((size_t)pl->nres * nsteps * sizeof(float))) return rc;
    if (pl->collect_cost) {
        if (int rc = pl->it_sum.ensure((size_t)np * sizeof(uint16_t))) return rc;
        pl->cost_nsteps = nsteps;
    }
    // a fresh range of tags for this window: nothing an earlier window left in the plane can pass for a live granule
    if ((uint64_t)pl->tag_base + (uint64_t)pl->tag_span + (uint64_t)nsteps + 2 >= 0xffffffffull) {
        HIP_TRY(hipMemsetAsync(pl->tm.p, 0, pl->tm.bytes, st));
        HIP_TRY(hipMemsetAsync(pl->d_gran.p, 0, pl->d_gran.bytes, st));
        pl->tag_base = 1;
        pl->tag_span = 0;
    }
    pl->tag_base += (uint32_t)pl->tag_span;
    pl->tag_span = nsteps + 1;
    const int32_t *row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
    HIP_TRY(hipEventRecord(pl->ev[0], st));
    pl->q0_staged = false; // (consumed by this window)
    if (int rc = pl->mk_dec.order(st)) return rc; // (trmc_fetch_begin_fvd: the copy stream reads `out`)
    if (pl->fstream)
        if (int rc = pl->mk_dec.order(pl->fstream)) return rc;
    pl->mk_dec.settle();
    if (int rc = pl->mk_forcing.order(st)) return rc; // (trmc_stage_forcing: the copy into in_qlat runs on the copy stream)
    pl->mk_forcing.settle();
    HIP_TRY(hipMemsetAsync(pl->it_prev.p, 0, (size_t)np, st));
    HIP_TRY(hipMemsetAsync(pl->ticket.p, 0, 16 * sizeof(int32_t), st));
    pl->flow_next = pl->flow_last = 0;
    if (pl->collect_cost) HIP_TRY(hipMemsetAsync(pl->it_sum.p, 0, (size_t)np * sizeof(uint16_t), st));
    if (n > 0) {
        if (!pl->qlat_direct)
            hipLaunchKernelGGL((k_prep_qlat<float>), dim3((n + 63) / 64, (unsigned)((pl->nq + 31) / 32)), dim3(kBlock), 0, st,
                               (const float *)pl->in_qlat.p, row_of_pos, (float *)pl->qlat_tm.p, n, np, (int32_t)pl->nq);
        hipLaunchKernelGGL(k_flow_init, dim3(blocks_for(n)), dim3(kBlock), 0, st, (const float *)pl->in_q0.p, row_of_pos,
                           (unsigned long long *)pl->tm.p, (float *)pl->d_state.p, (unsigned long long *)pl->d_gran.p, n,
                           pl->tag_base);
    }
    RouteRun &r = pl->run;
    r = RouteRun{};
    r.active = true;
    r.nsteps = nsteps;
    r.qts = qts;
    r.short_ts = short_ts ? 1 : 0;
    r.boundary_through = tp.nboundary > 0 ? 0 : nsteps;
    if (tp.nboundary > 0 && pl->have_boundary) {
        hipLaunchKernelGGL(k_flow_boundary, dim3(blocks_for(tp.nboundary * (int64_t)nsteps)), dim3(kBlock), 0, st,
                           (const float *)pl->in_bfvd.p, (unsigned long long *)pl->tm.p, (float *)pl->out.p, row_of_pos,
                           (int32_t)tp.nboundary, nsteps, np, 0, nsteps, (int64_t)nsteps * 3, 3, 3, pl->tag_base, (const int64_t *)nullptr);
        r.boundary_through = nsteps;
    }
    HIP_TRY(hipEventRecord(pl->ev[1], st));
    HIP_TRY(hipStreamWaitEvent(pl->fstream, pl->ev[1], 0)); // the second compute stream starts behind the window's set-up
    HIP_TRY(hipGetLastError());
    pl->routed_nsteps = -1;
    return 0;
}

// Which form of the short-timestep kernel a window uses, and whether consecutive launches of it may overlap.
// The lean form pays where every block of the launch is resident at once (6 workgroups per compute unit: one rank of a
// multi-GPU job, a regional network) -- there the pace is set by latency and by the slowest wavefront, and occupancy plus
// wavefront priorities win (349 k rows, 288 steps: 4.8 ms against 6.1 ms).  Where blocks run in many rounds (CONUS on one
// GPU: 10 661 blocks) throughput counts and the staged form, which spills nothing and writes whole sectors, is ahead
// (25.4 ms against 30.5 ms).
static bool flow_lean(const trmc_plan *pl, int nsteps)
{
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device);
    const int32_t force = pl->opt.flow_lean; // (trmc_plan_options.flow_lean: > 0 always, < 0 never -- A/B measurements)
    return (uint64_t)pl->nseg * (uint64_t)nsteps * 3ull < (1ull << 32)
           && (force ? force > 0 : pl->sh->topo.nblocks <= TRMC_LEAN_WAVES * (256 / kFlowBlock) * ncu);
}
// Optional (trmc_plan_options.flow_overlap; off by default): consecutive launches of a short-timestep window on the lean kernel
// alternate between two compute streams.  Rows hand their state from launch to launch through granules (flow plane,
// d_gran), so launch c+1 needs no kernel boundary behind launch c -- its cheap blocks take the slots launch c's cheap blocks
// have left while c's costly blocks are still finishing.  Safe because every block of a launch is resident (flow_lean):
// launch c+2, behind c on its stream, starts when all of c+1 is.  Measured on 349 k-row ranks (8 chunks per window): no
// gain -- 4.9 ms either way once both streams have a hardware queue each, and the two streams share one under
// GPU_MAX_HW_QUEUES=1, which troute_amd.distributed sets (DESIGN.md section 7b) -- hence opt-in.
static bool flow_overlap(const trmc_plan *pl)
{
    return pl->opt.flow_overlap && pl->run.short_ts && flow_lean(pl, pl->run.nsteps);
}
static hipStream_t flow_stream(const trmc_plan *pl, int which) { return which ? pl->fstream : pl->stream; }

// one launch routes every row through the launches / steps (t_done, t_end]
int flow_route_advance(trmc_plan *pl, int t_end)
{
    RouteRun &r = pl->run;
    if (pl->nrouted > 0 && t_end > r.t_done) {
        const bool lean = r.short_ts && flow_lean(pl, r.nsteps);
        const int which = flow_overlap(pl) ? pl->flow_next : 0;
        hipStream_t st = flow_stream(pl, which);
        FlowArgs a = flow_args(pl, r.nsteps, r.qts, r.short_ts != 0);
        a.ticket += 8 * which;                                       // every compute stream has its own block tickets
        HIP_TRY(hipMemsetAsync(a.ticket, 0, sizeof(int32_t), st));   // they restart; the abort flag stays
        if (lean && pl->ncuq > 0) { // blocks by compute unit (lean_pick_block)
            a.cuq_ptr = (const int32_t *)pl->sh->cuq_ptr.p;
            a.cuq_blk = (const int32_t *)pl->sh->cuq_blk.p;
            a.cu_index = (const int32_t *)pl->sh->cu_index.p;
            a.cuq_perm = (const uint8_t *)pl->sh->cuq_perm.p;
            a.cuq_head = (int32_t *)pl->cuq_head.p + (size_t)pl->ncuq * which;
            a.ncuq = pl->ncuq;
            HIP_TRY(hipMemsetAsync(a.cuq_head, 0, (size_t)pl->ncuq * sizeof(int32_t), st));
        }
        const dim3 grid((unsigned)pl->sh->topo.nblocks), block(kFlowBlock);
        if (a.res_da) { // (exact arithmetic: trmc_set_reservoir_da)
            if (lean && a.lag) hipLaunchKernelGGL((k_mc_flow_lean_rda<true>), grid, block, 0, st, a, r.t_done, t_end);
            else if (lean) hipLaunchKernelGGL((k_mc_flow_lean_rda<false>), grid, block, 0, st, a, r.t_done, t_end);
            else if (r.short_ts) hipLaunchKernelGGL((k_mc_flow_rda<true>), grid, block, 0, st, a, r.t_done, t_end);
            else hipLaunchKernelGGL((k_mc_flow_rda<false>), grid, block, 0, st, a, r.t_done, t_end);
        } else if (pl->opt.tol) {
            if (lean && a.lag)
                hipLaunchKernelGGL((k_mc_flow_lean<true, true>), grid, block, 0, st, a, r.t_done, t_end);
            else if (lean)
                hipLaunchKernelGGL((k_mc_flow_lean<false, true>), grid, block, 0, st, a, r.t_done, t_end);
            else if (r.short_ts)
                hipLaunchKernelGGL((k_mc_flow<true, true>), grid, block, 0, st, a, r.t_done, t_end);
            else
                hipLaunchKernelGGL((k_mc_flow<false, true>), grid, block, 0, st, a, r.t_done, t_end);
        } else if (lean && a.lag)
            hipLaunchKernelGGL((k_mc_flow_lean<true>), grid, block, 0, st, a, r.t_done, t_end);
        else if (lean)
            hipLaunchKernelGGL((k_mc_flow_lean<false>), grid, block, 0, st, a, r.t_done, t_end);
        else if (r.short_ts)
            hipLaunchKernelGGL((k_mc_flow<true>), grid, block, 0, st, a, r.t_done, t_end);
        else
            hipLaunchKernelGGL((k_mc_flow<false>), grid, block, 0, st, a, r.t_done, t_end);
        HIP_TRY(hipEventRecord(pl->ev_chunk[which], st));
        pl->flow_last = which;
        if (flow_overlap(pl)) pl->flow_next = 1 - which;
        ++r.launches;
    }
    HIP_TRY(hipGetLastError());
    r.t_done = t_end;
    return 0;
}

int flow_route_end(trmc_plan *pl)
{
    RouteRun &r = pl->run;
    hipStream_t st = pl->stream;
    if (r.launches > 0) { // whatever the second compute stream still runs belongs to the window
        HIP_TRY(hipStreamWaitEvent(st, pl->ev_chunk[0], 0));
        if (flow_overlap(pl) && r.launches > 1) HIP_TRY(hipStreamWaitEvent(st, pl->ev_chunk[1], 0));
    }
    HIP_TRY(hipEventRecord(pl->ev[2], st));
    HIP_TRY(hipEventRecord(pl->ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));
    pl->flow_next = pl->flow_last = 0;
    int32_t both[16] = {0};
    HIP_TRY(hipMemcpy(both, pl->ticket.p, sizeof both, hipMemcpyDeviceToHost));
    const int32_t *flags = both[1] != 0 ? both : both + 8;
    if (flags[1] != 0) {
        r.active = false;
        const uint64_t idx = ((uint64_t)(uint32_t)flags[3] << 32) | (uint32_t)flags[2];
        const uint64_t np = (uint64_t)pl->nseg_pad;
        return fail(TRMC_EHIP, "dataflow engine: a row waited longer than the watchdog allows for an upstream flow "
                               "(boundary hydrographs missing for the steps routed, or an internal error); window abandoned"
                               " [waited for position " + std::to_string(idx % np) + " (" + (idx % np < (uint64_t)pl->sh->topo.nboundary ? "a boundary row" : "a routed row")
                               + ") at step " + std::to_string(idx / np) + ", tag " + std::to_string((uint32_t)flags[4]) + ", found tag "
                               + std::to_string((uint32_t)flags[5]) + ", window tag base " + std::to_string(pl->tag_base) + "]");
    }
    if (pl->opt.flow_debug && pl->sh->topo.nblocks > 0) { // developer aid: when did every block run?
        const int32_t nb = pl->sh->topo.nblocks;
        std::vector<unsigned long long> d((size_t)nb * 2);
        HIP_TRY(hipMemcpy(d.data(), pl->dbg.p, d.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::vector<uint32_t> cu_key(nb);
        for (int32_t b = 0; b < nb; ++b) { // (the start word carries the compute unit in its top 16 bits)
            cu_key[b] = (uint32_t)(d[2 * b] >> 48);
            d[2 * b] &= 0xffffffffffffull;
        }
        std::vector<unsigned long long> dx((size_t)nb * 4, 0ull); // per row group: 1 + SIMD + 256 * wavefront of the workgroup
        HIP_TRY(hipMemcpy(dx.data(), (unsigned long long *)pl->dbg.p + 2 * (size_t)(nb + 1), dx.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
        if (const char *path = std::getenv("TRMC_FLOW_DEBUG_FILE")) { // one line per block: id, compute unit, start, end (ms)
            if (FILE *f = std::fopen(path, "a")) {
                std::fprintf(f, "# launch of %d blocks\n", nb);
                for (int32_t b = 0; b < nb; ++b)
                {
                    std::fprintf(f, "%d %u %.5f %.5f", b, cu_key[b], d[2 * b] * 1e-5, d[2 * b + 1] * 1e-5);
                    for (int q = 0; q < kFlowBlock / 64; ++q) {
                        const size_t w = (size_t)b * (kFlowBlock / 64) + q;
                        std::fprintf(f, " %d", w < pl->sh->topo.cost_of_wave.size() ? (int)pl->sh->topo.cost_of_wave[w] : -1);
                    }
                    for (int q = 0; q < kFlowBlock / 64; ++q) std::fprintf(f, " %llu", dx[(size_t)4 * b + q]);
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
        }
        unsigned long long t_min = ~0ull, t_max = 0;
        for (int32_t b = 0; b < nb; ++b) {
            t_min = std::min(t_min, d[2 * b]);
            t_max = std::max(t_max, d[2 * b + 1]);
        }
        std::vector<int32_t> by_end(nb);
        for (int32_t b = 0; b < nb; ++b) by_end[b] = b;
        std::sort(by_end.begin(), by_end.end(), [&](int32_t x, int32_t y) { return d[2 * x + 1] > d[2 * y + 1]; });
        std::fprintf(stderr, "[flow debug] %d blocks, span %.3f ms; blocks ending last (id, start ms, end ms, duration ms):\n", nb,
                     (t_max - t_min) * 1e-5);
        for (int32_t i = 0; i < std::min(nb, 12); ++i) {
            const int32_t b = by_end[i];
            std::fprintf(stderr, "   %6d  %9.3f %9.3f %9.3f\n", b, (d[2 * b] - t_min) * 1e-5, (d[2 * b + 1] - t_min) * 1e-5,
                         (d[2 * b + 1] - d[2 * b]) * 1e-5);
        }
        // how many blocks are running at a few instants
        for (int k = 1; k <= 10; ++k) {
            const unsigned long long tt = t_min + (t_max - t_min) * k / 11;
            int32_t live = 0;
            for (int32_t b = 0; b < nb; ++b) live += d[2 * b] <= tt && d[2 * b + 1] > tt;
            std::fprintf(stderr, "   at %8.3f ms: %d blocks live\n", (tt - t_min) * 1e-5, live);
        }
    }
    float ms01 = 0, ms12 = 0;
    HIP_TRY(hipEventElapsedTime(&ms01, pl->ev[0], pl->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms12, pl->ev[1], pl->ev[2]));
    trmc_stats &s = pl->stats;
    s.nseg = pl->nseg;
    s.nseg_routed = pl->nrouted;
    s.nlevels = pl->sh->topo.nlevels;
    s.nsteps = r.nsteps;
    s.assume_short_ts = r.short_ts;
    s.main_launches = r.launches;
    s.segment_steps = pl->nrouted * (int64_t)r.nsteps;
    s.ms_prep = ms01;
    s.ms_main = ms12;
    s.ms_emit = 0.0; // results are written in the caller's layout by the routing kernel itself
    s.ms_total = (double)ms01 + ms12;
    s.wide_levels = s.wide_k = s.wide_launches = s.mid_levels = s.mid_k = s.mid_launches = 0;
    s.wide_segment_steps = 0;
    s.ms_wide = 0.0;
    s.arithmetic = pl->opt.tol ? TRMC_ARITH_TOLERANCE : TRMC_ARITH_EXACT;
    pl->routed_nsteps = r.nsteps;
    r.active = false;
    return 0;
}

