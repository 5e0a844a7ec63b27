// host_levels.inc -- included by trmc.hip: a routing window on the level engine (route_begin_t / route_advance_t / route_end_t).

int quot_selfcheck(int device, bool *ok); // host_misc.inc

template <class T> T *col(trmc_plan *pl, int c) { return (T *)pl->sh->params.p + (size_t)c * pl->nseg_pad; }

template <class T> int upload_params(trmc_plan *pl, const float *params)
{
    const int64_t n = pl->nseg, np = pl->nseg_pad;
    std::vector<T> host((size_t)TRMC_NPARAM * np, T(0));
    const size_t all_cols = (size_t)kTotalCols * np;
    // a benign channel for the padding lanes (never routed, never read back)
    bool sane = true;
    auto in_range = [](float v) { return v >= 0x1p-14f && v <= 0x1p17f; };
    auto within = [](float v, float lo, float hi) { return v >= lo && v <= hi; };
    for (int64_t p = 0; p < n; ++p) {
        const float *src = params + (size_t)pl->sh->topo.row_of_pos[p] * TRMC_NPARAM;
        for (int c = 0; c < TRMC_NPARAM; ++c) host[(size_t)c * np + p] = (T)src[c];
        const float cs = src[TRMC_P_CS];
        // (the operands of those divisions are made of bw, the side slope, n, ncc, twcc and the depth only)
        sane = sane && in_range(src[TRMC_P_BW]) && in_range(src[TRMC_P_N]) && (cs == 0.0f || in_range(cs))
               && (src[TRMC_P_TWCC] == 0.0f || in_range(src[TRMC_P_TWCC])) && (src[TRMC_P_NCC] == 0.0f || in_range(src[TRMC_P_NCC]))
               // (... and the Muskingum K of an in-bank point of dt, dx, s0 too: DevMathF::k_of)
               && within(src[TRMC_P_DT], 0x1p-20f, 0x1p40f) && within(src[TRMC_P_DX], 0x1p-10f, 0x1p19f)
               && within(src[TRMC_P_S0], 0x1p-30f, 0x1p10f);
    }
    // (... and all of them stand on this device's refined reciprocal being the correctly rounded one: DevMathF::quot)
    bool quot_ok = false;
    if (int rc = quot_selfcheck(pl->device, &quot_ok)) return rc;
    pl->params_sane = sane && quot_ok && sizeof(T) == 4;
    if (int rc = pl->sh->params.ensure(all_cols * sizeof(T))) return rc;
    HIP_TRY(hipMemcpy(pl->sh->params.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    if (n > 0) {
        hipLaunchKernelGGL((k_make_const<T>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, pl->stream,
                           (T *)pl->sh->params.p, (int32_t)n, np);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(pl->stream));
    }
    return 0;
}

int upload_i32(DevBuf &b, const std::vector<int32_t> &v, size_t min_elems)
{
    const size_t n = v.size() > min_elems ? v.size() : min_elems;
    if (int rc = b.ensure(n * sizeof(int32_t))) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

int use_device(const trmc_plan *pl)
{
    HIP_TRY(hipSetDevice(pl->device));
    return 0;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// f(T()) with T the plan's element type
template <class F> inline int by_precision(const trmc_plan *pl, F &&f) { return pl->precision == 32 ? f(float()) : f(double()); }
// ... whose body is one launch: what it returns behind it
inline int launched()
{
    HIP_TRY(hipGetLastError());
    return 0;
}

// `v` grown to n events: ones that time (hipEventCreate) or ones that only order streams (hipEventDisableTiming)
inline int ensure_events(std::vector<DevEvent> &v, size_t n, bool timing)
{
    while (v.size() < n) {
        DevEvent e;
        if (int rc = e.ensure(timing)) return rc;
        v.push_back(std::move(e));
    }
    return 0;
}

// the stream the tiles run on (k_mc_tile, k_mc_ctile) and its "every tile queued so far is complete", made on first use.
// Ordinary priority: between the tail's step launches (high) and the result transpose (low); one hardware queue each
inline int ensure_tile_stream(trmc_plan *pl)
{
    if (int rc = pl->wstream.ensure(hipStreamNonBlocking)) return rc;
    return pl->ev_tail.ensure(false);
}

// a kernel that reads the result planes of the last window has just been queued on the plan's stream (outside a window)
int note_gather(trmc_plan *pl, bool also_in_window = false)
{
    if (pl->run.active && !also_in_window) return 0;
    return pl->mk_gather.record(pl->stream);
}

// ---- the utility kernels with more than one caller: each launched here alone, in the plan's precision, on the plan's stream

// NaN -> 0 in the `n` elements of a freshly uploaded block (trmc_plan_set_nan_is_zero)
int nan_to_zero(trmc_plan *pl, void *buf, int64_t n)
{
    return by_precision(pl, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_nan_to_zero<T>), dim3(blocks_for(n)), dim3(kBlock), 0, pl->stream, (T *)buf, n);
        return launched();
    });
}

// every stride-th step of `out`, the result of a window of T_ steps, into dst[row][nkeep][3]: of every row, or (rowset >= 0) of
// the rows of a registered set in the set's order
int decimate_out(trmc_plan *pl, void *dst, int32_t T_, int32_t stride, int32_t nkeep, int32_t rowset)
{
    return by_precision(pl, [&](auto t) {
        using T = decltype(t);
        const int64_t nrows = rowset < 0 ? pl->nseg : pl->rowset_n[(size_t)rowset];
        const dim3 grid(blocks_for(nrows * (int64_t)nkeep)), block(kBlock);
        if (rowset < 0)
            hipLaunchKernelGGL((k_decimate<T>), grid, block, 0, pl->stream, (const T *)pl->out.p, (T *)dst, nrows, T_, stride, nkeep);
        else
            hipLaunchKernelGGL((k_decimate_rows<T>), grid, block, 0, pl->stream, (const T *)pl->out.p, (T *)dst,
                               (const int32_t *)pl->rowsets[(size_t)rowset].p, (const int32_t *)pl->sh->row_of_pos.p, nrows, T_, stride, nkeep);
        return launched();
    });
}

// the flow hydrographs of `nrows` plan positions (on the device) over the T_ steps of the time-major planes, into dst[nrows][T_]
int gather_rows(trmc_plan *pl, const int32_t *positions_dev, void *dst, int64_t nrows, int32_t T_)
{
    return by_precision(pl, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_gather_rows<T>), dim3(blocks_for(nrows * T_)), dim3(kBlock), 0, pl->stream, (const T *)pl->tm.p, positions_dev,
                           (T *)dst, nrows, pl->nseg_pad, T_, pl->flow ? 2 : 1); // (the dataflow engine's plane holds granules of two)
        return launched();
    });
}

// diagnosis: slot `which` (0 tiles begin, 1 tiles end, 2 tail begins, 3 window ends) of the current window's stamps
inline void stamp(trmc_plan *pl, hipStream_t st, int which)
{
    if (!pl->stamps || pl->stamp_seq < 0) return;
    hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, st, pl->stamps + (size_t)(pl->stamp_seq % pl->nstamp_windows) * 4 + which);
}

template <class T> StepArgs<T> step_args(trmc_plan *pl, int nsteps, int qts)
{
    StepArgs<T> a;
    a.dt_col = pl->dt_uniform ? nullptr : col<T>(pl, TRMC_P_DT);
    a.dt = (T)pl->dt;
    a.dx = col<T>(pl, TRMC_P_DX);
    a.bw = col<T>(pl, TRMC_P_BW);
    a.twcc = col<T>(pl, TRMC_P_TWCC);
    a.n = col<T>(pl, TRMC_P_N);
    a.ncc = col<T>(pl, TRMC_P_NCC);
    a.s0 = col<T>(pl, TRMC_P_S0);
    a.z = col<T>(pl, TRMC_NPARAM + 0);
    a.bfd = col<T>(pl, TRMC_NPARAM + 1);
    a.sqrt_s0 = col<T>(pl, TRMC_NPARAM + 2);
    a.sq1pz2 = col<T>(pl, TRMC_NPARAM + 3);
    a.s0_n = col<T>(pl, TRMC_NPARAM + 4);
    a.s0_ncc = col<T>(pl, TRMC_NPARAM + 5);
    a.inv_n = col<T>(pl, TRMC_NPARAM + 6);
    a.dec = nullptr; // (set for the tile launches of a window that decimates as it goes: route_advance_t)
    a.dec_stride = a.dec_keep = 0;
    a.v_every = 0;
    a.hot_list = a.hot_cnt = nullptr;
    a.hot_cap = a.hot_cur = a.hot_home = a.hot_seq = 0;
    a.hot_wave_rows = 64;
    a.seq_slots = a.seq_tpd = a.seq_day = a.seq_days = a.seq_day_min = 0;
    a.slot_tm = a.slot_qlat = a.slot_out = a.slot_dec = 0;
    a.slot_res = a.slot_da = 0;
    a.res_da_carry = nullptr; // (a stream of days with reservoir data assimilation: stream_args)
    a.slot_rda = 0;
    a.res_t_end = 0.0f;
    a.up_ptr = (const int32_t *)pl->sh->up_ptr.p;
    a.up_idx = (const int32_t *)pl->sh->up_idx.p;
    a.up2 = (const int2 *)pl->sh->up2.p;
    a.level = (const int32_t *)pl->sh->level.p;
    a.lag = pl->maxlag > 0 ? (const int32_t *)pl->sh->lag.p : nullptr;
    a.it_prev = (uint8_t *)pl->it_prev.p;
    a.it_sum = pl->collect_cost ? (uint16_t *)pl->it_sum.p : nullptr;
    a.sane = pl->params_sane;
    a.res_of_pos = pl->nres > 0 ? (const int32_t *)pl->res_of_pos.p : nullptr;
    a.res_par = (const T *)pl->res_par.p;
    a.res_inflow = (T *)pl->res_inflow.p;
    a.res_dt = (T)pl->res_dt;
    a.res_da = (pl->nres > 0 && pl->res_da_on) ? pl->res_da.p : nullptr;
    const bool da = pl->ngage > 0;
    a.gage_of_pos = da ? (const int32_t *)pl->gage_of_pos.p : nullptr;
    a.da_mode = (const uint8_t *)pl->da_mode.p;
    a.da_a = (const T *)pl->da_a.p;
    a.da_w = (const T *)pl->da_w.p;
    a.da_nudge = (T *)pl->da_nudge.p;
    a.raw_of_pos = da && pl->nraw > 0 ? (const int32_t *)pl->raw_of_pos.p : nullptr;
    a.da_raw = da && pl->nraw > 0 ? (T *)pl->da_raw.p : nullptr;
    a.qlat_tm = (const T *)pl->qlat_tm.p;
    const size_t plane = (size_t)(nsteps + 1) * pl->nseg_pad;
    a.q_tm = (T *)pl->tm.p;
    a.v_tm = a.q_tm + plane;
    a.d_tm = a.v_tm + plane;
    a.nseg_pad = pl->nseg_pad;
    a.nsteps = nsteps;
    a.qts = qts;
    a.out = (T *)pl->out.p;
    a.row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
    a.out_vec = sizeof(T) == 4 && nsteps % 4 == 0 && pl->run.wide_k % 4 == 0;
    a.cls_last = nullptr; // (tile_args switches the in-block partition on for the tiles of a window or a stream)
    return a;
}

// rows of the hot list per wavefront of the blocks that route it (trmc_plan_options.hot_wave_rows)
// (fewer per wavefront -- so that a wavefront less often holds a row of five or six iterations -- was measured on the ranks of an
// 8-way CONUS partition, ms per day: 64: 2.70, 32: 2.82, 16: 3.03, 8: 2.86 -- more wavefronts of that cost, not a shorter chain)
inline int32_t hot_wave_rows_of(const trmc_plan *pl) { return pl->opt.hot_wave_rows > 0 ? pl->opt.hot_wave_rows : 64; }

// WHAT THE TILES OF A PLAN'S W WIDE LEVELS ARE LAUNCHED WITH, for a window (route_advance_t) and for a stream of days
// (stream.inc) alike -- both use the plan's one set of buffers and hand it on to each other: the in-block partition (rows dealt to
// the threads of every block of a tile by the cost class they showed in the tile before, k_mc_tile's prologue;
// trmc_plan_options.tile_perm_group: > 0 on, 0 off, < 0 by the plan's kind) and, with it unless switched off, the hot rows
// (trmc_plan_options.hot_rows).  tile_setup is idempotent: the buffers are made, and cleared, only where they are new (no history yet:
// one class) or the tier is of another size (the lists start empty, the marks are cleared).
// Hot rows measured on the CONUS sequence (ms per day, with / without): plan built from the topology alone 17.4 / 19.5; cost-ordered
// plan on its own kind of days 16.22 / 16.34 -- once the list's blocks were made the FIRST of the launch: behind the others (the
// costliest rows of all started last, every launch ended on them) it was 16.7 / 16.2 and 18.3 / 19.4.
inline bool tile_partition_on(const trmc_plan *pl)
{
    return pl->opt.tile_perm_group > 0 || (pl->opt.tile_perm_group < 0 && kTilePartitionDefault(pl->hinted));
}
inline bool tile_hot_rows_on(const trmc_plan *pl, int32_t W) { return tile_partition_on(pl) && pl->opt.hot_rows != 0 && W > 0; }
// ... the buffers (the only place that makes or clears them; what is queued goes to `st`) ...
inline int tile_setup(trmc_plan *pl, hipStream_t st, int32_t W)
{
    if (!tile_partition_on(pl)) return 0;
    const size_t np = (size_t)pl->nseg_pad;
    const bool fresh = pl->cls_last.bytes < np;
    if (int rc = pl->cls_last.ensure(np)) return rc;
    if (fresh) HIP_TRY(hipMemsetAsync(pl->cls_last.p, 0, np, st));
    if (!tile_hot_rows_on(pl, W)) return 0;
    const int32_t rows = pl->sh->topo.lvl_ptr[W] - pl->sh->topo.lvl_ptr[0];
    const int32_t cap = std::max<int32_t>(kTileBlock, (rows / 32 + kTileBlock - 1) / kTileBlock * kTileBlock);
    if (pl->hot_cap != cap || !pl->hot_list.p) {
        const size_t hl = ((size_t)3 * cap + 2 * np) * sizeof(int32_t); // (lists + the two mark columns, k_mc_tile)
        if (int rc = pl->hot_list.ensure(hl)) return rc;
        const bool first = !pl->hot_cnt.p;
        if (int rc = pl->hot_cnt.ensure(4 * sizeof(int32_t))) return rc;
        HIP_TRY(hipMemsetAsync(pl->hot_cnt.p, 0, (first ? 4 : 3) * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(pl->hot_list.p, 0, hl, st)); // (no stamp equals a launch number: they start at 1)
        pl->hot_cap = cap;
    }
    return 0;
}
// ... and the arguments of the launches behind a tile_setup for the same W (step_args left all of them switched off)
template <class T> inline void tile_args(const trmc_plan *pl, int32_t W, StepArgs<T> &a)
{
    if (tile_partition_on(pl)) a.cls_last = (uint8_t *)pl->cls_last.p;
    if (!tile_hot_rows_on(pl, W)) return;
    a.hot_list = (int32_t *)pl->hot_list.p;
    a.hot_cnt = (int32_t *)pl->hot_cnt.p;
    a.hot_cap = pl->hot_cap;
    a.hot_wave_rows = hot_wave_rows_of(pl);
    a.hot_home = (a.hot_cap + a.hot_wave_rows * (kTileBlock / 64) - 1) / (a.hot_wave_rows * (kTileBlock / 64));
}
// the turn of one launch that carries the lists: its number among the plan's, and which of the three lists it reads
template <class T> inline void tile_turn(trmc_plan *pl, StepArgs<T> &a)
{
    a.hot_seq = (int32_t)(pl->tile_seq & 0x3fffffff) + 1;
    a.hot_cur = (int32_t)(pl->tile_seq++ % 3);
}

// THE INSTANCE OF A STEP OR TILE KERNEL is chosen here and nowhere else: every launch function below hands its kernel family a
// set of std::integral_constant flags.  The rules: reservoir data assimilation (_rda) on exact fp32 plans only
// (trmc_set_reservoir_da sees to that), the tolerance arithmetic on precision-32 plans only (trmc_plan_create_opt), never both.
template <bool B> using flag = std::integral_constant<bool, B>;
template <class T, class Go> inline void with_arithmetic(const StepArgs<T> &a, bool tol, Go &&go) // go(rda, tol)
{
    if constexpr (sizeof(T) == 4) {
        if (a.res_da) return go(flag<true>{}, flag<false>{});
        if (tol) return go(flag<false>{}, flag<true>{});
    }
    go(flag<false>{}, flag<false>{});
}
// ... and of k_mc_tile / k_mc_ctile: go(rda, tol, dec, lazy).  dec: the launch writes the kept steps of a decimated result; lazy:
// velocity where it is handed on only -- the LAZYV instances assemble no full result, and the _rda instances have no LAZYV form
template <class T, class Go> inline void with_tile_instance(const StepArgs<T> &a, bool tol, Go &&go)
{
    const bool dec = a.dec != nullptr, lazy = a.v_every != 0 && !a.out;
    with_arithmetic(a, tol, [&](auto rda, auto tl) {
        auto by_dec = [&](auto lz) { dec ? go(rda, tl, flag<true>{}, lz) : go(rda, tl, flag<false>{}, lz); };
        if constexpr (rda()) by_dec(flag<false>{});
        else lazy ? by_dec(flag<true>{}) : by_dec(flag<false>{});
    });
}

template <class T, bool SHORT>
inline void launch_step(hipStream_t st, const StepArgs<T> &a, int32_t s0, int32_t s1, int32_t d, bool tol)
{
    const int64_t n = (int64_t)s1 - s0;
    const dim3 grid((unsigned)((n + kStepBlock - 1) / kStepBlock)), block(kStepBlock);
    with_arithmetic(a, tol, [&](auto rda, auto tl) {
        auto go = [&](auto lag) {
            if constexpr (rda()) hipLaunchKernelGGL((k_mc_step_rda<SHORT, lag()>), grid, block, 0, st, a, s0, s1, d, (d - 1) / a.qts);
            else hipLaunchKernelGGL((k_mc_step<T, SHORT, lag(), tl()>), grid, block, 0, st, a, s0, s1, d, (d - 1) / a.qts);
        };
        (SHORT && a.lag) ? go(flag<SHORT>{}) : go(flag<false>{});
    });
}
// one launch of k_mc_tile: positions [p0, p1), `tile` = launch index + the first level of the tier, K steps
// The rows' peak depth of the day (TRMC_SUMMARY_PEAK_DEPTH) rides in instances of its own, k_mc_tile_pkd / k_mc_ctile_pkd: a launch
// carries it when it is given the two columns (pk_d, pk_at: stream_launch) -- and only a launch of a LAZYV form is (tile_carries:
// trmc_stream_begin refuses or reduces the full result wherever that does not hold).  Without the columns: the instances above.
// The depth of every step into the slot's depth plane (trmc_stream_set_stage) rides in k_mc_tile_dpl / k_mc_ctile_dpl, by the same
// rule: a launch told so (dpl: stream_launch) and of a LAZYV form; the peak depth's columns go along where the stream has both.
template <class T> inline bool tile_carries(const StepArgs<T> &a) { return a.v_every != 0 && !a.out && !a.res_da; }
template <class T>
inline void launch_tile(hipStream_t st, const StepArgs<T> &a, int32_t p0, int32_t p1, int32_t tile, int32_t K, bool tol, T *pk_d = nullptr,
                        int32_t *pk_at = nullptr, bool dpl = false)
{
    // (with hot rows: the first a.hot_home blocks take the list, the blocks behind them positions)
    const unsigned home = (unsigned)((p1 - p0 + kTileBlock - 1) / kTileBlock);
    const dim3 grid(home + (a.hot_list ? (unsigned)a.hot_home : 0u)), block(kTileBlock);
    with_tile_instance(a, tol, [&](auto rda, auto tl, auto dec, auto lazy) {
        if constexpr (rda()) hipLaunchKernelGGL((k_mc_tile_rda<dec()>), grid, block, 0, st, a, p0, p1, tile, K);
        else if (dpl && tile_carries(a)) {
            if (pk_d) hipLaunchKernelGGL((k_mc_tile_dpl<T, tl(), dec(), true>), grid, block, 0, st, a, p0, p1, tile, K, pk_d, pk_at);
            else hipLaunchKernelGGL((k_mc_tile_dpl<T, tl(), dec(), false>), grid, block, 0, st, a, p0, p1, tile, K, pk_d, pk_at);
        } else if (pk_d && tile_carries(a)) hipLaunchKernelGGL((k_mc_tile_pkd<T, tl(), dec()>), grid, block, 0, st, a, p0, p1, tile, K, pk_d, pk_at);
        else hipLaunchKernelGGL((k_mc_tile<T, tl(), dec(), lazy()>), grid, block, 0, st, a, p0, p1, tile, K);
    });
}
// one launch of k_mc_ctile: the cluster blocks [b0, b1) of the plan at tile index `tile`
template <class T>
inline void launch_ctile(hipStream_t st, const StepArgs<T> &a, const int32_t *cblk_ptr, int32_t b0, int32_t b1, int32_t tile, int32_t K,
                         bool tol, T *pk_d = nullptr, int32_t *pk_at = nullptr, bool dpl = false)
{
    const dim3 grid((unsigned)(b1 - b0)), block(kCtileBlock);
    with_tile_instance(a, tol, [&](auto rda, auto tl, auto dec, auto lazy) {
        if constexpr (rda()) hipLaunchKernelGGL((k_mc_ctile_rda<dec()>), grid, block, 0, st, a, cblk_ptr, b0, tile, K);
        else if (dpl && tile_carries(a)) {
            if (pk_d) hipLaunchKernelGGL((k_mc_ctile_dpl<T, tl(), dec(), true>), grid, block, 0, st, a, cblk_ptr, b0, tile, K, pk_d, pk_at);
            else hipLaunchKernelGGL((k_mc_ctile_dpl<T, tl(), dec(), false>), grid, block, 0, st, a, cblk_ptr, b0, tile, K, pk_d, pk_at);
        } else if (pk_d && tile_carries(a)) hipLaunchKernelGGL((k_mc_ctile_pkd<T, tl(), dec()>), grid, block, 0, st, a, cblk_ptr, b0, tile, K, pk_d, pk_at);
        else hipLaunchKernelGGL((k_mc_ctile<T, tl(), dec(), lazy()>), grid, block, 0, st, a, cblk_ptr, b0, tile, K);
    });
}

// A routing window runs in three parts so that a caller can interleave other device work (the multi-GPU
// hand-off of cut-edge hydrographs, distributed.py) with it, everything asynchronous on the plan's stream:
//   route_begin_t    forcing transpose, initial state, boundary rows (if already staged)
//   route_advance_t  the step launches for the timesteps (t_done, t_end]
//   route_end_t      the rest of the result transpose, completion, timing
template <class T> int emit_tiles_through(trmc_plan *pl, int32_t t_complete) // all steps <= t_complete are queued
{
    // The result transpose (memory-bound) runs on a second stream, one time tile at a time, as soon as the
    // launches that complete the tile have been queued: it overlaps with the VALU-bound step kernels
    // instead of trailing them.
    constexpr int32_t kTile = TRMC_EMIT_TILE;
    RouteRun &r = pl->run;
    const int32_t n = (int32_t)pl->nseg, nsteps = r.nsteps;
    const int32_t ntiles = (nsteps + kTile - 1) / kTile;
    const size_t plane = (size_t)(nsteps + 1) * pl->nseg_pad;
    const T *q_tm = (const T *)pl->tm.p;
    while (r.tiles_done < ntiles && ((r.tiles_done + 1) * kTile <= t_complete || t_complete >= nsteps)) {
        // (with wide tiles: the tail, on the plan's stream, trails them -- its progress is everybody's; without a tail the
        // tile stream's is)
        HIP_TRY(hipEventRecord(pl->tile_ev[r.tiles_done], (r.wide > 0 && !r.tail_active) ? pl->wstream : pl->stream));
        HIP_TRY(hipStreamWaitEvent(pl->stream2, pl->tile_ev[r.tiles_done], 0));
        // (rows of the wide levels wrote their results themselves, k_mc_tile: their positions are left out)
        // (with cluster tiles every routed row has: only boundary rows are left to this pass)
        const int32_t skip_lo = (r.wide > 0 || r.cl) ? pl->sh->topo.lvl_ptr[0] : 0;
        const int32_t skip_hi = r.cl ? pl->sh->topo.lvl_ptr[pl->sh->topo.nlevels] : (r.wide > 0 ? pl->sh->topo.lvl_ptr[r.wide + r.mid] : 0);
        const int32_t shift_from = (skip_lo + 63) / 64 * 64, shift = std::max(0, (skip_hi - shift_from) / 64 * 64);
        const int32_t n_emit = n - shift;
        if (n_emit > 0) {
            const int32_t tb = r.tiles_done * kTile, te = min(nsteps, tb + kTile);
            hipLaunchKernelGGL((k_emit<T>), dim3((n_emit + 63) / 64, (unsigned)((te - tb + kEmitSteps - 1) / kEmitSteps)),
                               dim3(kBlock), 0, pl->stream2, q_tm, q_tm + plane, q_tm + 2 * plane,
                               (const int32_t *)pl->sh->row_of_pos.p, (T *)pl->out.p, n, pl->nseg_pad, nsteps, tb, te, shift_from, shift,
                               skip_lo, skip_hi);
        }
        ++r.tiles_done;
    }
    return 0;
}

template <class T> int route_begin_t(trmc_plan *pl, int nsteps, int qts, int short_ts)
{
    const trmc::Topology &tp = pl->sh->topo;
    const int32_t n = (int32_t)pl->nseg;
    const int64_t np = pl->nseg_pad;
    hipStream_t st = pl->stream;
    const size_t plane = (size_t)(nsteps + 1) * np;
    if (int rc = pl->tm.ensure(3 * plane * sizeof(T))) return rc;
    const bool qlat_early = pl->qlat_alt_ready; // (the staged forcing is in plan order already: the other buffer becomes this window's)
    if (qlat_early) std::swap(pl->qlat_tm, pl->qlat_alt);
    pl->qlat_alt_ready = false;
    if (int rc = pl->qlat_tm.ensure((size_t)pl->nq * np * sizeof(T))) return rc;
    if (int rc = pl->out.ensure((size_t)pl->nseg * nsteps * 3 * sizeof(T))) return rc;
    if (pl->nres > 0)
        if (int rc = pl->res_inflow.ensure((size_t)pl->nres * nsteps * sizeof(T))) return rc;
    if (pl->collect_cost) {
        if (int rc = pl->it_sum.ensure((size_t)np * sizeof(uint16_t))) return rc;
        pl->cost_nsteps = nsteps;
    }
    StepArgs<T> a = step_args<T>(pl, nsteps, qts);
    const int32_t *row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
    constexpr int32_t kTile = TRMC_EMIT_TILE;
    const int32_t ntiles = (nsteps + kTile - 1) / kTile;
    if (int rc = ensure_events(pl->tile_ev, (size_t)std::max(0, ntiles), false)) return rc;

    for (DevMark &m : pl->mk_released) { // a receiver of this plan's last window (trmc_plan_chain_from) has read what this window overwrites
        if (int rc = m.order(st)) return rc;
        if (pl->wstream)
            if (int rc = m.order(pl->wstream)) return rc;
        m.settle();
    }
    HIP_TRY(hipEventRecord(pl->ev[0], st));
    // Sequence mode (trmc_plan_options.sequence_mode): the window's set-up (forcing transpose, initial state, boundary rows)
    // goes to the TILE stream instead of the plan's own.  For one plan it is all the same; for two plans that take turns on a device (two ensemble
    // members) it is what lets the tiles of one member's next window start behind the other
    // member's tiles while that member's tail is still running: with one hardware queue per stream priority the two plans'
    // high-priority streams share a queue, in order of submission, and a set-up queued there would sit behind the other
    // member's 288 tail launches -- and the tiles behind the set-up.
    const bool setup_aside = pl->opt.sequence && short_ts && pl->wstream != nullptr;
    hipStream_t const plan_st = st;
    if (setup_aside) {
        st = pl->wstream;
        // the gathers queued on the plan's own stream since the last window (trmc_fetch_begin, trmc_gather_flow_rows, the
        // final state) read planes this window's tiles overwrite: the set-up goes behind the last of them (an event
        // recorded when that gather was queued -- not ev[0] above, which sits behind whatever another plan has put into
        // the shared high-priority queue since)
        if (int rc = pl->mk_gather.order(st)) return rc;
    }
    pl->mk_gather.settle(); // (on the plan's own stream the set-up is behind them as it is)
    if (int rc = pl->mk_dec.order(st)) return rc; // (trmc_fetch_begin_fvd: the copy stream reads `out`, which this window's kernels overwrite)
    pl->mk_dec.settle();
    if (int rc = pl->mk_forcing.order(st)) return rc; // (trmc_stage_forcing: the copy into in_qlat runs on the copy stream)
    pl->mk_forcing.settle();
    HIP_TRY(hipMemsetAsync(pl->it_prev.p, 0, (size_t)np, st)); // no history at the start of a window
    if (pl->collect_cost) HIP_TRY(hipMemsetAsync(pl->it_sum.p, 0, (size_t)np * sizeof(uint16_t), st));
    // every element the result reads is written below: time row 0 by k_init_state, rows 1..nsteps
    // of routed positions by k_mc_step and of boundary positions by k_fill_boundary (the padding
    // lanes of each row are never read), so the reference's zero fill (mc_reach.pyx:253) is moot
    if (n > 0) {
        if (!pl->qlat_direct && !qlat_early)
            hipLaunchKernelGGL((k_prep_qlat<T>), dim3((n + 63) / 64, (unsigned)((pl->nq + 31) / 32)), dim3(kBlock), 0, st,
                               (const T *)pl->in_qlat.p, row_of_pos, (T *)pl->qlat_tm.p, n, np, (int32_t)pl->nq);
        if (!pl->chain_staged) // (else: time row 0 was set on the device by trmc_plan_chain_from)
            hipLaunchKernelGGL((k_init_state<T>), dim3(blocks_for(n)), dim3(kBlock), 0, st, (const T *)pl->in_q0.p,
                               row_of_pos, a.q_tm, a.v_tm, a.d_tm, n);
    }
    pl->chain_staged = false;
    pl->q0_staged = false; // (consumed: the next staging gathers this window's final state)
    pl->row0_replaced = false;
    RouteRun &r = pl->run;
    r = RouteRun{};
    r.active = true;
    r.nsteps = nsteps;
    r.qts = qts;
    r.short_ts = short_ts ? 1 : 0;
    if (pl->stamps) ++pl->stamp_seq;
    r.boundary_through = tp.nboundary > 0 ? 0 : nsteps;
    if (tp.nboundary > 0 && pl->have_boundary) {
        hipLaunchKernelGGL((k_fill_boundary<T>), dim3(blocks_for(tp.nboundary * (int64_t)nsteps)), dim3(kBlock), 0, st,
                           (const T *)pl->in_bfvd.p, a.q_tm, a.v_tm, a.d_tm, (int32_t)tp.nboundary, nsteps, np);
        r.boundary_through = nsteps;
    }
    HIP_TRY(hipEventRecord(pl->ev[1], st));
    if (setup_aside) {
        st = plan_st;
        HIP_TRY(hipStreamWaitEvent(st, pl->ev[1], 0)); // the plan's stream continues behind the set-up
    }
    // Short-timestep windows of a wide network: the leading levels that can fill the device by themselves are routed K
    // steps per launch (k_mc_tile), the rest one step per launch behind them.  Needs every boundary hydrograph up front
    // (wide rows run ahead of the window's progress) and no lagged rows (the multi-GPU trunk has its own skew).
    // TRMC_WIDE_MIN_ROWS (rows a level must have, default 384 per compute unit; 0 switches the path off), TRMC_WIDE_LEVELS (at
    // most, default 16) and TRMC_WIDE_K (steps per launch, default 16) are measurement / test knobs.
    // Rows with a lag (the trunk of a cut basin riding in its owner's launches) and rows fed by boundary rows whose values
    // arrive chunk by chunk stay in the TAIL: the leading levels are only routed ahead if none of them is among their rows
    // (plans built for assume_short_ts keep such rows below level kWideMaxLevels: topology.hpp, boundary_floor).
    if (pl->wide_safe_pos < 0) { // first plan position that is lagged or reads a boundary row (host arrays; once per plan / lag)
        int64_t first = pl->nseg;
        for (int64_t p = tp.nboundary; p < pl->nseg && first == pl->nseg; ++p) {
            bool unsafe = pl->maxlag > 0 && !pl->lag_of_row.empty() && pl->lag_of_row[(size_t)tp.row_of_pos[p]] != 0;
            for (int32_t k = tp.up_ptr[p]; !unsafe && k < tp.up_ptr[p + 1]; ++k) unsafe = tp.up_idx[k] < tp.nboundary;
            if (unsafe) first = p;
        }
        pl->wide_safe_pos = first;
    }
    if (short_ts && pl->nrouted > 0) {
        // (measured on the CONUS day, MI355X, with every tile queued up front: levels of at least 32 768 rows -- eleven of them
        // -- and K = 12: 17.5 ms; eight levels 16.9; six 16.6; five 16.5 with K = 12 and 16.25 with K = 16; four 16.6; three 16.9;
        // K = 24: 17.0.  Fewer wide levels shorten the ramps of the level skew and give the tail launches more rows to fill the
        // device with after the last tile; the threshold that picks five levels there is 30 % of the rows the device holds at
        // five wavefronts per SIMD.  DESIGN.md lists what else was tried on this schedule.)
        const int64_t min_rows = pl->opt.wide_min_rows;
        int32_t W = 0, M = 0;
        const bool all_in_place = pl->maxlag == 0 && r.boundary_through == nsteps; // (then every level may run ahead)
        const int32_t level_cap = tp.ncl > 0 ? tp.cl_from_level : (tp.tail_from_level > 0 ? tp.tail_from_level : tp.nlevels); // (deeper rows are not in level slices)
        auto level_ok = [&](int32_t l, int64_t need) {
            return l < level_cap && tp.lvl_ptr[l + 1] - tp.lvl_ptr[l] >= need && (all_in_place || (int64_t)tp.lvl_ptr[l + 1] <= pl->wide_safe_pos);
        };
        if (min_rows > 0)
            while (W < std::min<int32_t>(pl->opt.wide_levels, kWideMaxLevels) && level_ok(W, min_rows)) ++W;
        // the second tier: the levels right below, fewer steps per launch (a skew of mid_k steps per level instead of wide_k)
        if (W > 0 && pl->opt.mid_min_rows > 0)
            while (M < pl->opt.mid_levels && level_ok(W + M, pl->opt.mid_min_rows)) ++M;
        // CLUSTER TILES (k_mc_ctile): a plan in cluster order (topology.hpp) routes its deeper rows K steps per launch too --
        // if, like the wide levels, they find every boundary hydrograph in place and carry no lag of their own.  The slices
        // are then exactly the plan's (the same rule picked them when the order was made).
        if (tp.ncl > 0 && all_in_place) {
            r.cl = true;
            W = tp.cl_from_level;
            M = 0;
        }
        if (W > 0 || r.cl) {
            r.wide = W;
            r.wide_k = std::max(1, std::min(nsteps, pl->opt.wide_k > 0 ? pl->opt.wide_k : std::max(1, std::min(16, nsteps / 8))));
            r.mid = M;
            r.mid_k = M > 0 ? std::max(1, std::min(r.wide_k, pl->opt.mid_k)) : 0;
            r.cl_next = W;
            if (int rc = ensure_tile_stream(pl)) return rc;
            HIP_TRY(hipStreamWaitEvent(pl->wstream, pl->ev[1], 0)); // the tiles start behind the window's set-up
            const size_t ntile = (size_t)std::max(1, (nsteps + r.wide_k - 1) / r.wide_k + W - 1);
            if (int rc = ensure_events(pl->wide_t0, ntile, true)) return rc; // (only the first is used: a tile starts where the one before it ended)
            if (int rc = ensure_events(pl->wide_t1, ntile, true)) return rc;
        }
    }
    HIP_TRY(hipGetLastError());
    pl->routed_nsteps = -1;
    return 0;
}

// what ends a window on the device -- the rest of the result transpose and the events the clock reads -- queued (once)
template <class T> int route_end_queue(trmc_plan *pl)
{
    RouteRun &r = pl->run;
    if (r.end_queued) return 0;
    hipStream_t st = pl->stream;
    stamp(pl, st, 3);
    HIP_TRY(hipEventRecord(pl->ev[2], st));
    if (int rc = emit_tiles_through<T>(pl, r.nsteps)) return rc; // whatever is left (at least the last tile)
    HIP_TRY(hipEventRecord(pl->ev_emit, pl->stream2));
    HIP_TRY(hipStreamWaitEvent(st, pl->ev_emit, 0));
    HIP_TRY(hipEventRecord(pl->ev[3], st));
    HIP_TRY(hipGetLastError());
    r.end_queued = true;
    return 0;
}

template <class T> int route_advance_t(trmc_plan *pl, int t_end)
{
    const trmc::Topology &tp = pl->sh->topo;
    RouteRun &r = pl->run;
    constexpr int32_t kTile = TRMC_EMIT_TILE;
    const int32_t nsteps = r.nsteps, t0 = r.t_done;
    StepArgs<T> a = step_args<T>(pl, nsteps, r.qts);
    hipStream_t st = pl->stream;
    if (pl->nrouted > 0) {
        const int32_t L = tp.nlevels;
        if (r.short_ts && (r.wide > 0 || r.cl)) {
            // wide levels: K steps per launch, level l trailing level l - 1 by K steps (k_mc_tile), on the TILE stream
            // (ordinary priority); the narrow tail of the level order: one step per launch (k_mc_step) on the plan's own
            // high-priority stream, behind the last wide level (an event per tile).  The tail is what the window waits for
            // -- 288 launches that depend on each other -- so it gets the issue slots first and the tiles, which are pure
            // throughput, fill the rest; with the priorities the other way round the tail fell 140 steps behind and ran
            // 2.4 ms past the last tile.  A tile is queued when the tail needs it; at the end of the call the plan's stream
            // waits for the tiles queued so far, so whatever the caller queues next (a gather, the next window) sees every
            // row at t_end.
            const int32_t K = r.wide_k, W = r.wide, M = r.mid, K2 = r.mid_k;
            const int32_t w0 = tp.lvl_ptr[0], w1 = tp.lvl_ptr[W], m1 = tp.lvl_ptr[W + M], s1 = tp.lvl_ptr[L];
            const int32_t nt = (nsteps + K - 1) / K;
            const int32_t ntile = W > 0 ? nt + W - 1 : 0;
            const int32_t nmid = M > 0 ? (nsteps + K2 - 1) / K2 + M - 1 : 0;
            const bool tail = s1 > m1 && !r.cl;
            const bool tol = pl->opt.tol;
            hipStream_t ws = pl->wstream;
            r.tail_active = tail || M > 0 || r.cl;
            // Every tile of the window is queued at once, at the window's first call: the wide path needs all boundary
            // hydrographs up front (route_begin_t), so a tile depends on nothing but the tile before it.  (Queued one by one
            // as the tail came to need them, the last tiles of a window were late -- the host runs only a little ahead of the
            // device once the runtime's pool of dependency signals is in use -- and the tail, the critical path, waited
            // 1.2 ms for them.)  One event per tile: it ends the tile for the clock (a tile starts where the one before it
            // ended; the first has a start event of its own) and it is what the tail waits for.
            // what the tiles of this window are launched with: the in-block partition and the hot rows (tile_setup: made and
            // cleared on the first call only), the decimated output
            StepArgs<T> at = a;
            if (r.cl) at.level = (const int32_t *)pl->sh->lagk.p; // (tiles every position runs behind: the level in the slices)
            if (pl->out_stride > 0 && nsteps / pl->out_stride >= 1) {
                r.dec_stride = pl->out_stride;
                r.dec_keep = nsteps / pl->out_stride;
                if (int rc = pl->dec.ensure((size_t)pl->nseg * r.dec_keep * 3 * sizeof(T))) return rc;
                at.dec = (T *)pl->dec.p;
                at.dec_stride = r.dec_stride;
                at.dec_keep = r.dec_keep;
                r.dec_lo = w0;
                r.dec_hi = r.cl ? s1 : m1;
            }
            if (int rc = tile_setup(pl, ws, W)) return rc;
            tile_args(pl, W, at);
            if (r.wide_next == 0 && W > 0) {
                stamp(pl, ws, 0);
                HIP_TRY(hipEventRecord(pl->wide_t0[0], ws));
                for (int32_t j = 0; j < ntile; ++j) {
                    tile_turn(pl, at);
                    launch_tile<T>(ws, at, w0, w1, j, K, tol);
                    HIP_TRY(hipEventRecord(pl->wide_t1[(size_t)j], ws));
                    ++r.launches;
                }
                stamp(pl, ws, 1);
                stamp(pl, st, 2);
                r.wide_next = ntile;
                r.wide_through = -1; // (from here on: the last tile the tail has been told to wait for)
            }
            if (r.wide_next == 0 && W == 0) { // (cluster tiles only: no slices, nothing on the tile stream)
                stamp(pl, st, 2);
                r.wide_next = -1;
                r.wide_through = -1;
            }
            auto wait_tile = [&](int32_t need) -> int { // the plan's stream behind wide tile `need` (once per tile)
                if (ntile > 0 && need > r.wide_through) {
                    HIP_TRY(hipStreamWaitEvent(st, pl->wide_t1[(size_t)std::min(need, ntile - 1)], 0));
                    r.wide_through = need;
                }
                return 0;
            };
            // The SECOND tier (levels W .. W + M - 1, K2 steps per launch, level l trailing level l - 1 by K2 steps): the same
            // kernel on the plan's own stream, in order with the tail's launches.  Launch j2 routes level W + m through the
            // steps ((j2 - m) K2, (j2 - m + 1) K2]; its rows read the wide rows (any level below W) one step behind, so it goes
            // behind the tile that completes the LAST wide level through step (j2 + 1) K2 - 1; level W + m has completed
            // step s after launch m + ceil(s / K2) - 1.
            StepArgs<T> am = a;
            am.out_vec = a.out_vec && K2 % 4 == 0 && sizeof(T) == 4 && nsteps % 4 == 0;
            if (r.dec_stride > 0) {
                am.dec = (T *)pl->dec.p;
                am.dec_stride = r.dec_stride;
                am.dec_keep = r.dec_keep;
            }
            auto mid_through = [&](int32_t j2_last) -> int { // queue the second tier's launches up to index j2_last
                for (; r.mid_next <= std::min(j2_last, nmid - 1); ++r.mid_next) {
                    const int32_t j2 = r.mid_next;
                    const int32_t s_need = std::min((j2 + 1) * K2, nsteps) - 1; // the wide rows' step the launch reads up to
                    if (s_need >= 1)
                        if (int rc = wait_tile((s_need - 1) / K + W - 1)) return rc;
                    launch_tile<T>(st, am, w1, m1, j2 + W, K2, tol);
                    ++r.launches;
                }
                return 0;
            };
            if (r.cl) {
                // CLUSTER TILES on the plan's own stream: tile j routes cluster level c (W + c tiles behind level 0) through the
                // steps ((j - W - c) K, (j - W - c + 1) K]; its rows read rows outside their cluster at least one tile ahead of
                // them -- the last slice is there after wide tile j - 1, every cluster level above after cluster tile j - 1 (this
                // stream).  Every row has reached step t after tile W + C - 1 + ceil(t / K) - 1.
                const int32_t C = tp.ncl;
                const int32_t te = std::min(t_end, nsteps);
                const int32_t j_end = te <= 0 ? W - 1 : W + C - 1 + (te + K - 1) / K - 1;
                const int32_t *cblk_ptr = (const int32_t *)pl->sh->cblk_ptr.p;
                StepArgs<T> ac = at;
                ac.hot_list = ac.hot_cnt = nullptr;
                for (; r.cl_next <= j_end; ++r.cl_next) {
                    const int32_t j = r.cl_next;
                    const int32_t c_lo = std::max(0, j - W - nt + 1), c_hi = std::min(C - 1, j - W);
                    if (c_lo > c_hi) continue;
                    if (j >= 1)
                        if (int rc = wait_tile(std::min(j - 1, ntile - 1))) return rc;
                    const int32_t b0 = tp.cblk_of_cl[(size_t)c_lo], b1 = tp.cblk_of_cl[(size_t)c_hi + 1];
                    if (b1 > b0) {
                        launch_ctile<T>(st, ac, cblk_ptr, b0, b1, j, K, tol);
                        ++r.launches;
                    }
                }
            }
            // (with lagged rows -- always in the tail, route_begin_t -- launch t routes the tail's other rows at step t and the
            // lagged ones at step t - maxlag, and the window ends at launch nsteps + maxlag: k_mc_step's LAG form)
            const int32_t lagmax = pl->maxlag;
            for (int32_t t = t0 + 1; t <= t_end && !r.cl; ++t) {
                const int32_t tn = std::min(t, nsteps);
                // the tail's step t reads the rows above it at step t - 1: the last level of the second tier is there after
                // launch M - 2 + ceil((t - 1) / K2) ...
                if (M > 0 && tn >= 2)
                    if (int rc = mid_through(M - 2 + (tn - 1 + K2 - 1) / K2)) return rc;
                if (tail) {
                    // ... and the last wide level after tile ceil((t - 1) / K) + W - 2 (and, with it, through step
                    // ceil((t - 1) / K) K: the tail waits once per K steps)
                    if (tn >= 2)
                        if (int rc = wait_tile((tn - 2) / K + W - 1)) return rc;
                    launch_step<T, true>(st, a, m1, s1, t, tol);
                    ++r.launches;
                }
                const int32_t t_all = t - lagmax; // every row has reached step t_all
                if (t_all > 0 && t_all % kTile == 0 && t_all < nsteps)
                    if (int rc = emit_tiles_through<T>(pl, t_all)) return rc;
            }
            // what the caller queues next on the plan's stream (a gather of cut-edge flows through t_end, the next window) must
            // see every WIDE row at t_end too: the tile that completes the last wide level through that step -- not every
            // tile queued, they are all queued up front and a chunk's hand-off must not wait for the window's last tile --
            // and every row of the second tier: its launches through the one that completes its last level
            {
                const int32_t te = std::min(t_end, nsteps);
                if (M > 0 && te >= 1)
                    if (int rc = mid_through(M - 2 + (te + K2 - 1) / K2)) return rc;
                const int32_t need_end = (te <= 0 || ntile == 0) ? -1 : std::min((te - 1) / K + W - 1, ntile - 1);
                if (need_end >= 0)
                    if (int rc = wait_tile(need_end)) return rc;
            }
        } else if (r.short_ts) {
            const int32_t s0 = tp.lvl_ptr[0], s1 = tp.lvl_ptr[L];
            const int32_t lagmax = pl->maxlag;
            for (int32_t t = t0 + 1; t <= t_end; ++t) { // launch t: rows at step t, lagged rows at step t - lagmax
                launch_step<T, true>(st, a, s0, s1, t, pl->opt.tol);
                ++r.launches;
                const int32_t t_all = t - lagmax; // every row has reached step t_all
                if (t_all > 0 && t_all % kTile == 0 && t_all < nsteps)
                    if (int rc = emit_tiles_through<T>(pl, t_all)) return rc;
            }
        } else {
            // level wavefront over the window (t0, t_end]: diagonal d runs (level l, step t0 + d - l)
            const int32_t W = t_end - t0;
            for (int32_t d = 1; d <= L - 1 + W; ++d) {
                const int32_t lo = d - W > 0 ? d - W : 0;
                const int32_t hi = d - 1 < L - 1 ? d - 1 : L - 1;
                const int32_t s0 = tp.lvl_ptr[lo], s1 = tp.lvl_ptr[hi + 1];
                if (s1 > s0) {
                    launch_step<T, false>(st, a, s0, s1, t0 + d, pl->opt.tol);
                    ++r.launches;
                }
                const int32_t t_all = t0 + d - (L - 1); // every level has reached step t_all
                if (t_all > t0 && t_all % kTile == 0 && t_all < nsteps)
                    if (int rc = emit_tiles_through<T>(pl, t_all)) return rc;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    r.t_done = t_end;
    // Sequence mode (several plans taking turns on a device, route_begin_t): the window's end is queued with its last launch,
    // so that what ANOTHER plan queues next in the shared hardware queues comes after it -- trmc_route_end then waits for this
    // plan's window only, not for the other plan's as well
    if (t_end >= r.nsteps + pl->maxlag && pl->opt.sequence)
        if (int rc = route_end_queue<T>(pl)) return rc;
    return 0;
}

template <class T> int route_end_t(trmc_plan *pl)
{
    const trmc::Topology &tp = pl->sh->topo;
    RouteRun &r = pl->run;
    const int32_t nsteps = r.nsteps;
    if (int rc = route_end_queue<T>(pl)) return rc;
    // (The STREAM, not the event behind the window's last launch: measured on the sequence with the decimated result among
    // the products -- 22.8 ms per day with the event against 19.5; 26.4 against 19.0 once the windows decimate as they go.  Behind a kernel queued after the window the stream's wait
    // returns when the OTHER plan's next window has ended; the host then queues every day a little late -- a pacing under which
    // the copies of consecutive days, 14 ms each on one PCIe direction, were observed not to run into each other.)
    HIP_TRY(hipStreamSynchronize(pl->stream));
    float ms01 = 0, ms12 = 0, ms23 = 0;
    HIP_TRY(hipEventElapsedTime(&ms01, pl->ev[0], pl->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms12, pl->ev[1], pl->ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms23, pl->ev[2], pl->ev[3]));
    trmc_stats &s = pl->stats;
    s.nseg = pl->nseg;
    s.nseg_routed = pl->nrouted;
    s.nlevels = tp.nlevels;
    s.nsteps = nsteps;
    s.assume_short_ts = r.short_ts;
    s.main_launches = r.launches;
    s.segment_steps = pl->nrouted * (int64_t)nsteps;
    s.ms_prep = ms01;
    s.ms_main = ms12;
    s.ms_emit = ms23;
    s.ms_total = (double)ms01 + ms12 + ms23;
    s.wide_levels = r.wide;
    s.wide_k = r.wide_k;
    s.wide_launches = std::max(0, r.wide_next);
    s.mid_levels = r.mid;
    s.mid_k = r.mid_k;
    s.mid_launches = r.mid_next;
    s.arithmetic = pl->opt.tol ? TRMC_ARITH_TOLERANCE : TRMC_ARITH_EXACT;
    s.wide_segment_steps = r.cl ? (int64_t)(tp.lvl_ptr[tp.nlevels] - tp.lvl_ptr[0]) * nsteps
                                : (r.wide > 0 ? (int64_t)(tp.lvl_ptr[r.wide + r.mid] - tp.lvl_ptr[0]) * nsteps : 0);
    s.ms_wide = 0.0;
    {
        const size_t timed_n = std::min<size_t>((size_t)std::max(0, r.wide_next), pl->wide_t0.size());
        for (size_t i = 0; i < timed_n; ++i) { // (a tile's clock starts where the previous tile's stopped)
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, i == 0 ? pl->wide_t0[0] : pl->wide_t1[i - 1], pl->wide_t1[i]));
            s.ms_wide += ms;
        }
        if (timed_n > 0 && (int64_t)timed_n < (int64_t)r.wide_next) s.ms_wide *= (double)r.wide_next / (double)timed_n;
    }
    pl->routed_nsteps = nsteps;
    pl->dec_stride_done = r.dec_stride;
    pl->dec_keep_done = r.dec_keep;
    pl->dec_nsteps_done = nsteps;
    pl->dec_lo_done = r.dec_lo;
    pl->dec_hi_done = r.dec_hi;
    r.active = false;
    return 0;
}

