// kernels_levels.inc -- included by trmc.hip: the level engine's kernels (k_mc_step, k_mc_tile, k_mc_ctile) and the layout / product kernels.
// ---------------------------------------------------------------- kernels
// COLD kernel arguments.  hipcc reads the arguments a kernel uses into SGPRs at entry, in tuples of up to sixteen, and when
// the arithmetic of a step needs those registers (the power's double constants alone take forty) it parks the tuples in
// VGPR lanes and reads them back WHOLE -- eight v_readlane for one pointer -- wherever a member is used: the lean kernel
// executed some 120 of them per step (the tables of the rare branches, the watchdog of every poll loop, what the epilogue
// stores).  What the time loop needs only in rare branches or after its end is therefore read where it is used, through an
// opaque pointer to the kernel-argument segment: one scalar load from the constant cache, no register held across the loop.
// (The argument struct is the kernel's first parameter: offset 0 of the segment.)
template <class A> using ColdArgs = const __attribute__((address_space(4))) A *;
template <class A> __device__ __forceinline__ ColdArgs<A> cold_args()
{
    ColdArgs<A> p = (ColdArgs<A>)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
template <class T> struct StepArgs {
    const T *dx, *bw, *twcc, *n, *ncc, *s0;            // raw channel parameters the step still reads
    const T *z, *bfd, *sqrt_s0, *sq1pz2, *s0_n, *s0_ncc, *inv_n; // segment-invariant constants formed at plan time (k_make_const)
    const T *dt_col; // nullptr -> uniform dt
    T dt;
    const int32_t *up_ptr, *up_idx, *level;
    const int2 *up2; // first two upstream positions of every position (see k_mc_step)
    const int32_t *lag; // LAG form of the short-timestep kernel: position s is at step diag - lag[s]
    const T *qlat_tm;
    T *q_tm, *v_tm, *d_tm;
    uint8_t *it_prev; // secant iterations each position needed on the LAST step of the window (trmc_download_iterations)
    uint16_t *it_sum; // nullptr, or: sum over the window of min(iterations, 3) per position (trmc_plan_collect_cost)
    bool sane;        // every channel parameter of the plan lies in the range DevMathF::fast_ok's argument needs
    // level-pool reservoirs (nullptr = none): reservoir index of a position, parameters [nres][9],
    // inflow series [nres][nsteps] (the reference's upstream_array rows), routing period
    const int32_t *res_of_pos;
    const T *res_par;
    T *res_inflow;
    T res_dt;
    void *res_da; // nullptr, or the window's data-assimilation tables of those reservoirs (reservoir_da.hpp, trmc_set_reservoir_da)
    // streamflow nudging at gage positions (nullptr = off), tables [gage][nsteps], see trmc_set_nudging
    const int32_t *gage_of_pos;
    const uint8_t *da_mode;
    const T *da_a, *da_w;
    T *da_nudge;
    // gages INSIDE a reach, general mode only (trmc_set_nudging_successors): the segment below such a gage reads the gage
    // segment's flow of the current step as it was BEFORE the nudge (the reference nudges after the whole reach,
    // mc_reach.pyx:133-137,:761-796): raw_of_pos = gage whose raw flow a position reads (-1 = none), da_raw [gage][nsteps]
    const int32_t *raw_of_pos;
    T *da_raw;
    int64_t nseg_pad;
    int32_t nsteps, qts;
    // k_mc_tile writes its rows' results straight into the caller's layout out[row][step][q,v,d]
    T *out;
    const int32_t *row_of_pos;
    bool out_vec; // the runs it writes are 16-byte aligned (float, nsteps % 4 == 0, K % 4 == 0)
    // k_mc_tile: non-null = the threads of a block take the block's rows by descending cost class (see the kernel's prologue):
    // the class of every row at the last step it was routed in a tile, min(iterations, 3) + 4 if over bank
    uint8_t *cls_last;
    // k_mc_tile<.., DEC>: every dec_stride-th step of its rows' (q, v, d) also goes to dec[row][k][3], k = t / dec_stride - 1 <
    // dec_keep (trmc_plan_set_output_stride: what the reference's writers take of a window, written where it is produced)
    T *dec;
    int32_t dec_stride, dec_keep;
    // tile kernels: which steps' VELOCITY anybody is handed -- 0: every step (the full result is assembled, or nobody said otherwise);
    // n > 0: the multiples of n (a stream that keeps every n-th step of (q, v, d) and nothing else of it); < 0: none (a stream
    // whose products are hydrographs and final states).  The velocity feeds nothing: a step that is not handed on need not
    // form it (step_velocity: a division, a root, a logarithm and a power -- a tenth of a step's instructions).  Set by
    // stream_args for every stream begun without full_output (trmc_plan_options.velocity_on_demand < 0: left 0); != 0 only
    // where out == nullptr -- the LAZYV instances of the tile kernels assemble no full result.
    int32_t v_every;
    // k_mc_tile, hot rows: rows of class >= 3 at the end of a tile are routed by blocks of their own in the next one.  Three
    // lists of positions [3][hot_cap] and their lengths [3], used in turn: a launch reads `hot_cur`, appends to the next and
    // clears the length of the one after.  Who routes a listed row is settled by a STAMP, not by a byte both sides rewrite:
    // behind the lists, hot_list + 3 hot_cap, sit two columns of marks [2][nseg_pad]; a row appended to the list that launch
    // number n reads gets mark[n & 1][row] = n, and in launch n a block leaves exactly the rows whose mark[n & 1] is n to the
    // list's blocks.  Launch n writes column (n + 1) & 1 only, so what it reads cannot change under it: no row is routed twice.
    int32_t *hot_list, *hot_cnt;
    int32_t hot_cap, hot_cur, hot_home; // (hot_home: the launch's first so many blocks take the list, the ones behind them positions)
    int32_t hot_seq;                    // the number n >= 1 of this launch among the plan's launches that carry the lists
    int32_t hot_wave_rows;              // rows of the list per wavefront of those blocks (trmc_plan_options.hot_wave_rows)
    // STREAM of windows (trmc_stream_*; tile kernels only): the launch index counts tiles over ALL days -- a position `lag` tiles
    // behind works on tile (seq_day * seq_tpd + tile) - lag of the stream: day d = that / seq_tpd, in the buffers of slot d %
    // seq_slots (q_tm, d_tm, qlat_tm, out, dec: slot s begins s * slot_* elements behind the pointer above).  A row that ends a day
    // also writes its state into time row 0 of the next slot.  seq_slots <= 1: one window, no ring (everything above as it is).
    int32_t seq_slots, seq_tpd, seq_day, seq_days; // slots; tiles per day; day of the launch's tile index; days pushed so far
    int32_t seq_day_min;                           // days before this one have been queued to their end (trmc_stream_flush)
    int64_t slot_tm, slot_qlat, slot_out, slot_dec;
    // ... and, in a stream, the reservoirs' inflow record and the nudging tables of a row's day: res_inflow in slot s begins
    // s * slot_res elements behind the pointer, da_mode / da_a / da_w / da_nudge s * slot_da (0 in a single window).  COLD: read
    // inside the reservoir and gage branches only
    int64_t slot_res, slot_da;
    // ... and the reservoir data-assimilation tables of a row's day (the _rda instances; reservoir_da.hpp reservoir_da_row_day):
    // res_da in slot s begins s * slot_rda BYTES behind the pointer; the state lives outside the ring, res_da_carry [nres]
    // (nullptr: one window, the state lives in its tables); res_t_end = float(nsteps) * float(dt), what a day's end takes off the
    // times, rounded once on the host.  COLD
    void *res_da_carry;
    int64_t slot_rda;
    float res_t_end;
};

// which tile of which day a position `lag` tiles behind works on in a launch of the stream: false = none (before the first
// day, or behind the last one pushed)
template <class T>
__device__ __forceinline__ bool seq_locate(const StepArgs<T> &a, int32_t tile, int32_t lag, int32_t &behind, int32_t &slot, int32_t &slot_next)
{
    behind = tile - lag;
    slot = slot_next = 0;
    if (a.seq_slots <= 1) return behind >= 0;
    int32_t d = a.seq_day;
    while (behind < 0) {
        behind += a.seq_tpd;
        --d;
    }
    if (d < a.seq_day_min || d >= a.seq_days) return false;
    slot = d % a.seq_slots;
    slot_next = slot + 1 == a.seq_slots ? 0 : slot + 1;
    return true;
}

#include "k_tile_row.inc"

// One launch = one timestep (SHORT) or one wavefront diagonal (!SHORT) over the plan
// positions [s_begin, s_end); thread w of the launch takes position s_begin + w.
//
// Divergence control is the PLAN's business, not the kernel's: the secant loop runs 0 (no flow), 1 (depth below
// the 1 cm floor: early exit, f90:120-122), 2 (wet channel) or, rarely, 3+ iterations per segment-step, a segment
// repeats its count from one step to the next 99.3 % of the time, and a plan built with a cost hint
// (trmc_plan_create_hinted) stores the rows of a level grouped by that cost, so that a wavefront holds rows of one
// class.  (Rounds 1-2 also carried a per-block partition by the previous step's class for plans without a hint --
// ballots, a shuffle scan and three barriers; since the step's control flow got cheaper it cost more than the mixed
// wavefronts it avoided, 23.0 against 21.7 ms per CONUS day, and it is gone.)
#ifndef TRMC_STEP_BLOCK // threads per block of the step kernel (measured on MI355X, CONUS: 64 -> 100.4 us per launch,
// 128 -> 97.2, 192 -> 99.1, 256 -> 100.2, 512 -> 115.5, 1024 -> 132: small blocks free their wave slots sooner)
#define TRMC_STEP_BLOCK 128
#endif
constexpr int kStepBlock = TRMC_STEP_BLOCK;
#ifndef TRMC_EMIT_TILE // timesteps per overlapped transpose launch (a multiple of kEmitSteps).  The last tile's
// transpose trails the last step launch: CONUS day 22.3 ms with tiles of 128 steps, 21.7 with 64, 21.5 with 32
#define TRMC_EMIT_TILE 32
#endif
// The rows of a launch are routed by mc_step_rows; the kernels are thin instances of it.  RDA: the window has reservoir
// data-assimilation tables (StepArgs::res_da) -- kernels of their own (k_mc_step_rda), so that the ones every other window runs are
// compiled without the call: it would cost them registers and stack whether a table is there or not.
template <class T, bool SHORT, bool LAG, bool TOL, bool RDA>
__device__ __forceinline__ void mc_step_rows(const StepArgs<T> &a, int32_t s_begin, int32_t s_end, int32_t diag, int32_t ql_col);
template <class T, bool SHORT, bool LAG = false, bool TOL = false>
__global__ void __launch_bounds__(kStepBlock)
k_mc_step(const StepArgs<T> a, const int32_t s_begin, const int32_t s_end, const int32_t diag, const int32_t ql_col)
{
    mc_step_rows<T, SHORT, LAG, TOL, false>(a, s_begin, s_end, diag, ql_col);
}
template <bool SHORT, bool LAG = false>
__global__ void __launch_bounds__(kStepBlock)
k_mc_step_rda(const StepArgs<float> a, const int32_t s_begin, const int32_t s_end, const int32_t diag, const int32_t ql_col)
{
    mc_step_rows<float, SHORT, LAG, false, true>(a, s_begin, s_end, diag, ql_col);
}
template <class T, bool SHORT, bool LAG, bool TOL, bool RDA>
__device__ __forceinline__ void mc_step_rows(const StepArgs<T> &a, const int32_t s_begin, const int32_t s_end, const int32_t diag,
                                             const int32_t ql_col)
{   // ql_col: the lateral-inflow column (diag - 1) / qts of a launch whose rows are all at step diag (SHORT, no lag) -- formed
    // by the host: an integer division by a run-time divisor is some 35 instructions per thread
    using M = typename DevMath<T, TOL>::type;
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    // Issue priority over whatever else is resident: beside the wide tiles (k_mc_tile) these launches are the narrow tail of
    // the level order -- 288 launches that wait for each other, the critical path of the window -- and a wavefront of theirs
    // that shares its SIMD with four tile wavefronts at equal priority needs 43 us for a step it does in 20 us alone.  (Alone
    // on the device every wavefront has the same priority and nothing changes.)
    __builtin_amdgcn_s_setprio(3);
    M m{stage_pow_tables(s_tab), false};
    m.sane = a.sane;

    {
        const int32_t s = s_begin + (int32_t)blockIdx.x * kStepBlock + (int32_t)threadIdx.x;
        // (the block's rows dealt to its threads by the class of the step before, as k_mc_tile does once per K steps, was
        // built and measured here in round 5 -- some fifty instructions and four barriers per step: untuned plan 19.39 ms per
        // day against 19.44 without, tuned plan 16.15 against 16.09, tolerance arithmetic 13.5 against 12.4 -- and removed.
        // So were k_mc_tile's hot rows per STEP -- the rows of three or more iterations in the step before routed by the
        // launch's first blocks, an atomic append per hot row and launch: cost-ordered plan 16.67 ms per day against 16.2,
        // unordered 20.1 against 17.3 -- these launches are the window's dependent chain, and what lengthens one lengthens it.)
        if (s >= s_end) return;
        const int32_t t = SHORT ? (LAG ? diag - a.lag[s] : diag) : diag - a.level[s];
        if (t < 1 || t > a.nsteps) return;

        // 32-bit unsigned position: with uniform (SGPR) array bases every load below is
        // `global_load v, v_off, s[base]` with ONE shared byte offset instead of a 64-bit add per array
        const uint32_t su = (uint32_t)s;
        uint32_t ob = su * (uint32_t)sizeof(T); // byte offset of position s in any T column (nseg_pad * 8 < 2**32)
        const size_t row_p = (size_t)(t - 1) * (size_t)a.nseg_pad; // previous time level
        const size_t row_c = (size_t)t * (size_t)a.nseg_pad;       // current time level
        const T *const q_prev = a.q_tm + row_p;
        const T *const q_curr = a.q_tm + row_c;

        trmc::ChannelParams<T> p;
        trmc::ChannelConst<T> c;
        load_row_params(a, ob, p, c);

        trmc::Inflow<T> f;
        f.qdp = at(q_prev, ob);
        const T depthp = at(a.d_tm + row_p, ob);
        f.ql = at(a.qlat_tm + (size_t)((SHORT && !LAG) ? ql_col : (t - 1) / a.qts) * (size_t)a.nseg_pad, ob);

        // junction sums in the reference's order (mc_reach.pyx:499-502).  The first two upstream positions of a row
        // sit in a table of their own (-1 = none; bit 30 of the second = "the CSR list has more"): one load beside
        // the parameter loads instead of the dependent chain up_ptr -> up_idx -> q, and no loop for fan-in <= 2.
        T qup = T(0), quc = T(0);
        {
            const int2 u = a.up2[su];
            if (u.x >= 0) {
                const uint32_t ub = (uint32_t)u.x * (uint32_t)sizeof(T);
                qup += at(q_prev, ub);
                if (!SHORT) quc += at(q_curr, ub);
            }
            if (u.y >= 0) {
                const uint32_t ub = (uint32_t)(u.y & 0x3fffffff) * (uint32_t)sizeof(T);
                qup += at(q_prev, ub);
                if (!SHORT) quc += at(q_curr, ub);
                if (u.y & 0x40000000) {
                    const int32_t k1 = a.up_ptr[su + 1];
                    for (int32_t k = a.up_ptr[su] + 2; k < k1; ++k) {
                        const uint32_t uk = (uint32_t)a.up_idx[k] * (uint32_t)sizeof(T);
                        qup += at(q_prev, uk);
                        if (!SHORT) quc += at(q_curr, uk);
                    }
                }
            }
        }
        if (!SHORT && a.raw_of_pos) {
            const int32_t g = a.raw_of_pos[s];
            if (g >= 0) quc = a.da_raw[(size_t)g * (size_t)a.nsteps + (size_t)(t - 1)]; // (its one upstream row is that gage)
        }
        f.qup = qup;
        f.quc = SHORT ? qup : quc;

        if (a.res_of_pos) { // reference loop branch mc_reach.pyx:507-510,:551-553,:706-710
            const int32_t ri = a.res_of_pos[s];
            if (ri >= 0) {
                const T *rp = a.res_par + (size_t)ri * 9;
                const trmc::LevelPoolParams<T> lp{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8]};
                T H = depthp; // a reservoir row keeps its water elevation in the depth slot
                T outflow = trmc::levelpool_step<T, M>(f.quc, T(0), a.res_dt, H, lp, m);
                if constexpr (RDA) {
                    void *const da = cold_args<StepArgs<T>>()->res_da; // hybrid persistence / RFC series, mc_reach.pyx:555-703
                    const trmc::ResDaResult r = trmc::reservoir_da_row(da, ri, t, f.quc, depthp, a.res_dt, rp, outflow, H);
                    outflow = r.outflow;
                    H = r.water_elevation;
                }
                a.q_tm[row_c + s] = outflow;
                a.v_tm[row_c + s] = T(0);
                a.d_tm[row_c + s] = H;
                a.res_inflow[(size_t)ri * (size_t)a.nsteps + (size_t)(t - 1)] = f.quc;
                if (t == a.nsteps) a.it_prev[s] = 0;
                return;
            }
        }

        m.coef_ok = coef_guard(p.dt, f.ql);
        const trmc::StepResult<T> r = trmc::mc_segment_step<T, M>(p, c, f, depthp, m);
        T q_new = r.qdc;
        if (a.gage_of_pos) { // reference hook mc_reach.pyx:761-796; arithmetic of simple_da.pyx:47-76
            const int32_t g = a.gage_of_pos[s];
            if (g >= 0) {
                const size_t e = (size_t)g * (size_t)a.nsteps + (size_t)(t - 1);
                const uint8_t mode = a.da_mode[e];
                T nudge = T(0);
                if (!SHORT && a.da_raw) a.da_raw[e] = q_new;
                if (mode == 1) {            // valid observation: replace
                    nudge = a.da_a[e] - q_new;
                    q_new = a.da_a[e];
                } else if (mode == 2) {     // decay the last observation towards the model value
                    nudge = (a.da_a[e] - q_new) * a.da_w[e];
                    q_new = q_new + nudge;
                }
                a.da_nudge[e] = nudge;
            }
        }
        asm volatile("" : "+v"(ob));
        at(a.q_tm + row_c, ob) = q_new;
        at(a.d_tm + row_c, ob) = r.depthc;
        at(a.v_tm + row_c, ob) = r.velc;
        // (only trmc_download_iterations reads it, after the window: one byte-masked store per row and step would be
        // 3 % of the launch)
        if (t == a.nsteps) a.it_prev[su] = (uint8_t)min(r.iters, 255);
        // cost of the step for the plan's cost hint: the iteration class, plus 4 where the compound-channel branch ran
        // (a wavefront pays that branch -- two more divisions, one more power per evaluation -- as soon as one lane takes it)
        if (a.it_sum) a.it_sum[su] = (uint16_t)min(65535, (int)a.it_sum[su] + min(r.iters, 3) + (r.over ? 4 : 0));
    }
}

// The WIDE levels of a short-timestep window, K timesteps per launch, a row in ONE thread for all of them.
//
// With assume_short_ts a row at step t reads flows of step t - 1 only (mc_reach.pyx:504-505, :135-136).  So if level l
// of the network runs K steps BEHIND level l - 1, every flow a row reads during a tile of K steps was written by an
// EARLIER launch: launch `tile` routes level l through the steps ((tile - l) K, (tile - l + 1) K], and a row of that level
// reads its upstream rows (levels < l, hence at least K steps ahead) at steps it finds complete.  No flag, no poll, no
// barrier -- the kernel boundary is the only synchronisation -- and inside a launch a thread keeps its row's thirteen
// parameter / constant columns and its state (flow, depth) in registers, reads the forcing once per column and its
// upstream flows once per step, and writes (q, v, d) per step: 12 + 8 bytes of traffic per segment-step after the first
// instead of the 94 the one-step kernel moves, and no memory phase that the arithmetic of a 70-microsecond launch cannot hide.
// The level skew costs `wide - 1` partly filled launches at either end of the window; only levels wide enough to fill the
// device by themselves are routed this way (route_advance_t picks them), the narrow tail of the level order keeps the
// one-step launches of k_mc_step, trailing the last wide level.  Results are the same bits: the same segment steps on the
// same inputs, visited in another order (tests run both paths against the oracle).
// Results go straight into the caller's layout out[row][step][q,v,d]: a thread stages kTileStage steps in LDS (lane-
// contiguous columns: conflict-free) and writes them as one 96-byte run -- three whole 32-byte sectors -- so these rows
// need no transposing pass (k_emit skips them) and no velocity plane at all; of the time-major planes only the flow row
// of every step (what downstream rows and the gathers read) and the depth row of a tile's last step (where the row's next
// tile, or the final state, picks it up) are written.
#ifndef TRMC_TILE_PARTITION_UNHINTED
#define TRMC_TILE_PARTITION_UNHINTED 1
#endif
constexpr int kTileStage = 8;
#ifndef TRMC_TILE_BLOCK // threads per block of k_mc_tile: also the group its in-block partition deals rows in
#define TRMC_TILE_BLOCK 128
#endif
constexpr int kTileBlock = TRMC_TILE_BLOCK;
constexpr int32_t kWideMaxLevels = 64; // at most this many leading levels are routed by k_mc_tile (wide_levels, default 16, is capped by it)
// in-block partition of a tile's rows by cost class: on.  Measured on the CONUS sequence (ms per day, on / off): plan built from
// the topology alone 19.3 / 20.4, tuned plan on days whose forcing is drawn anew 19.8 / 20.8, tuned plan on its own kind of days
// 16.7 / 16.6, tolerance arithmetic 12.55 / 12.54 -- what a stale or missing cost hint loses, the partition wins back in part
constexpr bool kTilePartitionDefault(bool hinted) { return hinted || TRMC_TILE_PARTITION_UNHINTED; }
constexpr int32_t kMidMaxLevels = 32;  // ... and at most this many more by its second tier (mid_levels)
constexpr int64_t kMidDefaultRowsPerCu = 0; // default threshold of the second tier in rows per compute unit; 0 = off unless asked for
#ifndef TRMC_TILE_WAVES // wavefronts per SIMD the register allocation of k_mc_tile must allow.  Measured on the CONUS day by
// padding the blocks' LDS (TRMC_TILE_LDS_PAD) and by this cap: 1 wavefront per SIMD 36.7 ms, 2: 23.9, 3: 20.7, 3.5: 19.5,
// 4: 18.45, 5 (95 registers, 4 spilled): 17.9, 6 (80 registers, 27 spilled): 19.4 -- the curve of a kernel that hides its
// latencies with other wavefronts and is close to its issue limit at four
#define TRMC_TILE_WAVES 5
#endif
#ifndef TRMC_TILE_WAVES_LAZY // ... of the LAZYV instances (a stream without full_output: no velocity in the step loop, nothing
// staged unless DEC).  Registers per lane at 5 / 6 wavefronts (spilled): k_mc_tile 95 (2) / 80 (24), k_mc_ctile 89 (0) / 80 (9);
// the CONUS stream, median of five interleaved runs: 13.43 / 13.49 ms per day
#define TRMC_TILE_WAVES_LAZY TRMC_TILE_WAVES
#endif
#ifndef TRMC_HOT_WAVE_MAX // a wavefront with at least so many hot rows keeps them (k_mc_tile's epilogue); measured on the CONUS
// sequence, ms per day on the cost-ordered / the unordered plan: 6: 16.06 / 17.55, 16: 16.07 / 17.33, 40: 16.06 / 17.36
#define TRMC_HOT_WAVE_MAX 16
#endif
template <class T, bool TOL, bool DEC, bool LAZYV, bool RDA, bool PKD = false, bool DPL = false> // (see mc_step_rows; PKD: see k_mc_tile_pkd; DPL: k_mc_tile_dpl)
__device__ __forceinline__ void mc_tile_rows(const StepArgs<T> &a, int32_t s_begin, int32_t s_end, int32_t tile, int32_t K,
                                             T *pk_d = nullptr, int32_t *pk_at = nullptr);
template <class T, bool TOL = false, bool DEC = false, bool LAZYV = false> // (LAZYV: StepArgs::v_every != 0)
__global__ void __launch_bounds__(kTileBlock, sizeof(T) == 4 ? (LAZYV ? TRMC_TILE_WAVES_LAZY : TRMC_TILE_WAVES) : 1)
k_mc_tile(const StepArgs<T> a, const int32_t s_begin, const int32_t s_end, const int32_t tile, const int32_t K)
{
    mc_tile_rows<T, TOL, DEC, LAZYV, false>(a, s_begin, s_end, tile, K);
}
template <bool DEC>
__global__ void __launch_bounds__(kTileBlock, TRMC_TILE_WAVES)
k_mc_tile_rda(const StepArgs<float> a, const int32_t s_begin, const int32_t s_end, const int32_t tile, const int32_t K)
{
    mc_tile_rows<float, false, DEC, false, true>(a, s_begin, s_end, tile, K);
}
// PKD: THE ROW'S PEAK DEPTH OF THE DAY rides along (trmc_stream_set_summary, TRMC_SUMMARY_PEAK_DEPTH).  Every step's depth is in a
// register here and nowhere else -- the planes hold the depth of a tile's last step only -- so the row keeps (dmax, at) through
// its K steps: `peak = d[1], step = 1`, then `if (d[t] > peak) { peak = d[t]; step = t; }`, peak_flow's rule.  Between the tiles
// of a day they live in two columns of the row's slot, pk_d / pk_at [slots][nseg_pad] in plan order: read at the tile's start
// unless the tile begins the day (a slot's last occupant leaves nothing behind), written at its end; where the day is handed
// over k_stream_peak_depth puts them into row order.  Instances of their own (the LAZYV forms: a stream that assembles no full
// result; one that does reduces out[row][step][2]), so that every other instance compiles as it did.
template <class T, bool TOL = false, bool DEC = false>
__global__ void __launch_bounds__(kTileBlock, sizeof(T) == 4 ? TRMC_TILE_WAVES_LAZY : 1)
k_mc_tile_pkd(const StepArgs<T> a, const int32_t s_begin, const int32_t s_end, const int32_t tile, const int32_t K, T *const pk_d,
              int32_t *const pk_at)
{
    mc_tile_rows<T, TOL, DEC, true, false, true>(a, s_begin, s_end, tile, K, pk_d, pk_at);
}
// DPL: THE DEPTH PLANE (trmc_stream_set_stage).  A stream's slot has a time-major depth plane with room for every step beside its
// flow plane, and the instances above write the row of a tile's last step only (hand_on_row).  With DPL a row stores its depth of
// EVERY step there, next to the step's flow store and through the same address -- the flow row's element moved by the distance
// between the two planes, a launch constant -- so a wavefront writes 64 consecutive depths per step as it writes 64 consecutive
// flows.  The tile's last step is still hand_on_row's: no row stores it twice.  A reservoir row's depth is its pool's elevation.
// stream_complete_day gathers a row set's stage from the plane as it gathers its hydrographs from the flow plane.  Instances of
// their own, as PKD has (the LAZYV forms; PKD rides along where the stream asks for the peak depth too), so that every other
// instance compiles as it did.
template <class T, bool TOL = false, bool DEC = false, bool PKD = false>
__global__ void __launch_bounds__(kTileBlock, sizeof(T) == 4 ? TRMC_TILE_WAVES_LAZY : 1)
k_mc_tile_dpl(const StepArgs<T> a, const int32_t s_begin, const int32_t s_end, const int32_t tile, const int32_t K, T *const pk_d,
              int32_t *const pk_at)
{
    mc_tile_rows<T, TOL, DEC, true, false, PKD, true>(a, s_begin, s_end, tile, K, pk_d, pk_at);
}
template <class T, bool TOL, bool DEC, bool LAZYV, bool RDA, bool PKD, bool DPL>
__device__ __forceinline__ void mc_tile_rows(const StepArgs<T> &a, const int32_t s_begin, const int32_t s_end, const int32_t tile,
                                             const int32_t K, T *const pk_d, int32_t *const pk_at)
{
    using M = typename DevMath<T, TOL>::type;
    const ColdArgs<StepArgs<T>> cold = cold_args<StepArgs<T>>(); // (see cold_args: what the loop rarely needs is not kept in registers)
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    // (an instance that stages nothing -- LAZYV without DEC: a stream whose callers take products only -- declares one element)
    __shared__ T s_out[(DEC || !LAZYV) ? 3 * kTileStage * kTileBlock : 1]; // [step slot * 3 + c][thread]
    M m{stage_pow_tables(s_tab), false};
    m.sane = a.sane;

    int32_t s;
    bool from_hot = false;
    int32_t *const hot_list = a.cls_last ? cold->hot_list : nullptr;
    const int32_t hot_blocks = hot_list ? cold->hot_home : 0; // (the launch's FIRST blocks: the costliest rows start first)
    if ((int32_t)blockIdx.x < hot_blocks) {
        // HOT ROWS.  The first blocks of the launch take the list the tile before left: the rows that ended it in
        // class 3 or above -- three or more secant iterations, over bank; 1.5 % of the rows of an unordered CONUS plan, and one of
        // them in a wavefront makes all 64 lanes wait through its extra iterations (they sat in half of the wavefronts: 903
        // instructions per wavefront-step against 619 on the cost-ordered plan).  Gathered here they pace each other only.
        // Bookkeeping: a row appended to the list this launch reads was stamped with this launch's number at the same moment
        // (StepArgs::hot_seq, the mark columns behind the lists); its block leaves it alone on that stamp, which nothing in this
        // launch rewrites -- exactly one thread routes a row, whichever of the two gets to it first.
        // A wavefront of these blocks takes hot_wave_rows entries (its other lanes leave): a wavefront's step costs what its
        // costliest row's does, and where the launch does not fill the device many times over (a rank of a multi-GPU job) the
        // K dependent steps of its slowest wavefront ARE the launch -- sixteen rows per wavefront have a row of five or six
        // iterations among them a quarter as often as sixty-four.
        const int32_t cur = cold->hot_cur, cap = cold->hot_cap, H = cold->hot_wave_rows;
        const int32_t lane = (int32_t)(threadIdx.x & 63u), wave = (int32_t)blockIdx.x * (kTileBlock / 64) + (int32_t)(threadIdx.x >> 6);
        const int32_t i = wave * H + lane;
        const int32_t nlist = min(cold->hot_cnt[cur], cap);
        if (lane >= H || i >= nlist) return;
        if (lane == 0) atomicAdd(&cold->hot_cnt[3], min(nlist - i, H)); // (trmc_plan_hot_rows: a running total)
        s = hot_list[(size_t)cur * (size_t)cap + (size_t)i];
        from_hot = true;
        if (s < s_begin || s >= s_end) return; // (listed by a window whose tiled levels reached further: routed elsewhere now)
    } else {
        const int32_t home = (int32_t)blockIdx.x - hot_blocks;
        const int32_t s_mine = s_begin + home * kTileBlock + (int32_t)threadIdx.x;
        s = s_mine;
        if (a.cls_last) {
            // Which row a thread takes: the block's kTileBlock positions dealt out by DESCENDING cost class -- the class every row
            // showed at the end of the tile before (a row repeats its secant iteration count from step to step 99.3 % of the time)
            // -- so that a wavefront holds rows of one class whatever the forcing does and however old the plan's cost hint is.
            // Once per K steps, inside the launch: a count per class in LDS, a prefix over the eight classes, a scatter of lane
            // numbers.  (Until round 5 a launch of its own between the tiles, k_tile_perm, over groups of 256 positions: 13-25 us
            // of the tile stream per tile, 0.55 ms of a CONUS day spent between tiles.)  Order inside a class is whatever the
            // atomics give; results do not depend on which thread routes a row.  (A row stamped for this launch is the list's.)
            if (hot_list && home == 0 && threadIdx.x == 0) cold->hot_cnt[(cold->hot_cur + 2) % 3] = 0; // (the list after next)
            int32_t c = s_mine < s_end ? (int32_t)(a.cls_last[s_mine] & 0x7f) : 0x80;
            if (hot_list && s_mine < s_end) {
                const int32_t n = cold->hot_seq;
                if (hot_list[(size_t)3 * (size_t)cold->hot_cap + (size_t)(n & 1) * (size_t)a.nseg_pad + (size_t)s_mine] == n) c = 0x80;
            }
            const int32_t key = (c & 0x80) ? 8 : 7 - min(c, 7); // bucket 0 = the costliest; 8 = no row
            bool none;
            s = s_begin + home * kTileBlock + block_partition_by_class<kTileBlock>(key, none);
            if (none) return; // (behind the tier's last position, or routed by a block of the hot list)
        }
        if (s >= s_end) return;
    }
    int32_t behind, slot, slot_next;
    const bool in_range = seq_locate(a, tile, a.level[s], behind, slot, slot_next);
    const int32_t t_lo = behind * K + 1, t_hi = min(behind * K + K, a.nsteps);
    if (!in_range || t_lo > t_hi) return; // (not routed in this launch by anyone)
    // Issue priority by cost.  A launch cannot end before its slowest wavefront has made its K dependent steps, and a step of
    // rows that take three secant iterations or run over bank is some 2 200 instructions against 600-900 for the others: on a
    // device that the launch does not fill many times over (one rank of a multi-GPU job: five wavefronts per SIMD, all
    // resident at once) those wavefronts ARE the launch -- 12.5 us per step when they share their SIMD's issue slots equally
    // with four cheaper ones, measured as 200 us per launch of 16 steps whatever the number of rows.  So the costlier a
    // wavefront's rows showed themselves in the tile before, the higher its priority (the list's blocks: the highest).
    if (a.cls_last) {
        const int32_t cp = from_hot ? 7 : (int32_t)(a.cls_last[s] & 0x7f);
        if (__any(cp >= 3)) __builtin_amdgcn_s_setprio(3);
        else if (__any(cp == 2)) __builtin_amdgcn_s_setprio(1);
    }

    const uint32_t su = (uint32_t)s;
    uint32_t ob = su * (uint32_t)sizeof(T);
    const size_t np = (size_t)a.nseg_pad;
    trmc::ChannelParams<T> p;
    trmc::ChannelConst<T> c;
    load_row_params(a, ob, p, c);
    const int2 u = a.up2[su];
    const int32_t ri = a.res_of_pos ? a.res_of_pos[s] : -1;
    const int32_t gi = a.gage_of_pos ? a.gage_of_pos[s] : -1;

    // (a stream of windows: this row's day lives in its slot of the ring)
    T *const q_tm = a.q_tm + (size_t)slot * (size_t)a.slot_tm;
    const size_t ql_base = (size_t)slot * (size_t)a.slot_qlat;
    T q_prev = at(q_tm + (size_t)(t_lo - 1) * np, ob);
    T d_prev = at(a.d_tm + (size_t)slot * (size_t)a.slot_tm + (size_t)(t_lo - 1) * np, ob);
    T *const out_row = a.out + (size_t)slot * (size_t)a.slot_out + (size_t)a.row_of_pos[su] * (size_t)a.nsteps * 3;
    // the lateral-inflow column of step t is (t - 1) / qts: found by division once, by a counter from then on
    int32_t ql_col = (t_lo - 1) / a.qts, ql_left = a.qts - (t_lo - 1) % a.qts;
    T ql = at(a.qlat_tm + ql_base + (size_t)ql_col * np, ob);
    m.coef_ok = coef_guard(p.dt, ql); // (depends on the forcing column only: formed when that changes, not every step)
    const bool count_cost = a.it_sum != nullptr;
    int32_t it_acc = 0, it_last = 0, staged = 0;
    bool over_last = false;
    // flows of the step before (complete: earlier launches); advanced a row per step -- t differs from lane to lane (the
    // level skew), and (size_t)t * np in vector registers is a 64-bit multiplication per step
    T *q_up = q_tm + (size_t)(t_lo - 1) * np;
    const ptrdiff_t d_of_q = DPL ? a.d_tm - a.q_tm : 0; // (DPL: from a slot's flow plane to its depth plane, in elements)
    // (asking for the upstream flows of step t + 1 while step t is computed -- they were all written by earlier launches -- was built
    // and measured in round 6: the CONUS stream 14.3 ms per day against 13.9, the ranks of an 8-way partition 2.76 against 2.70: two
    // more live registers in a kernel that already spills four cost more than the L2 trip they take off the chain)
    // LAZYV: a stream that assembles no full result (a.out == nullptr).  The step's velocity is formed out of line, behind the
    // step's stores, and only at the steps whose velocity is kept (DEC); without DEC nothing is staged and none of it is compiled.
    const int32_t v_every = (LAZYV && DEC) ? cold->v_every : 0;
    int32_t v_left = v_every > 0 ? (v_every - 1) - ((t_lo - 1) % v_every) : 0; // steps before the next one whose velocity is wanted
    T dmax = T(0);
    int32_t dmax_at = 1;
    if constexpr (PKD) {
        if (t_lo != 1) { // (the day's earlier tiles of this row; step 1 starts the day's peak over)
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
        if (ql_left == 0) {
            ++ql_col;
            ql = at(cold->qlat_tm + ql_base + (size_t)ql_col * np, ob);
            m.coef_ok = coef_guard(p.dt, ql);
            ql_left = cold->qts;
        }
        --ql_left;
        // junction sum in the reference's order (mc_reach.pyx:499-502); see k_mc_step for the table of the first two
        T qup = T(0);
        if (u.x >= 0) qup += at(q_up, (uint32_t)u.x * (uint32_t)sizeof(T));
        if (u.y >= 0) {
            qup += at(q_up, (uint32_t)(u.y & 0x3fffffff) * (uint32_t)sizeof(T));
            if (u.y & 0x40000000) {
                const int32_t *const up_ptr = cold->up_ptr, *const up_idx = cold->up_idx;
                const int32_t k1 = up_ptr[su + 1];
                for (int32_t k = up_ptr[su] + 2; k < k1; ++k) qup += at(q_up, (uint32_t)up_idx[k] * (uint32_t)sizeof(T));
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
        hand_on_row<T>(cold, slot, slot_next, ob, np, t, t_hi, q_new, d_new);
        q_prev = q_new;
        d_prev = d_new;
        if constexpr (PKD) {
            if (t == 1 || d_new > dmax) { // (the first of equal peaks wins; a NaN never replaces a number)
                dmax = d_new;
                dmax_at = t;
            }
        }
        // (LAZYV: the velocity of a kept step, from the depth the step ended on -- what mc_segment_step forms; 0 where the step
        // had no flow, iters == 0, as there.  Nudging changes the flow only.)
        if (LAZYV && want_v && it_last > 0) v_new = trmc::step_velocity<T, M>(p, c, d_new, m);
        if (DEC || (!LAZYV && a.out)) { // stage (q, v, d) of step t; a run ends when kTileStage steps are staged and at the tile's last step
            // (a.out == nullptr: a stream of windows whose callers take products only -- nothing of the full result is assembled)
            T *so = s_out + (size_t)(staged * 3) * kTileBlock + threadIdx.x;
            so[0] = q_new;
            so[kTileBlock] = v_new;
            so[2 * kTileBlock] = d_new;
            ++staged;
            if (staged == kTileStage || t == t_hi) {
                T *dst = out_row + (size_t)(t - staged) * 3;
                const T *si = s_out + threadIdx.x;
                if (LAZYV || !a.out) {
                } else if (a.out_vec && (staged & 3) == 0) { // (float: 3 * staged values = 3 * staged / 4 pieces of 16 bytes)
                    for (int j = 0; j < 3 * staged / 4; ++j) {
                        float4 v;
                        v.x = (float)si[(4 * j + 0) * kTileBlock];
                        v.y = (float)si[(4 * j + 1) * kTileBlock];
                        v.z = (float)si[(4 * j + 2) * kTileBlock];
                        v.w = (float)si[(4 * j + 3) * kTileBlock];
                        reinterpret_cast<float4 *>(dst)[j] = v;
                    }
                } else {
                    for (int32_t e = 0; e < 3 * staged; ++e) dst[e] = si[e * kTileBlock];
                }
                if constexpr (DEC) {
                    // the kept steps among the ones just written, (t - staged, t]: the multiples of dec_stride, newest first
                    const int32_t ds = cold->dec_stride;
                    for (int32_t k = t / ds; k >= 1 && k * ds > t - staged; --k) {
                        if (k > cold->dec_keep) continue;
                        const int32_t kslot = k * ds - (t - staged) - 1;
                        T *dd = cold->dec + (size_t)slot * (size_t)cold->slot_dec + ((size_t)cold->row_of_pos[su] * (size_t)cold->dec_keep + (size_t)(k - 1)) * 3;
                        dd[0] = si[(kslot * 3 + 0) * kTileBlock];
                        dd[1] = si[(kslot * 3 + 1) * kTileBlock];
                        dd[2] = si[(kslot * 3 + 2) * kTileBlock];
                    }
                }
                staged = 0;
            }
        }
    }
    if constexpr (PKD) {
        const size_t col = (size_t)slot * np + (size_t)su;
        pk_d[col] = dmax;
        pk_at[col] = dmax_at;
    }
    if (t_hi == cold->nsteps) cold->it_prev[su] = (uint8_t)min(it_last, 255);
    if (uint8_t *const cls = cold->cls_last) {
        uint8_t c = (uint8_t)(min(it_last, 3) + (over_last ? 4 : 0));
        // (a row that has finished the window starts the next one in its block; and a wavefront that holds sixteen or more of
        // them -- the first blocks of every level of a cost-ordered plan -- keeps them: they pace each other where they are)
        const bool hot = hot_list && c >= 3 && (t_hi < cold->nsteps || cold->seq_slots > 1);
        if (hot && (from_hot || __builtin_popcountll(__ballot(hot)) < TRMC_HOT_WAVE_MAX)) {
            const int32_t nxt = (cold->hot_cur + 1) % 3, cap = cold->hot_cap;
            const int32_t i = atomicAdd(&cold->hot_cnt[nxt], 1);
            if (i < cap) {
                hot_list[(size_t)nxt * (size_t)cap + (size_t)i] = s;
                const int32_t n = cold->hot_seq + 1; // (the launch that reads that list)
                hot_list[(size_t)3 * (size_t)cap + (size_t)(n & 1) * (size_t)a.nseg_pad + (size_t)su] = n;
            }
        }
        cls[su] = c;
    }
    if (uint16_t *const it_sum = cold->it_sum) it_sum[su] = (uint16_t)min(65535, (int)it_sum[su] + it_acc);
}

#include "k_mc_ctile.inc"

// plan time: the segment-invariant constants of mc_segment.hpp::make_const, one thread per position,
// written as six more SoA columns behind the nine parameter columns (same device arithmetic the
// step kernel would otherwise repeat every timestep: 4 divisions and 2 square roots per segment-step)
constexpr int kConstCols = 7, kTotalCols = TRMC_NPARAM + kConstCols;
template <class T>
__global__ void __launch_bounds__(kBlock)
k_make_const(T *cols, int32_t nseg, int64_t nseg_pad)
{
    using M = typename DevMath<T>::type;
    const int32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= nseg) return;
    const M m{nullptr, false}; // make_const uses sqrt and divide only, never the power tables
    trmc::ChannelParams<T> p;
    p.dt = cols[(size_t)TRMC_P_DT * nseg_pad + s];
    p.dx = cols[(size_t)TRMC_P_DX * nseg_pad + s];
    p.bw = cols[(size_t)TRMC_P_BW * nseg_pad + s];
    p.tw = cols[(size_t)TRMC_P_TW * nseg_pad + s];
    p.twcc = cols[(size_t)TRMC_P_TWCC * nseg_pad + s];
    p.n = cols[(size_t)TRMC_P_N * nseg_pad + s];
    p.ncc = cols[(size_t)TRMC_P_NCC * nseg_pad + s];
    p.cs = cols[(size_t)TRMC_P_CS * nseg_pad + s];
    p.s0 = cols[(size_t)TRMC_P_S0 * nseg_pad + s];
    const trmc::ChannelConst<T> c = trmc::make_const<T, M>(p, m);
    T *o = cols + (size_t)TRMC_NPARAM * nseg_pad + s;
    o[0 * nseg_pad] = c.z;
    o[1 * nseg_pad] = c.bfd;
    o[2 * nseg_pad] = c.sqrt_s0;
    o[3 * nseg_pad] = c.sq1pz2;
    o[4 * nseg_pad] = c.s0_n;
    o[5 * nseg_pad] = c.s0_ncc;
    o[6 * nseg_pad] = c.inv_n;
}

// forcing: in[row][nq] (caller order) -> qlat_tm[j][pos]; LDS tile of 64 positions x 32 columns
template <class T>
__global__ void __launch_bounds__(kBlock)
k_prep_qlat(const T *__restrict__ in, const int32_t *__restrict__ row_of_pos, T *__restrict__ qlat_tm,
            int32_t nseg, int64_t nseg_pad, int32_t nq)
{
    __shared__ T tile[32][65];
    const int32_t p0 = blockIdx.x * 64;
    const int32_t j0 = blockIdx.y * 32;
    const int32_t nj = min(32, nq - j0);
    for (int32_t i = threadIdx.x; i < 64 * 32; i += kBlock) {
        const int32_t pl = i / 32, jl = i % 32;
        const int32_t p = p0 + pl;
        if (p < nseg && jl < nj) tile[jl][pl] = in[(size_t)row_of_pos[p] * nq + j0 + jl];
    }
    __syncthreads();
    for (int32_t i = threadIdx.x; i < 64 * 32; i += kBlock) {
        const int32_t jl = i / 64, pl = i % 64;
        const int32_t p = p0 + pl;
        if (p < nseg && jl < nj) qlat_tm[(size_t)(j0 + jl) * nseg_pad + p] = tile[jl][pl];
    }
}

// forcing from packed CHRTOUT columns: raw_a/raw_b [nq][nfeat] int32 (file order) -> qlat_tm[j][pos], decoding,
// the join on feature id (feat_of_pos) and the transposition in one pass.  Unpacking follows netCDF4-python's
// default read (nhd_io.py:397-434 get_ql_from_chrtout: masked where == _FillValue / missing_value or outside the
// valid range, filled with 0; otherwise raw * scale_factor + add_offset evaluated in double), the sum of the two
// variables in double, then the reference's cast to float32 (compute.py / qlat_sub.values.astype("float32")).
struct PackSpec {
    double scale, offset;
    int32_t fill1, fill2, vmin, vmax;
    int32_t use1, use2; // a fill value that is absent from the file arrives as NaN
};
__device__ __forceinline__ double unpack_cf(int32_t raw, const PackSpec &k)
{
    if ((k.use1 && raw == k.fill1) || (k.use2 && raw == k.fill2) || raw < k.vmin || raw > k.vmax) return 0.0;
    return (double)raw * k.scale + k.offset;
}
// THE RULE for one value: feature f (-1: the files do not hold the row, inflow 0) of the file whose columns begin at `col`
// (= j * nfeat).  Both ingest kernels call it, so a window and a stream day decode to the same bits.
template <class T>
__device__ __forceinline__ T ingest_packed_at(const int32_t *__restrict__ raw_a, const int32_t *__restrict__ raw_b, const PackSpec &ka,
                                              const PackSpec &kb, int32_t f, size_t col)
{
    double v = 0.0;
    if (f >= 0) {
        v = unpack_cf(raw_a[col + (size_t)f], ka);
        if (raw_b) v = v + unpack_cf(raw_b[col + (size_t)f], kb);
    }
    return (T)(float)v;
}
template <class T>
__global__ void __launch_bounds__(kBlock)
k_ingest_packed(const int32_t *__restrict__ raw_a, const int32_t *__restrict__ raw_b, const PackSpec ka, const PackSpec kb,
                const int32_t *__restrict__ feat_of_pos, T *__restrict__ qlat_tm, int32_t nseg, int64_t nseg_pad, int32_t nq,
                int64_t nfeat)
{
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const int32_t f = feat_of_pos[p];
    for (int32_t j = 0; j < nq; ++j)
        qlat_tm[(size_t)j * nseg_pad + p] = ingest_packed_at<T>(raw_a, raw_b, ka, kb, f, (size_t)j * (size_t)nfeat);
}
// The same for a DAY OF A STREAM (trmc_stream_push_day_packed), into the forcing area of the day's ring slot -- the layout
// k_prep_qlat leaves there.  A stream day is pushed while the tile launches of earlier days own the device, so the grid is cut along
// the columns as well: a thread decodes kIngestCols values of one position, its gathers independent of each other and in flight
// together; feat_of_pos is read coalesced (and again from the cache by the blocks of the other columns), the raw values by index,
// and a wavefront stores 64 consecutive positions of a column.
constexpr int32_t kIngestCols = 4;
template <class T>
__global__ void __launch_bounds__(kBlock)
k_ingest_packed_day(const int32_t *__restrict__ raw_a, const int32_t *__restrict__ raw_b, const PackSpec ka, const PackSpec kb,
                    const int32_t *__restrict__ feat_of_pos, T *__restrict__ qlat_tm, int32_t nseg, int64_t nseg_pad, int32_t nq,
                    int64_t nfeat)
{
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const int32_t f = feat_of_pos[p];
    const int32_t j0 = (int32_t)blockIdx.y * kIngestCols;
    T v[kIngestCols];
#pragma unroll
    for (int32_t k = 0; k < kIngestCols; ++k)
        v[k] = j0 + k < nq ? ingest_packed_at<T>(raw_a, raw_b, ka, kb, f, (size_t)(j0 + k) * (size_t)nfeat) : T(0);
#pragma unroll
    for (int32_t k = 0; k < kIngestCols; ++k)
        if (j0 + k < nq) qlat_tm[(size_t)(j0 + k) * nseg_pad + p] = v[k];
}

// initial state: time row 0 <- q0[row] = (qu0, qd0, h0)   (mc_reach.pyx:361)
template <class T>
__global__ void __launch_bounds__(kBlock)
k_init_state(const T *__restrict__ q0, const int32_t *__restrict__ row_of_pos, T *q_tm, T *v_tm, T *d_tm,
             int32_t nseg)
{
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const size_t r = (size_t)row_of_pos[p] * 3;
    q_tm[p] = q0[r + 0];
    v_tm[p] = q0[r + 1];
    d_tm[p] = q0[r + 2];
}

// boundary rows: prescribed hydrographs bfvd[b][t-1][c] -> time rows 1..nsteps at position b
template <class T>
__global__ void __launch_bounds__(kBlock)
k_fill_boundary(const T *__restrict__ bfvd, T *q_tm, T *v_tm, T *d_tm, int32_t nboundary, int32_t nsteps,
                int64_t nseg_pad)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)nboundary * nsteps) return;
    const int32_t b = (int32_t)(i / nsteps), t = (int32_t)(i % nsteps) + 1;
    const size_t src = ((size_t)b * nsteps + (t - 1)) * 3;
    const size_t dst = (size_t)t * nseg_pad + b;
    q_tm[dst] = bfvd[src + 0];
    v_tm[dst] = bfvd[src + 1];
    d_tm[dst] = bfvd[src + 2];
}

// result: time-major SoA -> out[row][t-1][3]; tile = 64 positions x kEmitSteps steps through LDS
// (32 steps: 24.8 KB of LDS per block -> 6 blocks per CU keep enough loads in flight; row chunks of
// 384 contiguous bytes on the store side)
#ifndef TRMC_EMIT_STEPS
#define TRMC_EMIT_STEPS 32
#endif
constexpr int kEmitSteps = TRMC_EMIT_STEPS;
// Index arithmetic is what this kernel's VALU instructions are, and it runs beside the VALU-bound step launches, so
// both passes are written to need little of it: a thread keeps ONE position through the load pass (its time-major
// addresses advance by a constant), and the store pass moves 16 bytes per lane -- a row's run of 32 steps is 24 such
// pieces, two rows per wave instruction -- when the result's rows are 16-byte aligned (nsteps % 4 == 0 in fp32).
template <class T>
__global__ void __launch_bounds__(kBlock)
k_emit(const T *__restrict__ q_tm, const T *__restrict__ v_tm, const T *__restrict__ d_tm,
       const int32_t *__restrict__ row_of_pos, T *__restrict__ out, int32_t nseg, int64_t nseg_pad,
       int32_t nsteps, int32_t t_begin, int32_t t_end, int32_t shift_from, int32_t shift, int32_t skip_lo, int32_t skip_hi)
{   // positions [skip_lo, skip_hi) have written their results themselves (k_mc_tile): they are passed over, and the whole
    // 64-position blocks inside that range are not launched at all (blocks from position shift_from on move up by `shift`)
    static_assert(kBlock == 256 && kEmitSteps % 4 == 0, "the passes below assume 4 waves and whole groups of 4 steps");
    constexpr int kRow = 3 * kEmitSteps + 4; // row stride in elements: a multiple of 4, so that 16-byte reads are aligned
    __shared__ __attribute__((aligned(16))) T tile[64][kRow]; // [position][step*3 + c]
    int32_t p0 = (int32_t)blockIdx.x * 64;
    if (p0 >= shift_from) p0 += shift;
    const int32_t t0 = t_begin + (int32_t)blockIdx.y * kEmitSteps; // zero-based output step
    const int32_t nt = min(kEmitSteps, t_end - t0);
    const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    {
        const int32_t p = p0 + lane;
        if (p < nseg && !(p >= skip_lo && p < skip_hi)) {
            size_t src = (size_t)(t0 + 1 + wave) * (size_t)nseg_pad + (size_t)p;
            T *dst = &tile[lane][wave * 3];
            for (int32_t tl = wave; tl < nt; tl += 4) {
                dst[0] = q_tm[src];
                dst[1] = v_tm[src];
                dst[2] = d_tm[src];
                src += 4 * (size_t)nseg_pad;
                dst += 12;
            }
        }
    }
    __syncthreads();
    const bool vec = sizeof(T) == 4 && nt == kEmitSteps && ((size_t)nsteps * 3 * sizeof(T)) % 16 == 0 && (t0 % 4) == 0;
    if (vec) {
        // 24 lanes per row (96 floats = 24 x 16 B), two rows per pass: lanes 0-23 and 24-47
        constexpr int kVecPerRow = 3 * kEmitSteps / 4;
        const int32_t half = lane / kVecPerRow, j = lane - half * kVecPerRow;
        if (half < 2) {
            for (int32_t pl = wave * 16 + half; pl < wave * 16 + 16; pl += 2) {
                const int32_t p = p0 + pl;
                if (p >= nseg) break;
                if (p >= skip_lo && p < skip_hi) continue;
                const float4 v = *reinterpret_cast<const float4 *>(&tile[pl][4 * j]);
                float4 *dst = reinterpret_cast<float4 *>(out + ((size_t)row_of_pos[p] * nsteps + t0) * 3);
                dst[j] = v;
            }
        }
    } else {
        for (int32_t pl = wave; pl < 64; pl += kBlock / 64) {
            const int32_t p = p0 + pl;
            if (p >= nseg) break;
            if (p >= skip_lo && p < skip_hi) continue;
            T *dst = out + ((size_t)row_of_pos[p] * nsteps + t0) * 3;
            for (int32_t e = lane; e < nt * 3; e += 64) dst[e] = tile[pl][e];
        }
    }
}

// (`qs`: element stride of the flow plane -- 1 for the time-major planes of the level engine, 2 for the granule plane
// of the dataflow engine, whose elements are {flow, tag} pairs; `d_tm` is then the depth-state column, d_row = 0)
template <class T>
__global__ void __launch_bounds__(kBlock)
k_final_state(const T *__restrict__ q_tm, const T *__restrict__ d_tm, const int32_t *__restrict__ row_of_pos,
              T *__restrict__ q0_out, int32_t nseg, int64_t nseg_pad, int32_t nsteps, int32_t qs, int32_t d_row)
{
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const size_t src = (size_t)nsteps * nseg_pad + p;
    const size_t r = (size_t)row_of_pos[p] * 3;
    const T q = q_tm[src * qs];
    q0_out[r + 0] = q;
    q0_out[r + 1] = q;
    q0_out[r + 2] = d_tm[(size_t)d_row * nseg_pad + p];
}

// A day's per-row summary from its slot's time-major flow plane (csrc/stream.inc: launched where the day is handed over, beside
// k_final_state): peak flow and the 1-based step it was first reached at, and the mean flow, written in ROW order.  One thread
// per plan position walks the time rows 1..nsteps, so a wavefront reads 64 consecutive flows of a time row per load.  The
// compares and the adds are a dependent chain in time order -- `>` keeps the first of equal peaks and never lets a NaN replace a
// number, the sum is the left-to-right one in T (np.cumsum) -- but the loads are independent: kSummaryUnroll of them are issued
// before the first is used.  `peak` (with `step`) or `mean` may be NULL.
constexpr int kSummaryUnroll = 8;
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_summary(const T *__restrict__ q_tm, const int32_t *__restrict__ row_of_pos, T *__restrict__ peak, int32_t *__restrict__ step,
                 T *__restrict__ mean, int32_t nseg, int64_t nseg_pad, int32_t nsteps)
{
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const T *q = q_tm + (size_t)nseg_pad + p; // (time row 1)
    T pk = q[0], s = pk;
    int32_t at = 1, t = 2;
    for (; t + kSummaryUnroll - 1 <= nsteps; t += kSummaryUnroll) {
        T v[kSummaryUnroll];
#pragma unroll
        for (int j = 0; j < kSummaryUnroll; ++j) v[j] = q[(size_t)(t - 1 + j) * (size_t)nseg_pad];
#pragma unroll
        for (int j = 0; j < kSummaryUnroll; ++j) {
            if (v[j] > pk) {
                pk = v[j];
                at = t + j;
            }
            s += v[j];
        }
    }
    for (; t <= nsteps; ++t) {
        const T v = q[(size_t)(t - 1) * (size_t)nseg_pad];
        if (v > pk) {
            pk = v;
            at = t;
        }
        s += v;
    }
    const size_t r = (size_t)row_of_pos[p];
    if (peak) {
        peak[r] = pk;
        step[r] = at;
    }
    if (mean) mean[r] = s / T(nsteps);
}

// A day's peak depth and its step in ROW order, beside k_stream_summary.  From the slot's two carry columns (k_mc_tile_pkd: plan
// order, one thread per position): boundary rows are routed by nobody and have no depth -- (0, 1), what the reduction below gives
// there, a full result holding zeros at those rows ...
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_peak_depth(const T *__restrict__ pk_d, const int32_t *__restrict__ pk_at, const int32_t *__restrict__ row_of_pos,
                    T *__restrict__ peak, int32_t *__restrict__ step, int32_t nseg, int32_t nboundary)
{
    const int32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= nseg) return;
    const size_t r = (size_t)row_of_pos[p];
    peak[r] = p < nboundary ? T(0) : pk_d[p];
    step[r] = p < nboundary ? 1 : pk_at[p];
}
// ... or, in a stream that assembles the full result, from out[row][step][2] of the day (one thread per row; the same compares in
// the same order on the same depths: the same bits)
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_peak_depth_out(const T *__restrict__ out, T *__restrict__ peak, int32_t *__restrict__ step, int32_t nseg, int32_t nsteps)
{
    const int32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nseg) return;
    const T *d = out + (size_t)r * (size_t)nsteps * 3 + 2;
    T pk = d[0];
    int32_t at = 1;
    for (int32_t t = 2; t <= nsteps; ++t) {
        const T v = d[(size_t)(t - 1) * 3];
        if (v > pk) {
            pk = v;
            at = t;
        }
    }
    peak[r] = pk;
    step[r] = at;
}

// The totals over the days of a stream (TRMC_SUMMARY_TOTAL): day `day`'s summary folded into the running values, [nseg] in row
// order, one thread per row.  Day 0 starts them; then `if (pk_D > pk) { pk = pk_D; step = D * nsteps + st_D; }` for the flow and
// for the depth, and the days' means summed left to right in T (the fetch divides by the number of days).  Any part may be NULL.
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_total(const T *__restrict__ pk_day, const int32_t *__restrict__ st_day, const T *__restrict__ mean_day,
               const T *__restrict__ pd_day, const int32_t *__restrict__ pds_day, T *__restrict__ pk, int64_t *__restrict__ st,
               T *__restrict__ mean_sum, T *__restrict__ pd, int64_t *__restrict__ pds, int32_t nseg, int64_t day, int32_t nsteps)
{
    const int32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nseg) return;
    const int64_t t0 = day * (int64_t)nsteps;
    if (pk_day) {
        const T v = pk_day[r];
        if (day == 0 || v > pk[r]) {
            pk[r] = v;
            st[r] = t0 + st_day[r];
        }
    }
    if (pd_day) {
        const T v = pd_day[r];
        if (day == 0 || v > pd[r]) {
            pd[r] = v;
            pds[r] = t0 + pds_day[r];
        }
    }
    if (mean_day) mean_sum[r] = day == 0 ? mean_day[r] : mean_sum[r] + mean_day[r];
}

template <class T>
__global__ void __launch_bounds__(kBlock)
k_gather_rows(const T *__restrict__ q_tm, const int32_t *__restrict__ pos, T *__restrict__ out, int64_t nrows,
              int64_t nseg_pad, int32_t nsteps, int32_t qs)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nrows * nsteps) return;
    const int64_t r = i / nsteps;
    const int32_t t = (int32_t)(i % nsteps) + 1;
    out[i] = q_tm[((size_t)t * nseg_pad + pos[r]) * qs];
}

// the depths of selected positions from a full result out[row][step][q, v, d]: out_rows[r][t - 1] (a stream day's stage where the
// stream assembles the full result: the same depths the depth plane of a stream without it holds)
template <class T>
__global__ void __launch_bounds__(kBlock)
k_gather_rows_depth_out(const T *__restrict__ out, const int32_t *__restrict__ pos, const int32_t *__restrict__ row_of_pos,
                        T *__restrict__ out_rows, int64_t nrows, int32_t nsteps)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nrows * nsteps) return;
    const int64_t r = i / nsteps;
    const int32_t t = (int32_t)(i % nsteps);
    out_rows[i] = out[((size_t)row_of_pos[pos[r]] * (size_t)nsteps + (size_t)t) * 3 + 2];
}

// flows of selected positions over the steps (t_begin, t_end]: out[r * stride + (t - 1 - t_begin)]
template <class T>
__global__ void __launch_bounds__(kBlock)
k_gather_range(const T *__restrict__ q_tm, const int32_t *__restrict__ pos, T *__restrict__ out, int64_t nrows,
               int64_t nseg_pad, int32_t t_begin, int32_t t_end, int64_t stride, int32_t qs)
{
    const int32_t w = t_end - t_begin;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nrows * w) return;
    const int64_t r = i / w;
    const int32_t k = (int32_t)(i % w);
    out[r * stride + k] = q_tm[((size_t)(t_begin + 1 + k) * nseg_pad + pos[r]) * qs];
}

// boundary positions (the first nboundary of the plan order) <- q[b * stride + (t - 1 - t_begin)], t in (t_begin, t_end]
template <class T>
__global__ void __launch_bounds__(kBlock)
k_fill_boundary_range(const T *__restrict__ q, T *q_tm, T *v_tm, T *d_tm, int32_t nboundary, int64_t nseg_pad,
                      int32_t t_begin, int32_t t_end, int64_t stride, const int64_t *__restrict__ src_index)
{
    const int32_t w = t_end - t_begin;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)nboundary * w) return;
    const int32_t b = (int32_t)(i / w), k = (int32_t)(i % w);
    const size_t dst = (size_t)(t_begin + 1 + k) * nseg_pad + b;
    q_tm[dst] = q[(size_t)(src_index ? src_index[b] : b) * stride + k]; // (src_index: which source row feeds boundary row b)
    v_tm[dst] = T(0);
    d_tm[dst] = T(0);
}

// independent single-segment steps: in[n][15] -> out[n][6] (with courant), cf. reach.pyx:66-103
template <class T, bool TOL = false>
__global__ void __launch_bounds__(kBlock)
k_segments(const T *__restrict__ in, T *__restrict__ out, int32_t *__restrict__ iters_out, int64_t n)
{
    using M = typename DevMath<T, TOL>::type;
    using MX = typename DevMath<T, false>::type; // (the segment-invariant constants are exact in either arithmetic, as in a plan: k_make_const)
    __shared__ uint64_t s_tab[TRMC_POW_TAB_WORDS];
    M m{stage_pow_tables(s_tab), false};
    const MX mx{s_tab, false};
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const T *x = in + i * 15;
    trmc::ChannelParams<T> p;
    trmc::Inflow<T> f;
    p.dt = x[0]; f.qup = x[1]; f.quc = x[2]; f.qdp = x[3]; f.ql = x[4];
    p.dx = x[5]; p.bw = x[6]; p.tw = x[7]; p.twcc = x[8]; p.n = x[9]; p.ncc = x[10];
    p.cs = x[11]; p.s0 = x[12];
    const T depthp = x[14];
    m.coef_ok = coef_guard(p.dt, f.ql);
    const trmc::ChannelConst<T> c = trmc::make_const<T, MX>(p, mx);
    const trmc::StepResult<T> r = trmc::mc_segment_step<T, M>(p, c, f, depthp, m);
    T ck, cn;
    trmc::courant_at<T, M>(r.h, p, c, ck, cn, m);
    T *o = out + i * 6;
    o[0] = r.qdc; o[1] = r.velc; o[2] = r.depthc; o[3] = ck; o[4] = cn; o[5] = r.X;
    if (iters_out) iters_out[i] = r.iters;
}

