/*
 * trmc.h -- C ABI of the MI355X-native Muskingum-Cunge routing engine
 * (libtrmc.so, built from t-route_amd/csrc/ for gfx950).
 *
 * This is the drop-in boundary for ONE reference path:
 *
 *   troute.routing.compute.compute_nhd_routing_v02
 *     -> troute.routing.fast_reach.mc_reach.compute_network_structured
 *        -> reach.muskingcunge -> c_muskingcungenwm (Fortran)
 *
 * Reference interfaces replaced (paths relative to the T-Route tree):
 *   [R1] src/troute-routing/troute/routing/fast_reach/mc_reach.pyx:164-224
 *        compute_network_structured(...)  -- whole-network, all timesteps
 *   [R2] src/troute-routing/troute/routing/fast_reach/reach.pyx:66-103
 *        compute_reach_kernel(...) -> dict  -- one segment, one timestep
 *   [R3] src/kernel/muskingum/pyMCsingleSegStime_NoLoop.f90:8-21 and
 *        src/troute-routing/troute/routing/fast_reach/pyMCsingleSegStime_NoLoop.h:1-21
 *        c_muskingcungenwm(21 float*)  -- the Fortran bind(c) symbol
 *   [R4] src/troute-network/troute/network/musking/mc_reach_structs.h:8-17,
 *        reach_structs.h:11-25  -- AoS _MC_Segment/_MC_Reach/_Reach, replaced
 *        by the plan's SoA columns + CSR upstream lists
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns 0 on success or a
 *     negative trmc_status and leaves a message in trmc_last_error()
 *     (thread-local).  The reference raises ValueError for shape errors
 *     (mc_reach.pyx:243-250); the Python shim maps TRMC_EINVAL to ValueError
 *     and everything else to RuntimeError.
 *   - "row" = position in the caller's segment table (the reference's
 *     data_idx order: ascending segment id, compute.py:1447-1461).
 *   - real arrays are float (precision 32) or double (precision 64), chosen at
 *     plan creation; the reference computes in float
 *     (src/kernel/muskingum/varPrecision.f90:5).
 *   - there is no CPU fallback: with no HIP device every entry point that
 *     computes fails with TRMC_ENODEVICE.
 */
#ifndef TRMC_H
#define TRMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRMC_ABI_VERSION 19

typedef enum trmc_status {
    TRMC_OK = 0,
    TRMC_EINVAL = -1,    /* bad argument / shape mismatch  -> ValueError     */
    TRMC_ECYCLE = -2,    /* upstream graph is not acyclic  -> ValueError     */
    TRMC_ENODEVICE = -3, /* no usable HIP device           -> RuntimeError   */
    TRMC_EHIP = -4,      /* HIP runtime error              -> RuntimeError   */
    TRMC_ENOMEM = -5,    /* allocation failed              -> MemoryError    */
    TRMC_ESTATE = -6,    /* call order violated (e.g. download before route) */
    TRMC_EUNSUPPORTED = -7 /* a combination that is not built  -> NotImplementedError */
} trmc_status;

/* Parameter column order of `params` (9 columns, row-major [nseg][9]): the
 * order column_mapper produces for the reference kernel, mc_reach.pyx:150-162 */
enum { TRMC_P_DT = 0, TRMC_P_DX, TRMC_P_BW, TRMC_P_TW, TRMC_P_TWCC, TRMC_P_N,
       TRMC_P_NCC, TRMC_P_CS, TRMC_P_S0, TRMC_NPARAM };

typedef struct trmc_plan trmc_plan;

/* Per-route timing and shape facts, filled by trmc_route_device().  Times are
 * HIP-event times on the plan's own stream. */
typedef struct trmc_stats {
    int64_t nseg;            /* rows in the plan (incl. boundary rows)        */
    int64_t nseg_routed;     /* rows that are computed                         */
    int32_t nlevels;         /* topological depth in segments                  */
    int32_t nsteps;          /* timesteps of the last route                    */
    int32_t assume_short_ts;
    int32_t main_launches;   /* launches of the segment-step kernel            */
    int64_t segment_steps;   /* nseg_routed * nsteps                           */
    double ms_prep;          /* forcing transpose + initial-state scatter      */
    double ms_main;          /* all launches of the segment-step kernel        */
    double ms_emit;          /* [t][seg] -> [row][t][q,v,d] transpose          */
    double ms_total;         /* prep + main + emit                             */
    /* short-timestep windows of a wide network: the leading `wide_levels` levels are routed `wide_k` timesteps per
     * launch by k_mc_tile (0: every level one step per launch) */
    int32_t wide_levels, wide_k;
    int32_t wide_launches;   /* launches of k_mc_tile (part of main_launches)  */
    int32_t mid_levels;      /* ... and the `mid_levels` levels right below them `mid_k` steps per launch (second tier; 0: none) */
    int64_t wide_segment_steps; /* segment-steps routed by the launches of both tiers */
    double ms_wide;          /* summed duration of the first tier's launches (they run beside the tail's, so this is not a share of ms_main) */
    int32_t mid_k, mid_launches;
    int32_t arithmetic;      /* TRMC_ARITH_EXACT / TRMC_ARITH_TOLERANCE of the plan */
    int32_t reserved0;
} trmc_stats;

const char *trmc_last_error(void);
int trmc_abi_version(void);
int trmc_device_count(int *count);

/*
 * Build a routing plan: topology flattened to segment levels, parameters laid
 * out as SoA columns in level-major order, everything resident in HBM.
 * Replaces the MC_Segment/MC_Reach object construction of [R1]
 * (mc_reach.pyx:283-378) and [R4].
 *
 *   nseg      rows
 *   up_ptr    [nseg+1] CSR offsets; up_idx[up_ptr[r]..up_ptr[r+1]) are the rows
 *             whose flow enters row r, IN THE ORDER THE REFERENCE SUMS THEM
 *             (mc_reach.pyx:499-502: upstream_connections[reach[0]] for the
 *             head of a reach, the previous segment inside a reach)
 *   params    [nseg][TRMC_NPARAM] float (always float: compute.py:549)
 *   boundary  [nseg] or NULL; 1 marks a row that is not routed but
 *             carries a prescribed hydrograph (the reference's
 *             upstream_results rows, mc_reach.pyx:451-469); 2 marks a
 *             ROUTED row that a short-timestep plan of the level engine
 *             keeps out of its leading levels -- the ones routed several
 *             timesteps per launch ahead of the window -- like the rows
 *             boundary rows feed (rows that will carry a lag,
 *             trmc_plan_set_lag); results do not depend on it
 *   precision 32 or 64
 *   device    HIP device ordinal
 */
int trmc_plan_create(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx,
                     const float *params, const uint8_t *boundary, int precision,
                     int device, trmc_plan **out);
/* The same with a per-row cost hint [nseg] (or NULL): the secant iterations each row needed at the end of an
 * earlier window (trmc_download_iterations).  Inside a level the order of the rows is free; with a hint rows of equal
 * cost sit together (wavefronts of one cost) and the costly blocks of a launch start first.  Results do not depend
 * on the hint.  No counterpart in the reference (its reach lists are traversed serially). */
int trmc_plan_create_hinted(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx,
                            const float *params, const uint8_t *boundary, const uint8_t *cost_hint,
                            int precision, int device, trmc_plan **out);
/* The same with flags: which engine runs the plan, and which timestep mode it is meant for.
 *   engine  TRMC_ENGINE_LEVELS   level engine: rows in level-major order, one launch per timestep (assume_short_ts) or per
 *                                wavefront diagonal (k_mc_step); the only engine of precision-64 plans
 *           TRMC_ENGINE_FLOW     dataflow engine (precision 32): rows in block order, one persistent launch per window,
 *                                rows exchange flows through tagged granules (k_mc_flow)
 *           TRMC_ENGINE_AUTO     flow, except for a precision-32 plan of 1 000 000 routed rows or more that is meant for
 *                                assume_short_ts: there every launch fills the device many times over and wavefronts
 *                                that are uniform in cost across a whole level outweigh the launch boundaries
 *   mode    TRMC_PLAN_SHORT_TS / TRMC_PLAN_FULL_TS: the assume_short_ts value the plan will be routed with, if the caller
 *           knows it (compute_nhd_routing_v02 does).  A plan routes correctly in either mode whatever it was built for;
 *           the flag chooses the row order that is fast for that mode (block order with cost tiers for the first, plain
 *           sub-tree blocks for the second and when unknown).
 * (troute_amd.plan maps the environment variable TRMC_ENGINE=levels|flow onto the engine flag of an "auto" plan: A/B runs.) */
enum { TRMC_ENGINE_AUTO = 0, TRMC_ENGINE_LEVELS = 1, TRMC_ENGINE_FLOW = 2, TRMC_ENGINE_MASK = 3,
       TRMC_PLAN_SHORT_TS = 4, TRMC_PLAN_FULL_TS = 8 };
int trmc_plan_create_ex(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx,
                        const float *params, const uint8_t *boundary, const uint8_t *cost_hint,
                        int precision, int device, int flags, trmc_plan **out);
/* The same with OPTIONS (since ABI 16): everything that used to be an environment variable read inside the library is a
 * field here, read ONCE when the plan is created (a clone inherits them).  A NULL pointer or a zero-filled struct means
 * the defaults; struct_size = sizeof(trmc_plan_options) lets the struct grow.  The library itself reads no environment
 * variable that decides how a plan routes (the Python host layer maps its documented TRMC_* test / measurement variables
 * onto this struct, troute_amd/plan.py).
 *   arithmetic     TRMC_ARITH_EXACT (0): every segment-step bit-identical to the reference Fortran (fp32: glibc's powf
 *                  restated, IEEE division and square root; fp64: glibc's pow restated).
 *                  TRMC_ARITH_TOLERANCE (1), precision 32 only: hardware log2 / exp2 power, reciprocal-multiply division,
 *                  hardware square root -- each within one unit in the last place, NOT bit-comparable.  Stated tolerance
 *                  against the reference Fortran (tests/test_gpu_tolerance.py asserts it, profiles/r05_tolerance_report.json
 *                  holds the measured distributions): a routed window with assume_short_ts: >= 99.9 % of all (row, step)
 *                  flows within rtol 1e-4 + atol 1e-6 m3/s, >= 99.99 % within rtol 3e-2 + atol 1e-4, every one within rtol
 *                  1e-1 + atol 1e-3; one segment-step on the reference's own kernel-vector population: 99 % of q / velocity /
 *                  depth within rtol 2e-5, 99.8 % within 1e-3, at most 0.1 % of the steps beyond 3e-2 -- the tail is the secant
 *                  iteration's 1 % exit test (MCsingleSegStime_f2py_NOLOOP.f90:83) amplifying a last-place difference where it
 *                  converges slowly, not the arithmetic's.  Without assume_short_ts the reference recurrence amplifies
 *                  differences from a cold start and no tolerance is claimed.
 *   wide_min_rows  rows a leading level must have to be routed wide_k steps per launch (k_mc_tile); 0 = default (288 per
 *                  compute unit; 256 in tolerance arithmetic), < 0 = never.  wide_levels: at most so many (0 = default 16).  wide_k: 0 = default 16.
 *   mid_min_rows   the same for a SECOND tier: the levels right below the wide ones, mid_k steps per launch under their own
 *                  skew, queued on the plan's stream between the tail's launches; 0 = default (OFF: measured slower on the
 *                  CONUS day at every setting tried), < 0 = never.  mid_levels (0 = 12), mid_k (0 = 4).
 *   tile_perm_group  the threads of every block of a wide tile take the block's rows by the cost class the rows showed in the
 *                  tile before (inside the launch; wavefronts of one class whatever the forcing does): 0 = default (ON, with or
 *                  without a cost hint), > 0 = on, < 0 = off.
 *   hot_rows       the few rows of a wide tile that showed three or more secant iterations (or went over bank) in the tile before
 *                  are routed by blocks of their own in the next one, so that they do not set the pace of the wavefront they
 *                  would otherwise sit in (1.5 % of the rows of an unordered CONUS plan are in half of its wavefronts); those
 *                  blocks are the first of the launch.  0 = default (on when the in-block partition is), > 0 = on, < 0 = off.
 *   cluster_rows   (since ABI 18) > 0: a plan created with TRMC_PLAN_SHORT_TS on the level engine lays the rows BELOW its wide
 *                  levels out in clusters -- connected pieces of the network of at most so many rows (at most 128)
 *                  -- and routes them wide_k steps per launch as well (k_mc_ctile: flows inside a cluster through LDS, a cluster
 *                  level one tile behind the one that feeds it) instead of one launch per timestep: what a STREAM of windows
 *                  needs (trmc_stream_*; there wide_min_rows may be small -- more levels in slices cost nothing).  0 (default):
 *                  no cluster order -- a single window pays for the clusters' skew with some thirty small launches at its end.
 *                  Such a plan routes with assume_short_ts only.  Single windows whose boundary hydrographs arrive chunk by
 *                  chunk or whose rows carry a lag (trmc_plan_set_lag) keep the one-step launches.
 *   cluster_late_lag  cluster order: rows fed by boundary rows (and rows marked 2 in `boundary`) run at least so many tiles
 *                  behind the headwaters -- the trunk of a cut basin in a multi-GPU stream, whose inflows are exchanged once a
 *                  day (troute_amd.sequence.RouteStream).
 *   hot_wave_rows  rows of the hot list per WAVEFRONT of the blocks that route it (1..64; 0 and below = default 64, above 64 = 64).  An experiment's knob:
 *                  fewer rows per wavefront were meant to shorten the slowest wavefront's chain of wide_k dependent steps on a
 *                  device one launch does not fill (a rank of a multi-GPU job); measured slower at 32, 16 and 8.
 *   stream_split   s > 0: in a stream of windows the slices from level s on are launched on the clusters' stream instead of the
 *                  tile stream (an experiment: 3 % faster on CONUS on one GPU, twice as slow on a rank of eight; default 0).
 *   velocity_on_demand  >= 0 (default): in a stream of windows begun without full_output, a step's velocity is formed only
 *                  where it is handed on -- at the kept steps of output_stride, or nowhere when the products are hydrographs and
 *                  final states.  The velocity feeds nothing (MCsingleSegStime_f2py_NOLOOP.f90:163-169 computes it from the final
 *                  depth; the next step takes velp and does not read it), so every product keeps its bits, and a tenth of a
 *                  step's instructions are not issued.  < 0: every step forms it anyway (an A/B override).  Streams with
 *                  full_output, single windows and the dataflow engine always form every velocity.
 *   tail_sort      < 0: keep the per-level order below the tiled levels of a hinted short-timestep plan (default: by cost).
 *   stem_min_rows  general-mode dataflow plans: basins whose longest path has at least so many rows are laid out stem-last
 *                  (0 = default 1 024, < 0 = off).
 *   sequence_mode  != 0: the plan is one of several that take turns on the device (trmc_plan_clone, trmc_plan_chain_from):
 *                  a window's set-up is queued on the tile stream and its end with its last launch, so that another plan's
 *                  launches in the shared hardware queues do not hold it back.  Also trmc_plan_set_sequence_mode.
 *   flow_watchdog_ms  how long a poll of the dataflow engine may wait before the window is abandoned (0 = default 30 000).
 *   flow_overlap   != 0: consecutive time chunks of a dataflow window alternate between two compute streams.
 *   flow_lean      0 = automatic, > 0 always, < 0 never: the lean form of the dataflow kernel.
 *   flow_debug     != 0: the dataflow engine records when every block ran, and trmc_route_end prints a summary on stderr
 *                  (one line per block into the file named by TRMC_FLOW_DEBUG_FILE, if set) -- a diagnostic. */
enum { TRMC_ARITH_EXACT = 0, TRMC_ARITH_TOLERANCE = 1 };
typedef struct trmc_plan_options {
    int32_t struct_size;
    int32_t arithmetic;
    int64_t wide_min_rows;
    int32_t wide_levels, wide_k;
    int64_t mid_min_rows;
    int32_t mid_levels, mid_k;
    int32_t tile_perm_group;
    int32_t tail_sort;
    int32_t stem_min_rows;
    int32_t sequence_mode;
    int32_t flow_watchdog_ms;
    int32_t flow_overlap;
    int32_t flow_lean;
    int32_t flow_debug;
    int32_t hot_rows;
    int32_t cluster_rows;
    int32_t cluster_late_lag;
    int32_t stream_split;
    int32_t hot_wave_rows;
    int32_t velocity_on_demand;
    int32_t reserved[2];
} trmc_plan_options;
int trmc_plan_create_opt(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx,
                         const float *params, const uint8_t *boundary, const uint8_t *cost_hint,
                         int precision, int device, int flags, const trmc_plan_options *options, trmc_plan **out);
/* A STREAM OF WINDOWS on one plan (since ABI 18; csrc/stream.inc): the reference's run-set loop -- compute_nhd_routing_v02 per run
 * set, every call with that window's qlat_values (mc_reach.pyx:173,:723), new_q0 between them (AbstractNetwork.py:177-191; loop
 * nwm_routing/__main__.py:195-333) -- as ONE sequence of tile launches whose tile index runs on over the days.  assume_short_ts
 * only; the plan must be in cluster order (TRMC_PLAN_SHORT_TS on the level engine, cluster_rows >= 0), without lagged rows
 * (level-pool reservoirs and gages: see trmc_stream_set_gages below).  Every launch routes every row through the next wide_k steps of ITS place in the stream (a row
 * `lag` tiles behind the headwaters works on an earlier tile, possibly of the day before): nsteps / wide_k launches per day, no
 * launches that only part of the network has work in, nothing between two days.  Results are the bits of the same days routed
 * one by one.
 *   trmc_stream_begin  after trmc_upload_forcing (the state q0 -- or NULL: what the plan's last window left -- and the shape of
 *                      the forcing: every day has its nq columns).  slots: days the ring holds (0 = as many as the rows' lag needs:
 *                      2 + ceil((lag_max + 1) / tiles_per_day)); full_output != 0: every day's out[nseg][nsteps][3] is assembled
 *                      (9.4 GB per slot for CONUS) and may be asked for; output_stride = n > 0: every n-th step of every row's
 *                      (q, v, d) is (what the reference's writers take, nwm_routing/output.py:209-216) -- otherwise a day's
 *                      products are its row-set hydrographs and its final state only and nothing else is written.
 *   trmc_stream_push   the next day: qlat [nseg][nq] on the host (page-locked memory for a copy that runs beside the launches; it
 *                      must stay unchanged until the day has begun on the device -- e.g. until the push after next returns);
 *                      boundary_q_dev: flows of the plan's boundary rows for the day [nboundary][nsteps] in DEVICE memory (NULL
 *                      without boundary rows); where the day's products go (any may be NULL): hyd_host [rows of rowset][nsteps],
 *                      q0_host [nseg][3], fvd_host [nseg][nsteps / output_stride][3] (or [nseg][nsteps][3] with full_output and no
 *                      stride) -- page-locked host arrays, filled when the day's LAST row has been routed through it, lag_max
 *                      launches into the days that follow.
 *   trmc_stream_flush  queues the launches that end every pushed day (nothing new starts); further days may be pushed afterwards.
 *   trmc_stream_wait   blocks until the products of `day` (0-based count of pushes) are on the host; TRMC_ESTATE if the day has
 *                      not been queued to its end yet (push on, or flush).
 *   trmc_stream_end    flush + wait for the device; the last day's final state stays staged (trmc_upload_forcing with q0 = NULL,
 *                      or another stream, continues from it).
 *   trmc_stream_info   facts: slots, tiles per day, the largest lag in tiles, wide levels, cluster levels, days pushed, days
 *                      queued to their end, tile launches so far (any pointer may be NULL). */
int trmc_stream_begin(trmc_plan *plan, int nsteps, int qts_subdivisions, int slots, int full_output, int output_stride);
int trmc_stream_push(trmc_plan *plan, const void *qlat, int64_t nq, const void *boundary_q_dev, int32_t rowset, void *hyd_host,
                     void *q0_host, void *fvd_host);
/* A stream on a plan with LEVEL-POOL RESERVOIRS and GAGES (additions within ABI 19; csrc/stream.inc).  trmc_set_reservoirs before
 * trmc_stream_begin puts the plan's waterbodies into the stream: a reservoir row keeps its water elevation in the depth slot and
 * hands it from day to day like any depth; TRMC_ESTATE while a stream is in progress.  A plan whose staged window has reservoir
 * data-assimilation tables (trmc_set_reservoir_da, types 2-5) is refused by trmc_stream_begin unless the plan's streams were told to
 * carry them: trmc_stream_set_reservoir_da and trmc_stream_reservoir_da, below trmc_set_reservoir_da.
 *   trmc_stream_set_gages  the rows [ngage] whose flow the streams on this plan nudge (ngage = 0: none), declared ONCE, before
 *                      trmc_stream_begin; no tables yet.  They stay until the next call (trmc_set_nudging's tables, which
 *                      belong to one window, are not touched and not used by a stream).  One gage per row: the last listed
 *                      wins; a gage on a reservoir or boundary row is TRMC_EINVAL; TRMC_ESTATE while a stream is in progress.
 *   trmc_stream_push_day   trmc_stream_push with the day's tables: the members of trmc_stream_push by name, then
 *                      da_mode / da_a / da_w [da_ngage][da_nsteps] -- what trmc_set_nudging takes for a window, resolved by the
 *                      caller for THIS day (mode uint8; a, w in the plan's precision; host memory, page-locked or not; they must
 *                      stay unchanged until the day has begun on the device) -- required when the stream has gage rows, with
 *                      da_ngage / da_nsteps equal to the declared gages and the stream's nsteps (else TRMC_EINVAL); da_q0
 *                      [da_ngage] (plan precision; NULL = none), the day's FIRST observations, usgs_values[:, 0]: where one is
 *                      not NaN it replaces the flow the gage row starts the day from (mc_reach.pyx:404-411 -- what the drop-in
 *                      writes into a window's initial state on the host; in a stream that state lives on the device); and two more
 *                      products (either may be NULL): nudge_host [ngage][nsteps], the nudge applied at every gage and step, and
 *                      res_inflow_host [res_nres][res_nsteps], the inflow of every reservoir at every step (the reference's
 *                      upstream_array rows) -- page-locked host arrays, filled with the day's other products; trmc_stream_wait
 *                      covers them.  Zero the struct first: members added later then keep their meaning. */
typedef struct trmc_stream_day {
    const void *qlat;
    int64_t nq;
    const void *boundary_q_dev;
    int32_t rowset;
    int32_t reserved0;
    void *hyd_host, *q0_host, *fvd_host;
    int64_t da_ngage;
    int32_t da_nsteps, res_nsteps;
    const uint8_t *da_mode;
    const void *da_a, *da_w;
    void *nudge_host;
    int64_t res_nres;
    void *res_inflow_host;
    const void *da_q0;
    const struct trmc_stream_reservoir_da *reservoir_da; /* (these three were reserved[3]: zero keeps today's meaning) */
    void *res_da_state_host, *res_da_tsidx_host;
} trmc_stream_day;
int trmc_stream_set_gages(trmc_plan *plan, int64_t ngage, const int64_t *gage_rows);
int trmc_stream_push_day(trmc_plan *plan, const trmc_stream_day *day);
/* A STREAM DAY AS PACKED CHRTOUT COLUMNS (additions within ABI 19; csrc/stream.inc): trmc_upload_forcing_packed's counterpart for a
 * stream -- the day's forcing arrives as the files hold it, one or two int32 variables in file order, and ONE kernel on the forcing's
 * stream decodes, joins on the feature id and writes the forcing of the day's ring slot.  The rule is trmc_upload_forcing_packed's,
 * the same device function: masked where == _FillValue / missing_value or outside the valid range and then 0, otherwise
 * raw * scale_factor + add_offset in double; the sum of the two variables in double; the reference's cast to float32 (widened to the
 * plan's precision).  A row the files do not hold gets inflow 0.  The decode produces no NaN.
 *   trmc_stream_set_packed_forcing  the join and the packing facts, declared ONCE, before trmc_stream_begin: nfeat, the length of the
 *                      files' feature axis (at most INT32_MAX); feat_of_row [nseg], the index of every row on that axis (-1: not in
 *                      the files; an entry >= nfeat is TRMC_EINVAL), put into plan order and uploaded here; pack_a[6], and pack_b[6] or
 *                      NULL for the single-variable (q_lateral) form: (scale_factor, add_offset, _FillValue, missing_value,
 *                      valid_min, valid_max), NaN where the file defines none -- trmc_upload_forcing_packed's, field for field.  Host
 *                      memory, copied before the call returns.  nfeat = 0 or feat_of_row = NULL withdraws the declaration.  It stays
 *                      until the next call, as trmc_stream_set_gages does; TRMC_ESTATE while a stream is in progress.  A stream
 *                      begun behind it sizes its staging area for the raw blocks (up to twice the float forcing's bytes).
 *   trmc_stream_push_day_packed  trmc_stream_push_day with raw_a, raw_b [nq][nfeat] int32 in place of day->qlat (which must be NULL;
 *                      every other member keeps its meaning, nudging and reservoir tables included): page-locked host memory for a
 *                      copy that runs beside the launches, unchanged until the day has begun on the device.  raw_b is given exactly
 *                      when pack_b was.  TRMC_ESTATE without the declaration, TRMC_EINVAL for raw_a = NULL, a raw_b that does not
 *                      match the declaration, and a day->nq other than the stream's.  Float days and packed days may alternate in
 *                      one stream.
 *   trmc_stream_packed_forcing_kernel_ms  device time (HIP events, ms) of the last decode queued, beside whatever else ran; waits for
 *                      it.  TRMC_ESTATE before the stream's first packed day. */
int trmc_stream_set_packed_forcing(trmc_plan *plan, int64_t nfeat, const int64_t *feat_of_row, const double *pack_a, const double *pack_b);
int trmc_stream_push_day_packed(trmc_plan *plan, const trmc_stream_day *day, const int32_t *raw_a, const int32_t *raw_b);
int trmc_stream_packed_forcing_kernel_ms(trmc_plan *plan, double *ms_out);
/* A PER-ROW SUMMARY of every day (additions within ABI 19; csrc/stream.inc): how high every row got, when, and how much water
 * passed -- 3 x [nseg] per day instead of the hourly block or the full result.  It is formed from ALL nsteps flows of the day
 * (not from every output_stride-th one) where the day is handed over, by one reduction over the slot's flow plane; the tile
 * kernels carry nothing for it, and a stream without a summary allocates and launches nothing.  The flows are those of the day's
 * result, out[row][step][0]: after nudging at gage rows, the outflow at reservoir rows, the prescribed flow at boundary rows.
 *   peak_flow [nseg] (plan precision), peak_step [nseg] (int32, 1-based step of the day): peak = q[1], step = 1, then for
 *                      t = 2 .. nsteps in order `if (q[t] > peak) { peak = q[t]; step = t; }` -- the first of equal peaks wins, a
 *                      NaN never replaces a number and a NaN at step 1 stays.
 *   mean_flow [nseg] (plan precision): ((q[1] + q[2]) + ... + q[nsteps]) / nsteps, summed in that order in the plan's
 *                      precision (numpy: np.cumsum(q, axis=1, dtype=T)[:, -1] / T(nsteps)).
 *   peak_depth [nseg] (plan precision), peak_depth_step [nseg] (int32, 1-based): the same rule over the day's depths
 *                      d[t] = out[row][step][2] -- the channel depth, the pool's water elevation at a reservoir row, 0 at a step
 *                      without flow; nudging changes flows only.  The planes hold the depth of a tile's last step only, so this
 *                      part is carried by the tile kernels (instances of their own, k_mc_tile_pkd / k_mc_ctile_pkd: a stream
 *                      without the part launches what it always launched); a stream with full_output reduces its full result
 *                      instead, to the same bits.  A boundary row is routed by nobody and has no depth: (0, 1) -- what the
 *                      reduction of the rank's own full result gives there (such a stream's full result holds zeros at boundary
 *                      rows).  TRMC_EUNSUPPORTED from trmc_stream_begin in a stream with reservoir data assimilation
 *                      (trmc_stream_set_reservoir_da), and without full_output on a plan with velocity_on_demand < 0.
 *   trmc_stream_set_summary   what: a mask of TRMC_SUMMARY_PEAK (flow and step), TRMC_SUMMARY_MEAN, TRMC_SUMMARY_PEAK_DEPTH (depth
 *                      and step) and TRMC_SUMMARY_TOTAL (below; with at least one of the others), 0 = none (the default).
 *                      Before trmc_stream_begin; it stays until the next call, as trmc_stream_set_gages does; TRMC_ESTATE while
 *                      a stream is in progress.  Works with full_output, output_stride or neither, with reservoirs, gages and
 *                      (but the peak depth) reservoir data assimilation, in both arithmetics and precisions.
 *   trmc_stream_summary_dest  page-locked host arrays [nseg] for the summary of the NEXT day pushed (any may be NULL): the next
 *                      trmc_stream_push / trmc_stream_push_day that is accepted consumes them, a day pushed without this call
 *                      has no summary.  They are filled with the day's other products; trmc_stream_wait covers them.
 *                      TRMC_ESTATE if the stream in progress was begun without a summary, TRMC_EINVAL for an array whose part
 *                      of the mask is off.
 *   trmc_stream_summary_depth_dest  the same for peak_depth and peak_depth_step of the NEXT day pushed, with the same rules:
 *                      TRMC_ESTATE if the stream in progress was begun without TRMC_SUMMARY_PEAK_DEPTH.
 * THE TOTALS OVER THE DAYS (TRMC_SUMMARY_TOTAL): running values over all days handed over since trmc_stream_begin, [nseg] arrays in
 * row order that live on the device outside the ring; every day's summary is folded into them in day order where the day is
 * handed over, whether or not the day's own arrays go to the host (no trmc_stream_summary_dest: nothing of the summary crosses
 * to the host but the totals).  All of them fold the per-day products:
 *   peak_flow, peak_step (int64, 1-based from the stream's first step): day 0's values; then for day D >= 1 (0-based)
 *                      `if (pk_D > pk) { pk = pk_D; step = D * nsteps + st_D; }` -- the first of equal day peaks wins, a NaN
 *                      day peak after day 0 never replaces (the totals keep the earlier days'), a NaN on day 0 stays (with
 *                      step 1: the peak rule's own NaN at step 1), so np.maximum over the days' peaks is this fold only
 *                      while no day's peak is a NaN
 *   peak_depth, peak_depth_step (int64): the same fold, with TRMC_SUMMARY_PEAK_DEPTH
 *   mean_flow          (((m_0 + m_1) + m_2) + ...) / T(ndays) in the plan's precision, left to right (NaN where any day's mean is)
 *   trmc_stream_summary_total  HOST arrays [nseg] (any may be NULL); synchronous: returns when the totals of all days handed over
 *                      so far are on the host and writes that number of days to days_out.  TRMC_ESTATE when no stream is in
 *                      progress, when it was begun without TRMC_SUMMARY_TOTAL or when no day is complete yet; TRMC_EINVAL for an
 *                      array whose part of the mask is off.
 * Velocities have no summary (a stream that assembles no full result forms no velocity). */
enum { TRMC_SUMMARY_PEAK = 1, TRMC_SUMMARY_MEAN = 2, TRMC_SUMMARY_PEAK_DEPTH = 4, TRMC_SUMMARY_TOTAL = 8 };
int trmc_stream_set_summary(trmc_plan *plan, int what);
int trmc_stream_summary_dest(trmc_plan *plan, void *peak_flow_host, int32_t *peak_step_host, void *mean_flow_host);
int trmc_stream_summary_depth_dest(trmc_plan *plan, void *peak_depth_host, int32_t *peak_depth_step_host);
int trmc_stream_summary_total(trmc_plan *plan, void *peak_flow, int64_t *peak_step, void *mean_flow, void *peak_depth,
                              int64_t *peak_depth_step, int64_t *days_out);
/* Multi-GPU streams (the trunk of a cut basin: rows fed by boundary rows, cluster_late_lag tiles behind).  trmc_stream_gather: the
 * flows of a row set over `day` [rows][nsteps] into DEVICE memory, queued on `stream` (NULL: the plan's) behind the launches
 * queued so far -- TRMC_ESTATE if the set's rows have not been queued through that day yet.  trmc_stream_boundary: the boundary
 * rows' flows of `day` (already pushed, with boundary_q_dev = NULL) from a block of hydrographs in DEVICE memory -- boundary row b
 * takes row index_dev[b] (NULL: row b) of q_dev, rows src_row_stride elements apart -- queued on `stream` (NULL: the copy stream);
 * the launches of the NEXT push go behind it, so the rows that read boundary rows must run at least that far behind
 * (trmc_plan_options.cluster_late_lag).  Calls for consecutive days in order. */
int trmc_stream_gather(trmc_plan *plan, int64_t day, int32_t rowset, void *dst_dev, void *stream);
int trmc_stream_boundary(trmc_plan *plan, int64_t day, const void *q_dev, int64_t src_row_stride, const int64_t *index_dev, void *stream);
/* The next ntiles launches without a new day (the rows still under way move on; at most up to the launch that ends the last day
 * pushed).  trmc_stream_flush = all of them.  A stream advanced this way takes a new day only once it has been flushed. */
int trmc_stream_advance(trmc_plan *plan, int ntiles);
int trmc_stream_flush(trmc_plan *plan);
int trmc_stream_wait(trmc_plan *plan, int64_t day);
int trmc_stream_info(const trmc_plan *plan, int32_t *slots, int32_t *tiles_per_day, int32_t *lag_max, int32_t *wide_levels,
                     int32_t *cluster_levels, int64_t *days_pushed, int64_t *days_complete, int64_t *launches);
/* Device time (HIP events, ms) from the first to the last of the nsteps / wide_k launches that pushing `day` queued on the stream
 * that carries the slices (the dominant kernel, k_mc_tile): / tiles_per_day = the mean duration of one launch beside whatever
 * else runs.  Waits for those launches.  The day must still be in the ring. */
int trmc_stream_day_ms(trmc_plan *plan, int64_t day, double *ms_out);
int trmc_stream_end(trmc_plan *plan);

/* Switch the sequence mode of a plan (see trmc_plan_options) between windows. */
int trmc_plan_set_sequence_mode(trmc_plan *plan, int on);
/* 1 if the plan computes in TRMC_ARITH_TOLERANCE, else 0. */
int trmc_plan_arithmetic(const trmc_plan *plan, int32_t *arithmetic);
/* 1 if the plan runs on the dataflow engine, 0 on the level engine. */
int trmc_plan_engine(const trmc_plan *plan, int32_t *is_flow);
void trmc_plan_destroy(trmc_plan *plan);

/* Host-only topology flattening (no device needed): the same routine the plan
 * uses.  level_of_row[nseg] (-1 for boundary rows), plan_pos_of_row[nseg],
 * *nlevels; any output pointer may be NULL.  TRMC_ECYCLE if the graph is cyclic. */
int trmc_topology_levels(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx,
                         const uint8_t *boundary, int32_t *level_of_row,
                         int64_t *plan_pos_of_row, int32_t *nlevels);

/* The same with the cost hint of trmc_plan_create_hinted (or NULL). */
int trmc_topology_levels_hinted(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx,
                                const uint8_t *boundary, const uint8_t *cost_hint, int32_t *level_of_row,
                                int64_t *plan_pos_of_row, int32_t *nlevels);

/* Host-only (since ABI 18): the CLUSTER ORDER a short-timestep plan of the level engine is laid out in (trmc_plan_options.cluster_rows;
 * csrc/topology.hpp).  The leading levels of at least wide_min_rows rows (at most wide_max_levels of them) stay level slices; the
 * rows below them form clusters of at most cluster_rows rows, packed into blocks of one cluster level each (here: of at most
 * cluster_rows rows; a plan packs them up to the width of its kernel's workgroup, trmc_plan_cluster_blocks).  lag_of_row[nseg]:
 * tiles a row runs behind level 0 (-1 for boundary rows) -- a row only reads rows of its own block with its own lag, or rows
 * with a smaller one; block_of_row[nseg]: its cluster block, -1 in the slices.  Outputs may be NULL.
 * Reference analogue: build_subnetworks (nhd_network.py:691-771). */
int trmc_topology_clusters(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const uint8_t *boundary,
                           const uint8_t *cost_hint, int64_t wide_min_rows, int32_t wide_max_levels, int32_t cluster_rows,
                           int64_t *plan_pos_of_row, int32_t *lag_of_row, int32_t *block_of_row, int32_t *wide_levels,
                           int32_t *cluster_levels, int32_t *cluster_blocks);

/* Host-only: the BLOCK ORDER of the dataflow engine (fp32 plans; csrc/topology.hpp) -- routed rows in depth-first
 * post-order, stably sorted by a downstream-monotone cost tier (cost_tiers != 0), cut into blocks of *block_rows positions (one workgroup
 * each; boundary rows come first and belong to no block), rows of a block grouped by cost.  Every row's upstream rows
 * sit in its own block or an earlier one.  plan_pos_of_row[nseg]; rank_of_row[nseg] = dependency depth of the row
 * inside its block (the steps it trails by without assume_short_ts).  Outputs may be NULL.
 * Reference analogue: dfs_decomposition's reach order (nhd_network.py:503-557) and build_subnetworks (:691-771). */
int trmc_topology_blocks(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx,
                         const uint8_t *boundary, const uint8_t *cost_hint, int cost_tiers,
                         int64_t *plan_pos_of_row, int32_t *rank_of_row, int32_t *block_rows, int32_t *nblocks);

/* Host-only: the block order of a plan built for the GENERAL mode (TRMC_PLAN_FULL_TS on the dataflow engine) -- the plain
 * post-order (no cost tiers), except that a basin whose longest path has at least stem_min_rows rows (the library's
 * default: 1 024, TRMC_STEM_MIN_ROWS) is laid out as [its side tributaries, those joining at the TOP of that path first]
 * [the path, top to bottom], the path's run of positions beginning and ending on a block boundary (the gap filled with
 * whole small networks).  early_blocks[min(*nearly, early_cap)]: the blocks that hold such paths, ascending -- the general
 * mode's kernel starts them first, so that the dependent chain of mc_reach.pyx:499-505 (a row needs its upstream rows at the
 * SAME timestep) runs down behind the sweep over its basin instead of after it.  Outputs may be NULL. */
int trmc_topology_blocks_general(int64_t nseg, const int64_t *up_ptr, const int64_t *up_idx, const uint8_t *boundary,
                                 int32_t stem_min_rows, int64_t *plan_pos_of_row, int32_t *rank_of_row, int32_t *block_rows,
                                 int32_t *nblocks, int32_t *early_blocks, int32_t early_cap, int32_t *nearly);

/* Facts about the flattened topology (host side, no device work). */
int trmc_plan_info(const trmc_plan *plan, int64_t *nseg, int64_t *nseg_routed,
                   int32_t *nlevels, int32_t *precision, int32_t *device);
/* A plan in cluster order (trmc_plan_options.cluster_rows): lag_of_row[nseg] = tiles every row runs behind the headwaters (-1:
 * boundary row), the number of levels kept as slices, the number of cluster levels.  Pointers may be NULL. */
int trmc_plan_lags(const trmc_plan *plan, int32_t *lag_of_row, int32_t *wide_levels, int32_t *cluster_levels);
/* ... and its cluster blocks: block_of_row[nseg] = the cluster block that routes the row (-1: a row of the slices, a boundary row)
 * -- one workgroup of k_mc_ctile, whole clusters of one cluster level; *block_width = the most rows such a block holds (the
 * workgroup's threads, a build-time constant of the library); *cluster_blocks = their number.  Pointers may be NULL. */
int trmc_plan_cluster_blocks(const trmc_plan *plan, int32_t *block_of_row, int32_t *block_width, int32_t *cluster_blocks);
/* level_of_row[nseg] (-1 for boundary rows); plan_pos_of_row[nseg] = position in
 * the level-major device order.  Either pointer may be NULL. */
int trmc_plan_levels(const trmc_plan *plan, int32_t *level_of_row, int64_t *plan_pos_of_row);

/*
 * Stage one routing window's forcing into HBM (H2D).  Arrays are in row order,
 * element type per the plan's precision.
 *   qlat          [nseg][nq]   lateral inflow per forcing interval
 *   q0            [nseg][3]    qu0 qd0 h0  (mc_reach.pyx:361: initial q = column
 *                              0, initial depth = column 2); NULL = continue from the state
 *                              the previous window left in HBM (the reference's new_q0 warm
 *                              start between max_loop_size windows, AbstractNetwork.py:177-191,
 *                              without the host round trip)
 *   boundary_fvd  [nboundary][nsteps][3] q,v,d hydrographs of the boundary rows
 *                 in ascending row order, or NULL when the plan has none
 */
int trmc_upload_forcing(trmc_plan *plan, int nsteps, const void *qlat, int64_t nq,
                        const void *q0, const void *boundary_fvd);

/*
 * The same, with the lateral inflow taken straight from packed WRF-Hydro CHRTOUT columns:
 * the device decodes, joins on the feature axis and lays the forcing out -- replaces the host-side
 * get_ql_from_chrtout + DataFrame join (src/troute-network/troute/nhd_io.py:397-434, NHDNetwork.py:376-386).
 *   raw_a, raw_b  [nq][nfeat] int32, one row per forcing file, file order of the feature axis (qBucket and
 *                 qSfcLatRunoff; raw_b may be NULL: single variable q_lateral)
 *   pack_a/b      [6] doubles: scale_factor, add_offset, _FillValue, missing_value, valid_min, valid_max
 *                 (NaN for a fill value or bound the file does not define)
 *   feat_of_row   [nseg] position of each row's id on the feature axis, -1 = not in the files (inflow 0)
 * value = float32( unpack(a) + unpack(b) ), unpack(raw) = 0 where raw is masked (equal to a fill value or outside
 * the valid range, netCDF4's default auto-mask then .filled(0.0)), else raw * scale_factor + add_offset in double.
 */
int trmc_upload_forcing_packed(trmc_plan *plan, int nsteps, int64_t nq, int64_t nfeat, const int32_t *raw_a,
                               const int32_t *raw_b, const double *pack_a, const double *pack_b,
                               const int64_t *feat_of_row, const void *q0, const void *boundary_fvd);

/*
 * Supply the boundary rows' flow hydrographs from a DEVICE buffer q_dev[nboundary][nsteps] (ascending
 * boundary row order) after trmc_upload_forcing(..., boundary_fvd = NULL): the multi-GPU hand-off of
 * sub-basin outlet hydrographs to the trunk (reference: flowveldepth_interorder, compute.py:882-897)
 * without a host round trip.  Velocity/depth of boundary rows are not inputs of the routing.
 */
int trmc_set_boundary_flow_device(trmc_plan *plan, int nsteps, const void *q_dev);

/*
 * Level-pool reservoirs of the plan.  Reference: the RESERVOIR_LP branch of the
 * network loop, mc_reach.pyx:283-356 (setup) and :507-716 (wbody_type_code 1), around
 * LEVELPOOL_PHYSICS (src/kernel/reservoir/Level_Pool/module_levelpool.F:233-427).  A reservoir is one
 * row of the table (the reference's waterbody node); its inflow is the junction sum of its upstream
 * rows, its result row holds (outflow, 0, water elevation).
 *   res_rows [nres]     rows of the reservoirs
 *   par      [nres][9]  area max_depth orifice_area orifice_coefficient orifice_elevation
 *                       weir_coefficient weir_elevation weir_length dam_length  (plan precision)
 *   routing_period      seconds (the dt argument of compute_network_structured)
 * The initial outflow and water elevation of a reservoir row travel in q0[row] = (qd0, -, h0) of
 * trmc_upload_forcing.  nres = 0 removes the reservoirs.
 */
int trmc_set_reservoirs(trmc_plan *plan, int64_t nres, const int64_t *res_rows, const void *par,
                        double routing_period);
/* inflow_out[nres][nsteps]: the inflow every reservoir received at every step (the reservoir rows of the
 * reference's upstream_array, mc_reach.pyx:710).  D2H. */
int trmc_download_reservoir_inflow(trmc_plan *plan, void *inflow_out);

/*
 * Reservoir data assimilation on top of the level pool, for the staged window: hybrid persistence of gage
 * observations (reservoir types 2 USGS, 3 USACE) and RFC forecast series (types 4 RFC, 5 glacially dammed lake).
 * Reference: the reservoir branch of the network loop, mc_reach.pyx:548-710, with reservoir_hybrid_da
 * (fast_reach/reservoir_hybrid_da.py) and reservoir_RFC_da (fast_reach/reservoir_RFC_da.py:193-319); arithmetic types:
 * csrc/reservoir_da.hpp.  Precision 32 plans only.  At every step the level-pool step runs first; the data-
 * assimilation step then replaces its outflow and water elevation and moves the reservoir's state on.
 *   kind      [nres]  per reservoir of trmc_set_reservoirs: 0 = level pool only, 2 / 3 / 4 / 5 = the reservoir type
 *   table_row [nres]  its row in the table of its kind (usgs: 2, usace: 3, rfc: 4 and 5); ignored for kind 0
 * A table (NULL or n = 0: none) has n rows of ncol entries:
 *   usgs, usace: obs [n][ncol] observations (NaN = none), time [ncol] their times in seconds from the window's
 *                start, state [n][4] = update_time prev_persisted_outflow persistence_index persistence_update_time
 *   rfc:         obs [n][ncol] the series, state [n] = update_time, ipar [n][5] = timeseries_idx totalCounts
 *                use_forecast da_timestep rfc_persist_days; time unused
 * Everything is copied.  Must follow trmc_set_reservoirs (which drops the tables); nres = 0 drops them too.  The
 * lookback is 48 h, the intervals 3600 s and 86400 s, the persistence limit 11, as the loop calls the functions.
 */
typedef struct trmc_reservoir_da_table {
    int64_t n, ncol;
    const float *obs, *time, *state;
    const int32_t *ipar;
} trmc_reservoir_da_table;
int trmc_set_reservoir_da(trmc_plan *plan, int64_t nres, const int32_t *kind, const int32_t *table_row,
                          const trmc_reservoir_da_table *usgs, const trmc_reservoir_da_table *usace,
                          const trmc_reservoir_da_table *rfc);
/* The state the routed window left, per reservoir of the plan: state_out [nres][4] (the four values above; RFC
 * reservoirs: [0] = update_time), timeseries_idx_out [nres].  Times are in seconds from the START of the window
 * (the loop's return shifts them by its length, mc_reach.pyx:820-837).  D2H. */
int trmc_download_reservoir_da(trmc_plan *plan, float *state_out, int32_t *timeseries_idx_out);
/*
 * The same in a STREAM OF DAYS (additions within ABI 19; csrc/stream.inc).  trmc_stream_set_reservoir_da(plan, on != 0, ...) before
 * trmc_stream_begin tells the streams on this plan to carry the reservoirs' data assimilation (until the next call; on = 0: a plan
 * with tables is refused by trmc_stream_begin as before); precision 32, exact arithmetic only.  trmc_set_reservoir_da before
 * trmc_stream_begin is then the stream's DECLARATION: kind and table_row of every reservoir and the tables' row counts n hold for
 * the whole stream, and its state members (update_time, prev_persisted_outflow, persistence_index, persistence_update_time; RFC:
 * update_time and timeseries_idx) are what day 0 starts from.  From there the state lives on the device: a reservoir row that ends
 * a day takes float(nsteps) * float(routing_period) off update_time and persistence_update_time in fp32 (RFC: update_time), as the
 * loop's return does (mc_reach.pyx:820-837), and starts the next day from that.
 *   usgs_ncol, usace_ncol, rfc_ncol  the most columns a day's table of that kind may have (the ring's slots are sized by them);
 *                      0, or less than the declared table's ncol: the declared table's ncol.
 * Every day brings its own tables, trmc_stream_day::reservoir_da (required on such a stream, TRMC_EINVAL on any other): the three
 * tables with the declaration's n and an ncol of the day's own, at most the capacity.  Of their members count
 *   obs, time          the day's, times in seconds from the day's start
 *   ipar               RFC: totalCounts use_forecast da_timestep rfc_persist_days are the day's; timeseries_idx only when
 *                      rfc_reset_idx != 0 (the reference replaces the index when it reads a new forecast file,
 *                      DataAssimilation.py:1978-1980), else the device's own is carried on
 *   state              ignored (may be NULL)
 * Host memory, page-locked or not; copied before trmc_stream_push_day returns.  Two more products of a day (either may be NULL):
 * res_da_state_host [nres][4] float32 and res_da_tsidx_host [nres] int32, what trmc_download_reservoir_da hands over for a window
 * but with the times ALREADY shifted to the next day's start -- tuple elements [4], [5], [7] of compute_network_structured; page-
 * locked host arrays, filled with the day's other products, covered by trmc_stream_wait.
 */
typedef struct trmc_stream_reservoir_da {
    trmc_reservoir_da_table usgs, usace, rfc;
    int32_t rfc_reset_idx;
    int32_t reserved0;
} trmc_stream_reservoir_da;
int trmc_stream_set_reservoir_da(trmc_plan *plan, int on, int64_t usgs_ncol, int64_t usace_ncol, int64_t rfc_ncol);
/*
 * Batch of n independent data-assimilation steps on the device, through the device functions the step kernels call.
 *   TRMC_RESERVOIR_DA_HYBRID: obs [n][ncol], time [n][ncol],
 *       fin [n][12] = now prev_persisted_outflow persistence_update_time persistence_index levelpool_outflow inflow
 *                     routing_period lake_area(km2) max_depth orifice_elevation initial_water_elevation update_time
 *       fout [n][6] = outflow persisted_outflow water_elevation update_time persistence_index persistence_update_time
 *       (iin, iout unused)
 *   TRMC_RESERVOIR_DA_RFC: obs [n][ncol] (time unused),
 *       fin [n][9] = now update_time inflow water_elevation levelpool_outflow levelpool_water_elevation lake_area(km2)
 *                    max_water_elevation routing_period
 *       iin [n][6] = use_forecast timeseries_idx totalCounts da_timestep rfc_persist_days reservoir_type
 *       fout [n][3] = outflow water_elevation update_time;  iout [n] = timeseries_idx
 */
#define TRMC_RESERVOIR_DA_HYBRID 2
#define TRMC_RESERVOIR_DA_RFC 4
int trmc_reservoir_da_steps(int device, int kind, int64_t n, int64_t ncol, const float *obs, const float *time,
                            const float *fin, const int32_t *iin, float *fout, int32_t *iout);

/*
 * Streamflow nudging at gages for the staged window.  Reference: simple_da
 * (src/troute-routing/troute/routing/fast_reach/simple_da.pyx:22-95) applied to the gage segment after
 * its reach has been routed for the timestep (mc_reach.pyx:761-796).  Which of simple_da's three
 * branches is taken at (gage, step) depends on the observation record only, so the caller resolves it
 * (troute_amd does, with the reference's float/double arithmetic incl. libc exp for the decay weight):
 *   mode[g][t-1] = 0  no observation, no last observation: the model value passes through
 *                  1  valid observation a[g][t-1]: flow := a, nudge := a - model
 *                  2  decay: nudge := (a - model) * w, flow := model + nudge   (a = last observation)
 * arrays [ngage][nsteps] (a, w in the plan's precision); gage_rows = rows of the gage segments.
 * Call after trmc_upload_forcing (which clears the tables); ngage = 0 switches nudging off.
 */
int trmc_set_nudging(trmc_plan *plan, int nsteps, int64_t ngage, const int64_t *gage_rows,
                     const uint8_t *mode, const void *a, const void *w);
/* Gages INSIDE a reach when the window is routed WITHOUT assume_short_ts (with it nothing is needed: a segment then reads
 * only stored flows of the step before).  successor_rows[g] = the row directly below gage g in its reach, or -1 when the
 * gage ends its reach.  The reference nudges after the whole reach has been routed (mc_reach.pyx:133-137, :761-796), so
 * that one row reads the gage segment's flow of the current step as it was BEFORE the nudge while every other reader gets
 * the nudged value.  Level engine only (TRMC_ESTATE on a dataflow plan); after trmc_set_nudging, per window. */
int trmc_set_nudging_successors(trmc_plan *plan, int64_t ngage, const int64_t *successor_rows);
/* nudge_out[ngage][nsteps]: the nudge applied at every gage and step (mc_reach.pyx:793). D2H. */
int trmc_download_nudge(trmc_plan *plan, void *nudge_out);

/*
 * Route nsteps timesteps on the device (asynchronous launches on the plan's
 * stream, then waits for completion).  Replaces the time x reach loop of [R1]
 * (mc_reach.pyx:492-505, :719-750) and the per-reach chain of
 * compute_reach_kernel (mc_reach.pyx:70-138).
 *   qts_subdivisions  timesteps per forcing interval (qlat column = (t-1)/qts)
 *   assume_short_ts   non-zero: quc := qup (mc_reach.pyx:504-505, :135-136)
 * Results stay in HBM until downloaded.
 */
int trmc_route_device(trmc_plan *plan, int nsteps, int qts_subdivisions, int assume_short_ts);

/*
 * The same window in parts, so that a caller can interleave other device work with it -- the multi-GPU
 * hand-off: sub-basin outlet hydrographs leave for the trunk's owner one time chunk at a time while the
 * later chunks are still being routed (reference: the ordered sub-network loop with its
 * flowveldepth_interorder hand-off, compute.py:553-1209, here pipelined in time instead of serialised).
 * Every call only queues work on the plan's stream (trmc_plan_stream) and returns; trmc_route_end waits.
 *   trmc_route_begin     as trmc_route_device up to the first timestep; boundary hydrographs may still be
 *                        missing (they then arrive through trmc_set_boundary_flow_range)
 *   trmc_route_advance   queue the launches (done, t_end]; launch d = timestep d (of the rows without lag)
 *   trmc_route_end       finish the result layout, wait, fill trmc_stats
 * trmc_route_device == begin + advance(nsteps) + end.
 */
int trmc_route_begin(trmc_plan *plan, int nsteps, int qts_subdivisions, int assume_short_ts);
int trmc_route_advance(trmc_plan *plan, int t_end);
int trmc_route_end(trmc_plan *plan);
/* The plan's HIP stream (hipStream_t as void*), for ordering foreign work (RCCL) against the plan's.  With
 * TRMC_FLOW_OVERLAP=1 in the environment (off by default: no gain measured), a window of the dataflow engine whose
 * launches are all resident alternates consecutive trmc_route_advance calls between two compute streams so that time
 * chunks overlap: the call then returns the stream the NEXT advance uses -- ask again before every advance;
 * trmc_gather_flow_range is queued behind the launches that hold its steps. */
int trmc_plan_stream(trmc_plan *plan, void **stream_out);
/* Register a set of rows once (their plan positions are kept in HBM); *id_out names it. */
int trmc_rowset_create(trmc_plan *plan, const int64_t *rows, int64_t nrows, int32_t *id_out);
/* Queue: dst_dev[i * dst_stride + (t - 1 - t_begin)] = flow of row i of the set at step t, t in (t_begin, t_end],
 * all of which must already be queued (trmc_route_advance) or routed.  dst_dev is device memory. */
int trmc_gather_flow_range(trmc_plan *plan, int32_t rowset, int t_begin, int t_end, void *dst_dev,
                           int64_t dst_stride);
/* Queue: boundary row b (ascending row order) takes flow q_dev[b * src_stride + (t - 1 - t_begin)] at the steps
 * (t_begin, t_end]; ranges must be supplied in order, t_begin = end of the previous one (0 first). */
int trmc_set_boundary_flow_range(trmc_plan *plan, int t_begin, int t_end, const void *q_dev, int64_t src_stride,
                                 void *stream /* hipStream_t to queue the copy on; NULL = the plan's */);
/* The same with a gather: boundary row b takes the source row src_index_dev[b] (device int64 [nboundary]) of q_dev --
 * e.g. its cut row's place in the block an all-gather delivered -- so that no separate gather kernel sits between the
 * collective and the boundary rows.  NULL = the identity. */
int trmc_set_boundary_flow_range_indexed(trmc_plan *plan, int t_begin, int t_end, const void *q_dev,
                                         int64_t src_stride, const int64_t *src_index_dev, void *stream);
/*
 * Time-skewed rows (assume_short_ts only).  lag_of_row[nseg] holds 0 or one common value L: launch d of the
 * window routes the rows without lag at step d and the lagged rows at step d - L, so a window takes
 * nsteps + L launches (trmc_route_advance counts launches).  Use: the trunk of a cut basin rides in the
 * launches of this GPU's sub-basins L steps behind them, which gives the cut-edge hydrographs of the other
 * GPUs L steps to arrive (boundary rows may feed lagged rows only) -- no launch of its own, no waiting.
 * With assume_short_ts a row at step t reads its upstream rows at step t-1 only, which the skew preserves.
 * NULL clears the lag.  Call before trmc_rowset_create.
 */
int trmc_plan_set_lag(trmc_plan *plan, const int32_t *lag_of_row);

/* Full result, row order: fvd_out[nseg][nsteps][3] = (q, vel, depth) per step,
 * i.e. flowveldepth[:, 1:, :] of [R1] (mc_reach.pyx:807-813).  D2H. */
int trmc_download_fvd(trmc_plan *plan, void *fvd_out);
/* Every `stride`-th step of it, decimated ON THE DEVICE: fvd_out[nseg][nsteps / stride][3], entry k = step stride (k + 1)
 * (1-based) -- the steps the reference's writers keep of a window (nwm_routing/output.py:209-216, :232-240: those whose end
 * falls on a multiple of dt * qts_subdivisions; stride = qts_subdivisions for hourly output of 5-minute steps).  A twelfth
 * of the bytes crosses the host link: a CONUS day 0.78 GB instead of 9.4.  Bit-identical to slicing the full array. */
int trmc_download_fvd_strided(trmc_plan *plan, int stride, void *fvd_out);
/* The same for the rows of a registered set (trmc_rowset_create), in the set's order: fvd_out[rows of the set][nsteps / stride][3]
 * (stride = 1: every step).  compute_nhd_routing_v02 hands its result back as one block per tailwater (compute.py:1738, the
 * per-network loop :1399-1738): with the set = the table's rows grouped by tailwater, each of those is a slice of fvd_out and
 * the host never permutes the block. */
int trmc_download_fvd_rowset(trmc_plan *plan, int stride, int32_t rowset, void *fvd_out);
/*
 * Per-row summary of the last WINDOW, reduced on the device from the same result trmc_download_fvd copies -- every step of it,
 * whatever stride the caller takes the block itself at: a few bytes per row cross the host link instead of nsteps * 3 values.
 *   peak_flow, peak_step                  the largest flow of the window and the 1-based step it was FIRST reached at
 *   mean_flow                             the flows summed left to right in the plan's precision, divided by nsteps
 *                                         (np.cumsum(q, dtype=T)[-1] / T(nsteps))
 *   peak_depth, peak_depth_step           the same compare on the depths
 *   peak_velocity, peak_velocity_step     ... and on the velocities
 * A peak is `pk = x[1]; at = 1; for t = 2..nsteps: if (x[t] > pk) { pk = x[t]; at = t; }`: of equal values the first wins, a NaN
 * never replaces a number.  The first five are what a stream of days leaves with TRMC_SUMMARY_PEAK | _MEAN | _PEAK_DEPTH, bit
 * for bit.  Value destinations hold nrows elements of the plan's precision, step destinations nrows int32; any of them may be
 * NULL (all NULL: TRMC_EINVAL), a step destination needs its value destination.  rowset: -1 = every row in row order, else a
 * registered set (trmc_rowset_create): its rows, in its order.  Valid wherever trmc_download_fvd is -- after a window of either
 * engine, either timestep mode, either precision and either arithmetic -- and TRMC_ESTATE before any window, while a window is
 * open and while a stream of windows is in progress (a stream does not fill the plan's window result).  Synchronous: one kernel
 * on the plan's stream behind the window, the columns into plan-owned scratch, then to the host.  nseg == 0: nothing is written.
 *
 * trmc_window_summary_tile: the kernel's tile for a precision (32 / 64) -- rows per block and steps per chunk of a row's record
 * (csrc/k_window_summary.inc); the sizes at which its tests probe the tile's edges.  Host only.
 * trmc_window_summary_kernel_ms: device time of the last trmc_window_summary's kernel on this plan, from events around it (the
 * copies to the host not included); TRMC_ESTATE before the first.  Host only.
 */
int trmc_window_summary(trmc_plan *plan, int32_t rowset, void *peak_flow, int32_t *peak_step, void *mean_flow,
                        void *peak_depth, int32_t *peak_depth_step, void *peak_velocity, int32_t *peak_velocity_step);
int trmc_window_summary_tile(int precision, int32_t *rows, int32_t *steps);
int trmc_window_summary_kernel_ms(const trmc_plan *plan, double *ms_out);
/*
 * Courant metrics of the last WINDOW: for every row and step the triple (cn, ck, X) -- Courant number ck * dt / dx, kinematic
 * celerity and the Muskingum weighting factor the step ended on -- in the order of the reference's output_buf[3:6] and of its
 * writers' columns (mc_reach.pyx:128-131, nwm_routing/output.py:262-272; compute_parameters.return_courant).  No routing kernel
 * forms them: one pass (csrc/k_window_courant.inc) recomputes every row-step from what the plan still holds after the window --
 * the assembled result, the initial state, the staged forcing, the upstream lists -- in the plan's own precision and arithmetic,
 * so the triple is the one the step itself would have left (trmc_segments at the same inputs, bit for bit).  A gage's stored flow
 * is the nudged one; the triple is that of the un-nudged step at those inputs.  Reservoir rows of every type and boundary rows
 * route no Muskingum-Cunge step: (0, 0, 0).
 *   trmc_window_courant          dst[rows][nsteps / stride][3] in the plan's precision; kept steps stride, 2 stride, ... as in
 *                                trmc_download_fvd_rowset, and only those are computed.  rowset: -1 = every row in row order,
 *                                else a registered set (trmc_rowset_create): its rows, in its order.
 *   trmc_window_courant_summary  per row: the highest cn of the window, the 1-based step it was FIRST reached at (the rule of
 *                                trmc_window_summary: pk = cn[1]; t = 2..: if (cn[t] > pk) -- the first of equal peaks wins, a NaN
 *                                never replaces a number, a NaN at step 1 stays) and the number of steps with cn > limit (compared
 *                                in the plan's precision; a NaN is not counted).  Nothing of size rows x nsteps is written.  Any
 *                                destination may be NULL (all NULL: TRMC_EINVAL); peak_cn_step needs peak_cn.
 * Refusals as trmc_window_summary's: TRMC_EINVAL for a NULL plan, an unknown row set, stride < 1; TRMC_ESTATE before any window,
 * while a window is open, while a stream of windows is in progress, and after trmc_plan_chain_from has overwritten the state the
 * last window began from; TRMC_EUNSUPPORTED for a plan with lagged rows (trmc_plan_set_lag).  Valid until the next upload or
 * staging of a forcing.  Synchronous, on the plan's stream.
 *   trmc_window_courant_tile       rows per block and steps per chunk of the kernel, for a precision (32 / 64).  Host only.
 *   trmc_window_courant_kernel_ms  device time of the last of the two calls' kernel on this plan, from events around it (copies
 *                                  to the host not included); TRMC_ESTATE before the first.  Host only.
 */
int trmc_window_courant(trmc_plan *plan, int32_t rowset, int stride, void *dst);
int trmc_window_courant_summary(trmc_plan *plan, int32_t rowset, double limit, void *peak_cn, int32_t *peak_cn_step,
                                int32_t *steps_over);
int trmc_window_courant_tile(int precision, int32_t *rows, int32_t *steps);
int trmc_window_courant_kernel_ms(const trmc_plan *plan, double *ms_out);
/*
 * Threshold exceedance of the last WINDOW: did a row go over its threshold -- bankfull, an action / flood stage, a recurrence
 * flow --, when first, until when and for how long.  For an output row i, a quantity x (flow, velocity or depth: the columns 0,
 * 1, 2 of the window's result out[row][t][c]) and a level k < K (1 <= K <= 4), with x[t], t = 1..nsteps, and the row's threshold
 * th[row][k] in the plan's precision:  over(t) := x[t] > th, compared in the plan's precision -- false if either side is a NaN,
 * and equality is not over.
 *   steps_over[i][k]   number of t with over(t)
 *   first_step[i][k]   the smallest such t, 1-based; 0 if none
 *   last_step[i][k]    the largest such t; 0 if none
 *   longest_run[i][k]  length of the longest run of consecutive t with over(t); 0 if none
 * All four int32 [nrows][K], row-major.  The levels need not be ascending.  -inf is always over: (nsteps, 1, nsteps, nsteps);
 * +inf and a NaN never are.  EVERY step of the window is seen, whatever trmc_plan_set_output_stride keeps of the block.
 *   trmc_plan_set_thresholds   th: host array [nseg][nlevels], row order, the plan's precision; copied to a device table the plan
 *                              handle owns, so thresholds -- static per network -- cross PCIe once, not once per window, and stay
 *                              across windows until replaced.  nlevels == 0 or th == NULL clears the table; nlevels outside 0..4
 *                              is TRMC_EINVAL; TRMC_ESTATE while a window is open or a stream of windows is in progress.  Per
 *                              handle: a clone (trmc_plan_clone) has none until they are set on it, as with reservoir and
 *                              nudging tables and row sets.
 *   trmc_window_exceedance     quantity: TRMC_X_*.  rowset as in trmc_window_summary (-1: every row in row order); a set's row i
 *                              is compared with the thresholds of the row it names.  Any destination may be NULL (all NULL:
 *                              TRMC_EINVAL); only those asked for are formed.  Valid and refused as trmc_window_summary, plus
 *                              TRMC_ESTATE with no thresholds set and TRMC_EINVAL for an unknown quantity or row set.
 *                              Synchronous: one kernel (csrc/k_window_exceed.inc) on the plan's stream behind the window, then
 *                              the columns to the host.  nseg == 0 writes nothing.  Independent of trmc_window_summary and
 *                              trmc_window_courant*: the three may follow one window in any order.
 *   trmc_window_exceedance_tile, trmc_window_exceedance_kernel_ms   as trmc_window_summary_tile / _kernel_ms.  Host only.
 *   trmc_plan_bankfull_depth   dst[nseg], row order, the plan's precision: the bankfull depth the step kernels use (the plan's own
 *                              column; MUSKINGCUNGE f90:55-61:  bw > tw: bw / 0.00001;  bw == tw: bw / (2 z);  else (tw - bw) /
 *                              (2 z), with z = 1 / cs, 1 where cs == 0).  Rows that route no Muskingum-Cunge step at the time of
 *                              the call -- boundary rows, rows declared by trmc_set_reservoirs: a pool's elevation has no
 *                              bankfull -- get +inf.  "Out of bank" is then quantity = TRMC_X_DEPTH against this array.
 * A stream of windows (trmc_stream_*) has no exceedance PRODUCT of the day; it has the exceedance over all its days: below.
 */
enum { TRMC_X_FLOW = 0, TRMC_X_VELOCITY = 1, TRMC_X_DEPTH = 2 };
int trmc_plan_set_thresholds(trmc_plan *plan, int32_t nlevels, const void *th);
int trmc_window_exceedance(trmc_plan *plan, int32_t rowset, int quantity, int32_t *steps_over, int32_t *first_step,
                           int32_t *last_step, int32_t *longest_run);
int trmc_window_exceedance_tile(int precision, int32_t *rows, int32_t *steps);
int trmc_window_exceedance_kernel_ms(const trmc_plan *plan, double *ms_out);
int trmc_plan_bankfull_depth(trmc_plan *plan, void *dst);
/*
 * Threshold exceedance OVER A WHOLE STREAM OF DAYS (trmc_stream_*): the four figures above for the flow of every row against the
 * plan's thresholds, over every step of every day handed over since trmc_stream_begin -- t runs on over the days, 1-based from the
 * stream's first step, and a run that is open at a day's last step goes on at the next day's first: a flood from day 3 to day 6
 * is one run, which is why this is not a product of the day.  The state (per row and level: count, first, last, longest and
 * current run) lives on the device outside the ring, as the totals of TRMC_SUMMARY_TOTAL do; where a day is handed over one pass
 * over the day's flow plane (csrc/k_stream_exceed.inc, beside the summary's) folds it in, in day order.  Nothing of it is a member
 * of trmc_stream_day or crosses to the host per day.  Off (the default): no buffer, no launch.
 *   trmc_stream_set_exceedance  quantity: TRMC_X_FLOW, or -1 for none.  Before trmc_stream_begin; it stays until the next call, as
 *                              trmc_stream_set_summary's mask does; TRMC_ESTATE while a stream is in progress, and without
 *                              thresholds on this plan handle (trmc_plan_set_thresholds: the levels and values a stream uses are
 *                              those set when it begins; trmc_stream_begin is TRMC_ESTATE if they were cleared meanwhile).
 *                              TRMC_EUNSUPPORTED for TRMC_X_VELOCITY and TRMC_X_DEPTH: the ring's planes hold every step's flow
 *                              but only a tile's last depth, and a stream without full_output forms no velocity -- route the
 *                              day in question as a window (trmc_window_exceedance).  TRMC_EINVAL for any other value and on
 *                              the dataflow engine, which runs no stream.  Works with full_output, output_stride or neither,
 *                              with reservoirs (the pool's outflow), gages (the nudged flow) and reservoir data assimilation, in
 *                              both arithmetics and precisions.  The steps are counted in 32 bits on the device:
 *                              trmc_stream_push_day is TRMC_EUNSUPPORTED for the day that would take the stream past 2^31 - 1.
 *   trmc_stream_exceedance     HOST arrays int64 [nseg][K], row order, exactly the K columns of trmc_plan_set_thresholds (any may
 *                              be NULL); synchronous on the copy stream behind the last fold queued: returns when the figures
 *                              over all days handed over so far are on the host and writes that number of days to days_out.
 *                              TRMC_ESTATE when no stream is in progress, when it was begun without an exceedance or when no
 *                              day is complete yet.
 */
int trmc_stream_set_exceedance(trmc_plan *plan, int quantity);
int trmc_stream_exceedance(trmc_plan *plan, int64_t *steps_over, int64_t *first_step, int64_t *last_step, int64_t *longest_run,
                           int64_t *days_out);
/*
 * The Courant number OVER A WHOLE STREAM OF DAYS (trmc_stream_*): trmc_window_courant_summary's three figures for every row, over
 * every step of every day handed over since trmc_stream_begin -- t runs on over the days, 1-based from the stream's first step.
 * cn[t] of a routed row is the reference's courant() at the depth its step t ended on (where the step had no flow: at the upper end
 * of the bracket it would have started from), in the plan's precision and arithmetic, bit for bit what trmc_window_courant gives
 * for the same days routed as windows; a gage row's is that of the un-nudged step; reservoir rows of every type and boundary rows
 * route no step: cn = 0.  Per row
 *     peak_cn       pk = cn[1]; t = 2..: if (cn[t] > pk) -- the first of equal peaks wins, a NaN never replaces a number, a NaN
 *                   at the stream's step 1 stays
 *     peak_cn_step  the step the peak was first reached at (1 for rows that route no step)
 *     steps_over    number of steps with cn[t] > limit, compared in the plan's precision (a NaN is not counted)
 * The state lives on the device outside the ring, as the exceedance's does; where a day is handed over one pass over the day's flow
 * and depth planes and its forcing (csrc/k_stream_courant.inc: one courant() per row-step, no secant solve) folds it in, in day
 * order.  Nothing of it is a member of trmc_stream_day or crosses to the host per day.  It needs every step's depth: without
 * full_output the stream launches the tile-kernel instances that write the depth plane at every step, as for trmc_stream_set_stage;
 * with full_output the depth is read from the day's result.  So trmc_stream_begin refuses what it refuses for stage: TRMC_EUNSUPPORTED
 * in a stream with reservoir data assimilation and, without full_output, on a plan with velocity_on_demand < 0; a plan with lagged
 * rows (trmc_plan_set_lag) runs no stream at all.  Off (the default): no buffer, no launch, the instances of a stream without it.
 *   trmc_stream_set_courant  on != 0: the streams on this plan keep the figures against `limit`; on == 0: none.  Before
 *                            trmc_stream_begin; it stays until the next call.  TRMC_ESTATE while a stream is in progress;
 *                            TRMC_EINVAL on the dataflow engine, which runs no stream, and for a NULL plan.  The steps are counted
 *                            in 32 bits on the device: trmc_stream_push_day is TRMC_EUNSUPPORTED for the day that would take the
 *                            stream past 2^31 - 1.
 *   trmc_stream_courant      HOST arrays [nseg] in row order, peak_cn in the plan's precision (any may be NULL; all NULL, or
 *                            peak_cn_step without peak_cn: TRMC_EINVAL); synchronous on the copy stream behind the last fold
 *                            queued: returns when the figures over all days handed over so far are on the host and writes that
 *                            number of days to days_out.  TRMC_ESTATE when no stream is in progress, when it was begun without
 *                            the Courant number or when no day is complete yet.
 *   trmc_stream_courant_kernel_ms  device time (ms) of the last fold queued, from a pair of events around the kernel; waits for it.
 *                            TRMC_ESTATE as trmc_stream_courant.
 * With the feature on, the launches of every trmc_stream_push_day go behind the last fold queued: the fold reads the time row the
 * day's rows started from, which the rows that end the day `slots - 1` days later write again (csrc/stream.inc, ORDER).
 */
int trmc_stream_set_courant(trmc_plan *plan, int on, double limit);
int trmc_stream_courant(trmc_plan *plan, void *peak_cn, int64_t *peak_cn_step, int64_t *steps_over, int64_t *days_out);
int trmc_stream_courant_kernel_ms(trmc_plan *plan, double *ms_out);
/*
 * DEPTH exceedance OVER A WHOLE STREAM OF DAYS (trmc_stream_*): how long a row is out of bank, or over an action / flood stage, when
 * it first goes over and the longest continuous inundation of the forecast -- trmc_stream_exceedance's four figures, on depth:
 * over(t) := d[t] > th[row][k], compared in the plan's precision (false when either side is a NaN; equality is not over), t running
 * on over the days, 1-based from the stream's first step, a run that is open at a day's last step going on at the next day's first.
 * d[t] is the depth the stream holds for the row and step, the bits trmc_stream_set_stage and full_output hand out: the pool's water
 * elevation at a reservoir row (trmc_set_reservoirs), 0 at a boundary row, the step's own depth at a gage row (nudging changes the
 * flow only).  The figures equal, integer for integer, the plain loop over the days' depths one after the other.
 * It is a SECOND accumulator beside the flow one, not a quantity of trmc_stream_set_exceedance (which goes on refusing
 * TRMC_X_DEPTH): its threshold table is the stream's own -- metres and m3/s never share a table -- and one stream may keep both, flow
 * recurrence and out of bank over the same forecast.  The state lives on the device outside the ring; where a day is handed over
 * one pass over the day's depths (csrc/k_stream_exceed_depth.inc) folds it in, in day order.  Nothing of it is a member of
 * trmc_stream_day or crosses to the host per day.  It needs every step's depth: without full_output the stream launches the
 * tile-kernel instances that write the depth plane at every step, as for trmc_stream_set_stage; with full_output the depth is read
 * from the day's result (a strided walk: slower).  So trmc_stream_begin refuses what it refuses for stage: TRMC_EUNSUPPORTED in a
 * stream with reservoir data assimilation and, without full_output, on a plan with velocity_on_demand < 0.  Off (the default): no
 * buffer, no launch, the instances of a stream without it.
 *   trmc_stream_set_depth_exceedance  th: HOST array [nseg][nlevels], row order, the plan's precision, nlevels 1..4 (for out of bank:
 *                              what trmc_plan_bankfull_depth gives -- +inf, never over, on rows that route no Muskingum-Cunge
 *                              step); copied, before the call returns, into a device table of the stream's own, independent of
 *                              trmc_plan_set_thresholds.  nlevels == 0 withdraws the declaration and releases its buffers.  Before
 *                              trmc_stream_begin; it stays until the next call.  TRMC_ESTATE while a stream is in progress;
 *                              TRMC_EINVAL on the dataflow engine, for nlevels outside 0..4, for a NULL th with nlevels > 0 and
 *                              for a NULL plan.  The steps are counted in 32 bits on the device: trmc_stream_push_day is
 *                              TRMC_EUNSUPPORTED for the day that would take the stream past 2^31 - 1.
 *   trmc_stream_depth_exceedance  HOST arrays int64 [nseg][nlevels], row order (any may be NULL); synchronous on the copy stream
 *                              behind the last fold queued: returns when the figures over all days handed over so far are on the
 *                              host and writes that number of days to days_out.  TRMC_ESTATE when no stream is in progress, when
 *                              it was begun without a depth exceedance or when no day is complete yet.
 *   trmc_stream_depth_exceedance_kernel_ms  device time (ms) of the last fold queued, from a pair of events around the kernel; waits
 *                              for it.  TRMC_ESTATE as trmc_stream_depth_exceedance.
 * With the feature on, the launches of every trmc_stream_push_day go behind the last fold queued, as for the Courant number.
 */
int trmc_stream_set_depth_exceedance(trmc_plan *plan, int32_t nlevels, const void *th);
int trmc_stream_depth_exceedance(trmc_plan *plan, int64_t *steps_over, int64_t *first_step, int64_t *last_step, int64_t *longest_run,
                                 int64_t *days_out);
int trmc_stream_depth_exceedance_kernel_ms(trmc_plan *plan, double *ms_out);
/*
 * PEAK VELOCITY and VELOCITY exceedance OVER A WHOLE STREAM OF DAYS (trmc_stream_*; additions within ABI 19): the third of the
 * quantities the reference hands out per reach, for scour and erosion limits, bridge and culvert limits, wading and boating safety.
 * v[t] of a routed row is, bit for bit, column 1 of the same days routed as a window on the same plan: the reference's velocity at the
 * depth the row's step t ended on, and 0 where the step had no flow, in the plan's precision and arithmetic; a gage row's is that of
 * the un-nudged step (nudging changes the flow only); reservoir rows of every type and boundary rows route no step: v = 0.  t runs
 * on over the days, 1-based from the stream's first step.  Per row
 *     peak_velocity       pk = v[1]; t = 2..: if (v[t] > pk) -- the first of equal peaks wins, a NaN never replaces a number, a
 *                         NaN at the stream's step 1 stays
 *     peak_velocity_step  the step the peak was first reached at (1 for rows that route no step)
 * and, where thresholds were given, per row and level trmc_stream_exceedance's four figures on velocity: over(t) := v[t] > th[row][k],
 * compared in the plan's precision (false when either side is a NaN; equality is not over), a run that is open at a day's last step
 * going on at the next day's first.  A FOURTH accumulator beside the flow, depth and Courant ones, with a threshold table of the
 * stream's own (m/s); one stream may keep all four.  trmc_stream_set_exceedance goes on refusing TRMC_X_VELOCITY.
 * A products-only stream forms no velocity in its step loop, and does not with this on: where a day is handed over one pass over the
 * day's flow and depth planes and its forcing (csrc/k_stream_velocity.inc: one velocity per row-step, no secant solve) folds it in, in
 * day order.  Nothing of it is a member of trmc_stream_day or crosses to the host per day.  It needs every step's depth: without
 * full_output the stream launches the tile-kernel instances that write the depth plane at every step, as for trmc_stream_set_stage;
 * with full_output the depth is read from the day's result.  So trmc_stream_begin refuses what it refuses for stage: TRMC_EUNSUPPORTED
 * in a stream with reservoir data assimilation and, without full_output, on a plan with velocity_on_demand < 0.  Off (the default): no
 * buffer, no launch, the instances of a stream without it.
 *   trmc_stream_set_velocity  on != 0: the streams on this plan keep the figures; th: HOST array [nseg][nlevels], row order, the
 *                            plan's precision, nlevels 0..4 -- 0: the peak and its step only, th may be NULL; copied, before the
 *                            call returns, into a device table of the stream's own.  on == 0 withdraws the declaration and releases
 *                            its buffers (nlevels and th are not read; where nothing was declared, the dataflow engine included,
 *                            it does nothing).  Before trmc_stream_begin; it stays until the next call.
 *                            TRMC_ESTATE while a stream is in progress; TRMC_EINVAL with on != 0 on the dataflow engine, for nlevels outside
 *                            0..4, for a NULL th with nlevels > 0 and for a NULL plan.  The steps are counted in 32 bits on the
 *                            device: trmc_stream_push_day is TRMC_EUNSUPPORTED for the day that would take the stream past 2^31 - 1.
 *   trmc_stream_velocity     HOST arrays in row order: peak [nseg] in the plan's precision, peak_step int64 [nseg], the four
 *                            figures int64 [nseg][nlevels].  Any may be NULL; all NULL, peak_step without peak, or one of the four
 *                            in a stream declared with nlevels = 0: TRMC_EINVAL.  Synchronous on the copy stream behind the last
 *                            fold queued: returns when the figures over all days handed over so far are on the host and writes that
 *                            number of days to days_out.  TRMC_ESTATE when no stream is in progress, when it was begun without the
 *                            declaration or when no day is complete yet.
 *   trmc_stream_velocity_kernel_ms  device time (ms) of the last fold queued, from a pair of events around the kernel; waits for it.
 *                            TRMC_ESTATE as trmc_stream_velocity.
 * With the feature on, the launches of every trmc_stream_push_day go behind the last fold queued, as for the Courant number.
 */
int trmc_stream_set_velocity(trmc_plan *plan, int on, int32_t nlevels, const void *th);
int trmc_stream_velocity(trmc_plan *plan, void *peak, int64_t *peak_step, int64_t *steps_over, int64_t *first_step, int64_t *last_step,
                         int64_t *longest_run, int64_t *days_out);
int trmc_stream_velocity_kernel_ms(trmc_plan *plan, double *ms_out);
/*
 * STAGE HYDROGRAPHS of a stream day: the depth of EVERY step at the rows of the day's row set (trmc_stream_day::rowset, the rows of
 * its hydrographs), [rows of the set][nsteps] in the plan's precision -- column 2 of the same day routed as a window with the full
 * result, at those rows, bit for bit.  A reservoir row (trmc_set_reservoirs) gives its pool's water elevation; nudging changes a
 * gage row's flow only, its stage is the step's own depth; a boundary row has none: 0.  The ring's depth planes have room for every
 * step; a stream told to carry stage launches the tile-kernel instances that write them all (one more coalesced store per row and
 * step) and gathers the set's rows where the day is handed over; the array leaves on the copy stream with the day's other products.
 * A stream with full_output gathers the day's full result instead.  Off (the default): no buffer, no launch, the kernels of a
 * stream without it.
 *   trmc_stream_set_stage   on != 0: the streams begun on this plan from now on carry stage; 0: they do not.  Before
 *                           trmc_stream_begin; it stays until the next call, as trmc_stream_set_summary's mask does.  TRMC_ESTATE
 *                           while a stream is in progress, TRMC_EINVAL on the dataflow engine, which runs no stream.
 *                           trmc_stream_begin is then TRMC_EUNSUPPORTED on a plan whose stream carries reservoir data assimilation
 *                           (trmc_stream_set_reservoir_da: the _rda tile instances do not write the depth plane), and, without
 *                           full_output, with trmc_plan_options.velocity_on_demand < 0 -- as for TRMC_SUMMARY_PEAK_DEPTH.  Works
 *                           with output_stride, full_output or neither, together with every summary part, in both precisions and
 *                           arithmetics.
 *   trmc_stream_stage_dest  where the stage of the NEXT day pushed goes: a page-locked HOST array [rows of that day's set][nsteps]
 *                           (NULL: that day hands none over); the push consumes it, trmc_stream_wait covers it.  TRMC_ESTATE when
 *                           no stream is in progress or it was begun without stage.  The push is TRMC_EINVAL if the day names no
 *                           row set -- the array is then dropped, it does not wait for another day --, and TRMC_ESTATE for a larger
 *                           set than the first one that asked for stage (as for hydrographs).
 */
int trmc_stream_set_stage(trmc_plan *plan, int on);
int trmc_stream_stage_dest(trmc_plan *plan, void *stage_host);
/* on != 0: trmc_upload_forcing turns every NaN of qlat and q0 into 0 on the device, behind the copy.  The reference's reindexed
 * tables hold NaN on waterbody rows (compute.py:1466-1467), which the Muskingum-Cunge rows never read; the drop-in used to screen
 * the caller's frames for them on the host -- 20 ms of a CONUS call.  Default off: values go to the kernels as they are. */
int trmc_plan_set_nan_is_zero(trmc_plan *plan, int on);
/* Page-locked host memory for result arrays: a D2H copy into it runs at the speed of the link instead of through the
 * driver's staging buffers (the 9.4 GB flowveldepth array of a CONUS day: 0.2 s instead of 0.8 s).  The Python host side
 * keeps a small pool of these behind download_fvd(); a C caller may use them for any *_out argument.  Plain memory to the
 * host; release with trmc_host_free, not free(). */
int trmc_host_alloc(size_t bytes, void **ptr_out);
int trmc_host_free(void *ptr);
/* Final state in the reference's q0 layout, new_q0 = fvd[:, [-3,-3,-1]]
 * (AbstractNetwork.py:182-190): q0_out[nseg][3] = (q_T, q_T, depth_T).  D2H. */
int trmc_download_final_state(trmc_plan *plan, void *q0_out);
/* Cost collection for trmc_plan_create_hinted: with it enabled, every routing window also sums, per row,
 * min(secant iterations, 3) (+ 4 in a step that took the compound-channel branch) over its timesteps (2 more bytes read and written per segment-step); trmc_download_cost
 * returns the sums of the last window [nseg] and its length.  Off by default.  No counterpart in the reference. */
int trmc_plan_collect_cost(trmc_plan *plan, int enable);
int trmc_download_cost(trmc_plan *plan, uint16_t *cost_out, int32_t *nsteps_out);

/* Convergence diagnostic: iters_out[nseg] = secant iterations (all retries together, capped at 255) each row
 * spent on the LAST routed timestep (0 for boundary/reservoir rows and rows without flow; the reference
 * does not report its count, MCsingleSegStime_f2py_NOLOOP.f90:83-134).  Rows of slices too narrow for
 * the class partition keep 0.  D2H. */
int trmc_download_iterations(trmc_plan *plan, uint8_t *iters_out);
/* Flow hydrographs of selected rows (e.g. network outlets):
 * out[nrows][nsteps].  dst_is_device != 0: `out` is a device pointer on the
 * plan's device (used to hand outlet hydrographs to RCCL without a host trip). */
int trmc_gather_flow_rows(trmc_plan *plan, const int64_t *rows, int64_t nrows, void *out,
                          int dst_is_device);
/* With out == NULL and dst_is_device != 0 the gathered block stays in plan-owned HBM (results are
 * device-resident); this copies it to the host later: out[nrows][nsteps] of that gather. */
int trmc_download_gathered(trmc_plan *plan, void *out);

/* Throughput mode, copy hidden: what a caller consumes of a window -- the flow hydrographs of a registered row set (the
 * network outlets) and the final state (new_q0, AbstractNetwork.py:182-190) -- is gathered on the plan's stream into
 * plan-owned HBM and copied to the host on a SEPARATE copy stream, so the copy of window k runs beside the kernels of
 * window k + 1 (the planes the gathers read are only overwritten by kernels queued after them).  hyd_host
 * [rows of the set][nsteps] and q0_host [nseg][3] should be page-locked (trmc_host_alloc); either may be NULL.
 * trmc_fetch_wait returns when both arrays are complete; one fetch in flight per plan. */
/* Diagnosis: how many rows the tiles of this plan have routed from the hot list so far (trmc_plan_options.hot_rows; a running
 * total over all launches and windows, modulo 2^31; waits for the device). */
int trmc_plan_hot_rows(trmc_plan *plan, int64_t *rows_out);
/* Diagnosis, host only (an addition within ABI 19; no launch, no device buffer of its own): the hot lists as the launches queued so
 * far leave them -- waits for the device.  cap: entries one list holds (0: the plan has no lists yet -- no tiled window or stream
 * so far, or hot_rows off); hot_home: blocks at the front of the next tile launch that take the list, ceil(cap / (hot_wave_rows *
 * tile_block / 64)); counts[3]: the three lengths, as ATTEMPTED appends -- a row past cap is counted, neither stored nor stamped,
 * and stays with its home block, so a length above cap says the list overflowed (a launch routes min(length, cap) rows from the list
 * it reads); cur_next: which of the three the next launch reads (it appends to (cur_next + 1) % 3 and clears (cur_next + 2) % 3,
 * so counts[cur_next] is what the last launch appended).  tile_block, wave_max: the build's constants -- threads per block of the
 * tile kernel, and the number of hot rows from which a wavefront keeps them (TRMC_HOT_WAVE_MAX).  Any output may be NULL. */
int trmc_plan_hot_state(trmc_plan *plan, int32_t *cap, int32_t *hot_home, int32_t counts[3], int32_t *cur_next, int32_t *tile_block,
                        int32_t *wave_max);

/* Tell a plan which steps a caller will ask for with trmc_fetch_begin_fvd: windows begun afterwards write every stride-th step
 * of (q, v, d) into a block of their own AS THEY GO -- the rows of the tiled leading levels from the kernel that routes them,
 * the others gathered from the time-major planes when the block is fetched -- instead of reading the whole result once more
 * (9.4 GB of a CONUS day) to pick them out.  Results are the same; 0 switches it off.  A fetch with another stride, or of a
 * window that ran without tiles, decimates the result as before. */
int trmc_plan_set_output_stride(trmc_plan *plan, int32_t stride);

/* Diagnosis: a timeline of consecutive windows without a profiler attached (one that serialises what overlaps).  host_ring
 * [nwindows][4] uint64 in page-locked memory (trmc_host_alloc), or NULL to switch it off: window k since the call (level
 * engine, assume_short_ts, leading levels tiled) leaves in row k % nwindows the device's 100 MHz clock when its tiles
 * begin, when its last tile has ended, when its tail begins (the plan's stream is past the set-up and the hand-over) and
 * when its last step launch has ended -- four one-thread launches per window.  Clocks of plans on one device compare. */
int trmc_plan_set_stamps(trmc_plan *plan, void *host_ring, int32_t nwindows);

int trmc_fetch_begin(trmc_plan *plan, int32_t rowset, void *hyd_host, void *q0_host);
/* The same, and with it every `stride`-th step of (q, v, d) of EVERY row -- fvd_host [nseg][nsteps / stride][3], page-locked;
 * the steps stride, 2 stride, ... counted from 1, as trmc_download_fvd_strided -- decimated behind the window's last launch
 * and copied beside the next window: what the reference's writers take of a window at stream_output_internal_frequency
 * (nwm_routing/output.py:209-216).  The plan's next window starts its set-up behind the decimation (behind the copy itself
 * when stride == 1: the whole array then leaves straight from the result buffer).  fvd_host NULL: trmc_fetch_begin. */
int trmc_fetch_begin_fvd(trmc_plan *plan, int32_t rowset, void *hyd_host, void *q0_host, int stride, void *fvd_host);
int trmc_fetch_wait(trmc_plan *plan);

int trmc_get_stats(const trmc_plan *plan, trmc_stats *stats);

/* Convenience: upload + route + download in one call (what the drop-in
 * compute_network_structured shim uses). */
int trmc_route(trmc_plan *plan, int nsteps, int qts_subdivisions, int assume_short_ts,
               const void *qlat, int64_t nq, const void *q0, const void *boundary_fvd,
               void *fvd_out);

/*
 * Batch of independent single-segment steps on the device: the GPU
 * counterpart of calling [R3]/[R2] n times.
 *   in   [n][15]  dt qup quc qdp ql dx bw tw twcc n ncc cs s0 velp depthp
 *   out  [n][6]   qdc velc depthc ck cn X
 * precision 32: float arrays; 64: double arrays.  qdc is taken as 0 on entry,
 * as reach.pyx:55 passes it.
 */
int trmc_segments(int device, int precision, int64_t n, const void *in, void *out);
/* The same in a chosen arithmetic (TRMC_ARITH_EXACT / TRMC_ARITH_TOLERANCE, see trmc_plan_options), and -- iters_out [n]
 * or NULL -- the secant iterations every step took (f90:83-134, all retries together; 0 where nothing was routed). */
int trmc_segments_ex(int device, int precision, int arithmetic, int64_t n, const void *in, void *out, int32_t *iters_out);

/*
 * [R3] with its own signature: the reference's bind(c) entry point of one segment-step,
 * c_muskingcungenwm (src/kernel/muskingum/pyMCsingleSegStime_NoLoop.f90:8-21; C header
 * src/troute-routing/troute/routing/fast_reach/pyMCsingleSegStime_NoLoop.h:1-21; Cython declaration
 * fast_reach/fortran_wrappers.pxd:19-40; call site reach.pyx:37-94).  21 float pointers: dt qup quc qdp ql dx bw tw twcc
 * n ncc cs s0 velp depthp in, qdc velc depthc ck cn X out; no return value.  One step on the device per call (device
 * TRMC_DEVICE, default 0) -- the binding a maintainer swaps in for the Fortran symbol; batches go through trmc_segments.
 * It cannot signal either: on failure the six outputs are NaN and trmc_last_error() holds the reason.
 */
void trmc_muskingcungenwm(float *dt, float *qup, float *quc, float *qdp, float *ql, float *dx, float *bw, float *tw,
                          float *twcc, float *n, float *ncc, float *cs, float *s0, float *velp, float *depthp,
                          float *qdc, float *velc, float *depthc, float *ck, float *cn, float *X);

/*
 * Windows of ONE sequence on TWO plans of the same network (same inputs, same cost hint: the same order), taking turns:
 * the receiving plan's next window starts from the state the source plan's window leaves, handed over on the device --
 * the rows of the source's leading ("wide") levels behind its last tile, on the receiver's tile stream, the others behind
 * its tail, on the receiver's own stream -- so that the receiver's tiles can run while the source's tail is still
 * finishing its window (both plans in sequence mode: trmc_plan_options.sequence_mode).  The source's window must have been queued to its
 * end (trmc_route_advance to nsteps); the receiver must have its forcing staged; the next trmc_route_begin of the receiver
 * takes the handed-over state instead of the one staged with its forcing.  Level engine only.
 */
int trmc_plan_chain_from(trmc_plan *receiver, trmc_plan *source);

/*
 * A second set of WINDOW buffers on the static data of `plan`: the clone shares the original's topology, parameter and
 * constant columns in HBM (no second copy of them, no second flattening) and owns its own forcing, state planes, result
 * and streams -- so that consecutive windows of one sequence can take turns on the two (trmc_plan_chain_from), the next
 * day's forcing travelling to the idle one (trmc_stage_forcing) and its leading levels starting while the current day's
 * narrow levels finish.  The clone inherits the plan's options (trmc_plan_options) and the lag of its rows
 * (trmc_plan_set_lag: set it BEFORE cloning); reservoir / nudging tables, row sets and the cost collection are per clone
 * (set them on each).  Destroy order is free: the shared memory goes with the last user, the window buffers of a destroyed
 * original at once -- and with them everything else of it: a destroyed handle, of an original or of a clone, is simply
 * invalid from then on, for trmc_plan_clone as for every other call (clone from a plan that is alive).
 */
int trmc_plan_clone(trmc_plan *plan, trmc_plan **out);

/*
 * Stage the NEXT window's forcing without waiting for anything: qlat [nseg][nq] (row order, the plan's precision; page-
 * locked host memory -- trmc_host_alloc -- for the copy to run asynchronously) is copied on the plan's copy stream, beside
 * whatever the device is routing; the next trmc_route_begin orders its set-up behind the copy.  The initial state is what
 * trmc_plan_chain_from hands over, else the state the plan's last window left (q0 = NULL of trmc_upload_forcing).  The
 * caller's counterpart in the reference: qlat_values arrives with every compute_network_structured call
 * (mc_reach.pyx:173,:723), the state through AbstractNetwork.new_q0 (AbstractNetwork.py:177-191).  A plan with
 * boundary rows gets their hydrographs of the staged window afterwards (trmc_set_boundary_flow_device before the
 * window begins, or trmc_set_boundary_flow_range while it runs).  The plan is idle (its last window ended), or routing a window that has been queued to its end -- the
 * staging area is only read by a window's set-up, so the copy goes behind that; the state then comes from
 * trmc_plan_chain_from, or, if nobody hands one over, from that very window once it has ended (trmc_route_end before the next
 * trmc_route_begin): one plan routing day after day with every day's forcing on its way a whole window ahead.
 */
int trmc_stage_forcing(trmc_plan *plan, int nsteps, const void *qlat, int64_t nq);

/*
 * Self-check, on the device, of the short exact forms the fp32 step takes under its range proofs (csrc/trmc.hip,
 * DevMathF: sqrt_r, k_of / quot, max_num) against the plain correctly rounded operations they stand for:
 *   what = 0   sqrt(x) for EVERY float x in [2**-60, 2**63], the range of the velocity's radicand under fast_ok
 *              (n and seed are ignored)
 *   what = 1   a / b and max(c, a / b) for n pseudo-random triples drawn from `seed`: a in [2**-10, 2**19] (dx), b in
 *              [2**-76, 2**62] (the celerity of an in-bank point), c in [2**-20, 2**40] (dt) -- significands uniform
 *              over all 2**23, exponents uniform over the ranges, both ends included; one triple in eight has a divisor
 *              whose significand is all ones, all ones but the last bit, zero or one (the hard cases of division by a
 *              refined reciprocal)
 *   what = 2   the refined reciprocal (v_rcp_f32 and one Newton step) against the correctly rounded reciprocal for ALL
 *              2**23 significands of the binade 2**n, n in [-126, 126] (seed is ignored): the hypothesis under which
 *              DevMathF::quot forms a correctly rounded quotient in three operations.  The library's compiled-in set of
 *              excepted significands is EMPTY, so any mismatch is one outside it; a plan created on a device that has one
 *              takes the plain divisions (checked once per device where its first plan is created).
 *   what = 3   DevMathF::quot(a, b, refined reciprocal of b) against a / b: 65 666 divisors (2**16 significands at a stride
 *              of 128 and every one within 64 of 0 and of 2**23 - 1, exponents drawn from [-14, 35]), each with n
 *              numerators drawn from `seed` -- random significands at every exponent distance in [-40, 50], and
 *              a = b*q moved by -1, 0, +1 units in the last place for q next to the boundary between two floats (bits going
 *              on ...0111... or ...1000...) -- and with the numerator +0, whose quotient must be +0
 *   what = 4   the same quotient over the operands of the four Muskingum coefficients (DevMathF::div4), which what = 3 does
 *              not reach: the same 65 666 significands as divisors with exponents drawn from [-21, 52] (2**52 itself as the
 *              top value), each with n numerators drawn from `seed` at ABSOLUTE magnitudes and of both signs -- in turn
 *              2**-60 <= |a| <= 2**60 (ql*dt), 2**-45 <= |a| <= 2**52 twice (the two differences) and 2**-21 <= a <= 2**52
 *              (the positive sum): exponent distances from -112 to +81 -- half of them random significands at exponents
 *              uniform over the range, both ends included, half a = d*q moved by -1, 0, +1 units in the last place for q of
 *              either sign next to the boundary between two floats; and with the numerators +0 and -0 through div4 under
 *              coef_guard's verdict, which must give the +0 and the -0 of the IEEE division (-0, what a negative ql*dt that
 *              underflows is, has to fail the guard).  n + 2 pairs per divisor.
 * checked_out receives the number of values / triples / pairs compared, mismatches_out how many results differ in any
 * bit (0 is the claim).  No routing state is touched.
 */
int trmc_selfcheck_fast_arith(int device, int what, int64_t n, uint64_t seed, int64_t *checked_out, int64_t *mismatches_out);

/*
 * The values behind what = 2 above, for a caller that forms the correctly rounded reciprocals itself: out[s], s in
 * [0, 2**23), receives the device's refined reciprocal of the float with significand s in the binade 2**exponent
 * (exponent in [-126, 126]; `out` holds 2**23 floats of host memory).  No routing state is touched.
 */
int trmc_selfcheck_rcp_values(int device, int exponent, float *out);

/*
 * ---- communicator: the ranks of a multi-GPU job on one node (one process, or thread, per rank) ------------------
 * What ranks exchange on this path is what the reference hands from one sub-network order to the next as
 * flowveldepth_interorder (src/troute-routing/troute/routing/compute.py:882-897, consumed mc_reach.pyx:458-469):
 * hydrographs of the rows where the partition cuts a basin, and at the end the outlet hydrographs -- an all-gather of
 * equal-sized blocks.  Two transports behind one handle:
 *   trmc_comm_init      RCCL over xGMI (librccl.so is loaded when the first communicator is made, never by the
 *                       single-GPU path): rank 0 obtains an id with trmc_comm_unique_id and hands its
 *                       TRMC_COMM_ID_BYTES bytes to the other ranks by any means (a file, a socket); collectives on
 *                       device pointers are asynchronous on the caller's stream, like ncclAllGather.
 *   trmc_comm_init_shm  a POSIX shared-memory segment `name` ("/something", unique to the job) of `capacity_bytes`
 *                       (0: 64 MiB): blocks are staged through host memory, calls are synchronous.  For ranks that
 *                       share a device (RCCL refuses that) and, with device < 0, for hosts without a GPU, where only
 *                       the *_host collectives work.
 * Every rank makes the same sequence of collective calls.
 */
#define TRMC_COMM_ID_BYTES 128
typedef struct trmc_comm trmc_comm;
int trmc_comm_unique_id(void *id_out /* [TRMC_COMM_ID_BYTES] */);
int trmc_comm_init(int rank, int world, const void *id, int device, trmc_comm **out);
int trmc_comm_init_shm(int rank, int world, const char *name, int device, int64_t capacity_bytes, trmc_comm **out);
int trmc_comm_info(const trmc_comm *comm, int32_t *rank, int32_t *world, int32_t *is_rccl);
/* recv_dev[world][bytes] <- every rank's send_dev[bytes]; device pointers on the communicator's device; ordered on
 * `stream` (a hipStream_t; NULL = the null stream) */
int trmc_comm_all_gather(trmc_comm *comm, const void *send_dev, void *recv_dev, int64_t bytes, void *stream);
/* the same for host memory (small control data: a timing, a cost hint); returns when recv is complete */
int trmc_comm_all_gather_host(trmc_comm *comm, const void *send, void *recv, int64_t bytes);
int trmc_comm_barrier(trmc_comm *comm);
void trmc_comm_destroy(trmc_comm *comm);

/* Device buffers, streams and events for the hand-off between a plan's stream (trmc_plan_stream) and the collectives:
 * thin, typed-by-convention wrappers of hipMalloc / hipStream* / hipEvent* so that a host language needs no other GPU
 * library in the process.  `stream` / `event` are hipStream_t / hipEvent_t values. */
int trmc_dev_alloc(int device, int64_t bytes, void **ptr_out); /* zero-filled */
int trmc_dev_free(int device, void *ptr);
int trmc_dev_upload(int device, void *dst_dev, const void *src_host, int64_t bytes);
int trmc_dev_copy(int device, void *dst_dev, const void *src_dev, int64_t bytes, void *stream); /* device to device, on `stream` */
int trmc_dev_download(int device, void *dst_host, const void *src_dev, int64_t bytes, void *stream); /* waits for `stream` */
/* ... and without waiting: complete after trmc_stream_synchronize(stream); dst_host should be page-locked (trmc_host_alloc) */
int trmc_dev_download_async(int device, void *dst_host, const void *src_dev, int64_t bytes, void *stream);
/* dst_dev[i][row_bytes] <- src_dev[index_dev[i]][row_bytes], i < nrows (row_bytes a multiple of 4): picks the outlet
 * rows out of an all-gathered block */
int trmc_dev_gather_rows(int device, const void *src_dev, const int64_t *index_dev, int64_t nrows, int64_t row_bytes,
                         void *dst_dev, void *stream);
int trmc_stream_create(int device, void **stream_out);
/* ... with a priority: -1 low, 0 ordinary, +1 high (clamped to what the device offers).  A plan's own streams are: step
 * launches high, wide tiles ordinary, result transpose and result copies low; with one hardware queue per priority
 * (GPU_MAX_HW_QUEUES=1, which troute_amd sets) a caller's stream shares the queue of the plan stream of its priority, and
 * work in it that waits for an event holds back what was queued behind it in that queue. */
int trmc_stream_create_prio(int device, int priority, void **stream_out);
int trmc_stream_destroy(int device, void *stream);
int trmc_stream_synchronize(int device, void *stream);
int trmc_device_synchronize(int device);
int trmc_event_create(int device, void **event_out);
int trmc_event_destroy(int device, void *event);
int trmc_event_record(int device, void *event, void *stream);
int trmc_stream_wait_event(int device, void *stream, void *event);

#ifdef __cplusplus
}
#endif
#endif /* TRMC_H */
