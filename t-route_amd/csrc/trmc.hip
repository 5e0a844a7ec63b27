// trmc.hip -- HIP kernels and C ABI of the MI355X Muskingum-Cunge engine (gfx950).
//
// Data layout in HBM (plan order = level-major, see topology.hpp):
//   params      8 SoA columns [nseg_pad] (dx bw tw twcc n ncc cs s0) + dt (scalar, or a
//               9th column when the caller's dt column is not uniform)
//   up_ptr/idx  CSR of upstream plan positions (int32)
//   level       int32 [nseg_pad]
//   qlat_tm     [nq][nseg_pad]           forcing, one coalesced row per forcing interval
//   q/v/d_tm    [nsteps+1][nseg_pad]     time-major state AND result: step t reads row
//               t-1 (own previous flow/depth, upstream previous flows) and, without the
//               short-timestep assumption, row t of upstream levels
//   out         [nseg][nsteps][3]        caller layout (mc_reach.pyx:807-813), produced
//               by an LDS-tiled transpose at the end of the route
// nseg_pad rounds nseg up to 64 so every time row starts on a 256-byte boundary.
//
// Launch structure
//   assume_short_ts = 1 : step t of every segment depends only on step t-1
//       (mc_reach.pyx:504-505, :135-136) -> one launch per timestep over all
//       routed segments.
//   assume_short_ts = 0 : (level l, step t) depends on (<l, t) and (l, t-1)
//       -> anti-diagonal wavefront d = l + t; the segments of all levels on
//       one diagonal form ONE contiguous slice of the plan order and run as
//       one launch; nlevels + nsteps - 1 launches in total.
// One thread per segment-step; all loads/stores are unit-stride except the
// upstream gather, which the intra-level ordering keeps near-monotone.
//
// No CPU fallback exists in this library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/trmc.h"
#include "det_pow.h"
#include "det_pow64.h"
#include "mc_segment.hpp"
#include "levelpool.hpp"
#include "reservoir_da.hpp"
#include "topology.hpp"
#include "internal.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

} // namespace
namespace trmc {
int fail_with(int code, const std::string &msg) { return fail(code, msg); }
} // namespace trmc
namespace {

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? TRMC_ENOMEM : TRMC_EHIP,                   \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                    \
    } while (0)

#include "dev_math.inc"
#include "kernels_levels.inc"
#include "kernels_flow.inc"
#include "k_record_tile.inc"
#include "k_window_summary.inc"
#include "k_window_courant.inc"
#include "k_window_exceed.inc"
#include "k_stream_exceed.inc"
#include "k_stream_exceed_depth.inc"
#include "k_stream_courant.inc"
#include "k_stream_velocity.inc"
// ---------------------------------------------------------------- plan
#include "dev_owner.hpp"

// Device time of the last kernel of ONE kind of call on a plan, from a pair of events around it: begin(), the launch, end() on the
// kernel's stream and, once that stream has been synchronised, read().  ms < 0: none timed yet, or the last call failed on its way.
struct KernelTimer {
    DevEvent ev[2];
    double ms = -1.0;
    int begin(hipStream_t st)
    {
        for (DevEvent &e : ev)
            if (int rc = e.ensure(true)) return rc;
        ms = -1.0;
        HIP_TRY(hipEventRecord(ev[0], st));
        return 0;
    }
    int end(hipStream_t st)
    {
        HIP_TRY(hipEventRecord(ev[1], st));
        return 0;
    }
    int read()
    {
        float elapsed = 0;
        HIP_TRY(hipEventElapsedTime(&elapsed, ev[0], ev[1]));
        ms = elapsed;
        return 0;
    }
};

} // namespace

struct RouteRun { // the routing window in progress (route_begin_t .. route_end_t)
    bool active = false;
    int32_t nsteps = 0, qts = 1, short_ts = 0;
    int32_t t_done = 0;           // launches ("diagonals") 1..t_done are queued: rows without lag are at step t_done,
                                  // lagged rows at step t_done - maxlag; the window ends at nsteps + maxlag
    int32_t boundary_through = 0; // boundary rows hold their hydrographs for steps 1..boundary_through
    int32_t tiles_done = 0, launches = 0;
    // wide levels routed K steps per launch with a skew of K steps per level (k_mc_tile); 0 = every level one step per launch
    int32_t wide = 0, wide_k = 0, wide_next = 0, wide_through = 0; // levels; K; tiles queued; last tile the tail waits for
    // second tier: the `mid` levels right below the wide ones, mid_k steps per launch under their own skew (k_mc_tile again),
    // queued on the plan's stream between the tail's launches
    int32_t mid = 0, mid_k = 0, mid_next = 0;
    // cluster tiles (k_mc_ctile): the rows below the wide levels K steps per launch too, cluster level c another tile behind;
    // `wide` is then the plan's cl_from_level (possibly 0: no slices at all), there is no one-step tail and no transposing pass
    bool cl = false;
    int32_t cl_next = 0;          // index of the next cluster tile to queue (they begin at tile `wide`)
    bool tail_active = false;     // the tail launches of this window go to the tail stream
    bool end_queued = false;      // route_end_queue has run for this window
    int32_t dec_stride = 0, dec_keep = 0; // the tiles of this window write the kept steps of their rows into the plan's `dec`
    int32_t dec_lo = 0, dec_hi = 0;       // ... the plan positions [dec_lo, dec_hi) that do
};

// What a plan and its clones (trmc_plan_clone) share: the static data on the device and its host image.  Nothing writes it once
// trmc_plan_create_opt has returned -- but trmc_plan_set_lag, which is refused on a clone and on a plan that has live clones.
// It goes with the last plan that holds it.
struct PlanShared {
    trmc::Topology topo;
    DevBuf params; // 9 columns x nseg_pad
    DevBuf up_ptr, up_idx, up2, level, row_of_pos, pos_of_row, lag; // plan order
    DevBuf lagk, cblk_ptr;               // cluster order (topology.hpp): tiles every position runs behind level 0; the cluster blocks
    DevBuf prio;                         // (dataflow engine) issue priority per wavefront
    DevBuf ticket_map;                   // [nblocks] ticket -> block of a general-mode plan with long main stems (topo.early_blocks)
    DevBuf rank;                         // level rank of a position inside its block
    DevBuf cuq_ptr, cuq_blk, cu_index, cuq_perm; // blocks dealt to compute units by cost (flow_place_blocks)
};

struct StreamRun;
// THE DECLARATION ORDER IS THE ORDER OF TEARDOWN, reversed (members are destroyed last to first): the stream of windows goes
// first (`seq`, the last member), then the plan's own device buffers -- hipFree waits for the device, so whatever was queued has
// run by then -- then its hold on the shared block, and the events and streams at the very end.  So: streams and events stay at
// the top, a new buffer goes below `sh`, and `seq` stays last.  trmc_plan_destroy is `delete`; nothing else releases anything.
struct trmc_plan {
    trmc_plan();  // (both defaulted in stream.inc, where StreamRun is complete)
    ~trmc_plan();
    DevStream stream;
    DevEvent ev[4];
    DevStream stream2;                   // result transpose, overlapped with the step launches
    DevStream wstream;                   // the wide tiles (k_mc_tile), ordinary priority: the narrow tail of the level order runs one
                                         // step per launch on the plan's own high-priority stream BESIDE them -- the tail's 288
                                         // dependent launches are the latency-critical part, the tiles fill whatever they leave
    DevEvent ev_tail;                    // "every tile queued so far is complete" (tile stream -> plan stream)
    std::vector<DevEvent> wide_t0, wide_t1; // timing events around the wide launches of the window (trmc_stats.ms_wide)
    std::vector<DevEvent> tile_ev;       // "time tile b is complete" (main stream -> stream2)
    DevEvent ev_emit;                    // "all tiles emitted" (stream2 -> main stream)
    DevEvent ev_chain[4];                // trmc_plan_chain_from: source's tiles / tail done; this plan's two copies done
    // as the SOURCE of a hand-over (trmc_plan_chain_from): "the receiver has read my planes" (its two copies); my next window's
    // set-up and tiles go behind both
    DevMark mk_released[2];
    DevStream fstream;                   // dataflow engine, second compute stream: consecutive time chunks of a resident window overlap
    DevEvent ev_chunk[2];                // the last launch queued on {stream, fstream}
    DevEvent ev_ctl;                     // ordering of the two compute streams against each other
    DevMark mk_dec;                      // "the copy stream has read `out`" / `dec` (a fetch that copies from them, trmc_fetch_begin_fvd):
                                         // the next window's set-up, which lets its kernels overwrite them, goes behind it
    DevStream cstream;                   // copy stream: D2H of window k runs beside the kernels of window k + 1
    DevStream hstream;                   // ... and the one of the other direction: a staged forcing on its way to the device
    DevEvent ev_fetch_ready;             // "the gathers of a fetch are through" (plan stream -> copy stream)
    DevMark mk_fetch_done;               // "the copies of the fetch in flight have reached the host": trmc_fetch_wait waits for it
    // "the last gather queued on the plan's stream after a window has read the planes" -- what a set-up queued on ANOTHER stream
    // (TRMC_SETUP_ASIDE) waits for before it lets a new window's tiles overwrite them
    DevMark mk_gather;
    KernelTimer t_wsum;                  // the last trmc_window_summary's kernel (trmc_window_summary_kernel_ms)
    KernelTimer t_cour;                  // ... the last trmc_window_courant / _summary's (trmc_window_courant_kernel_ms)
    KernelTimer t_wexc;                  // ... and the last trmc_window_exceedance's (trmc_window_exceedance_kernel_ms): each reports alone
    DevMark mk_forcing;                  // "the staged forcing is in in_qlat" (trmc_stage_forcing: the copy, and in sequence mode its
                                         // transpose, on the forcing's copy stream): the next window's set-up goes behind it
    // trmc_plan_clone: a second set of WINDOW buffers on the static data of the plan it was made from
    std::shared_ptr<PlanShared> sh;
    bool is_clone = false;               // for its whole life, whoever else still holds `sh` (trmc_plan_set_lag)
    int device = 0;
    int precision = 32;
    size_t esz = 4;
    int64_t nseg = 0, nseg_pad = 0, nrouted = 0;
    bool dt_uniform = true;
    double dt = 0.0;
    DevBuf it_prev;
    DevBuf it_sum;                       // per-position cost of the window (trmc_plan_collect_cost)
    bool collect_cost = false;
    bool hinted = false;                 // created with a cost hint: rows of a level are grouped by cost
    bool params_sane = false;            // see DevMathF::fast_ok
    int32_t cost_nsteps = -1;            // nsteps of the window it_sum was collected over
    int32_t maxlag = 0;                  // trmc_plan_set_lag: rows routed `maxlag` launches behind the others
    int64_t wide_safe_pos = -1;          // first plan position that is lagged or fed by a boundary row (-1: not looked for yet)
    // trmc_plan_chain_from: the next window's initial state has been set on the device from another plan's window
    bool chain_staged = false;
    std::vector<int32_t> lag_of_row;
    DevBuf gage_of_pos, da_mode, da_a, da_w, da_nudge; // nudging tables of the staged window
    DevBuf res_of_pos, res_par, res_inflow;             // level-pool reservoirs of the plan
    int64_t nres = 0;
    double res_dt = 0.0;
    std::vector<int64_t> res_rows;       // the rows trmc_set_reservoirs declared (trmc_plan_bankfull_depth)
    DevBuf thresholds;                   // trmc_plan_set_thresholds: [nseg][th_pad] in the plan's precision, row order, +inf behind
    int32_t th_levels = 0, th_pad = 0;   // the th_levels levels of a row (th_pad = 1, 2 or 4: k_window_exceed's KP); 0 levels: none set
    DevBuf res_da;                       // data-assimilation tables of those reservoirs for the staged window (reservoir_da.hpp)
    bool res_da_on = false;
    std::vector<int32_t> res_da_kind, res_da_trow; // what trmc_set_reservoir_da declared, and its tables' shapes {usgs, usace, rfc}:
    int64_t res_da_n[3] = {0, 0, 0}, res_da_ncol[3] = {0, 0, 0}; // fixed for a stream of days that carries them (stream.inc)
    int64_t ngage = 0;
    int64_t nraw = 0;                    // gages inside a reach whose successor reads the un-nudged flow (general mode)
    DevBuf raw_of_pos, da_raw;
    int32_t da_nsteps = -1;
    // per window
    DevBuf in_qlat, in_q0, in_bfvd, qlat_tm, tm, out, scratch, gathered;
    size_t gathered_bytes = 0;
    int64_t nq = 0;
    bool qlat_direct = false;   // qlat_tm was filled by trmc_upload_forcing_packed: no transpose at route time
    DevBuf qlat_alt;            // sequence mode: the STAGED forcing already transposed (trmc_stage_forcing, behind its copy) into
    bool qlat_alt_ready = false; // the buffer the window in progress does not read; the next window's set-up swaps the two
    bool have_boundary = true;  // boundary hydrographs present for the staged window
    int32_t staged_nsteps = -1; // nsteps the staged forcing was uploaded for
    int32_t routed_nsteps = -1; // nsteps of the last completed route
    // dataflow engine (k_mc_flow): the plan is in block order, `tm` holds the granule plane
    bool flow = false;
    uint32_t tag_base = 1;               // tag of step 0 of the current window (0 is never a live tag)
    int32_t tag_span = 0;                // tags the current window may use (nsteps + 1)
    DevBuf d_gran;                       // depth hand-over granules (k_mc_flow_lean)
    int flow_next = 0;                   // which of the two compute streams the next trmc_route_advance uses (only toggles in overlap mode)
    int flow_last = 0;                   // ... and which one the last launch went to
    DevBuf d_state, ticket, dbg;         // depth column; {block ticket, abort flag}
    DevBuf cuq_head;                     // heads of the shared block's compute-unit queues: one set per compute stream
    int32_t ncuq = 0;                    // number of queues (= compute units found), 0 = block tickets
    uint64_t watchdog_ticks = 3000000000ull; // 30 s of wall_clock64 (100 MHz): long enough for a device that is shared or profiled (TRMC_FLOW_WATCHDOG_MS)
    // trmc_plan_options, resolved at creation (a clone copies them)
    struct Opt {
        bool tol = false;                    // TRMC_ARITH_TOLERANCE
        int64_t wide_min_rows = 0;           // <= 0: no wide tier
        int32_t wide_levels = 16, wide_k = 16;
        int64_t mid_min_rows = 0;            // <= 0: no second tier
        int32_t mid_levels = 12, mid_k = 4;
        int32_t tile_perm_group = -1;        // -1: the default (see route_advance_t); 0: off; 1: on
        int32_t hot_rows = -1;               // -1 (default) or 1: with the partition; 0: off
        int32_t cluster_rows = 0;            // rows per cluster block of a short-timestep plan's deeper rows; 0: no cluster order
        int32_t cluster_late_lag = 0;        // tiles the rows fed by boundary rows run behind at least (cluster order)
        int32_t stream_split = 0;            // a stream's slices from this level on ride on the clusters' stream (0: all on the tile stream)
        int32_t hot_wave_rows = 0;           // rows of the hot list per wavefront (0: by the plan's size)
        int32_t velocity_on_demand = 0;      // >= 0: a stream without full_output forms a step's velocity only where it is handed on; < 0: every step's
        bool sequence = false;
        bool flow_overlap = false;
        int32_t flow_lean = 0;
        bool flow_debug = false;
    } opt;
    trmc_stats stats{};
    RouteRun run;
    // asynchronous fetch of what a throughput-mode caller consumes (trmc_fetch_begin / trmc_fetch_wait)
    // trmc_plan_set_output_stride: windows write every out_stride-th step of every row's (q, v, d) into `dec` as they go (the
    // tiled rows from k_mc_tile; the others are gathered from the time-major planes when the block is fetched)
    int32_t out_stride = 0;
    DevBuf dec;
    int32_t dec_stride_done = 0, dec_keep_done = 0, dec_nsteps_done = 0, dec_lo_done = 0, dec_hi_done = 0; // ... what the last window left there
    unsigned long long *stamps = nullptr; // trmc_plan_set_stamps: [nstamp_windows][4] in page-locked host memory (the caller's)
    int32_t nstamp_windows = 0;
    int64_t stamp_seq = -1;               // windows begun since the ring was set, minus one
    DevBuf fetch_hyd, fetch_q0, fetch_fvd;
    bool row0_replaced = false;          // trmc_plan_chain_from has overwritten time row 0 -- the last window's initial state -- since it ended
    bool state_missing = false;          // a forcing is staged and there is no initial state yet: trmc_plan_chain_from must supply it
    bool q0_staged = false;              // in_q0 holds the initial state of the window that is staged (an upload's q0, or the last
                                         // window's final state gathered by an upload with q0 = NULL / trmc_stage_forcing): valid
                                         // until a window consumes it, whatever routed_nsteps says in the meantime
    DevBuf hot_list, hot_cnt;            // k_mc_tile's hot rows (StepArgs::hot_list): [3][hot_cap] positions, [3] lengths
    int32_t hot_cap = 0;
    bool nan_is_zero = false;            // uploads of forcing and state: NaN -> 0 on the device (trmc_plan_set_nan_is_zero)
    int64_t tile_seq = 0;                // tile launches of the wide tier so far, all windows: which of the three lists is read
    DevBuf cls_last;                     // the cost class every wide row showed at the end of its last tile (k_mc_tile's in-block partition)
    std::vector<DevBuf> rowsets;        // positions of registered row sets (trmc_rowset_create)
    std::vector<int64_t> rowset_n;
    std::vector<int32_t> rowset_lag;
    std::vector<int32_t> rowset_lagk;   // cluster order: the largest tile lag among the set's rows (trmc_stream_gather)
    std::unique_ptr<StreamRun> seq;     // trmc_stream_*: a stream of windows on a ring of day slots (stream.inc).  LAST: it goes first
};

namespace {
#include "host_levels.inc"
#include "host_flow.inc"
#include "host_misc.inc"
} // namespace

// ---------------------------------------------------------------- C ABI
extern "C" {
#include "abi.inc"
#include "stream.inc"

} // extern "C"
