// stream.inc -- included by trmc.hip inside its extern "C" block.
//
// A STREAM OF WINDOWS on one plan (trmc_stream_*): what an operational cycle does with the reference -- compute_nhd_routing_v02
// once per run set, every call with that window's qlat_values (mc_reach.pyx:173,:723), the state carried on by new_q0
// (AbstractNetwork.py:177-191; loop nwm_routing/__main__.py:195-333) -- as ONE continuous sequence of tile launches.
//
// With assume_short_ts a row at step t reads flows of step t - 1 only, so a row may run any number of tiles behind the rows
// that drain into it (k_mc_tile, k_mc_ctile: the levels' and the clusters' lag).  Inside one window that skew is paid for at both
// ends -- launches in which only part of the network has work -- and the window's last rows finish `lag` launches after its
// first ones.  Here the tile index simply runs on over the days: launch g routes a position `lag` tiles behind through tile
// g - lag of the stream, whichever day that falls into.  Every launch carries every row -- no ramps, no drain between days, no
// hand-over between plans -- and a day costs exactly nsteps / K launches.  The days live in a ring of SLOTS (time-major flow
// and depth planes, the forcing in plan order, optionally the full result and the decimated one); a row that ends a day leaves
// its state in time row 0 of the next slot.  A day's products (outlet hydrographs, final state, decimated result) are gathered
// from its slot when its LAST row has been queued through it -- `lag_max` launches into the following days -- and copied to
// the caller's page-locked arrays beside the launches that follow; the slot is reused `slots` days later.  What a day can hand
// over is ONE TABLE (P_*, StreamRun::tab below): every product named further down is a row of it, and nothing else lists them.
//
//   trmc_stream_begin   the state: what trmc_upload_forcing staged (or the state the plan's last window left)
//   trmc_stream_push    one more day: its forcing (host, page-locked for an asynchronous copy), where its products go
//   trmc_stream_flush   queue the launches that bring every pushed day to its end (nothing new starts)
//   trmc_stream_wait    block until a day's products are on the host
//   trmc_stream_end     flush, wait for everything, leave the final state staged for whatever routes next
//
// LEVEL-POOL RESERVOIRS AND STREAMFLOW NUDGING ride along (SURVEY f2, f1).  A reservoir row keeps its water elevation in the depth
// slot, so the end-of-day hand-off into the next slot's time row 0 carries it on like any depth.  What is per DAY lives in the
// day's slot, as its forcing does: the reservoirs' inflow record [nres][nsteps] and, for the gage rows declared once with
// trmc_stream_set_gages, the nudging tables (mode, a, w) and the nudge record [ngage][nsteps] -- a row finds them through its
// slot (StepArgs::slot_res, slot_da).  The tables arrive with the day's push (trmc_stream_push_day) on the forcing's stream,
// behind the slot's ev_free and in front of its ev_forcing -- never over a day whose rows still read them -- and the two records
// leave on the copy stream with the day's other products.
//
// RESERVOIR DATA ASSIMILATION (types 2-5: hybrid persistence, RFC series; reservoir_da.hpp) rides along too once the plan's streams
// were told to carry it (trmc_stream_set_reservoir_da; without that trmc_stream_begin still refuses a plan that has such tables).
// trmc_set_reservoir_da is the declaration: which reservoir is of which kind and on which row of which table, the tables' row
// counts, and the state day 0 starts from.  Every day brings its own tables (trmc_stream_day::reservoir_da: observations and
// times counted from the day's start, the RFC parameters of the day); they are laid out on the host as a window's are
// (ResDaRec [nres], then the float rows, every table at its column CAPACITY so that a slot's size is fixed), copied into the
// day's slot with its forcing, and a row reads them through its own slot (StepArgs::slot_rda).  The STATE does not live in the
// ring -- a slot is filled while rows further behind are still in the day before -- but in a carry [nres] that the one thread
// owning a reservoir row reads and writes; when that row ends a day it takes the day's length off the times (reservoir_da_handover,
// mc_reach.pyx:820-837) and leaves the result both in the carry and in the day's record, from where the day's products
// res_da_state_host / res_da_tsidx_host are gathered.  Such a stream forms every step's velocity: the _rda tile instances have no
// LAZYV form (DESIGN.md 10).
//
// A PER-ROW SUMMARY OF THE DAY (trmc_stream_set_summary: peak flow, the step of the peak, mean flow) is one more product, for the
// caller who asks about every reach but wants neither the hourly block nor the full result.  The tile kernels carry nothing for
// it: they already leave every step's flow of every row in the slot's flow plane (the rows below read it there), so when a day is
// handed over one column reduction over that plane (k_stream_summary, beside k_final_state) forms the three arrays [nseg] in row
// order in the slot's summary buffers, and they leave on the copy stream with the day's other products.  Off (the default): no
// buffer, no launch.
// THE PEAK DEPTH of the day (TRMC_SUMMARY_PEAK_DEPTH) is the one part the planes cannot give -- they hold the depth of a tile's last
// step only -- so the tile kernels carry it, in instances of their own (k_mc_tile_pkd, k_mc_ctile_pkd: two registers through a
// tile's steps, two columns [slots][nseg_pad] between the tiles), and k_stream_peak_depth puts the slot's columns into row order
// where the day is handed over.  A stream with full_output runs the instances it always ran and reduces the day's
// out[row][step][2] instead (k_stream_peak_depth_out): the same bits.  Every row of a stream is routed by one of the two tile
// kernels (stream_launch), the hot-list blocks of k_mc_tile included; boundary rows by nobody: (0, 1).
// THE TOTALS over the days of the stream (TRMC_SUMMARY_TOTAL) live outside the ring: [nseg] arrays in row order into which
// k_stream_total folds every day's summary, in day order, right behind the kernels that formed it; trmc_stream_summary_total
// fetches them.
// THRESHOLD EXCEEDANCE OVER THE WHOLE STREAM (trmc_stream_set_exceedance) has that shape too, and for a stronger reason: a flood that
// begins on day 3 and ends on day 6 is ONE run, which no product of a day can hold.  The state -- per row and level the count, the
// first and the last step, the longest and the current run -- is an accumulator outside the ring; k_stream_exceed
// (k_stream_exceed.inc) folds every day's flow plane into it where the day is handed over, in day order, against the plan's
// threshold table, and trmc_stream_exceedance fetches it.  No row of the product table, no member of trmc_stream_day, nothing per
// day on the copy stream.  Flows only: the planes hold a tile's last depth and a products-only stream forms no velocity.  Off (the
// default): no buffer, no launch.
// THE COURANT NUMBER OVER THE WHOLE STREAM (trmc_stream_set_courant) is the third accumulator of that shape: per row the highest
// cn = ck dt / dx, the step it was first reached at and the number of steps with cn > limit, trmc_window_courant_summary's definition
// with the steps counted on over the days.  cn of a row-step is courant_at of a depth the ring already holds (k_stream_courant.inc: no
// secant solve), but it needs EVERY step's depth: such a stream launches the tile instances that write the depth plane at every step
// (stage's: k_mc_tile_dpl, k_mc_ctile_dpl) or, with full_output, reads the day's out[row][step][2] -- and inherits stage's refusals.
// k_stream_courant folds every day where it is handed over, in day order, and trmc_stream_courant fetches the accumulator.
// ORDER.  The fold of day e reads TIME ROW 0 of the day's slot -- step 0 of the day, of the row and of its upstream rows -- later than
// anything else does: the tile launches read it in the day's first tile, the other products read rows 1..nsteps.  That row is written
// again when a row ends day e + slots - 1 (hand_on_row: the next day's slot is this one), first by the rows of lag 0 in the last
// launch of that day's push.  Those launches wait for the slot's ev_free of day e - 1 only, and where the fold runs on the clusters'
// stream the slices' stream never waits for it.  So, with the feature on, the launches of every push go behind the last fold queued
// (stream_push_t: ev_cou; on the fold's own stream by queue order).  That fold is day e's or a later one: day e is handed over at
// launch (e + 1) tpd - 1 + lmax, and the push of day d = e + slots - 1 begins behind launch d tpd - 1, which is later because
// slots >= 2 + ceil((lmax + 1) / tpd) gives (slots - 2) tpd >= lmax + 1.  Rows 1..nsteps, the forcing and the full result of the slot
// are rewritten behind ev_free of day e, which is recorded behind the fold.  Off (the
// default): no buffer, no launch, the instances of a stream without it.
// DEPTH EXCEEDANCE OVER THE WHOLE STREAM (trmc_stream_set_depth_exceedance) -- how long a reach is out of bank or over an action / flood
// stage, when it first goes over, the longest continuous inundation of the forecast -- is a SECOND accumulator of the exceedance's
// shape beside the flow one, not a quantity of it: its threshold table is the stream's own (metres and m3/s never share a table), and
// one stream may keep both.  As the Courant number it needs EVERY step's depth: such a stream launches stage's depth-plane tile
// instances or, with full_output, reads the day's out[row][step][2], and inherits stage's refusals.  k_stream_exceed_depth
// (k_stream_exceed_depth.inc) folds every day where it is handed over, in day order, and trmc_stream_depth_exceedance fetches the
// accumulator.  ORDER: the fold reads the time rows 1..nsteps of the slot's depth plane, or the slot's full result, which are
// rewritten behind the slot's ev_free -- recorded behind the fold -- only; the launches of a push are kept behind the last fold
// queued all the same (stream_push_t: ev_dex), as for the Courant number, so that one rule covers every fold that reads the ring's
// depths.  Off (the default): no buffer, no launch, the instances of a stream without it.
// PEAK VELOCITY AND VELOCITY EXCEEDANCE OVER THE WHOLE STREAM (trmc_stream_set_velocity) is the FOURTH accumulator of that shape: per row
// the highest velocity and the step it was first reached at and, against a threshold table of the stream's own (m/s), the exceedance's
// four figures.  A products-only stream forms no velocity in its step loop; the velocity of a row-step is step_velocity of a depth the
// ring already holds, or 0 where the step had no flow (k_stream_velocity.inc: no secant solve, the tile kernels unchanged), but it
// needs EVERY step's depth: such a stream launches stage's depth-plane tile instances or, with full_output, reads the day's
// out[row][step][2], and inherits stage's refusals.  k_stream_velocity folds every day where it is handed over, in day order, and
// trmc_stream_velocity fetches the accumulator.  ORDER: the fold reads time row 0 of the slot's FLOW plane as the Courant fold does, so
// the launches of a push go behind the last fold queued (stream_push_t: ev_vel).  Off (the default): no buffer, no launch, the
// instances of a stream without it.
// STAGE HYDROGRAPHS (trmc_stream_set_stage): the depth of EVERY step at the rows of the day's row set -- the hydrographs' rows --
// for the caller who compares stage at forecast points and gages, and pool elevation at reservoirs, with action and flood stages.
// A slot's depth plane has room for every step, but the tile kernels write the row of a tile's last step only; the stream that was
// told to carry stage launches the instances that write them all (k_mc_tile_dpl, k_mc_ctile_dpl: one more coalesced store per
// step), and where the day is handed over the hydrographs' gather kernel, pointed at the depth plane, forms the product
// [rows of the set][nsteps] (P_STAGE), which leaves on the copy stream with the day's other products.  A reservoir row gives its
// pool's elevation; nudging changes a gage row's flow only.  A stream with full_output runs the instances it always ran and
// gathers the day's out[row][step][2] instead: the same bits.  Off (the default): no buffer, no launch, the instances of a stream
// without it.
// A DAY AS PACKED CHRTOUT COLUMNS (trmc_stream_set_packed_forcing, trmc_stream_push_day_packed): the caller who runs the reference's
// run-set loop from WRF-Hydro's files hands over what the files hold -- one or two int32 variables [nq][nfeat] in file order -- instead
// of the float array.  The join (feature of every position, uploaded once with the declaration) and the packing facts belong to the
// plan's streams as the gage rows do; a day's raw blocks take the float forcing's road: host -> the staging area (in_qlat, sized at
// trmc_stream_begin for the larger of the two forms) on the forcing's stream, then ONE kernel (k_ingest_packed_day, the window's rule
// ingest_packed_at) decodes, joins and writes the slot's forcing area in the layout k_prep_qlat leaves there.  ORDER: the copies and the
// kernel stand where the float copy and k_prep_qlat stand -- behind the slot's ev_free, in front of its ev_forcing -- and the staging
// area is reused in the forcing stream's queue order, so the raw blocks of a push never land on ones a pending decode still reads;
// float days and packed days may alternate for the same reason.  The decode produces no NaN.
extern "C++" {
// THE PRODUCTS A DAY CAN HAND TO THE HOST, one row of StreamRun::tab each.  trmc_stream_begin fills the row (stream_begin_t: whether
// the stream carries the product, a slot's bytes, where a slot's bytes begin on the device), a push names the day's destinations
// (StreamProd::host), and everything else -- the buffers' life, "has the copy stream anything to carry", the copies, the
// destinations named in front of a push -- is a loop over the rows.  A new product: an enumerator, its row in stream_begin_t, the
// kernel that forms it in stream_complete_day (and, unless it is a summary part, its member of trmc_stream_day in stream_push_t).
enum : int {
    P_HYD,      // outlet hydrographs [rows of the day's set][nsteps]: a slot is sized by the stream's first push
    P_Q0,       // final state [nseg][3]
    P_FVD,      // the (q, v, d) block: no buffer of its own, a slot of `dec` (output_stride) or of `out` (full_output)
    P_NUDGE,    // nudge record [ngage][nsteps]: the slot's record itself, which the gage rows write (StepArgs::da_nudge)
    P_RES,      // reservoir inflow [nres][nsteps]: likewise (StepArgs::res_inflow)
    P_RDA,      // reservoir-DA state float [nres][4] ...
    P_RDA_IDX,  // ... and timeseries_idx int32 [nres] behind it in the same slot
    P_PEAK,     // the summary parts [nseg] in row order, the totals' order (tot[k - P_PEAK]): peak flow,
    P_STEP,     // its step,
    P_MEAN,     // mean flow,
    P_PD,       // peak depth,
    P_PDS,      // its step
    P_N
};
// ... and, behind the rows that the host's table (stream_products.PRODUCTS) mirrors one for one, the products whose destination a
// call of its own names (StreamProdRow::next, as the summary parts'): rows of the same table, P_ALL in all
enum : int {
    P_STAGE = P_N, // stage hydrographs [rows of the day's set][nsteps]: sized and slotted as P_HYD is (trmc_stream_stage_dest)
    P_ALL
};
struct StreamProdRow {
    bool on = false;      // the stream in progress carries the product
    size_t bytes = 0;     // what a day's copy takes (P_HYD, P_STAGE: of the day's row set, stream_prod_bytes)
    size_t stride = 0;    // a slot's bytes on the device: slot s begins at base + s * stride
    char *base = nullptr;
    DevBuf buf;           // [slots][stride], where the product has a buffer of its own
    void *next = nullptr; // (summary parts, stage) where the part of the NEXT day pushed goes: trmc_stream_summary_dest, _depth_dest
};
struct StreamProd {
    int64_t day = -1;
    void *host[P_ALL] = {};         // the day's destinations (NULL: not asked for)
    int32_t rowset = -1;
    bool queued = false;          // the gathers and copies of this day are queued
    DevEvent ev_done;             // ... and this fires when they are through
};
// The order of the members is the order of teardown, reversed, as in trmc_plan: the forcing's stream and the events at the top go
// last, behind the buffers (hipFree waits for the device).  The plan destroys this before anything of its own.
struct StreamRun {
    DevStream fst;                      // the forcing's own stream (H2D + its reordering; the products leave on the plan's copy stream)
    DevEvent ev_begin, ev_gat;
    DevMark mk_bnd;                     // "the boundary rows of the day are in its slot" (trmc_stream_boundary, on a stream of the
                                        // caller's): the next push's forcing stream, or the next launches, go behind it
    DevEvent ev_total;                  // (the totals over the days) the last fold queued is through
    DevEvent ev_exc;                    // (the exceedance over the days) likewise
    DevEvent ev_cou0, ev_cou;           // (the Courant number over the days) around the last fold queued: the second as ev_exc is,
                                        // and what the next day's first launches wait for (stream_push_t)
    DevEvent ev_dex0, ev_dex;           // (the depth exceedance over the days) likewise
    DevEvent ev_vel0, ev_vel;           // (the velocity over the days) likewise
    DevEvent ev_pk0, ev_pk1;            // (days pushed as packed columns) around the last decode queued, on the forcing's stream (timing)
    std::vector<DevEvent> ev_slab;      // ring: "slab launch g is complete" (the cluster launch g + 1 waits for it)
    std::vector<DevEvent> ev_free;      // [slots] the day that used the slot has handed its products over
    std::vector<DevEvent> ev_ready;     // [slots] the gathers of that day are through (copy stream waits)
    std::vector<DevEvent> ev_forcing;   // [slots] the slot's forcing (and boundary rows) are in place
    std::vector<DevEvent> ev_t0, ev_t1; // [slots] around the launches of the day's push on the stream that carries the slices (timing)
    std::vector<StreamProd> prod;       // [slots]
    HostBlock rda_stage;                // page-locked host image of every slot's reservoir-DA tables (the copy runs beside the launches)
    bool active = false;
    int32_t nsteps = 0, qts = 1, K = 0, tpd = 0, slots = 0, W = 0, C = 0, lmax = 0;
    int64_t nq = 0;
    int64_t days_pushed = 0, day_min = 0, days_complete = 0, g_done = -1, launches = 0;
    size_t plane = 0, slot_tm = 0, slot_qlat = 0, slot_out = 0, slot_dec = 0;
    bool want_out = false;
    int32_t dec_stride = 0, dec_keep = 0;
    int32_t rowset = -1;
    DevBuf tm, qlat, out, dec;
    StreamProdRow tab[P_ALL];        // the day's products (above)
    // reservoirs and gages (see the head of this file): per-slot element counts, the per-slot tables, and the gage rows of the
    // streams on this plan (trmc_stream_set_gages: they outlive a stream, unlike the window's tables of trmc_set_nudging)
    size_t slot_res = 0, slot_da = 0;
    DevBuf da_mode, da_a, da_w;
    DevBuf da_q0;                  // [slots][ngage] the days' first observations (NaN = none): the flow a gage row starts the day from
    DevBuf gage_of_pos, gage_pos_dev; // [nseg_pad] gage of a position (-1: none); [ngage] position of a gage
    std::vector<int32_t> gage_pos; // plan position of every declared gage
    int64_t ngage = 0;
    // reservoir data assimilation (see the head of this file).  rda_want / rda_cap_want: trmc_stream_set_reservoir_da, they outlive
    // a stream as the gage rows do; the rest belongs to the stream in progress
    bool rda_want = false, rda = false;
    int64_t rda_cap_want[3] = {0, 0, 0}, rda_cap[3] = {0, 0, 0}; // columns a day's {usgs, usace, rfc} table may have
    int64_t rda_off[3] = {0, 0, 0}, rda_time_off[3] = {0, 0, 0};  // where a slot's observation rows / time rows begin, in floats
    size_t slot_rda = 0;           // bytes of a slot's tables
    float t_end = 0.0f;            // float(nsteps) * float(routing period): what a day's end takes off the times
    DevBuf rda_tab, rda_carry;     // [slots][slot_rda]; ResDaState [nres]
    // the per-row summary of a day (see the head of this file).  sum_want: trmc_stream_set_summary, it outlives a stream as the gage
    // rows do; sum: the mask of the stream in progress
    int32_t sum_want = 0, sum = 0;
    // the peak depth: carry = the tile launches carry it in pkd_d / pkd_at [slots][nseg_pad] (plan order; otherwise the full result
    // is reduced)
    bool carry = false;
    DevBuf pkd_d, pkd_at;
    // stage hydrographs (the head of this file).  stage_want: trmc_stream_set_stage, it outlives a stream as sum_want does; stage: of
    // the stream in progress; dpl: its tile launches write the depth plane at every step (otherwise the full result is gathered)
    bool stage_want = false, stage = false, dpl = false;
    // the Courant number over the days (the head of this file).  cou_want, cou_limit_want: trmc_stream_set_courant, they outlive a
    // stream as stage_want does; cou, cou_limit: of the stream in progress; cou_peak T, cou_step and cou_count int32 [nseg_pad] in plan
    // order; cou_rows: T [nseg], then int64 [2][nseg] behind it on a 256-byte boundary, in row order: what a fetch gathers for the
    // host; cou_days days are folded in (queued).  A stream that carries it has every step's depth: dpl, or the full result.
    bool cou_want = false, cou = false, cou_ms_ok = false; // (cou_ms_ok: a fold of this stream lies between ev_cou0 and ev_cou)
    double cou_limit_want = 0.0, cou_limit = 0.0;
    DevBuf cou_peak, cou_step, cou_count, cou_rows;
    int64_t cou_days = 0;
    // the totals over the days (TRMC_SUMMARY_TOTAL): [nseg] in row order, outside the ring, one per summary part (tot[k - P_PEAK]:
    // the steps are int64 here); tot_days days are folded in (queued)
    DevBuf tot[P_N - P_PEAK];
    int64_t tot_days = 0;
    // the exceedance over the days (the head of this file).  exc_want: trmc_stream_set_exceedance's quantity (-1: none), it outlives
    // a stream as sum_want does; exc, exc_K, exc_KP: of the stream in progress (the plan's levels and its table's row width, which
    // cannot change while a stream runs); exc_acc: int32 [5][exc_KP][nseg_pad] in plan order; exc_rows: int64 [4][nseg][exc_K] in row
    // order, what a fetch gathers for the host; exc_days days are folded in (queued)
    int32_t exc_want = -1, exc = -1, exc_K = 0, exc_KP = 0;
    DevBuf exc_acc, exc_rows;
    int64_t exc_days = 0;
    // the depth exceedance over the days (the head of this file).  dex_K_want, dex_th: trmc_stream_set_depth_exceedance's levels (0:
    // none) and its table on the device, T [nseg][dex_KP_want] in row order, +inf behind the levels asked for -- they outlive a stream as
    // exc_want does; dex_K, dex_KP: of the stream in progress; dex_acc: int32 [5][dex_KP][nseg_pad] in plan order; dex_rows: int64
    // [4][nseg][dex_K] in row order, what a fetch gathers for the host; dex_days days are folded in (queued).  A stream that carries it
    // has every step's depth: dpl, or the full result.
    int32_t dex_K_want = 0, dex_KP_want = 0, dex_K = 0, dex_KP = 0;
    bool dex_ms_ok = false; // (a fold of this stream lies between ev_dex0 and ev_dex)
    DevBuf dex_th, dex_acc, dex_rows;
    int64_t dex_days = 0;
    // the velocity over the days (the head of this file).  vel_want, vel_K_want, vel_th: trmc_stream_set_velocity's declaration, its
    // levels (0: peak and step only) and its table on the device, T [nseg][vel_KP_want] in row order, +inf behind the levels asked
    // for -- they outlive a stream as dex_th does; vel, vel_K, vel_KP: of the stream in progress; vel_peak T and vel_step int32
    // [nseg_pad] in plan order, vel_acc: int32 [5][vel_KP][nseg_pad] in plan order; vel_rows: T [nseg], then int64 [nseg] behind it
    // on a 256-byte boundary, then int64 [4][nseg][vel_K] on the next, in row order: what a fetch gathers for the host; vel_days days
    // are folded in (queued).  A stream that carries it has every step's depth: dpl, or the full result.
    bool vel_want = false, vel = false, vel_ms_ok = false; // (vel_ms_ok: a fold of this stream lies between ev_vel0 and ev_vel)
    int32_t vel_K_want = 0, vel_KP_want = 0, vel_K = 0, vel_KP = 0;
    DevBuf vel_th, vel_peak, vel_step, vel_acc, vel_rows;
    int64_t vel_days = 0;
    // days pushed as packed CHRTOUT columns (the head of this file).  trmc_stream_set_packed_forcing's declaration, which outlives a
    // stream as the gage rows do: the feature axis' length (0: none), whether the days bring two variables, the packing facts, and
    // the feature of every POSITION (-1: the files do not hold the row), int32 [nseg].  pk_ms_ok: a decode of this stream lies
    // between ev_pk0 and ev_pk1
    int64_t pk_nfeat = 0;
    bool pk_two = false, pk_ms_ok = false;
    PackSpec pk_a{}, pk_b{};
    DevBuf pk_feat_of_pos;
};

} // extern "C++"
trmc_plan::trmc_plan() = default;
trmc_plan::~trmc_plan() = default;

extern "C++" {
namespace {

constexpr int kSlabEvents = 8;

// bytes of a packed day's raw blocks in the staging area: one or two variables [nq][nfeat] int32, the second behind the first
inline size_t stream_raw_bytes(const StreamRun &S, bool two) { return (two ? 2 : 1) * (size_t)S.nq * (size_t)S.pk_nfeat * sizeof(int32_t); }

// flows of the boundary rows for one day, [nboundary][nsteps], into the time rows 1..nsteps of a flow plane
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_boundary(const T *__restrict__ q_dev, T *__restrict__ q_plane, int32_t nboundary, int32_t nsteps, int64_t nseg_pad)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)nboundary * nsteps) return;
    const int32_t b = (int32_t)(i / nsteps), t = (int32_t)(i % nsteps) + 1;
    q_plane[(size_t)t * nseg_pad + b] = q_dev[i];
}
// the same from a block of hydrographs whose rows are picked by an index (the all-gathered cut-edge flows of a multi-GPU job)
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_boundary_idx(const T *__restrict__ q_dev, int64_t src_stride, const int64_t *__restrict__ index, T *__restrict__ q_plane,
                      int32_t nboundary, int32_t nsteps, int64_t nseg_pad)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)nboundary * nsteps) return;
    const int32_t b = (int32_t)(i / nsteps), t = (int32_t)(i % nsteps) + 1;
    const int64_t r = index ? index[b] : b;
    q_plane[(size_t)t * nseg_pad + b] = q_dev[(size_t)r * (size_t)src_stride + (size_t)(t - 1)];
}

// A gage row starts a day from the day's first observation where there is one (mc_reach.pyx:404-411: what the drop-in writes into
// a window's initial state on the host; a stream's state lives on the device).  Queued in FRONT of launch g on the stream that
// routes the positions [p0, p1): a gage row `lag` tiles behind begins day (g - lag) / tpd in that launch, and its time row 0 of the
// day's slot was written by the launch before (the end-of-day hand-off; k_init_state for day 0).  The rows below it read that
// row in later launches.  One thread per gage -- a kernel of its own, so that the tile kernels carry nothing for it.
template <class T>
__global__ void __launch_bounds__(kBlock)
k_stream_first_obs(const int32_t *__restrict__ gage_pos, const int32_t *__restrict__ gage_of_pos, const int32_t *__restrict__ lagk,
                   const T *__restrict__ da_q0, T *__restrict__ q_tm, int32_t ngage, int32_t p0, int32_t p1, int64_t g, int32_t tpd,
                   int32_t slots, int64_t day_min, int64_t days, int64_t slot_tm)
{
    const int32_t gi = (int32_t)blockIdx.x * kBlock + (int32_t)threadIdx.x;
    if (gi >= ngage) return;
    const int32_t p = gage_pos[gi];
    if (p < p0 || p >= p1 || gage_of_pos[p] != gi) return; // (two gages on one row: the last listed is the row's)
    const int64_t i = g - lagk[p];
    if (i < 0 || i % tpd != 0) return;
    const int64_t day = i / tpd;
    if (day < day_min || day >= days) return;
    const int32_t slot = (int32_t)(day % slots);
    const T v = da_q0[(size_t)slot * (size_t)ngage + (size_t)gi];
    if (v == v) q_tm[(size_t)slot * (size_t)slot_tm + (size_t)p] = v;
}

// a day's reservoir data-assimilation state for the host: the records its rows left in the slot's tables at their last step ->
// state [nres][4], timeseries_idx [nres] (trmc_download_reservoir_da's layout)
__global__ void __launch_bounds__(kBlock) k_stream_rda_state(const trmc::ResDaRec *__restrict__ rec, float *__restrict__ state,
                                                             int32_t *__restrict__ tsidx, int32_t nres)
{
    const int32_t i = (int32_t)blockIdx.x * kBlock + (int32_t)threadIdx.x;
    if (i >= nres) return;
    const trmc::ResDaState s = rec[i].st;
    state[4 * i + 0] = s.update_time;
    state[4 * i + 1] = s.prev_persisted;
    state[4 * i + 2] = s.persistence_index;
    state[4 * i + 3] = s.persistence_update_time;
    tsidx[i] = s.timeseries_idx;
}

// the tables of one day as a slot holds them (the head of this file), into `img` (slot_rda bytes, zeroed here)
inline void stream_rda_image(const trmc_plan *pl, const StreamRun &S, const trmc_stream_reservoir_da &d, float *img)
{
    std::memset(img, 0, S.slot_rda);
    const trmc_reservoir_da_table *tab[3] = {&d.usgs, &d.usace, &d.rfc};
    for (int k = 0; k < 3; ++k) {
        if (tab[k]->n <= 0) continue;
        std::memcpy(img + S.rda_off[k], tab[k]->obs, (size_t)(tab[k]->n * tab[k]->ncol) * sizeof(float));
        if (k < 2) std::memcpy(img + S.rda_time_off[k], tab[k]->time, (size_t)tab[k]->ncol * sizeof(float));
    }
    trmc::ResDaRec *rec = reinterpret_cast<trmc::ResDaRec *>(img);
    for (int64_t i = 0; i < pl->nres; ++i) {
        trmc::ResDaRec r{};
        r.kind = pl->res_da_kind[(size_t)i];
        if (r.kind != 0) {
            const int k = r.kind == 2 ? 0 : (r.kind == 3 ? 1 : 2);
            const trmc_reservoir_da_table &t = *tab[k];
            const int64_t j = pl->res_da_trow[(size_t)i];
            r.ncol = (int32_t)t.ncol;
            r.obs_off = S.rda_off[k] + j * t.ncol;
            r.time_off = S.rda_time_off[k];
            if (k == 2) {
                const int32_t *ip = t.ipar + 5 * j;
                r.st.timeseries_idx = ip[0];
                r.total_counts = ip[1];
                r.use_forecast = ip[2];
                r.da_timestep = ip[3];
                r.persist_days = ip[4];
                r.reset_idx = d.rfc_reset_idx != 0;
            }
        }
        rec[i] = r;
    }
}

// the stream on which the rows that run furthest behind are routed (a day's products go behind its launches)
inline hipStream_t stream_last(const trmc_plan *pl, const StreamRun &S)
{
    const bool split = pl->opt.stream_split > 0 && pl->opt.stream_split < S.W;
    return (S.C > 0 || split) ? pl->stream : pl->wstream;
}

// what every launch of a stream with `days` days pushed is given (but its day, seq_day, and the tiles' set-up: stream_launch)
template <class T> StepArgs<T> stream_args(trmc_plan *pl, const StreamRun &S, int64_t days)
{
    StepArgs<T> a = step_args<T>(pl, S.nsteps, S.qts);
    a.q_tm = (T *)S.tm.p;
    a.v_tm = nullptr;
    a.d_tm = a.q_tm + S.plane;
    a.qlat_tm = (const T *)S.qlat.p;
    a.out = S.want_out ? (T *)S.out.p : nullptr;
    a.out_vec = sizeof(T) == 4 && S.nsteps % 4 == 0 && S.K % 4 == 0;
    a.level = pl->sh->topo.ncl > 0 ? (const int32_t *)pl->sh->lagk.p : (const int32_t *)pl->sh->level.p;
    a.seq_slots = S.slots;
    a.seq_tpd = S.tpd;
    a.seq_days = (int32_t)days;
    a.seq_day_min = (int32_t)S.day_min;
    a.slot_tm = (int64_t)S.slot_tm;
    a.slot_qlat = (int64_t)S.slot_qlat;
    a.slot_out = (int64_t)S.slot_out;
    a.slot_dec = (int64_t)S.slot_dec;
    // the day's reservoir-inflow record and nudging tables: in the rows' slots (the window's own buffers are not used)
    a.slot_res = (int64_t)S.slot_res;
    a.slot_da = (int64_t)S.slot_da;
    a.res_inflow = (T *)S.tab[P_RES].base;
    a.res_da =S.rda ? S.rda_tab.p : nullptr; // (the _rda instances: the tables of a row's day, the state in the carry)
    a.res_da_carry = S.rda ? S.rda_carry.p : nullptr;
    a.slot_rda = (int64_t)S.slot_rda;
    a.res_t_end = S.t_end;
    a.gage_of_pos = S.ngage > 0 ? (const int32_t *)S.gage_of_pos.p : nullptr;
    a.da_mode = (const uint8_t *)S.da_mode.p;
    a.da_a = (const T *)S.da_a.p;
    a.da_w = (const T *)S.da_w.p;
    a.da_nudge = (T *)S.tab[P_NUDGE].base;
    a.raw_of_pos = nullptr;
    a.da_raw = nullptr;
    if (S.dec_stride > 0) {
        a.dec = (T *)S.dec.p;
        a.dec_stride = S.dec_stride;
        a.dec_keep = S.dec_keep;
    }
    // A stream that assembles no full result hands nobody a velocity but the kept steps' of output_stride -- or nobody at all
    // (hydrographs and final states are flows and depths): only those steps form it.  trmc_plan_options.velocity_on_demand < 0
    // has every step form it anyway (A/B), and so does a stream with reservoir data assimilation (no LAZYV _rda instances).
    if (!S.want_out && pl->opt.velocity_on_demand >= 0 && !S.rda) a.v_every = S.dec_stride > 0 ? S.dec_stride : -1;
    return a;
}

// bytes of product k that the day of `p` hands to the host (0: not carried by the stream, not asked for, or empty)
inline size_t stream_prod_bytes(const trmc_plan *pl, const StreamRun &S, const StreamProd &p, int k)
{
    const StreamProdRow &t = S.tab[k];
    if (!t.on || !p.host[k]) return 0;
    if (k == P_HYD || k == P_STAGE) return p.rowset >= 0 ? (size_t)pl->rowset_n[(size_t)p.rowset] * (size_t)S.nsteps * (size_t)pl->esz : 0;
    return t.bytes;
}

// the gathers and copies that hand day `e` over (its last row has just been queued through it on `pst`)
template <class T> int stream_complete_day(trmc_plan *pl, StreamRun &S, int64_t e, hipStream_t pst)
{
    const int32_t slot = (int32_t)(e % S.slots);
    StreamProd &p = S.prod[(size_t)slot];
    S.days_complete = e + 1;
    if (p.day != e) return fail(TRMC_ESTATE, "internal: the slot of a completed day holds another day");
    const T *q = (const T *)S.tm.p + (size_t)slot * S.slot_tm, *d = q + S.plane;
    size_t bytes[P_ALL]; // what the copy stream has to carry of every product
    bool any = false;
    for (int k = 0; k < P_ALL; ++k) any |= (bytes[k] = stream_prod_bytes(pl, S, p, k)) > 0;
    auto at = [&](int k, bool want = true) { return want ? S.tab[k].base + (size_t)slot * S.tab[k].stride : nullptr; }; // (the product's slot)
    // (the totals fold every day's summary: with them a part is formed whether or not the day's own arrays go to the host)
    const bool total = (S.sum & TRMC_SUMMARY_TOTAL) && pl->nseg > 0;
    const bool want_peak = S.tab[P_PEAK].on && (bytes[P_PEAK] || bytes[P_STEP] || total);
    const bool want_mean = S.tab[P_MEAN].on && (bytes[P_MEAN] || total);
    const bool want_pd = S.tab[P_PD].on && (bytes[P_PD] || bytes[P_PDS] || total);
    if (bytes[P_RDA] || bytes[P_RDA_IDX])
        hipLaunchKernelGGL(k_stream_rda_state, dim3(blocks_for(pl->nres)), dim3(kBlock), 0, pst,
                           (const trmc::ResDaRec *)((const char *)S.rda_tab.p + (size_t)slot * S.slot_rda), (float *)at(P_RDA), (int32_t *)at(P_RDA_IDX),
                           (int32_t)pl->nres);
    if (bytes[P_HYD]) {
        const int64_t nrows = pl->rowset_n[(size_t)p.rowset];
        hipLaunchKernelGGL((k_gather_rows<T>), dim3(blocks_for(nrows * S.nsteps)), dim3(kBlock), 0, pst, q,
                           (const int32_t *)pl->rowsets[(size_t)p.rowset].p, (T *)at(P_HYD), nrows, pl->nseg_pad, S.nsteps, 1);
    }
    if (bytes[P_STAGE]) { // (the depth of every step at the same rows: from the depth plane, or from the full result)
        const int64_t nrows = pl->rowset_n[(size_t)p.rowset];
        if (S.dpl)
            hipLaunchKernelGGL((k_gather_rows<T>), dim3(blocks_for(nrows * S.nsteps)), dim3(kBlock), 0, pst, d,
                               (const int32_t *)pl->rowsets[(size_t)p.rowset].p, (T *)at(P_STAGE), nrows, pl->nseg_pad, S.nsteps, 1);
        else
            hipLaunchKernelGGL((k_gather_rows_depth_out<T>), dim3(blocks_for(nrows * S.nsteps)), dim3(kBlock), 0, pst,
                               (const T *)S.out.p + (size_t)slot * S.slot_out, (const int32_t *)pl->rowsets[(size_t)p.rowset].p,
                               (const int32_t *)pl->sh->row_of_pos.p, (T *)at(P_STAGE), nrows, S.nsteps);
    }
    if (bytes[P_Q0])
        hipLaunchKernelGGL((k_final_state<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, q, d, (const int32_t *)pl->sh->row_of_pos.p,
                           (T *)at(P_Q0), (int32_t)pl->nseg, pl->nseg_pad, S.nsteps, 1, S.nsteps);
    T *const sum_peak = (T *)at(P_PEAK, want_peak), *const sum_mean = (T *)at(P_MEAN, want_mean), *const sum_pd = (T *)at(P_PD, want_pd);
    int32_t *const sum_step = (int32_t *)at(P_STEP, want_peak), *const sum_pds = (int32_t *)at(P_PDS, want_pd);
    if (want_peak || want_mean)
        hipLaunchKernelGGL((k_stream_summary<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, q, (const int32_t *)pl->sh->row_of_pos.p, sum_peak,
                           sum_step, sum_mean, (int32_t)pl->nseg, pl->nseg_pad, S.nsteps);
    if (want_pd && S.carry)
        hipLaunchKernelGGL((k_stream_peak_depth<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, (const T *)S.pkd_d.p + (size_t)slot * (size_t)pl->nseg_pad,
                           (const int32_t *)S.pkd_at.p + (size_t)slot * (size_t)pl->nseg_pad, (const int32_t *)pl->sh->row_of_pos.p, sum_pd, sum_pds,
                           (int32_t)pl->nseg, (int32_t)pl->sh->topo.nboundary);
    else if (want_pd)
        hipLaunchKernelGGL((k_stream_peak_depth_out<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, (const T *)S.out.p + (size_t)slot * S.slot_out,
                           sum_pd, sum_pds, (int32_t)pl->nseg, S.nsteps);
    if (total) {
        hipLaunchKernelGGL((k_stream_total<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, (const T *)sum_peak, (const int32_t *)sum_step,
                           (const T *)sum_mean, (const T *)sum_pd, (const int32_t *)sum_pds, (T *)S.tot[0].p, (int64_t *)S.tot[1].p, (T *)S.tot[2].p,
                           (T *)S.tot[3].p, (int64_t *)S.tot[4].p, (int32_t)pl->nseg, e, S.nsteps);
        HIP_TRY(hipEventRecord(S.ev_total, pst));
        S.tot_days = e + 1;
    }
    if (S.exc >= 0 && pl->nseg > 0) { // (the day's flow plane folded into the exceedance over the days: in day order, before the slot is freed)
        const int32_t t0 = (int32_t)(e * S.nsteps);   // (stream_push_t keeps the stream's steps within int32)
        auto fold = [&](auto kp) {
            hipLaunchKernelGGL((k_stream_exceed<T, decltype(kp)::value>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, q,
                               (const int32_t *)pl->sh->row_of_pos.p, (const T *)pl->thresholds.p, (int32_t *)S.exc_acc.p, (int32_t)pl->nseg,
                               pl->nseg_pad, S.nsteps, t0);
        };
        switch (S.exc_KP) {
        case 1: fold(std::integral_constant<int, 1>{}); break;
        case 2: fold(std::integral_constant<int, 2>{}); break;
        case 4: fold(std::integral_constant<int, 4>{}); break;
        default: return fail(TRMC_ESTATE, "internal: the stream's exceedance has no threshold table");
        }
        HIP_TRY(hipEventRecord(S.ev_exc, pst));
        S.exc_days = e + 1;
    }
    if (S.cou && pl->nseg > 0) { // (the day folded into the Courant number over the days: in day order, before the slot is freed)
        StreamCourantArgs<T> c;
        c.par = (const T *)pl->sh->params.p;
        c.nseg_pad = pl->nseg_pad;
        c.up_ptr = (const int32_t *)pl->sh->up_ptr.p;
        c.up_idx = (const int32_t *)pl->sh->up_idx.p;
        c.res_of_pos = pl->nres > 0 ? (const int32_t *)pl->res_of_pos.p : nullptr;
        c.q_tm = q;
        c.d0 = d;
        if (S.dpl) { // (every step's depth: in the slot's depth plane, or in the full result -- stage's two sources)
            c.row_of_pos = nullptr;
            c.d1 = d + (size_t)pl->nseg_pad;
            c.d_row = 1;
            c.d_step = pl->nseg_pad;
        } else {
            c.row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
            c.d1 = (const T *)S.out.p + (size_t)slot * S.slot_out + 2;
            c.d_row = 3 * (int64_t)S.nsteps;
            c.d_step = 3;
        }
        c.qlat = (const T *)S.qlat.p + (size_t)slot * S.slot_qlat;
        c.peak = (T *)S.cou_peak.p;
        c.step = (int32_t *)S.cou_step.p;
        c.count = (int32_t *)S.cou_count.p;
        c.nseg = (int32_t)pl->nseg;
        c.nboundary = (int32_t)pl->sh->topo.nboundary;
        c.nsteps = S.nsteps;
        c.qts = S.qts;
        c.t0 = (int32_t)(e * S.nsteps); // (stream_push_t keeps the stream's steps within int32)
        c.sane = pl->params_sane ? 1 : 0;
        c.limit = (T)S.cou_limit;
        HIP_TRY(hipEventRecord(S.ev_cou0, pst)); // (with ev_cou: the fold's device time, trmc_stream_courant_kernel_ms)
        bool tol = false; // (the plan's arithmetic, as window_courant_launch)
        if constexpr (std::is_same<T, float>::value) {
            tol = pl->opt.tol;
            if (tol) hipLaunchKernelGGL((k_stream_courant<float, true>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, c);
        }
        if (!tol) hipLaunchKernelGGL((k_stream_courant<T, false>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, c);
        HIP_TRY(hipEventRecord(S.ev_cou, pst));
        S.cou_days = e + 1;
        S.cou_ms_ok = true;
    }
    if (S.dex_K > 0 && pl->nseg > 0) { // (the day's depths folded into the depth exceedance over the days: in day order, before the slot is freed)
        const int32_t t0 = (int32_t)(e * S.nsteps);   // (stream_push_t keeps the stream's steps within int32)
        // (every step's depth: in the slot's depth plane from time row 1, or in the full result -- stage's two sources)
        const T *const d1 = S.dpl ? d + (size_t)pl->nseg_pad : (const T *)S.out.p + (size_t)slot * S.slot_out + 2;
        const int64_t d_row = S.dpl ? 1 : 3 * (int64_t)S.nsteps, d_step = S.dpl ? pl->nseg_pad : 3;
        auto fold = [&](auto kp) {
            hipLaunchKernelGGL((k_stream_exceed_depth<T, decltype(kp)::value>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, d1,
                               (const int32_t *)pl->sh->row_of_pos.p, (const T *)S.dex_th.p, (int32_t *)S.dex_acc.p, (int32_t)pl->nseg,
                               pl->nseg_pad, S.nsteps, t0, S.dpl ? 0 : 1, d_row, d_step);
        };
        HIP_TRY(hipEventRecord(S.ev_dex0, pst)); // (with ev_dex: the fold's device time, trmc_stream_depth_exceedance_kernel_ms)
        switch (S.dex_KP) {
        case 1: fold(std::integral_constant<int, 1>{}); break;
        case 2: fold(std::integral_constant<int, 2>{}); break;
        case 4: fold(std::integral_constant<int, 4>{}); break;
        default: return fail(TRMC_ESTATE, "internal: the stream's depth exceedance has no threshold table");
        }
        HIP_TRY(hipEventRecord(S.ev_dex, pst));
        S.dex_days = e + 1;
        S.dex_ms_ok = true;
    }
    if (S.vel && pl->nseg > 0) { // (the day folded into the velocity over the days: in day order, before the slot is freed)
        StreamVelocityArgs<T> c;
        c.par = (const T *)pl->sh->params.p;
        c.nseg_pad = pl->nseg_pad;
        c.up_ptr = (const int32_t *)pl->sh->up_ptr.p;
        c.up_idx = (const int32_t *)pl->sh->up_idx.p;
        c.res_of_pos = pl->nres > 0 ? (const int32_t *)pl->res_of_pos.p : nullptr;
        c.row_of_pos = (const int32_t *)pl->sh->row_of_pos.p;
        c.q_tm = q;
        // (every step's depth: in the slot's depth plane from time row 1, or in the full result -- stage's two sources)
        c.by_row = S.dpl ? 0 : 1;
        c.d1 = S.dpl ? d + (size_t)pl->nseg_pad : (const T *)S.out.p + (size_t)slot * S.slot_out + 2;
        c.d_row = S.dpl ? 1 : 3 * (int64_t)S.nsteps;
        c.d_step = S.dpl ? pl->nseg_pad : 3;
        c.qlat = (const T *)S.qlat.p + (size_t)slot * S.slot_qlat;
        c.th = (const T *)S.vel_th.p;
        c.peak = (T *)S.vel_peak.p;
        c.step = (int32_t *)S.vel_step.p;
        c.acc = (int32_t *)S.vel_acc.p;
        c.nseg = (int32_t)pl->nseg;
        c.nboundary = (int32_t)pl->sh->topo.nboundary;
        c.nsteps = S.nsteps;
        c.qts = S.qts;
        c.t0 = (int32_t)(e * S.nsteps); // (stream_push_t keeps the stream's steps within int32)
        c.sane = pl->params_sane ? 1 : 0;
        bool tol = false; // (the plan's arithmetic, as window_courant_launch)
        if constexpr (std::is_same<T, float>::value) tol = pl->opt.tol;
        auto fold = [&](auto kp) {
            constexpr int KP = decltype(kp)::value;
            if constexpr (std::is_same<T, float>::value) {
                if (tol) hipLaunchKernelGGL((k_stream_velocity<float, true, KP>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, c);
            }
            if (!tol) hipLaunchKernelGGL((k_stream_velocity<T, false, KP>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, c);
        };
        HIP_TRY(hipEventRecord(S.ev_vel0, pst)); // (with ev_vel: the fold's device time, trmc_stream_velocity_kernel_ms)
        switch (S.vel_KP) {
        case 0: fold(std::integral_constant<int, 0>{}); break;
        case 1: fold(std::integral_constant<int, 1>{}); break;
        case 2: fold(std::integral_constant<int, 2>{}); break;
        case 4: fold(std::integral_constant<int, 4>{}); break;
        default: return fail(TRMC_ESTATE, "internal: the stream's velocity has no threshold table");
        }
        HIP_TRY(hipEventRecord(S.ev_vel, pst));
        S.vel_days = e + 1;
        S.vel_ms_ok = true;
    }
    HIP_TRY(hipGetLastError());
    if (!any) {
        HIP_TRY(hipEventRecord(S.ev_free[(size_t)slot], pst));
        HIP_TRY(hipEventRecord(p.ev_done, pst));
        p.queued = true;
        return 0;
    }
    HIP_TRY(hipEventRecord(S.ev_ready[(size_t)slot], pst));
    HIP_TRY(hipStreamWaitEvent(pl->cstream, S.ev_ready[(size_t)slot], 0));
    for (int k = 0; k < P_ALL; ++k)
        if (bytes[k]) HIP_TRY(hipMemcpyAsync(p.host[k], at(k), bytes[k], hipMemcpyDeviceToHost, pl->cstream));
    HIP_TRY(hipEventRecord(S.ev_free[(size_t)slot], pl->cstream));
    HIP_TRY(hipEventRecord(p.ev_done, pl->cstream));
    p.queued = true;
    return 0;
}

// the launches (g_from .. g_to] of the stream with `days` days pushed: the slices on the tile stream, the clusters on the
// plan's own (cluster launch g waits for slab launch g - 1: k_mc_ctile); days that reach their end are handed over
template <class T> int stream_launch(trmc_plan *pl, StreamRun &S, int64_t g_from, int64_t g_to, int64_t days)
{
    const trmc::Topology &tp = pl->sh->topo;
    const bool tol = pl->opt.tol;
    // (trmc_plan_options.stream_split = s > 0: the slices from level s on are a launch of their own on the clusters' stream, in front of
    // the cluster blocks -- two chains of launches whose ends do not coincide, each filling the device while the other drains)
    const int32_t split = (pl->opt.stream_split > 0 && pl->opt.stream_split < S.W) ? pl->opt.stream_split : S.W;
    const int32_t w0 = tp.lvl_ptr[0], w1 = tp.lvl_ptr[split], w2 = tp.lvl_ptr[S.W];
    hipStream_t wst = pl->wstream, cst = pl->stream;
    hipStream_t pst = stream_last(pl, S);
    const int32_t ncblk = S.C > 0 ? (int32_t)tp.cblk_ptr.size() - 1 : 0;
    // the slices on the tile stream carry the partition and the hot rows as a window's do (tile_args: trmc_stream_begin has made
    // and cleared the buffers); the deeper slices and the clusters the partition alone -- the lists belong to the tile stream's
    // launches
    StepArgs<T> as = stream_args<T>(pl, S, days);
    tile_args(pl, S.W, as);
    StepArgs<T> a = as;
    a.hot_list = a.hot_cnt = nullptr;
    // (the rows' peak depth of the day rides in these launches: the slots' two columns -- NULL: the instances of a stream without it;
    // S.dpl: the instances that write the depth plane at every step)
    T *const pk_d = S.carry ? (T *)S.pkd_d.p : nullptr;
    int32_t *const pk_at = S.carry ? (int32_t *)S.pkd_at.p : nullptr;
    for (int64_t g = g_from + 1; g <= g_to; ++g) {
        a.seq_day = as.seq_day = (int32_t)(g / S.tpd);
        const int32_t tile = (int32_t)(g % S.tpd);
        auto first_obs = [&](hipStream_t st, int32_t p0, int32_t p1) {
            if (S.ngage > 0 && p1 > p0)
                hipLaunchKernelGGL((k_stream_first_obs<T>), dim3(blocks_for(S.ngage)), dim3(kBlock), 0, st, (const int32_t *)S.gage_pos_dev.p,
                                   (const int32_t *)S.gage_of_pos.p, a.level, (const T *)S.da_q0.p, (T *)S.tm.p, (int32_t)S.ngage, p0, p1, g, S.tpd,
                                   S.slots, S.day_min, days, (int64_t)S.slot_tm);
        };
        if (S.W > 0 && w1 > w0) {
            first_obs(wst, w0, w1);
            if (as.hot_list) tile_turn(pl, as);
            launch_tile<T>(wst, as, w0, w1, tile, S.K, tol, pk_d, pk_at, S.dpl);
            HIP_TRY(hipEventRecord(S.ev_slab[(size_t)(g % kSlabEvents)], wst));
            ++S.launches;
        }
        if (ncblk > 0 || w2 > w1) {
            if (S.W > 0 && g >= 1) HIP_TRY(hipStreamWaitEvent(cst, S.ev_slab[(size_t)((g - 1) % kSlabEvents)], 0));
            first_obs(cst, w1, (int32_t)pl->nseg_pad);
            if (w2 > w1) { // (the deeper slices)
                launch_tile<T>(cst, a, w1, w2, tile, S.K, tol, pk_d, pk_at, S.dpl);
                ++S.launches;
            }
            if (ncblk > 0) {
                launch_ctile<T>(cst, a, (const int32_t *)pl->sh->cblk_ptr.p, 0, ncblk, tile, S.K, tol, pk_d, pk_at, S.dpl);
                ++S.launches;
            }
        }
        HIP_TRY(hipGetLastError());
        S.g_done = g;
        // day e is through when its last row (lmax tiles behind) has done tile (e + 1) tpd - 1
        const int64_t i_last = g - S.lmax;
        if (i_last >= 0 && (i_last + 1) % S.tpd == 0) {
            const int64_t e = (i_last + 1) / S.tpd - 1;
            if (e >= S.days_complete && e < days)
                if (int rc = stream_complete_day<T>(pl, S, e, pst)) return rc;
        }
    }
    return 0;
}

template <class T> int stream_begin_t(trmc_plan *pl, int nsteps, int qts, int slots, int full_output, int output_stride)
{
    const trmc::Topology &tp = pl->sh->topo;
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    StreamRun &S = *pl->seq;
    const int32_t K = pl->opt.wide_k > 0 ? pl->opt.wide_k : 16;
    if (nsteps % K != 0) return fail(TRMC_EINVAL, "a stream of windows needs nsteps to be a multiple of the plan's wide_k (" + std::to_string(K) + ")");
    S.nsteps = nsteps;
    S.qts = qts;
    S.K = K;
    S.tpd = nsteps / K;
    S.W = tp.ncl > 0 ? tp.cl_from_level : tp.nlevels;
    S.C = tp.ncl;
    S.lmax = std::max(0, S.W + S.C - 1);
    const int32_t need = 2 + (S.lmax + 1 + S.tpd - 1) / S.tpd;
    S.slots = std::max(need, slots);
    S.nq = pl->nq;
    const size_t np = (size_t)pl->nseg_pad;
    S.plane = (size_t)(nsteps + 1) * np;
    S.slot_tm = 2 * S.plane; // [flow plane][depth plane]
    S.slot_qlat = (size_t)S.nq * np;
    S.want_out = full_output != 0;
    S.slot_out = S.want_out ? (size_t)pl->nseg * nsteps * 3 : 0;
    S.dec_stride = output_stride > 0 ? output_stride : 0;
    S.dec_keep = S.dec_stride > 0 ? nsteps / S.dec_stride : 0;
    if (S.dec_stride > 0 && S.dec_keep < 1) return fail(TRMC_EINVAL, "output_stride exceeds nsteps");
    S.slot_dec = (size_t)pl->nseg * S.dec_keep * 3;
    if (int rc = S.tm.ensure((size_t)S.slots * S.slot_tm * sizeof(T))) return rc;
    if (int rc = S.qlat.ensure((size_t)S.slots * S.slot_qlat * sizeof(T))) return rc;
    // the staging area of a day's forcing, for the larger of the float array and the declared raw blocks (up to twice its bytes)
    if (int rc = pl->in_qlat.ensure(std::max((size_t)pl->nseg * (size_t)S.nq * sizeof(T), stream_raw_bytes(S, S.pk_two)))) return rc;
    S.pk_ms_ok = false;
    if (S.pk_nfeat > 0)
        for (DevEvent *e : {&S.ev_pk0, &S.ev_pk1})
            if (int rc = e->ensure(true)) return rc;
    if (S.want_out)
        if (int rc = S.out.ensure((size_t)S.slots * S.slot_out * sizeof(T))) return rc;
    if (S.dec_stride > 0)
        if (int rc = S.dec.ensure((size_t)S.slots * S.slot_dec * sizeof(T))) return rc;
    S.slot_res = (size_t)pl->nres * (size_t)nsteps;
    S.slot_da = (size_t)S.ngage * (size_t)nsteps;
    if (S.slot_da > 0) {
        if (int rc = S.da_mode.ensure((size_t)S.slots * S.slot_da)) return rc;
        for (DevBuf *b : {&S.da_a, &S.da_w})
            if (int rc = b->ensure((size_t)S.slots * S.slot_da * sizeof(T))) return rc;
        if (int rc = S.da_q0.ensure((size_t)S.slots * (size_t)S.ngage * sizeof(T))) return rc;
    }
    // the peak depth of the day: carried by the tile launches unless the stream assembles the full result, which is reduced then
    S.sum = S.sum_want;
    const bool pd = (S.sum & TRMC_SUMMARY_PEAK_DEPTH) != 0;
    S.carry = pd && !S.want_out;
    if (S.carry && pl->opt.velocity_on_demand < 0)
        return fail(TRMC_EUNSUPPORTED, "the peak depth of a stream without full_output is carried by the tile kernels' on-demand-velocity instances: "
                                       "not with trmc_plan_options.velocity_on_demand < 0");
    S.rda = pl->nres > 0 && pl->res_da_on && S.rda_want;
    if (S.rda && pd)
        return fail(TRMC_EUNSUPPORTED, "the peak depth of the day (TRMC_SUMMARY_PEAK_DEPTH) is not supported in a stream with reservoir data "
                                       "assimilation: the _rda tile instances do not carry it");
    for (DevBuf *b : {&S.pkd_d, &S.pkd_at})
        if (!S.carry) b->release();
    if (S.carry) {
        if (int rc = S.pkd_d.ensure((size_t)S.slots * np * sizeof(T))) return rc;
        if (int rc = S.pkd_at.ensure((size_t)S.slots * np * sizeof(int32_t))) return rc;
    }
    // stage hydrographs, and the Courant number over the days, which needs every step's depth as well: the tile launches write the
    // depth plane at every step unless the stream assembles the full result, which is gathered (read) then
    S.stage = S.stage_want;
    S.cou = S.cou_want;
    S.cou_limit = S.cou_limit_want;
    S.cou_days = 0;
    S.cou_ms_ok = false;
    S.dex_K = S.dex_K_want;
    S.dex_KP = S.dex_KP_want;
    S.dex_days = 0;
    S.dex_ms_ok = false;
    S.vel = S.vel_want;
    S.vel_K = S.vel ? S.vel_K_want : 0;
    S.vel_KP = S.vel ? S.vel_KP_want : 0;
    S.vel_days = 0;
    S.vel_ms_ok = false;
    S.dpl = (S.stage || S.cou || S.dex_K > 0 || S.vel) && !S.want_out;
    if (S.dpl && pl->opt.velocity_on_demand < 0)
        return fail(TRMC_EUNSUPPORTED, "the stage, and the depths the Courant number, the depth exceedance and the velocity over the days are "
                                       "formed from, of a stream without full_output are written by the tile kernels' on-demand-velocity "
                                       "instances: not with trmc_plan_options.velocity_on_demand < 0");
    if (S.rda && S.stage)
        return fail(TRMC_EUNSUPPORTED, "stage hydrographs (trmc_stream_set_stage) are not supported in a stream with reservoir data "
                                       "assimilation: the _rda tile instances do not write the depth plane");
    if (S.rda && S.cou)
        return fail(TRMC_EUNSUPPORTED, "the Courant number over the days (trmc_stream_set_courant) is not supported in a stream with reservoir "
                                       "data assimilation: the _rda tile instances do not write the depth plane");
    if (S.rda && S.dex_K > 0)
        return fail(TRMC_EUNSUPPORTED, "the depth exceedance over the days (trmc_stream_set_depth_exceedance) is not supported in a stream with "
                                       "reservoir data assimilation: the _rda tile instances do not write the depth plane");
    if (S.rda && S.vel)
        return fail(TRMC_EUNSUPPORTED, "the velocity over the days (trmc_stream_set_velocity) is not supported in a stream with reservoir data "
                                       "assimilation: the _rda tile instances do not write the depth plane");
    // (boundary rows are routed by nobody and have no depth: zeros in the slots' depth planes, as in a full result)
    if (S.dpl && tp.nboundary > 0)
        HIP_TRY(hipMemset2DAsync((T *)S.tm.p + S.plane, S.slot_tm * sizeof(T), 0, S.plane * sizeof(T), (size_t)S.slots, pl->stream));
    // (boundary rows of the full result are written by nobody: zeros, so that their reduction is the (0, 1) the carry gives)
    if ((pd || S.stage || S.dex_K > 0) && S.want_out && tp.nboundary > 0) HIP_TRY(hipMemsetAsync(S.out.p, 0, (size_t)S.slots * S.slot_out * sizeof(T), pl->stream));
    // THE TABLE OF THE DAY'S PRODUCTS (the head of StreamRun), in the enumeration's order: {carried, bytes of a day's copy, bytes of a
    // slot, has a buffer of its own, bytes of its total over the days}.  A summary part that the mask does not ask for holds no
    // buffer; the other buffers are kept between streams.
    const size_t row = (size_t)pl->nseg * sizeof(T), irow = (size_t)pl->nseg * sizeof(int32_t), lrow = (size_t)pl->nseg * sizeof(int64_t);
    const size_t fvd = (S.dec_stride > 0 ? S.slot_dec : S.slot_out) * sizeof(T), da = S.slot_da * sizeof(T), res = S.slot_res * sizeof(T);
    const size_t rda4 = (size_t)pl->nres * 4 * sizeof(float), rda1 = (size_t)pl->nres * sizeof(int32_t);
    const bool peak = (S.sum & TRMC_SUMMARY_PEAK) != 0, mean = (S.sum & TRMC_SUMMARY_MEAN) != 0;
    const struct { bool on; size_t bytes, stride; bool own; size_t total; } rows[] = {
        /* P_HYD     */ {true, 0, 0, true, 0}, // (bytes: of the day's row set; a slot is sized by the first push of THIS stream)
        /* P_Q0      */ {true, 3 * row, 3 * row, true, 0},
        /* P_FVD     */ {S.dec_stride > 0 || S.want_out, fvd, fvd, false, 0}, // (in a slot of dec or of out: below)
        /* P_NUDGE   */ {S.slot_da > 0, da, da, true, 0},
        /* P_RES     */ {S.slot_res > 0, res, res, true, 0},
        /* P_RDA     */ {S.rda, rda4, rda4 + rda1, true, 0},
        /* P_RDA_IDX */ {S.rda, rda1, rda4 + rda1, false, 0}, // (behind the state in P_RDA's slot: below)
        /* P_PEAK    */ {peak, row, row, true, row},
        /* P_STEP    */ {peak, irow, irow, true, lrow},
        /* P_MEAN    */ {mean, row, row, true, row},
        /* P_PD      */ {pd, row, row, true, row},
        /* P_PDS     */ {pd, irow, irow, true, lrow},
        /* P_STAGE   */ {S.stage, 0, 0, true, 0}, // (as P_HYD)
    };
    static_assert(sizeof(rows) / sizeof(rows[0]) == P_ALL, "one row per product, in the enumeration's order");
    const bool tot = (S.sum & TRMC_SUMMARY_TOTAL) != 0;
    S.tot_days = 0;
    for (int k = 0; k < P_ALL; ++k) {
        StreamProdRow &t = S.tab[k];
        t.on = rows[k].on;
        t.bytes = rows[k].bytes;
        t.stride = rows[k].stride;
        t.next = nullptr;
        if (k >= P_PEAK && !t.on) t.buf.release();
        if (rows[k].own && t.on)
            if (int rc = t.buf.ensure((size_t)S.slots * t.stride)) return rc;
        t.base = (char *)t.buf.p;
        if (k < P_PEAK || k >= P_N) continue;
        // ... and the part's total over the days, outside the ring (the steps count on over the days: int64)
        DevBuf &b = S.tot[k - P_PEAK];
        if (!(tot && t.on)) b.release();
        else if (int rc = b.ensure(rows[k].total)) return rc;
    }
    S.tab[P_FVD].base = (char *)(S.dec_stride > 0 ? S.dec.p : S.out.p);
    if (S.rda) S.tab[P_RDA_IDX].base = S.tab[P_RDA].base + rda4;
    if (tot)
        if (int rc = S.ev_total.ensure(false)) return rc;
    // the exceedance over the days: the accumulator (zeroed below, in front of ev_begin) and what a fetch gathers into
    S.exc = S.exc_want;
    S.exc_days = 0;
    if (S.exc >= 0 && pl->th_levels < 1)
        return fail(TRMC_ESTATE, "the streams of this plan were told to form an exceedance (trmc_stream_set_exceedance), but its thresholds have been "
                                 "cleared since (trmc_plan_set_thresholds)");
    S.exc_K = S.exc >= 0 ? pl->th_levels : 0;
    S.exc_KP = S.exc >= 0 ? pl->th_pad : 0;
    const size_t exc_bytes = (size_t)kStreamExceedFields * (size_t)S.exc_KP * np * sizeof(int32_t);
    if (S.exc < 0) {
        S.exc_acc.release();
        S.exc_rows.release();
    } else {
        if (int rc = S.exc_acc.ensure(exc_bytes)) return rc;
        if (int rc = S.exc_rows.ensure(4 * (size_t)pl->nseg * (size_t)S.exc_K * sizeof(int64_t))) return rc;
        if (int rc = S.ev_exc.ensure(false)) return rc;
    }
    // the Courant number over the days: the accumulator (zeroed below, in front of ev_begin) and what a fetch gathers into
    const size_t cou_off = ((size_t)pl->nseg * sizeof(T) + 255) / 256 * 256;
    if (!S.cou) {
        for (DevBuf *b : {&S.cou_peak, &S.cou_step, &S.cou_count, &S.cou_rows}) b->release();
    } else {
        if (int rc = S.cou_peak.ensure(np * sizeof(T))) return rc;
        if (int rc = S.cou_step.ensure(np * sizeof(int32_t))) return rc;
        if (int rc = S.cou_count.ensure(np * sizeof(int32_t))) return rc;
        if (int rc = S.cou_rows.ensure(cou_off + 2 * (size_t)pl->nseg * sizeof(int64_t))) return rc;
        for (DevEvent *e : {&S.ev_cou0, &S.ev_cou})
            if (int rc = e->ensure(true)) return rc;
    }
    // the depth exceedance over the days: the accumulator (zeroed below, in front of ev_begin) and what a fetch gathers into
    const size_t dex_bytes = (size_t)kStreamExceedFields * (size_t)S.dex_KP * np * sizeof(int32_t);
    if (S.dex_K < 1) {
        S.dex_acc.release();
        S.dex_rows.release();
    } else {
        if (int rc = S.dex_acc.ensure(dex_bytes)) return rc;
        if (int rc = S.dex_rows.ensure(4 * (size_t)pl->nseg * (size_t)S.dex_K * sizeof(int64_t))) return rc;
        for (DevEvent *e : {&S.ev_dex0, &S.ev_dex})
            if (int rc = e->ensure(true)) return rc;
    }
    // the velocity over the days: the accumulator (zeroed below, in front of ev_begin) and what a fetch gathers into
    const size_t vel_bytes = (size_t)kStreamExceedFields * (size_t)S.vel_KP * np * sizeof(int32_t);
    if (!S.vel) {
        for (DevBuf *b : {&S.vel_peak, &S.vel_step, &S.vel_acc, &S.vel_rows}) b->release();
    } else {
        const size_t off = ((size_t)pl->nseg * sizeof(T) + 255) / 256 * 256, off2 = off + ((size_t)pl->nseg * sizeof(int64_t) + 255) / 256 * 256;
        if (int rc = S.vel_peak.ensure(np * sizeof(T))) return rc;
        if (int rc = S.vel_step.ensure(np * sizeof(int32_t))) return rc;
        if (S.vel_K < 1) S.vel_acc.release();
        else if (int rc = S.vel_acc.ensure(vel_bytes)) return rc;
        if (int rc = S.vel_rows.ensure(off2 + 4 * (size_t)pl->nseg * (size_t)S.vel_K * sizeof(int64_t))) return rc;
        for (DevEvent *e : {&S.ev_vel0, &S.ev_vel})
            if (int rc = e->ensure(true)) return rc;
    }
    // reservoir data assimilation: the slots' tables at their capacity, the carry with the state trmc_set_reservoir_da supplied
    // (or the plan's last window left in those tables); the days' state records are products (P_RDA)
    S.slot_rda = 0;
    if (S.rda) {
        int64_t floats = pl->nres * (int64_t)(sizeof(trmc::ResDaRec) / sizeof(float));
        for (int k = 0; k < 3; ++k) {
            const int64_t n = pl->res_da_n[k];
            S.rda_cap[k] = n > 0 ? std::max(S.rda_cap_want[k], pl->res_da_ncol[k]) : 0;
            S.rda_off[k] = floats;
            floats += n * S.rda_cap[k];
            S.rda_time_off[k] = floats;
            if (k < 2) floats += S.rda_cap[k];
        }
        S.slot_rda = ((size_t)floats * sizeof(float) + 63) / 64 * 64;
        S.t_end = (float)nsteps * (float)pl->res_dt;
        if (int rc = S.rda_tab.ensure((size_t)S.slots * S.slot_rda)) return rc;
        if (int rc = S.rda_carry.ensure((size_t)pl->nres * sizeof(trmc::ResDaState))) return rc;
        if (int rc = S.rda_stage.ensure((size_t)S.slots * S.slot_rda)) return rc;
        HIP_TRY(hipStreamSynchronize(pl->stream)); // (a window routed with these tables has left its state in them)
        std::vector<trmc::ResDaRec> rec((size_t)pl->nres);
        HIP_TRY(hipMemcpy(rec.data(), pl->res_da.p, rec.size() * sizeof(trmc::ResDaRec), hipMemcpyDeviceToHost));
        std::vector<trmc::ResDaState> carry((size_t)pl->nres);
        for (size_t i = 0; i < rec.size(); ++i) carry[i] = rec[i].st;
        HIP_TRY(hipMemcpy(S.rda_carry.p, carry.data(), carry.size() * sizeof(trmc::ResDaState), hipMemcpyHostToDevice));
    }
    if (int rc = ensure_copy_stream(pl)) return rc;
    if (int rc = ensure_tile_stream(pl)) return rc;
    if (int rc = ensure_events(S.ev_slab, kSlabEvents, false)) return rc;
    for (auto *v : {&S.ev_free, &S.ev_ready, &S.ev_forcing})
        if (int rc = ensure_events(*v, (size_t)S.slots, false)) return rc;
    for (auto *v : {&S.ev_t0, &S.ev_t1})
        if (int rc = ensure_events(*v, (size_t)S.slots, true)) return rc;
    S.prod.resize((size_t)S.slots);
    for (StreamProd &p : S.prod) {
        if (int rc = p.ev_done.ensure(false)) return rc;
        p.day = -1;
        p.queued = false;
    }
    for (DevEvent *e : {&S.ev_begin, &S.ev_gat})
        if (int rc = e->ensure(false)) return rc;
    S.mk_bnd.settle();
    S.days_pushed = S.day_min = S.days_complete = 0;
    S.g_done = -1;
    S.launches = 0;
    // the state every row starts from: time row 0 of slot 0 (trmc_upload_forcing's q0, or the last window's final state)
    hipStream_t st = pl->stream;
    if (int rc = pl->mk_forcing.order(st)) return rc;
    pl->mk_forcing.settle();
    HIP_TRY(hipMemsetAsync(pl->it_prev.p, 0, (size_t)np, st));
    if (S.exc >= 0 && exc_bytes > 0) HIP_TRY(hipMemsetAsync(S.exc_acc.p, 0, exc_bytes, st));
    if (S.dex_K > 0 && dex_bytes > 0) HIP_TRY(hipMemsetAsync(S.dex_acc.p, 0, dex_bytes, st));
    if (S.vel && np > 0) {
        HIP_TRY(hipMemsetAsync(S.vel_peak.p, 0, np * sizeof(T), st));
        HIP_TRY(hipMemsetAsync(S.vel_step.p, 0, np * sizeof(int32_t), st));
        if (S.vel_K > 0 && vel_bytes > 0) HIP_TRY(hipMemsetAsync(S.vel_acc.p, 0, vel_bytes, st));
    }
    if (S.cou && np > 0) {
        HIP_TRY(hipMemsetAsync(S.cou_peak.p, 0, np * sizeof(T), st));
        HIP_TRY(hipMemsetAsync(S.cou_step.p, 0, np * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(S.cou_count.p, 0, np * sizeof(int32_t), st));
    }
    if (pl->collect_cost) {
        if (int rc = pl->it_sum.ensure(np * sizeof(uint16_t))) return rc;
        HIP_TRY(hipMemsetAsync(pl->it_sum.p, 0, np * sizeof(uint16_t), st));
        pl->cost_nsteps = 0;
    }
    if (pl->nseg > 0) {
        T *q = (T *)S.tm.p;
        hipLaunchKernelGGL((k_init_state<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, st, (const T *)pl->in_q0.p,
                           (const int32_t *)pl->sh->row_of_pos.p, q, q + S.plane /* (the velocity of the state is not an input) */,
                           q + S.plane, (int32_t)pl->nseg);
    }
    // the in-block partition and the hot rows of the slices: made and cleared here, in front of ev_begin (the launches' arguments:
    // tile_args, stream_launch).  A stream leaves no history behind where the partition is off.
    if (int rc = tile_setup(pl, st, S.W)) return rc;
    if (!tile_partition_on(pl)) pl->cls_last.release();
    HIP_TRY(hipEventRecord(S.ev_begin, st));
    HIP_TRY(hipStreamWaitEvent(pl->wstream, S.ev_begin, 0));
    if (int rc = S.fst.ensure(hipStreamNonBlocking)) return rc;
    HIP_TRY(hipStreamWaitEvent(S.fst, S.ev_begin, 0));
    HIP_TRY(hipStreamWaitEvent(pl->hstream, S.ev_begin, 0));
    HIP_TRY(hipGetLastError());
    pl->q0_staged = false;
    pl->routed_nsteps = -1;
    S.active = true;
    return 0;
}

// raw_a != NULL: the day's forcing arrives as packed columns (raw_b: NULL in the single-variable form), day.qlat is not read
template <class T> int stream_push_t(trmc_plan *pl, const trmc_stream_day &day, const int32_t *raw_a, const int32_t *raw_b)
{
    StreamRun &S = *pl->seq;
    const void *const qlat = day.qlat, *const boundary_q_dev = day.boundary_q_dev;
    const int32_t rowset = day.rowset;
    const trmc::Topology &tp = pl->sh->topo;
    const int64_t d = S.days_pushed;
    const int32_t slot = (int32_t)(d % S.slots);
    const size_t np = (size_t)pl->nseg_pad;
    hipStream_t hst = S.fst; // (the forcing's own stream: the products of earlier days leave on the plan's copy stream meanwhile)
    if (d >= S.slots && S.days_complete <= d - S.slots)
        return fail(TRMC_ESTATE, "internal: the slot of the new day still belongs to a day that has not been queued to its end");
    if ((S.exc >= 0 || S.cou || S.dex_K > 0 || S.vel) && (d + 1) * (int64_t)S.nsteps > (int64_t)INT32_MAX)
        return fail(TRMC_EUNSUPPORTED, "the flow exceedance, the depth exceedance, the Courant number and the velocity over the days of a stream count "
                                       "its steps in 32 bits on the device: this day would take the stream past 2^31 - 1 steps -- begin a new "
                                       "stream");
    StreamProd &p = S.prod[(size_t)slot];
    // (the host image of the slot's reservoir tables is written below: the copy of the slot's last day must have read it)
    if (S.rda && p.day >= 0) HIP_TRY(hipEventSynchronize(S.ev_forcing[(size_t)slot]));
    if (p.day >= 0 && p.queued) HIP_TRY(hipStreamWaitEvent(hst, S.ev_free[(size_t)slot], 0)); // (the slot's last day has handed its products over)
    // (the hydrographs' slot, and the stage's, are sized by the stream's first push that asks for them)
    for (const int k : {(int)P_HYD, (int)P_STAGE}) {
        if (!(k == P_HYD ? day.hyd_host != nullptr : S.tab[P_STAGE].next != nullptr) || rowset < 0) continue;
        StreamProdRow &h = S.tab[k];
        const size_t hb = (size_t)pl->rowset_n[(size_t)rowset] * S.nsteps * sizeof(T);
        if (hb > h.stride) {
            if (d > S.day_min || S.days_complete < d) {
                if (h.stride > 0) return fail(TRMC_ESTATE, "a larger row set than the stream's first one: begin a new stream");
            }
            h.stride = hb;
            if (int rc = h.buf.ensure((size_t)S.slots * hb)) return rc;
            h.base = (char *)h.buf.p;
        }
    }
    p.day = d;
    p.queued = false;
    p.rowset = rowset;
    // the day's destinations: from the day, the summary parts' from the calls in front of this push, which consumes them
    void *const from_day[P_PEAK] = {day.hyd_host, day.q0_host, day.fvd_host, day.nudge_host, day.res_inflow_host, day.res_da_state_host,
                                    day.res_da_tsidx_host};
    for (int k = 0; k < P_ALL; ++k) {
        p.host[k] = k < P_PEAK ? from_day[k] : S.tab[k].next;
        S.tab[k].next = nullptr;
    }
    // the day's forcing: host -> staging area -> plan order in the slot, all on the copy stream of that direction
    // (a packed day: the raw blocks take the same road and one kernel decodes, joins and lays them out -- the head of this file)
    const size_t bytes = raw_a ? stream_raw_bytes(S, raw_b != nullptr) : (size_t)pl->nseg * S.nq * sizeof(T);
    if (int rc = pl->in_qlat.ensure(bytes)) return rc;
    if (pl->nseg > 0 && raw_a) {
        const size_t one = stream_raw_bytes(S, false);
        int32_t *const da = (int32_t *)pl->in_qlat.p, *const db = raw_b ? da + (size_t)S.nq * (size_t)S.pk_nfeat : nullptr;
        if (one > 0) HIP_TRY(hipMemcpyAsync(da, raw_a, one, hipMemcpyHostToDevice, hst));
        if (one > 0 && raw_b) HIP_TRY(hipMemcpyAsync(db, raw_b, one, hipMemcpyHostToDevice, hst));
        const int32_t n = (int32_t)pl->nseg;
        HIP_TRY(hipEventRecord(S.ev_pk0, hst));
        hipLaunchKernelGGL((k_ingest_packed_day<T>), dim3(blocks_for(n), (unsigned)((S.nq + kIngestCols - 1) / kIngestCols)), dim3(kBlock), 0, hst,
                           (const int32_t *)da, (const int32_t *)db, S.pk_a, S.pk_b, (const int32_t *)S.pk_feat_of_pos.p,
                           (T *)S.qlat.p + (size_t)slot * S.slot_qlat, n, pl->nseg_pad, (int32_t)S.nq, S.pk_nfeat);
        HIP_TRY(hipEventRecord(S.ev_pk1, hst));
        S.pk_ms_ok = true;
    } else if (pl->nseg > 0) {
        HIP_TRY(hipMemcpyAsync(pl->in_qlat.p, qlat, bytes, hipMemcpyHostToDevice, hst));
        const int32_t n = (int32_t)pl->nseg;
        hipLaunchKernelGGL((k_prep_qlat<T>), dim3((n + 63) / 64, (unsigned)((S.nq + 31) / 32)), dim3(kBlock), 0, hst, (const T *)pl->in_qlat.p,
                           (const int32_t *)pl->sh->row_of_pos.p, (T *)S.qlat.p + (size_t)slot * S.slot_qlat, n, pl->nseg_pad, (int32_t)S.nq);
    }
    if (S.slot_da > 0) {
        // the day's nudging tables [ngage][nsteps] into the slot, beside its forcing: behind ev_free (the slot's last day has been
        // read to its end), in front of ev_forcing (which this day's launches wait for).  The nudge record starts from zero: a gage
        // that shares its row with a later one of the list is never visited (trmc_stream_set_gages).
        const size_t n = S.slot_da, o = (size_t)slot * S.slot_da;
        HIP_TRY(hipMemcpyAsync((uint8_t *)S.da_mode.p + o, day.da_mode, n, hipMemcpyHostToDevice, hst));
        HIP_TRY(hipMemcpyAsync((T *)S.da_a.p + o, day.da_a, n * sizeof(T), hipMemcpyHostToDevice, hst));
        HIP_TRY(hipMemcpyAsync((T *)S.da_w.p + o, day.da_w, n * sizeof(T), hipMemcpyHostToDevice, hst));
        HIP_TRY(hipMemsetAsync((T *)S.tab[P_NUDGE].base + o, 0, n * sizeof(T), hst));
        // the day's first observations [ngage] (NaN = none; all bits set is a NaN in either precision)
        T *const q0o = (T *)S.da_q0.p + (size_t)slot * (size_t)S.ngage;
        if (day.da_q0) HIP_TRY(hipMemcpyAsync(q0o, day.da_q0, (size_t)S.ngage * sizeof(T), hipMemcpyHostToDevice, hst));
        else HIP_TRY(hipMemsetAsync(q0o, 0xff, (size_t)S.ngage * sizeof(T), hst));
    }
    if (S.rda) {
        // the day's reservoir tables into the slot, as the nudging tables: behind ev_free, in front of ev_forcing
        float *const img = (float *)((char *)S.rda_stage.p + (size_t)slot * S.slot_rda);
        stream_rda_image(pl, S, *day.reservoir_da, img);
        HIP_TRY(hipMemcpyAsync((char *)S.rda_tab.p + (size_t)slot * S.slot_rda, img, S.slot_rda, hipMemcpyHostToDevice, hst));
    }
    if (int rc = S.mk_bnd.order(hst)) return rc; // (trmc_stream_boundary on a stream of the caller's: this day's launches go behind it)
    S.mk_bnd.settle();
    if (tp.nboundary > 0 && boundary_q_dev) {
        // boundary rows: their flows of the day [nboundary][nsteps] into the slot's plane; time row 0 = where the day before ended
        T *q = (T *)S.tm.p + (size_t)slot * S.slot_tm;
        if (d > 0) {
            const T *qp = (const T *)S.tm.p + (size_t)((d - 1) % S.slots) * S.slot_tm + (size_t)S.nsteps * np;
            HIP_TRY(hipMemcpyAsync(q, qp, (size_t)tp.nboundary * sizeof(T), hipMemcpyDeviceToDevice, hst));
        }
        hipLaunchKernelGGL((k_stream_boundary<T>), dim3(blocks_for(tp.nboundary * (int64_t)S.nsteps)), dim3(kBlock), 0, hst,
                           (const T *)boundary_q_dev, q, (int32_t)tp.nboundary, S.nsteps, pl->nseg_pad);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S.ev_forcing[(size_t)slot], hst));
    HIP_TRY(hipStreamWaitEvent(pl->wstream, S.ev_forcing[(size_t)slot], 0));
    HIP_TRY(hipStreamWaitEvent(pl->stream, S.ev_forcing[(size_t)slot], 0));
    // (the Courant number: this day's last launches rewrite time row 0 of a slot whose fold may still read it -- the head of this file)
    if (S.cou && S.cou_days > 0) HIP_TRY(hipStreamWaitEvent(pl->wstream, S.ev_cou, 0));
    if (S.dex_K > 0 && S.dex_days > 0) HIP_TRY(hipStreamWaitEvent(pl->wstream, S.ev_dex, 0)); // (the depth exceedance: likewise)
    if (S.vel && S.vel_days > 0) HIP_TRY(hipStreamWaitEvent(pl->wstream, S.ev_vel, 0));       // (the velocity: as the Courant number)
    S.days_pushed = d + 1;
    hipStream_t tst = S.W > 0 ? pl->wstream : pl->stream; // (the stream whose launches a day's push is timed on)
    HIP_TRY(hipEventRecord(S.ev_t0[(size_t)slot], tst));
    const int rc = stream_launch<T>(pl, S, d * S.tpd - 1, (d + 1) * S.tpd - 1, d + 1);
    if (!rc) HIP_TRY(hipEventRecord(S.ev_t1[(size_t)slot], tst));
    return rc;
}

} // namespace
} // extern "C++"

static bool stream_active(const trmc_plan *pl) { return pl && pl->seq && pl->seq->active; }

// (the reservoir branch of the kernels ends a row's step before the nudging hook: trmc_set_nudging's rule)
static int stream_gages_check(trmc_plan *pl, const std::vector<int32_t> &gage_pos)
{
    if (pl->nres == 0 || gage_pos.empty()) return 0;
    if (int rc = use_device(pl)) return rc;
    std::vector<int32_t> res_of_pos((size_t)pl->nseg_pad);
    HIP_TRY(hipMemcpy(res_of_pos.data(), pl->res_of_pos.p, res_of_pos.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (const int32_t p : gage_pos)
        if (res_of_pos[(size_t)p] >= 0)
            return fail(TRMC_EINVAL, "a gage on a reservoir row is not supported (row " + std::to_string(pl->sh->topo.row_of_pos[(size_t)p]) + ")");
    return 0;
}

static int stream_check(trmc_plan *pl, bool want_active)
{
    if (!pl) return fail(TRMC_EINVAL, "plan is NULL");
    const bool act = pl->seq && pl->seq->active;
    if (want_active && !act) return fail(TRMC_ESTATE, "no stream of windows in progress (trmc_stream_begin)");
    if (!want_active && act) return fail(TRMC_ESTATE, "a stream of windows is in progress (trmc_stream_end it first)");
    return use_device(pl);
}

int trmc_stream_begin(trmc_plan *pl, int nsteps, int qts_subdivisions, int slots, int full_output, int output_stride)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (pl->run.active) return fail(TRMC_ESTATE, "a routing window is in progress");
    const trmc::Topology &tp = pl->sh->topo;
    if (!(tp.ncl > 0 || (tp.cl_rows > 0 && tp.cl_from_level == tp.nlevels)))
        return fail(TRMC_EINVAL, "a stream of windows needs a plan in cluster order (TRMC_PLAN_SHORT_TS on the level engine, "
                                 "trmc_plan_options.cluster_rows >= 0): every row is then routed in tiles");
    if (pl->maxlag > 0) return fail(TRMC_EINVAL, "rows with a lag (trmc_plan_set_lag) have no place in a stream of windows: every row has its tile lag");
    if (pl->nres > 0 && pl->res_da_on) {
        if (!(pl->seq && pl->seq->rda_want))
            return fail(TRMC_EINVAL, "reservoir data assimilation (reservoir types 2-5, trmc_set_reservoir_da) is routed window by window "
                                     "unless the plan's streams were told to carry it (trmc_stream_set_reservoir_da)");
        if (int rc = reservoir_da_plan_check(pl)) return rc; // (trmc_set_reservoir_da let no other plan have tables)
    }
    if (pl->ngage > 0 && !(pl->seq && pl->seq->ngage > 0))
        return fail(TRMC_EINVAL, "the nudging tables of trmc_set_nudging belong to one window: declare a stream's gage rows with "
                                 "trmc_stream_set_gages, its tables arrive with every day (trmc_stream_push_day)");
    if (pl->seq && pl->seq->ngage > 0)
        if (int rc = stream_gages_check(pl, pl->seq->gage_pos)) return rc;
    if (settle_deferred_state(pl)) return TRMC_ESTATE;
    if (pl->staged_nsteps < 0) return fail(TRMC_ESTATE, "trmc_upload_forcing (the state, and the shape of the forcing) must precede trmc_stream_begin");
    if (nsteps < 1 || qts_subdivisions < 1) return fail(TRMC_EINVAL, "nsteps and qts_subdivisions must be >= 1");
    if ((int64_t)(nsteps - 1) / qts_subdivisions >= pl->nq)
        return fail(TRMC_EINVAL, "Number of columns (timesteps) in Qlat is incorrect: need " + std::to_string((nsteps - 1) / qts_subdivisions + 1)
                                     + ", got " + std::to_string(pl->nq));
    if (output_stride < 0 || slots < 0) return fail(TRMC_EINVAL, "slots and output_stride must be >= 0");
    const int rc = by_precision(pl, [&](auto t) { return stream_begin_t<decltype(t)>(pl, nsteps, qts_subdivisions, slots, full_output, output_stride); });
    if (rc && pl->seq) pl->seq->active = false;
    return rc;
}

int trmc_stream_set_gages(trmc_plan *pl, int64_t ngage, const int64_t *gage_rows)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (ngage < 0) return fail(TRMC_EINVAL, "ngage < 0");
    if (ngage > 0 && !gage_rows) return fail(TRMC_EINVAL, "gage_rows is NULL");
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    StreamRun &S = *pl->seq;
    S.ngage = 0;
    S.gage_pos.clear();
    if (ngage == 0) return 0;
    std::vector<int32_t> g_of_pos((size_t)pl->nseg_pad, -1), pos((size_t)ngage);
    for (int64_t g = 0; g < ngage; ++g) {
        const int64_t r = gage_rows[g];
        if (r < 0 || r >= pl->nseg) return fail(TRMC_EINVAL, "gage row out of range");
        if (pl->sh->topo.level_of_row[r] < 0) return fail(TRMC_EINVAL, "gage on a boundary row");
        pos[(size_t)g] = pl->sh->topo.pos_of_row[r];
        g_of_pos[(size_t)pos[(size_t)g]] = (int32_t)g; // one gage per segment: the last listed wins (trmc_set_nudging)
    }
    if (int rc = stream_gages_check(pl, pos)) return rc;
    if (int rc = upload_i32(S.gage_of_pos, g_of_pos, 1)) return rc;
    if (int rc = upload_i32(S.gage_pos_dev, pos, 1)) return rc;
    S.gage_pos = std::move(pos);
    S.ngage = ngage;
    return 0;
}

int trmc_stream_set_reservoir_da(trmc_plan *pl, int on, int64_t usgs_ncol, int64_t usace_ncol, int64_t rfc_ncol)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (usgs_ncol < 0 || usace_ncol < 0 || rfc_ncol < 0 || usgs_ncol > INT32_MAX || usace_ncol > INT32_MAX || rfc_ncol > INT32_MAX)
        return fail(TRMC_EINVAL, "a table's column capacity must be >= 0 (0: as many as the declared table has)");
    if (on)
        if (int rc = reservoir_da_plan_check(pl)) return rc;
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    StreamRun &S = *pl->seq;
    S.rda_want = on != 0;
    S.rda_cap_want[0] = usgs_ncol;
    S.rda_cap_want[1] = usace_ncol;
    S.rda_cap_want[2] = rfc_ncol;
    return 0;
}

int trmc_stream_set_summary(trmc_plan *pl, int what)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    constexpr int parts = TRMC_SUMMARY_PEAK | TRMC_SUMMARY_MEAN | TRMC_SUMMARY_PEAK_DEPTH;
    if (what & ~(parts | TRMC_SUMMARY_TOTAL))
        return fail(TRMC_EINVAL, "what: a mask of TRMC_SUMMARY_PEAK, TRMC_SUMMARY_MEAN, TRMC_SUMMARY_PEAK_DEPTH and TRMC_SUMMARY_TOTAL (0: no summary)");
    if ((what & TRMC_SUMMARY_TOTAL) && !(what & parts))
        return fail(TRMC_EINVAL, "TRMC_SUMMARY_TOTAL needs at least one of the parts it totals (TRMC_SUMMARY_PEAK, TRMC_SUMMARY_MEAN, TRMC_SUMMARY_PEAK_DEPTH)");
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    pl->seq->sum_want = what;
    return 0;
}

int trmc_stream_summary_dest(trmc_plan *pl, void *peak_flow_host, int32_t *peak_step_host, void *mean_flow_host)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (S.sum == 0) return fail(TRMC_ESTATE, "the stream was begun without a summary (trmc_stream_set_summary precedes trmc_stream_begin)");
    if ((peak_flow_host || peak_step_host) && !(S.sum & TRMC_SUMMARY_PEAK))
        return fail(TRMC_EINVAL, "a peak array for a stream whose summary has no TRMC_SUMMARY_PEAK");
    if (mean_flow_host && !(S.sum & TRMC_SUMMARY_MEAN)) return fail(TRMC_EINVAL, "a mean array for a stream whose summary has no TRMC_SUMMARY_MEAN");
    S.tab[P_PEAK].next = peak_flow_host;
    S.tab[P_STEP].next = peak_step_host;
    S.tab[P_MEAN].next = mean_flow_host;
    return 0;
}

int trmc_stream_summary_depth_dest(trmc_plan *pl, void *peak_depth_host, int32_t *peak_depth_step_host)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!(S.sum & TRMC_SUMMARY_PEAK_DEPTH))
        return fail(TRMC_ESTATE, "the stream was begun without TRMC_SUMMARY_PEAK_DEPTH (trmc_stream_set_summary precedes trmc_stream_begin)");
    S.tab[P_PD].next = peak_depth_host;
    S.tab[P_PDS].next = peak_depth_step_host;
    return 0;
}

int trmc_stream_set_stage(trmc_plan *pl, int on)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (!on && !pl->seq) return 0; // (withdrawn where nothing was declared)
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    pl->seq->stage_want = on != 0;
    return 0;
}

int trmc_stream_stage_dest(trmc_plan *pl, void *stage_host)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!S.stage) return fail(TRMC_ESTATE, "the stream was begun without stage hydrographs (trmc_stream_set_stage precedes trmc_stream_begin)");
    S.tab[P_STAGE].next = stage_host;
    return 0;
}

int trmc_stream_summary_total(trmc_plan *pl, void *peak_flow, int64_t *peak_step, void *mean_flow, void *peak_depth, int64_t *peak_depth_step,
                              int64_t *days_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!(S.sum & TRMC_SUMMARY_TOTAL)) return fail(TRMC_ESTATE, "the stream was begun without TRMC_SUMMARY_TOTAL (trmc_stream_set_summary precedes trmc_stream_begin)");
    if (S.tot_days < 1)
        return fail(TRMC_ESTATE, "no day of the stream is complete yet: its last rows run " + std::to_string(S.lmax)
                                     + " tiles behind its first -- push further days or trmc_stream_flush");
    if ((peak_flow || peak_step) && !(S.sum & TRMC_SUMMARY_PEAK)) return fail(TRMC_EINVAL, "a peak array for a stream whose summary has no TRMC_SUMMARY_PEAK");
    if (mean_flow && !(S.sum & TRMC_SUMMARY_MEAN)) return fail(TRMC_EINVAL, "a mean array for a stream whose summary has no TRMC_SUMMARY_MEAN");
    if ((peak_depth || peak_depth_step) && !(S.sum & TRMC_SUMMARY_PEAK_DEPTH))
        return fail(TRMC_EINVAL, "a peak-depth array for a stream whose summary has no TRMC_SUMMARY_PEAK_DEPTH");
    const int64_t days = S.tot_days;
    const size_t n = (size_t)pl->nseg, esz = (size_t)pl->esz;
    // behind the last fold queued (nothing is queued meanwhile: the calls of a plan come from one thread)
    HIP_TRY(hipStreamWaitEvent(pl->cstream, S.ev_total, 0));
    void *const dst[P_N - P_PEAK] = {peak_flow, peak_step, mean_flow, peak_depth, peak_depth_step}; // (the parts' order: S.tot)
    for (int i = 0; i < P_N - P_PEAK; ++i) {
        const bool step = i == P_STEP - P_PEAK || i == P_PDS - P_PEAK;
        if (dst[i] && n) HIP_TRY(hipMemcpyAsync(dst[i], S.tot[i].p, n * (step ? sizeof(int64_t) : esz), hipMemcpyDeviceToHost, pl->cstream));
    }
    HIP_TRY(hipStreamSynchronize(pl->cstream));
    if (mean_flow) { // (((m_0 + m_1) + ...) was summed on the device; the division in the plan's precision)
        if (esz == 4) {
            float *m = (float *)mean_flow;
            for (size_t i = 0; i < n; ++i) m[i] = m[i] / (float)days;
        } else {
            double *m = (double *)mean_flow;
            for (size_t i = 0; i < n; ++i) m[i] = m[i] / (double)days;
        }
    }
    if (days_out) *days_out = days;
    return 0;
}

int trmc_stream_set_exceedance(trmc_plan *pl, int quantity)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (quantity == -1) { // (withdrawn: the next stream holds no accumulator and queues no fold)
        if (pl->seq) pl->seq->exc_want = -1;
        return 0;
    }
    if (quantity == TRMC_X_VELOCITY || quantity == TRMC_X_DEPTH)
        return fail(TRMC_EUNSUPPORTED, "the exceedance of a stream of windows is formed from the flow planes of its ring, which hold every step's flow "
                                       "of every row: they hold the depth of a tile's last step only, and a stream without full_output forms no "
                                       "velocity -- for depth, velocity or out of bank route the day in question as a window "
                                       "(trmc_window_exceedance)");
    if (quantity != TRMC_X_FLOW) return fail(TRMC_EINVAL, "quantity must be TRMC_X_FLOW (or -1: no exceedance)");
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (pl->th_levels < 1) return fail(TRMC_ESTATE, "no thresholds set on this plan (trmc_plan_set_thresholds)");
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    pl->seq->exc_want = quantity;
    return 0;
}

int trmc_stream_exceedance(trmc_plan *pl, int64_t *steps_over, int64_t *first_step, int64_t *last_step, int64_t *longest_run, int64_t *days_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (S.exc < 0) return fail(TRMC_ESTATE, "the stream was begun without an exceedance (trmc_stream_set_exceedance precedes trmc_stream_begin)");
    if (S.exc_days < 1)
        return fail(TRMC_ESTATE, "no day of the stream is complete yet: its last rows run " + std::to_string(S.lmax)
                                     + " tiles behind its first -- push further days or trmc_stream_flush");
    const int64_t days = S.exc_days;
    const size_t n = (size_t)pl->nseg * (size_t)S.exc_K;
    int64_t *const dst[4] = {steps_over, first_step, last_step, longest_run};
    // behind the last fold queued (nothing is queued meanwhile: the calls of a plan come from one thread)
    HIP_TRY(hipStreamWaitEvent(pl->cstream, S.ev_exc, 0));
    if (n && (steps_over || first_step || last_step || longest_run)) {
        hipLaunchKernelGGL(k_stream_exceed_rows, dim3(blocks_for((int64_t)n)), dim3(kBlock), 0, pl->cstream, (const int32_t *)S.exc_acc.p,
                           (const int32_t *)pl->sh->pos_of_row.p, (int64_t *)S.exc_rows.p, (int32_t)pl->nseg, pl->nseg_pad, S.exc_K, S.exc_KP);
        HIP_TRY(hipGetLastError());
        for (int f = 0; f < 4; ++f)
            if (dst[f]) HIP_TRY(hipMemcpyAsync(dst[f], (const int64_t *)S.exc_rows.p + (size_t)f * n, n * sizeof(int64_t), hipMemcpyDeviceToHost, pl->cstream));
    }
    HIP_TRY(hipStreamSynchronize(pl->cstream));
    if (days_out) *days_out = days;
    return 0;
}

int trmc_stream_set_courant(trmc_plan *pl, int on, double limit)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (!on && !pl->seq) return 0; // (withdrawn where nothing was declared)
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    pl->seq->cou_want = on != 0;
    pl->seq->cou_limit_want = on ? limit : 0.0;
    return 0;
}

int trmc_stream_courant(trmc_plan *pl, void *peak_cn, int64_t *peak_cn_step, int64_t *steps_over, int64_t *days_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!S.cou) return fail(TRMC_ESTATE, "the stream was begun without the Courant number (trmc_stream_set_courant precedes trmc_stream_begin)");
    if (!peak_cn && !peak_cn_step && !steps_over) return fail(TRMC_EINVAL, "every destination is NULL: nothing to fetch");
    if (peak_cn_step && !peak_cn) return fail(TRMC_EINVAL, "the step of a peak comes with the peak: its value destination is NULL");
    if (S.cou_days < 1)
        return fail(TRMC_ESTATE, "no day of the stream is complete yet: its last rows run " + std::to_string(S.lmax)
                                     + " tiles behind its first -- push further days or trmc_stream_flush");
    const int64_t days = S.cou_days;
    const size_t n = (size_t)pl->nseg;
    // behind the last fold queued (nothing is queued meanwhile: the calls of a plan come from one thread)
    HIP_TRY(hipStreamWaitEvent(pl->cstream, S.ev_cou, 0));
    if (n) {
        const size_t off = (n * (size_t)pl->esz + 255) / 256 * 256;
        int64_t *const rows64 = (int64_t *)((char *)S.cou_rows.p + off);
        const int rc = by_precision(pl, [&](auto t) -> int {
            using T = decltype(t);
            hipLaunchKernelGGL((k_stream_courant_rows<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pl->cstream, (const T *)S.cou_peak.p,
                               (const int32_t *)S.cou_step.p, (const int32_t *)S.cou_count.p, (const int32_t *)pl->sh->pos_of_row.p,
                               (T *)S.cou_rows.p, rows64, rows64 + n, (int32_t)pl->nseg);
            HIP_TRY(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
        if (peak_cn) HIP_TRY(hipMemcpyAsync(peak_cn, S.cou_rows.p, n * (size_t)pl->esz, hipMemcpyDeviceToHost, pl->cstream));
        if (peak_cn_step) HIP_TRY(hipMemcpyAsync(peak_cn_step, rows64, n * sizeof(int64_t), hipMemcpyDeviceToHost, pl->cstream));
        if (steps_over) HIP_TRY(hipMemcpyAsync(steps_over, rows64 + n, n * sizeof(int64_t), hipMemcpyDeviceToHost, pl->cstream));
    }
    HIP_TRY(hipStreamSynchronize(pl->cstream));
    if (days_out) *days_out = days;
    return 0;
}

int trmc_stream_courant_kernel_ms(trmc_plan *pl, double *ms_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!ms_out) return fail(TRMC_EINVAL, "ms_out is NULL");
    if (!S.cou || !S.cou_ms_ok) return fail(TRMC_ESTATE, "no day has been folded into the Courant number of this stream yet");
    HIP_TRY(hipEventSynchronize(S.ev_cou));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev_cou0, S.ev_cou));
    *ms_out = ms;
    return 0;
}

int trmc_stream_set_depth_exceedance(trmc_plan *pl, int32_t nlevels, const void *th)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (nlevels < 0 || nlevels > 4) return fail(TRMC_EINVAL, "nlevels must be 0..4 (0: no depth exceedance)");
    if (nlevels > 0 && !th) return fail(TRMC_EINVAL, "th is NULL");
    if (nlevels == 0) { // (withdrawn: the next stream holds no accumulator and queues no fold; nothing is kept)
        if (!pl->seq) return 0;
        StreamRun &S = *pl->seq;
        S.dex_K_want = S.dex_KP_want = 0;
        for (DevBuf *b : {&S.dex_th, &S.dex_acc, &S.dex_rows}) b->release();
        return 0;
    }
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    StreamRun &S = *pl->seq;
    // the table's rows are 1, 2 or 4 wide (k_stream_exceed_depth's KP), +inf -- never over -- behind the caller's levels
    const int32_t pad = nlevels == 3 ? 4 : nlevels;
    S.dex_K_want = S.dex_KP_want = 0; // (nothing half-set if the copy fails)
    const int rc = by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        const T *const src = (const T *)th;
        std::vector<T> host((size_t)pl->nseg * pad, std::numeric_limits<T>::infinity());
        for (int64_t r = 0; r < pl->nseg; ++r)
            for (int32_t k = 0; k < nlevels; ++k) host[(size_t)r * pad + k] = src[(size_t)r * nlevels + k];
        if (int rc = S.dex_th.ensure(host.size() * sizeof(T))) return rc;
        // (synchronous: the table is whole before the call returns, whichever stream reads it)
        if (!host.empty()) HIP_TRY(hipMemcpy(S.dex_th.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    });
    if (rc) return rc;
    S.dex_K_want = nlevels;
    S.dex_KP_want = pad;
    return 0;
}

int trmc_stream_depth_exceedance(trmc_plan *pl, int64_t *steps_over, int64_t *first_step, int64_t *last_step, int64_t *longest_run,
                                 int64_t *days_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (S.dex_K < 1)
        return fail(TRMC_ESTATE, "the stream was begun without a depth exceedance (trmc_stream_set_depth_exceedance precedes trmc_stream_begin)");
    if (S.dex_days < 1)
        return fail(TRMC_ESTATE, "no day of the stream is complete yet: its last rows run " + std::to_string(S.lmax)
                                     + " tiles behind its first -- push further days or trmc_stream_flush");
    const int64_t days = S.dex_days;
    const size_t n = (size_t)pl->nseg * (size_t)S.dex_K;
    int64_t *const dst[4] = {steps_over, first_step, last_step, longest_run};
    // behind the last fold queued (nothing is queued meanwhile: the calls of a plan come from one thread)
    HIP_TRY(hipStreamWaitEvent(pl->cstream, S.ev_dex, 0));
    if (n && (steps_over || first_step || last_step || longest_run)) {
        hipLaunchKernelGGL(k_stream_exceed_depth_rows, dim3(blocks_for((int64_t)n)), dim3(kBlock), 0, pl->cstream, (const int32_t *)S.dex_acc.p,
                           (const int32_t *)pl->sh->pos_of_row.p, (int64_t *)S.dex_rows.p, (int32_t)pl->nseg, pl->nseg_pad, S.dex_K, S.dex_KP);
        HIP_TRY(hipGetLastError());
        for (int f = 0; f < 4; ++f)
            if (dst[f]) HIP_TRY(hipMemcpyAsync(dst[f], (const int64_t *)S.dex_rows.p + (size_t)f * n, n * sizeof(int64_t), hipMemcpyDeviceToHost, pl->cstream));
    }
    HIP_TRY(hipStreamSynchronize(pl->cstream));
    if (days_out) *days_out = days;
    return 0;
}

int trmc_stream_depth_exceedance_kernel_ms(trmc_plan *pl, double *ms_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!ms_out) return fail(TRMC_EINVAL, "ms_out is NULL");
    if (S.dex_K < 1 || !S.dex_ms_ok) return fail(TRMC_ESTATE, "no day has been folded into the depth exceedance of this stream yet");
    HIP_TRY(hipEventSynchronize(S.ev_dex));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev_dex0, S.ev_dex));
    *ms_out = ms;
    return 0;
}

int trmc_stream_set_velocity(trmc_plan *pl, int on, int32_t nlevels, const void *th)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (!on) { // (withdrawn: the next stream holds no accumulator and queues no fold; nothing is kept.  On either engine: a plan
               // of the dataflow engine has nothing declared, and withdrawing nothing is no error)
        if (!pl->seq) return 0;
        StreamRun &S = *pl->seq;
        S.vel_want = false;
        S.vel_K_want = S.vel_KP_want = 0;
        for (DevBuf *b : {&S.vel_th, &S.vel_peak, &S.vel_step, &S.vel_acc, &S.vel_rows}) b->release();
        return 0;
    }
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (nlevels < 0 || nlevels > 4) return fail(TRMC_EINVAL, "nlevels must be 0..4 (0: the peak and its step only)");
    if (nlevels > 0 && !th) return fail(TRMC_EINVAL, "th is NULL");
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    StreamRun &S = *pl->seq;
    // the table's rows are 1, 2 or 4 wide (k_stream_velocity's KP), +inf -- never over -- behind the caller's levels
    const int32_t pad = nlevels == 3 ? 4 : nlevels;
    S.vel_want = false; // (nothing half-set if the copy fails)
    S.vel_K_want = S.vel_KP_want = 0;
    if (nlevels > 0) {
        const int rc = by_precision(pl, [&](auto t) -> int {
            using T = decltype(t);
            const T *const src = (const T *)th;
            std::vector<T> host((size_t)pl->nseg * pad, std::numeric_limits<T>::infinity());
            for (int64_t r = 0; r < pl->nseg; ++r)
                for (int32_t k = 0; k < nlevels; ++k) host[(size_t)r * pad + k] = src[(size_t)r * nlevels + k];
            if (int rc = S.vel_th.ensure(host.size() * sizeof(T))) return rc;
            // (synchronous: the table is whole before the call returns, whichever stream reads it)
            if (!host.empty()) HIP_TRY(hipMemcpy(S.vel_th.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
            return 0;
        });
        if (rc) return rc;
    } else {
        S.vel_th.release();
    }
    S.vel_want = true;
    S.vel_K_want = nlevels;
    S.vel_KP_want = pad;
    return 0;
}

int trmc_stream_velocity(trmc_plan *pl, void *peak, int64_t *peak_step, int64_t *steps_over, int64_t *first_step, int64_t *last_step,
                         int64_t *longest_run, int64_t *days_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!S.vel) return fail(TRMC_ESTATE, "the stream was begun without the velocity (trmc_stream_set_velocity precedes trmc_stream_begin)");
    int64_t *const dst[4] = {steps_over, first_step, last_step, longest_run};
    const bool levels = steps_over || first_step || last_step || longest_run;
    if (!peak && !peak_step && !levels) return fail(TRMC_EINVAL, "every destination is NULL: nothing to fetch");
    if (peak_step && !peak) return fail(TRMC_EINVAL, "the step of a peak comes with the peak: its value destination is NULL");
    if (levels && S.vel_K < 1)
        return fail(TRMC_EINVAL, "the stream's velocity was declared without thresholds (nlevels = 0): it holds no exceedance figures");
    if (S.vel_days < 1)
        return fail(TRMC_ESTATE, "no day of the stream is complete yet: its last rows run " + std::to_string(S.lmax)
                                     + " tiles behind its first -- push further days or trmc_stream_flush");
    const int64_t days = S.vel_days;
    const size_t n = (size_t)pl->nseg, nk = n * (size_t)S.vel_K;
    // behind the last fold queued (nothing is queued meanwhile: the calls of a plan come from one thread)
    HIP_TRY(hipStreamWaitEvent(pl->cstream, S.ev_vel, 0));
    if (n) {
        const size_t off = (n * (size_t)pl->esz + 255) / 256 * 256, off2 = off + (n * sizeof(int64_t) + 255) / 256 * 256;
        int64_t *const step64 = (int64_t *)((char *)S.vel_rows.p + off), *const lev64 = (int64_t *)((char *)S.vel_rows.p + off2);
        if (peak || peak_step) {
            const int rc = by_precision(pl, [&](auto t) -> int {
                using T = decltype(t);
                hipLaunchKernelGGL((k_stream_velocity_rows<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pl->cstream, (const T *)S.vel_peak.p,
                                   (const int32_t *)S.vel_step.p, (const int32_t *)pl->sh->pos_of_row.p, (T *)S.vel_rows.p, step64,
                                   (int32_t)pl->nseg);
                HIP_TRY(hipGetLastError());
                return 0;
            });
            if (rc) return rc;
            if (peak) HIP_TRY(hipMemcpyAsync(peak, S.vel_rows.p, n * (size_t)pl->esz, hipMemcpyDeviceToHost, pl->cstream));
            if (peak_step) HIP_TRY(hipMemcpyAsync(peak_step, step64, n * sizeof(int64_t), hipMemcpyDeviceToHost, pl->cstream));
        }
        if (levels) { // (the accumulator has k_stream_exceed_depth's layout: its gather)
            hipLaunchKernelGGL(k_stream_exceed_depth_rows, dim3(blocks_for((int64_t)nk)), dim3(kBlock), 0, pl->cstream, (const int32_t *)S.vel_acc.p,
                               (const int32_t *)pl->sh->pos_of_row.p, lev64, (int32_t)pl->nseg, pl->nseg_pad, S.vel_K, S.vel_KP);
            HIP_TRY(hipGetLastError());
            for (int f = 0; f < 4; ++f)
                if (dst[f]) HIP_TRY(hipMemcpyAsync(dst[f], lev64 + (size_t)f * nk, nk * sizeof(int64_t), hipMemcpyDeviceToHost, pl->cstream));
        }
    }
    HIP_TRY(hipStreamSynchronize(pl->cstream));
    if (days_out) *days_out = days;
    return 0;
}

int trmc_stream_velocity_kernel_ms(trmc_plan *pl, double *ms_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!ms_out) return fail(TRMC_EINVAL, "ms_out is NULL");
    if (!S.vel || !S.vel_ms_ok) return fail(TRMC_ESTATE, "no day has been folded into the velocity of this stream yet");
    HIP_TRY(hipEventSynchronize(S.ev_vel));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev_vel0, S.ev_vel));
    *ms_out = ms;
    return 0;
}

// the reservoir tables of a day against the declaration (trmc_set_reservoir_da) and the capacity fixed at trmc_stream_begin
static int stream_rda_check(const trmc_plan *pl, const StreamRun &S, const trmc_stream_day &day)
{
    if (!S.rda) {
        if (day.reservoir_da || day.res_da_state_host || day.res_da_tsidx_host)
            return fail(TRMC_EINVAL, "reservoir data-assimilation tables for a stream without them (trmc_set_reservoir_da and "
                                     "trmc_stream_set_reservoir_da precede trmc_stream_begin)");
        return 0;
    }
    if (!day.reservoir_da)
        return fail(TRMC_EINVAL, "the stream carries reservoir data assimilation: every day must bring its reservoir tables "
                                 "(trmc_stream_day::reservoir_da)");
    const trmc_reservoir_da_table *tab[3] = {&day.reservoir_da->usgs, &day.reservoir_da->usace, &day.reservoir_da->rfc};
    const char *const tname[3] = {"usgs", "usace", "rfc"};
    for (int k = 0; k < 3; ++k) {
        const trmc_reservoir_da_table &t = *tab[k];
        if (t.n != pl->res_da_n[k])
            return fail(TRMC_EINVAL, std::string(tname[k]) + " table of a day: " + std::to_string(t.n) + " rows, the stream was declared with "
                                         + std::to_string(pl->res_da_n[k]));
        if (t.n == 0) continue;
        if (t.ncol < 1) return fail(TRMC_EINVAL, std::string(tname[k]) + " table of a day: rows without columns");
        if (t.ncol > S.rda_cap[k])
            return fail(TRMC_EINVAL, std::string(tname[k]) + " table of a day: " + std::to_string(t.ncol) + " columns exceed the stream's capacity of "
                                         + std::to_string(S.rda_cap[k]) + " (trmc_stream_set_reservoir_da)");
        if (!t.obs || (k < 2 && !t.time) || (k == 2 && !t.ipar)) return fail(TRMC_EINVAL, std::string(tname[k]) + " table of a day: a pointer is NULL");
    }
    if (day.reservoir_da->rfc_reset_idx)
        for (int64_t i = 0; i < pl->nres; ++i)
            if (pl->res_da_kind[(size_t)i] >= 4) {
                const int32_t idx = tab[2]->ipar[5 * pl->res_da_trow[(size_t)i]];
                if (idx < 0 || idx >= tab[2]->ncol)
                    return fail(TRMC_EINVAL, "rfc table row " + std::to_string(pl->res_da_trow[(size_t)i]) + ": timeseries_idx outside the series");
            }
    return 0;
}

int trmc_stream_set_packed_forcing(trmc_plan *pl, int64_t nfeat, const int64_t *feat_of_row, const double *pack_a, const double *pack_b)
{
    if (int rc = stream_check(pl, false)) return rc;
    if (pl->flow) return fail(TRMC_EINVAL, "a stream of windows runs on the level engine");
    if (nfeat < 0) return fail(TRMC_EINVAL, "nfeat < 0");
    if (nfeat > INT32_MAX) return fail(TRMC_EINVAL, "feature axis too long");
    const bool off = nfeat == 0 || !feat_of_row;
    if (off && !pl->seq) return 0; // (withdrawn where nothing was declared)
    if (!off && !pack_a) return fail(TRMC_EINVAL, "pack_a is NULL");
    if (!pl->seq) pl->seq = std::make_unique<StreamRun>();
    StreamRun &S = *pl->seq;
    S.pk_nfeat = 0;
    if (off) {
        S.pk_feat_of_pos.release();
        return 0;
    }
    const int64_t n = pl->nseg;
    std::vector<int32_t> feat_of_pos((size_t)n);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t f = feat_of_row[pl->sh->topo.row_of_pos[p]];
        if (f >= nfeat) return fail(TRMC_EINVAL, "feat_of_row entry outside the feature axis");
        feat_of_pos[(size_t)p] = f < 0 ? -1 : (int32_t)f;
    }
    if (int rc = upload_i32(S.pk_feat_of_pos, feat_of_pos, 1)) return rc;
    S.pk_a = pack_spec(pack_a);
    S.pk_b = pack_spec(pack_b);
    S.pk_two = pack_b != nullptr;
    S.pk_nfeat = nfeat;
    return 0;
}

int trmc_stream_packed_forcing_kernel_ms(trmc_plan *pl, double *ms_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!ms_out) return fail(TRMC_EINVAL, "ms_out is NULL");
    if (!S.pk_ms_ok) return fail(TRMC_ESTATE, "no day of this stream has been pushed as packed columns yet");
    HIP_TRY(hipEventSynchronize(S.ev_pk1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev_pk0, S.ev_pk1));
    *ms_out = ms;
    return 0;
}

// a day's push, float (raw_a = raw_b = NULL, packed = false) or packed
static int stream_push_day(trmc_plan *pl, const trmc_stream_day *day, const int32_t *raw_a, const int32_t *raw_b, bool packed)
{
    if (int rc = stream_check(pl, true)) return rc;
    if (!day) return fail(TRMC_EINVAL, "day is NULL");
    StreamRun &S = *pl->seq;
    if (packed) {
        if (S.pk_nfeat < 1)
            return fail(TRMC_ESTATE, "a packed day for a stream without the declaration (trmc_stream_set_packed_forcing precedes trmc_stream_begin)");
        if (day->qlat) return fail(TRMC_EINVAL, "a packed day brings raw_a / raw_b: trmc_stream_day::qlat must be NULL");
        if (!raw_a) return fail(TRMC_EINVAL, "raw_a is NULL");
        if ((raw_b != nullptr) != S.pk_two)
            return fail(TRMC_EINVAL, S.pk_two ? "the stream's packed days were declared with two variables (pack_b): raw_b is NULL"
                                              : "the stream's packed days were declared with one variable (pack_b = NULL): raw_b must be NULL");
    }
    const void *const qlat = day->qlat;
    const int64_t nq = day->nq;
    const int32_t rowset = day->rowset;
    void *const hyd_host = day->hyd_host, *const fvd_host = day->fvd_host;
    if (S.ngage > 0) {
        if (!day->da_mode || !day->da_a || !day->da_w)
            return fail(TRMC_EINVAL, "the stream has gage rows (trmc_stream_set_gages): every day must carry its nudging tables (mode, a, w)");
        if (day->da_ngage != S.ngage || day->da_nsteps != S.nsteps)
            return fail(TRMC_EINVAL, "nudging tables of a day must be [" + std::to_string(S.ngage) + "][" + std::to_string(S.nsteps) + "], got ["
                                         + std::to_string(day->da_ngage) + "][" + std::to_string(day->da_nsteps) + "]");
    } else if (day->da_mode || day->da_a || day->da_w || day->da_q0 || day->nudge_host) {
        return fail(TRMC_EINVAL, "nudging tables for a stream without gage rows (trmc_stream_set_gages precedes trmc_stream_begin)");
    }
    if (int rc = stream_rda_check(pl, S, *day)) return rc;
    if (day->res_inflow_host && (day->res_nres != pl->nres || day->res_nsteps != S.nsteps))
        return fail(TRMC_EINVAL, "the reservoir-inflow record of a day is [" + std::to_string(pl->nres) + "][" + std::to_string(S.nsteps) + "], got ["
                                     + std::to_string(day->res_nres) + "][" + std::to_string(day->res_nsteps) + "]");
    if (pl->nseg > 0 && !qlat && !packed) return fail(TRMC_EINVAL, "qlat is NULL");
    if (nq != S.nq) return fail(TRMC_EINVAL, "every day of a stream has the forcing columns of the first (" + std::to_string(S.nq) + ")");
    if (S.g_done > S.days_pushed * S.tpd - 1 && S.days_complete < S.days_pushed)
        return fail(TRMC_ESTATE, "the stream has been advanced past its last day without being flushed: trmc_stream_flush first");
    if (hyd_host && (rowset < 0 || rowset >= (int32_t)pl->rowsets.size())) return fail(TRMC_EINVAL, "unknown row set");
    if (S.tab[P_STAGE].next && (rowset < 0 || rowset >= (int32_t)pl->rowsets.size())) {
        S.tab[P_STAGE].next = nullptr; // (the array does not wait for another day)
        return fail(TRMC_EINVAL, "a day's stage (trmc_stream_stage_dest) covers the rows of the day's row set: the day names none, or an unknown one");
    }
    if (fvd_host && S.dec_stride == 0 && !S.want_out)
        return fail(TRMC_EINVAL, "the stream was begun without full_output / output_stride: there is no (q, v, d) block to hand over");
    return by_precision(pl, [&](auto t) { return stream_push_t<decltype(t)>(pl, *day, raw_a, raw_b); });
}

int trmc_stream_push_day(trmc_plan *pl, const trmc_stream_day *day) { return stream_push_day(pl, day, nullptr, nullptr, false); }

int trmc_stream_push_day_packed(trmc_plan *pl, const trmc_stream_day *day, const int32_t *raw_a, const int32_t *raw_b)
{
    return stream_push_day(pl, day, raw_a, raw_b, true);
}

int trmc_stream_push(trmc_plan *pl, const void *qlat, int64_t nq, const void *boundary_q_dev, int32_t rowset, void *hyd_host,
                     void *q0_host, void *fvd_host)
{
    trmc_stream_day day{};
    day.qlat = qlat;
    day.nq = nq;
    day.boundary_q_dev = boundary_q_dev;
    day.rowset = rowset;
    day.hyd_host = hyd_host;
    day.q0_host = q0_host;
    day.fvd_host = fvd_host;
    return trmc_stream_push_day(pl, &day);
}

int trmc_stream_boundary(trmc_plan *pl, int64_t day, const void *q_dev, int64_t src_row_stride, const int64_t *index_dev, void *stream)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    const trmc::Topology &tp = pl->sh->topo;
    if (tp.nboundary == 0) return 0;
    if (!q_dev) return fail(TRMC_EINVAL, "q_dev is NULL");
    if (day < 0 || day >= S.days_pushed) return fail(TRMC_EINVAL, "the day has not been pushed");
    if (S.prod[(size_t)(day % S.slots)].day != day) return fail(TRMC_ESTATE, "the day's slot has been reused");
    if (src_row_stride < S.nsteps) return fail(TRMC_EINVAL, "src_row_stride must be at least nsteps");
    hipStream_t st = stream ? (hipStream_t)stream : S.fst;
    const size_t np = (size_t)pl->nseg_pad;
    const int32_t slot = (int32_t)(day % S.slots);
    const int rc = by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        T *q = (T *)S.tm.p + (size_t)slot * S.slot_tm;
        if (day > 0) { // time row 0: where the boundary rows' day before ended (filled by the call for that day, in order)
            const T *qp = (const T *)S.tm.p + (size_t)((day - 1) % S.slots) * S.slot_tm + (size_t)S.nsteps * np;
            HIP_TRY(hipMemcpyAsync(q, qp, (size_t)tp.nboundary * sizeof(T), hipMemcpyDeviceToDevice, st));
        }
        hipLaunchKernelGGL((k_stream_boundary_idx<T>), dim3(blocks_for(tp.nboundary * (int64_t)S.nsteps)), dim3(kBlock), 0, st, (const T *)q_dev,
                           src_row_stride, index_dev, q, (int32_t)tp.nboundary, S.nsteps, pl->nseg_pad);
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    return S.mk_bnd.record(st);
}

int trmc_stream_gather(trmc_plan *pl, int64_t day, int32_t rowset, void *dst_dev, void *stream)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (rowset < 0 || rowset >= (int32_t)pl->rowsets.size()) return fail(TRMC_EINVAL, "unknown row set");
    if (!dst_dev) return fail(TRMC_EINVAL, "dst_dev is NULL");
    if (day < 0 || day >= S.days_pushed) return fail(TRMC_EINVAL, "the day has not been pushed");
    if (S.prod[(size_t)(day % S.slots)].day != day) return fail(TRMC_ESTATE, "the day's slot has been reused");
    if (S.g_done < (day + 1) * S.tpd - 1 + pl->rowset_lagk[(size_t)rowset])
        return fail(TRMC_ESTATE, "the rows of the set have not been queued through day " + std::to_string(day) + " yet (they run up to "
                                     + std::to_string(pl->rowset_lagk[(size_t)rowset]) + " tiles behind)");
    const int64_t nrows = pl->rowset_n[(size_t)rowset];
    if (nrows == 0) return 0;
    hipStream_t pst = stream_last(pl, S);
    hipStream_t st = stream ? (hipStream_t)stream : pst;
    if (st != pst) {
        HIP_TRY(hipEventRecord(S.ev_gat, pst));
        HIP_TRY(hipStreamWaitEvent(st, S.ev_gat, 0));
    }
    // rows of the slices are on the tile stream, and the last launch queued there may still run while the clusters' stream is
    // done with the day (cluster launch g waits for slab launch g - 1 only): the gather waits for it -- on pst as well
    if (S.W > 0 && st != pl->wstream) {
        HIP_TRY(hipEventRecord(S.ev_gat, pl->wstream));
        HIP_TRY(hipStreamWaitEvent(st, S.ev_gat, 0));
    }
    const int32_t slot = (int32_t)(day % S.slots);
    return by_precision(pl, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((k_gather_rows<T>), dim3(blocks_for(nrows * S.nsteps)), dim3(kBlock), 0, st, (const T *)S.tm.p + (size_t)slot * S.slot_tm,
                           (const int32_t *)pl->rowsets[(size_t)rowset].p, (T *)dst_dev, nrows, pl->nseg_pad, S.nsteps, 1);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int trmc_stream_advance(trmc_plan *pl, int ntiles)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (ntiles < 0) return fail(TRMC_EINVAL, "ntiles < 0");
    const int64_t g_last = S.days_pushed * S.tpd - 1 + S.lmax; // the launch that ends the last day pushed
    const int64_t g_from = std::max<int64_t>(S.g_done, S.days_pushed * S.tpd - 1);
    const int64_t g_to = std::min<int64_t>(g_last, g_from + ntiles);
    int rc = 0;
    if (S.days_complete < S.days_pushed && g_to > g_from) {
        // (trmc_stream_boundary on a stream of the caller's: these launches go behind it)
        if (int rc = S.mk_bnd.order(pl->wstream)) return rc;
        if (int rc = S.mk_bnd.order(pl->stream)) return rc;
        S.mk_bnd.settle();
        rc = by_precision(pl, [&](auto t) { return stream_launch<decltype(t)>(pl, S, g_from, g_to, S.days_pushed); });
    }
    if (!rc && S.days_complete >= S.days_pushed) S.day_min = S.days_pushed; // (what follows starts with a new day; the rows' tiles of earlier days are done)
    return rc;
}

int trmc_stream_flush(trmc_plan *pl) { return trmc_stream_advance(pl, 1 << 30); }

int trmc_stream_wait(trmc_plan *pl, int64_t day)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (day < 0 || day >= S.days_pushed) return fail(TRMC_EINVAL, "no such day in the stream");
    StreamProd &p = S.prod[(size_t)(day % S.slots)];
    if (p.day != day) return fail(TRMC_ESTATE, "the day's slot has been reused: its products were handed over long ago");
    if (!p.queued)
        return fail(TRMC_ESTATE, "day " + std::to_string(day) + " has not been queued to its end: its last rows run " + std::to_string(S.lmax)
                                     + " tiles behind its first -- push further days or trmc_stream_flush");
    HIP_TRY(hipEventSynchronize(p.ev_done));
    return 0;
}

int trmc_stream_day_ms(trmc_plan *pl, int64_t day, double *ms_out)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (!ms_out) return fail(TRMC_EINVAL, "ms_out is NULL");
    if (day < 0 || day >= S.days_pushed || S.prod[(size_t)(day % S.slots)].day != day) return fail(TRMC_EINVAL, "no such day in the ring");
    const size_t slot = (size_t)(day % S.slots);
    HIP_TRY(hipEventSynchronize(S.ev_t1[slot]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev_t0[slot], S.ev_t1[slot]));
    *ms_out = ms;
    return 0;
}

int trmc_stream_info(const trmc_plan *pl, int32_t *slots, int32_t *tiles_per_day, int32_t *lag_max, int32_t *wide_levels,
                     int32_t *cluster_levels, int64_t *days_pushed, int64_t *days_complete, int64_t *launches)
{
    if (!pl || !pl->seq) return fail(TRMC_ESTATE, "no stream of windows was begun on this plan");
    const StreamRun &S = *pl->seq;
    if (slots) *slots = S.slots;
    if (tiles_per_day) *tiles_per_day = S.tpd;
    if (lag_max) *lag_max = S.lmax;
    if (wide_levels) *wide_levels = S.W;
    if (cluster_levels) *cluster_levels = S.C;
    if (days_pushed) *days_pushed = S.days_pushed;
    if (days_complete) *days_complete = S.days_complete;
    if (launches) *launches = S.launches;
    return 0;
}

int trmc_stream_end(trmc_plan *pl)
{
    if (int rc = stream_check(pl, true)) return rc;
    StreamRun &S = *pl->seq;
    if (int rc = trmc_stream_flush(pl)) return rc;
    // the state the stream leaves -- the last day's final (q, q, depth) -- staged for whatever routes next on this plan
    if (S.days_pushed > 0 && pl->nseg > 0) {
        const int32_t slot = (int32_t)((S.days_pushed - 1) % S.slots);
        if (int rc = pl->in_q0.ensure((size_t)pl->nseg * 3 * pl->esz)) return rc;
        hipStream_t pst = stream_last(pl, S);
        const int rc = by_precision(pl, [&](auto t) -> int {
            using T = decltype(t);
            const T *q = (const T *)S.tm.p + (size_t)slot * S.slot_tm;
            hipLaunchKernelGGL((k_final_state<T>), dim3(blocks_for(pl->nseg)), dim3(kBlock), 0, pst, q, q + S.plane, (const int32_t *)pl->sh->row_of_pos.p,
                               (T *)pl->in_q0.p, (int32_t)pl->nseg, pl->nseg_pad, S.nsteps, 1, S.nsteps);
            HIP_TRY(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
        pl->q0_staged = true;
        pl->state_missing = false;
    }
    HIP_TRY(hipStreamSynchronize(pl->wstream));
    HIP_TRY(hipStreamSynchronize(pl->stream));
    HIP_TRY(hipStreamSynchronize(pl->hstream));
    if (S.fst) HIP_TRY(hipStreamSynchronize(S.fst));
    HIP_TRY(hipStreamSynchronize(pl->cstream));
    if (pl->collect_cost) pl->cost_nsteps = (int32_t)std::min<int64_t>(S.days_pushed * S.nsteps, 1 << 30);
    for (StreamProdRow &t : S.tab) t.next = nullptr;
    S.active = false;
    return 0;
}
