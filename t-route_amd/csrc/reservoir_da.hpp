// reservoir_da.hpp -- reservoir data assimilation behind the level-pool step: hybrid persistence (reservoir types 2 USGS,
// 3 USACE) and RFC forecast series (types 4 RFC, 5 glacially dammed lake).
//
// Semantics: the reservoir branch of the reference's time x reach loop (mc_reach.pyx:548-710) with the two Python
// functions it calls, fast_reach/reservoir_hybrid_da.py (reservoir_hybrid_da, _modify_for_projected_storage) and
// fast_reach/reservoir_RFC_da.py:193-319 (reservoir_RFC_da).
//
// ARITHMETIC TYPES.  Those functions are Python, called from Cython, so the type of every operation follows from what
// the caller hands over:
//   * C `float` variables and struct members (the inflow, the level-pool outflow and elevation, dt, dt * timestep, the
//     pool's area / max_depth / orifice_elevation) and elements of `const float[:]` memoryviews (the observation and time
//     rows) arrive as Python floats: fp32 VALUES in fp64 arithmetic.
//   * the per-reservoir state is indexed out of numpy arrays with a Python object as the index (res_idx[0][0]) and
//     arrives as numpy.float32 scalars.  An operation between a numpy.float32 and a Python float or int is carried out
//     in fp32, the Python operand rounded to fp32 first (numpy's promotion of Python scalars, NEP 50, numpy >= 2; the
//     recorded vectors under tests/golden pin it) -- comparisons included.
// So the hybrid step is fp64 where the outflow is an observation or the level-pool value, and fp32 where a previously
// persisted value is carried on; `Num` below carries a value with that distinction.  The RFC step is fp64 throughout.
// Results are rounded to fp32 where the loop stores them into float variables and arrays.
// Compile with -ffp-contract=off (every operation rounds once, as the interpreter's do).
#pragma once
#include "mc_segment.hpp"
#include <cstdint>

namespace trmc {

// ---- one step of each kind, as values ---------------------------------------------------------------------------
struct HybridIn {   // what the loop passes to reservoir_hybrid_da (mc_reach.pyx:593-610); lookback 48 h
    float now, prev_persisted, persistence_update_time, persistence_index, levelpool_outflow, inflow, routing_period, lake_area,
        max_depth, orifice_elevation, initial_water_elevation, update_time;
};
struct HybridOut {  // its six returns, each as the loop stores it (float variables and float arrays)
    float outflow, persisted_outflow, water_elevation, update_time, persistence_index, persistence_update_time;
};
struct RfcIn {      // what the loop passes to reservoir_RFC_da (mc_reach.pyx:669-687); lake_area in km2 (the loop scales it)
    float now, update_time, inflow, water_elevation, levelpool_outflow, levelpool_water_elevation, lake_area, max_water_elevation,
        routing_period;
    int32_t use_forecast, timeseries_idx, total_counts, da_timestep, persist_days, reservoir_type;
};
struct RfcOut {
    float outflow, water_elevation, update_time;
    int32_t timeseries_idx;
};

namespace da_detail {
struct Num {        // a Python float (f32 = false) or a numpy.float32 (f32 = true, v holds an fp32 value)
    double v;
    bool f32;
};
MC_HD Num py(double v) { return Num{v, false}; }
MC_HD Num np32(float v) { return Num{(double)v, true}; }
MC_HD Num sub(Num a, Num b) { return (a.f32 || b.f32) ? np32((float)a.v - (float)b.v) : py(a.v - b.v); }
MC_HD Num add(Num a, Num b) { return (a.f32 || b.f32) ? np32((float)a.v + (float)b.v) : py(a.v + b.v); }
MC_HD Num mul(Num a, Num b) { return (a.f32 || b.f32) ? np32((float)a.v * (float)b.v) : py(a.v * b.v); }
MC_HD Num div(Num a, Num b) { return (a.f32 || b.f32) ? np32((float)a.v / (float)b.v) : py(a.v / b.v); }
MC_HD bool lt(Num a, Num b) { return (a.f32 || b.f32) ? (float)a.v < (float)b.v : a.v < b.v; }
MC_HD bool le(Num a, Num b) { return (a.f32 || b.f32) ? (float)a.v <= (float)b.v : a.v <= b.v; }
MC_HD bool gt(Num a, Num b) { return lt(b, a); }
MC_HD bool is_nan(double x) { return x != x; }
} // namespace da_detail

// reservoir_hybrid_da with update_time_interval 3600, persistence_update_time_interval 86400, lookback 48 h.
// obs / time: the gage's observation row and the table's time row, ncol >= 1 entries each.
MC_HD HybridOut hybrid_da_step(const float *obs, const float *time, int32_t ncol, const HybridIn &in)
{
    using namespace da_detail;
    const float persistence_limit = 11.0f;
    const Num now = py(in.now), lp_out = py(in.levelpool_outflow), inflow = py(in.inflow), rp = py(in.routing_period);
    const Num prev = np32(in.prev_persisted), put = np32(in.persistence_update_time), update_time = np32(in.update_time);
    float new_index = in.persistence_index, new_put = in.persistence_update_time, new_update_time = in.update_time;
    const float put_next = in.persistence_update_time + 86400.0f, index_next = in.persistence_index + 1.0f;
    const double area_m2 = (double)in.lake_area * 1e6;
    const Num initial_storage = py(((double)in.initial_water_elevation - (double)in.orifice_elevation) * area_m2);
    const Num maximum_storage = py(((double)in.max_depth - (double)in.orifice_elevation) * area_m2);

    Num persisted = prev;
    if (!lt(now, update_time)) { // look for an observation: the time nearest to, not later than, update_time ...
        int32_t t_idx = 0;
        float best = __builtin_inff();
        for (int32_t i = 0; i < ncol; ++i) {
            const float d = in.update_time - time[i];
            if (d >= 0.0f && d < best) {
                best = d;
                t_idx = i;
            }
        }
        int32_t found = -1; // ... and from there backwards the first one that is not NaN
        for (int32_t i = t_idx; i >= 0; --i)
            if (!is_nan(obs[i])) {
                found = i;
                break;
            }
        bool tick = true; // persist what was persisted before; the persistence index counts on when its time has come
        if (found >= 0) {
            new_update_time = in.update_time + 3600.0f;
            const float lookback = in.update_time - time[found];
            if (!(lookback > 172800.0f)) { // inside the window: the observation is the new persisted value
                persisted = py(obs[found]);
                new_index = 1.0f;
                new_put = put_next;
                tick = false;
            }
        }
        if (tick && !lt(now, put)) {
            new_index = index_next;
            new_put = put_next;
        }
    } else if (!lt(now, put)) {
        new_index = index_next;
        new_put = put_next;
        if (in.persistence_index > persistence_limit) { // persisted for too long: back to the level pool
            persisted = lp_out;
            new_index = 0.0f;
        }
    }
    Num outflow = persisted;
    if (is_nan(persisted.v)) {
        outflow = lp_out;
        new_index = 0.0f;
    }
    // _modify_for_projected_storage (min_storage = 0: its minimum-storage branch cannot be taken)
    const Num assess = outflow, zero = py(0.0);
    if (lt(assess, zero)) outflow = zero;
    const Num projected = add(initial_storage, mul(sub(inflow, assess), rp));
    const bool max_reached = gt(projected, maximum_storage);
    if (le(projected, zero)) outflow = inflow;
    if (lt(outflow, zero)) outflow = zero;
    if (max_reached && lt(outflow, lp_out)) outflow = lp_out;
    const Num delta_storage = mul(sub(inflow, outflow), rp);
    const Num elevation = add(py(in.initial_water_elevation), div(delta_storage, py(area_m2)));

    HybridOut o;
    o.outflow = (float)outflow.v;
    o.persisted_outflow = (float)persisted.v;
    o.water_elevation = (float)elevation.v;
    o.update_time = new_update_time;
    o.persistence_index = new_index;
    o.persistence_update_time = new_put;
    return o;
}

// reservoir_RFC_da.  series: the lake's forecast row, ncol >= 1 entries (an index past its end -- an IndexError in the
// reference -- reads the last entry).
MC_HD RfcOut rfc_da_step(const float *series, int32_t ncol, const RfcIn &in)
{
    using namespace da_detail;
    const double inflow = in.inflow, lp_out = in.levelpool_outflow, rp = in.routing_period;
    const double lake_area = (double)in.lake_area * 1.0e6; // (m2: a float times a double constant in the loop)
    const bool lake4 = in.reservoir_type == 4;
    auto at = [&](int32_t i) { return (double)series[i < 0 ? 0 : (i >= ncol ? ncol - 1 : i)]; };
    RfcOut o;
    o.update_time = in.update_time;
    o.timeseries_idx = in.timeseries_idx;
    double outflow = lake4 ? lp_out : inflow;
    double elevation = in.levelpool_water_elevation;
    if (in.use_forecast && (double)in.now <= (double)((int64_t)in.persist_days * 86400)) {
        if (in.now >= in.update_time && in.timeseries_idx < in.total_counts) {
            o.update_time = in.update_time + (float)in.da_timestep;
            o.timeseries_idx = in.timeseries_idx + 1;
        }
        double q = lake4 ? at(o.timeseries_idx) : inflow + at(o.timeseries_idx);
        double h = (double)in.water_elevation + ((inflow - q) / lake_area) * rp;
        if (h < 0.0) h = 0.0;
        else if (h > (double)in.max_water_elevation) h = in.max_water_elevation;
        if (q < 0.0) // the nearest earlier entry that is not negative (entry 0 is never looked at)
            for (int32_t i = o.timeseries_idx; q < 0.0 && i > 1;) q = at(--i);
        if (!(q < 0.0)) {
            outflow = q;
            elevation = h;
        }
    }
    o.outflow = (float)outflow;
    o.water_elevation = (float)elevation;
    return o;
}

// ---- the tables of a window on the device --------------------------------------------------------------------------
// One buffer: a record per level-pool reservoir of the plan (trmc_set_reservoirs order), then the float rows the records
// point into.  The four (hybrid) or two (RFC) state values of a record are read and written by the one thread that owns
// the reservoir's row at that step (mc_reach.pyx:624-636, :701-703).
// What a reservoir carries from step to step -- and, between two windows or two days of a stream, from one to the next.
struct ResDaState {
    float update_time, prev_persisted, persistence_index, persistence_update_time; // (RFC: update_time only)
    int32_t timeseries_idx;                                                         // (RFC only)
};
struct ResDaRec {
    int32_t kind;                // 0: level pool only; 2, 3: hybrid persistence; 4, 5: RFC series
    int32_t ncol;                // entries of the observation row (and of the time row)
    int64_t obs_off, time_off;   // where they begin, in floats from the start of the buffer
    ResDaState st;               // a window: the state lives here; a day of a stream: what the day ended on (see reservoir_da_row_day)
    int32_t total_counts, use_forecast, da_timestep, persist_days;
    int32_t reset_idx;           // a day of a stream, RFC: != 0 = the day starts from st.timeseries_idx of THIS record (a new forecast file)
};
static_assert(sizeof(ResDaRec) == 64, "ResDaRec layout");

// THE HAND-OVER between two windows: the loop returns update_time and persistence_update_time (RFC: update_time) less the
// window's length, so that they count from the start of the next one (mc_reach.pyx:820-837); everything else passes unchanged.
// t_end is float(nsteps) * float(dt) -- a C float product in the loop -- formed ONCE by the caller and handed over as a value,
// so that no compiler can fuse the product into the subtraction: the difference is one fp32 operation on two fp32 values.
MC_HD ResDaState reservoir_da_handover(int32_t kind, ResDaState s, float t_end)
{
    if (kind >= 2 && kind <= 5) s.update_time = s.update_time - t_end;
    if (kind == 2 || kind == 3) s.persistence_update_time = s.persistence_update_time - t_end;
    return s;
}

struct ResDaResult {
    float outflow, water_elevation;
};

#if defined(__HIPCC__)
// The reservoir branch of the step kernels calls reservoir_da_row right behind levelpool_step: reservoir `ri` at step t (1-based) of
// the window, inflow, the elevation before the level-pool step, the level-pool results.  par = the pool's nine
// parameters (LevelPoolParams order).  Out of line on purpose: a handful of rows in ten thousand come here, and inlined
// its fp64 arithmetic and loops would be allocated registers in every kernel that has the branch.
// Consecutive launches of one window may overlap in time (k_mc_flow_lean hands a row's depth over through a granule): the
// state written here is released before the caller publishes the step, and acquired behind the caller's wait for it.
__device__ __forceinline__ ResDaResult reservoir_da_apply(const ResDaRec *rec, const float *base, ResDaState *st, int32_t t, float inflow,
                                                          float h_before, float dt, const float *par, float lp_outflow, float lp_elevation)
{
    ResDaResult r;
    const int32_t kind = rec->kind;
    const float now = dt * (float)t;
    if (kind <= 3) {
        HybridIn in;
        in.now = now;
        in.update_time = __hip_atomic_load(&st->update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        in.prev_persisted = __hip_atomic_load(&st->prev_persisted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        in.persistence_index = __hip_atomic_load(&st->persistence_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        in.persistence_update_time = __hip_atomic_load(&st->persistence_update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        in.levelpool_outflow = lp_outflow;
        in.inflow = inflow;
        in.routing_period = dt;
        in.lake_area = par[0];
        in.max_depth = par[1];
        in.orifice_elevation = par[4];
        in.initial_water_elevation = h_before;
        const HybridOut o = hybrid_da_step(base + rec->obs_off, base + rec->time_off, rec->ncol, in);
        __hip_atomic_store(&st->update_time, o.update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->prev_persisted, o.persisted_outflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->persistence_index, o.persistence_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->persistence_update_time, o.persistence_update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.outflow = o.outflow;
        r.water_elevation = o.water_elevation;
    } else {
        RfcIn in;
        in.now = now;
        in.update_time = __hip_atomic_load(&st->update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        in.timeseries_idx = __hip_atomic_load(&st->timeseries_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        in.inflow = inflow;
        in.water_elevation = h_before;
        in.levelpool_outflow = lp_outflow;
        in.levelpool_water_elevation = lp_elevation;
        in.lake_area = par[0];
        in.max_water_elevation = par[1];
        in.routing_period = dt;
        in.use_forecast = rec->use_forecast;
        in.total_counts = rec->total_counts;
        in.da_timestep = rec->da_timestep;
        in.persist_days = rec->persist_days;
        in.reservoir_type = kind;
        const RfcOut o = rfc_da_step(base + rec->obs_off, rec->ncol, in);
        __hip_atomic_store(&st->update_time, o.update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->timeseries_idx, o.timeseries_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.outflow = o.outflow;
        r.water_elevation = o.water_elevation;
    }
    return r;
}
__device__ __noinline__ ResDaResult reservoir_da_row(void *tables, int32_t ri, int32_t t, float inflow, float h_before, float dt,
                                                     const float *par, float lp_outflow, float lp_elevation)
{
    ResDaRec *const rec = (ResDaRec *)tables + ri;
    if (rec->kind == 0) return ResDaResult{lp_outflow, lp_elevation};
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const ResDaResult r = reservoir_da_apply(rec, (const float *)tables, &rec->st, t, inflow, h_before, dt, par, lp_outflow, lp_elevation);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    return r;
}
// The same in a STREAM OF DAYS (stream.inc).  `tables` are the tables of the row's DAY -- its slot of the ring, pushed with the
// day's forcing: observations and times counted from the day's start, the RFC parameters of the day -- and the state lives in
// `carry` [nres], outside the ring: a slot's tables arrive while rows further behind are still in the day before.  At the day's
// first step an RFC row takes the day's timeseries_idx where the day says so (reset_idx: the reference replaces the index when
// it reads a new forecast file, DataAssimilation.py:1978-1980).  At the day's last step the state is handed over
// (reservoir_da_handover) -- into the carry, where the row finds it at step 1 of the next day, and into the day's own record,
// the day's product.  One thread owns a reservoir row at any step, and a row's launches follow each other on one stream.
__device__ __noinline__ ResDaResult reservoir_da_row_day(void *tables, ResDaState *carry, int32_t ri, int32_t t, int32_t nsteps, float t_end,
                                                         float inflow, float h_before, float dt, const float *par, float lp_outflow,
                                                         float lp_elevation)
{
    ResDaRec *const rec = (ResDaRec *)tables + ri;
    const int32_t kind = rec->kind;
    if (kind == 0) return ResDaResult{lp_outflow, lp_elevation};
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    ResDaState *const st = carry + ri;
    if (t == 1 && kind >= 4 && rec->reset_idx != 0)
        __hip_atomic_store(&st->timeseries_idx, rec->st.timeseries_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const ResDaResult r = reservoir_da_apply(rec, (const float *)tables, st, t, inflow, h_before, dt, par, lp_outflow, lp_elevation);
    if (t == nsteps) {
        ResDaState s;
        s.update_time = __hip_atomic_load(&st->update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.prev_persisted = __hip_atomic_load(&st->prev_persisted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.persistence_index = __hip_atomic_load(&st->persistence_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.persistence_update_time = __hip_atomic_load(&st->persistence_update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.timeseries_idx = __hip_atomic_load(&st->timeseries_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s = reservoir_da_handover(kind, s, t_end);
        __hip_atomic_store(&st->update_time, s.update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->persistence_update_time, s.persistence_update_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rec->st = s;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    return r;
}
#endif

} // namespace trmc
