#!/usr/bin/env python
"""Fixtures of reservoir data assimilation (hybrid persistence, reservoir types 2 / 3; RFC series, types 4 / 5):
tests/golden/reservoir_da_vectors.npz, reservoir_da_network.npz (+ reservoir_da_network_general.npz), reservoir_da_prep.npz.

Runs in the development container only: it IMPORTS, at run time and from where they lie, the reference's
fast_reach/reservoir_hybrid_da.py and fast_reach/reservoir_RFC_da.py (xarray stubbed in sys.modules: the functions used
do not touch it) and, for the drop-in helper, routing/compute.py (joblib and the troute packages stubbed).  It holds none
of their text, and no test reads the reference tree: the tests read the three files written here.

1. STEP VECTORS.  Rows of inputs for reservoir_hybrid_da and reservoir_RFC_da with the functions' recorded returns.  The
   functions are handed what the Cython loop hands them (mc_reach.pyx:556-687): Python floats made from fp32 values for
   the C-float variables and struct members, the builtin memoryview of a float32 array for a `const float[:]` (its items
   are Python floats, as a Cython memoryview's are), numpy.float32 / numpy.int32 scalars for what the loop indexes out
   of numpy arrays with a Python object (the per-reservoir state), Python ints for items of `const int[:]` views.
   Branch counts are stored and asserted > 0.  _modify_for_projected_storage's minimum-storage branch cannot be reached
   through reservoir_hybrid_da (min_storage = 0 makes its condition contradictory); the four storage modifications
   counted are: negative outflow, maximum storage reached, storage deficit, and the final clamp of a negative result.

2. NETWORK GOLDEN.  The oracle's network loop is C and has no data-assimilation branch, so the reference's time x reach
   loop (mc_reach.pyx:492-750) is restated below in Python from oracle.segments(det=True), oracle.levelpool and the
   imported functions.  With no DA reservoir it is asserted equal to oracle.network(..., res=...) bit for bit.
   Domain: LowerColorado collapsed at waterbodies (tests/test_reservoirs.py::reservoir_case, x40 forcing), NTS steps.
   Reservoir types come from the domain's reservoir_index_AnA.nc: it marks twelve lakes of this subset as type 4 (RFC)
   and NONE as type 2 or 3 (its USGS / USACE crosswalks name no lake of the subset), so no observation of the shipped
   usgs_TimeSlice files belongs to a lake here.  Therefore: two type-1 lakes are made type 2 and two type 3 with
   synthetic observation series at 15-minute spacing that have NaN gaps, and one of each pair has nothing but NaN in
   the 48 h before the window (a gap longer than the lookback); the index's type-4 lakes get synthetic forecast series
   (from_files=False) with negative entries, and one of them is made type 5.
   The loop's type-5 branch reads the table row of whichever reservoir was looked up last (mc_reach.pyx:640-651 looks
   the row up for type 4 only); the restatement -- and the engine -- look a type-5 lake up like a type-4 one.
   Stored: every lake row in full, ~300 rows downstream of lakes in full, every 12th step of all rows, the final state
   tuples -- for both assume_short_ts values.  (The two-window test routes the window in two halves and compares with
   this one long window.)

3. DROP-IN HELPER.  Returns of the reference's own _prep_reservoir_da_dataframes (compute.py imported with stubs) on
   small DataFrames built by prep_cases() below, which tests/test_reservoir_da_prep.py builds again.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference"
REF_ROUTING = os.path.join(REF, "src/troute-routing/troute/routing")
NTS = 72
F = np.float32


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_functions():
    sys.modules.setdefault("xarray", types.ModuleType("xarray"))
    hyb = _load("ref_reservoir_hybrid_da", os.path.join(REF_ROUTING, "fast_reach/reservoir_hybrid_da.py"))
    rfc = _load("ref_reservoir_RFC_da", os.path.join(REF_ROUTING, "fast_reach/reservoir_RFC_da.py"))
    return hyb.reservoir_hybrid_da, rfc.reservoir_RFC_da


def reference_prep():
    for name in ("joblib", "troute", "troute.nhd_network", "troute.routing", "troute.routing.fast_reach",
                 "troute.routing.fast_reach.mc_reach", "troute.routing.diffusive_utils_v02",
                 "troute.routing.fast_reach.diffusive"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["joblib"].delayed = sys.modules["joblib"].Parallel = None
    sys.modules["troute.routing.fast_reach.mc_reach"].compute_network_structured = None
    sys.modules["troute.routing.fast_reach"].diffusive = sys.modules["troute.routing.fast_reach.diffusive"]
    sys.modules["troute"].nhd_network = sys.modules["troute.nhd_network"]
    sys.modules["troute"].routing = sys.modules["troute.routing"]
    sys.modules["troute.routing"].diffusive_utils_v02 = sys.modules["troute.routing.diffusive_utils_v02"]
    sys.modules["troute.routing"].fast_reach = sys.modules["troute.routing.fast_reach"]
    return _load("ref_compute", os.path.join(REF_ROUTING, "compute.py"))._prep_reservoir_da_dataframes


# ---------------------------------------------------------------------------------------------------- the loop's calls
def call_hybrid(fn, obs, time, x):
    """x: float32 [12] = now prev_persisted persistence_update_time persistence_index levelpool_outflow inflow
    routing_period lake_area max_depth orifice_elevation initial_water_elevation update_time (trmc::HybridIn).
    Returns float32 [6] as the loop stores them (trmc::HybridOut)."""
    x = np.asarray(x, F)
    r = fn(1, memoryview(np.ascontiguousarray(obs, F)), memoryview(np.ascontiguousarray(time, F)), float(x[0]), x[1], x[2], x[3],
           float(x[4]), float(x[5]), float(x[6]), float(x[7]), float(x[8]), float(x[9]), float(x[10]), 48.0, x[11])
    outflow, persisted, elevation, update_time, index, put = r
    return np.array([outflow, persisted, elevation, update_time, index, put], dtype=np.float64).astype(F)


def call_rfc(fn, series, x, k):
    """x: float32 [9] = now update_time inflow water_elevation levelpool_outflow levelpool_water_elevation lake_area(km2)
    max_water_elevation routing_period; k: int32 [6] = use_forecast timeseries_idx total_counts da_timestep persist_days
    reservoir_type (trmc::RfcIn).  Returns (float32 [3] outflow elevation update_time, timeseries_idx)."""
    x, k = np.asarray(x, F), np.asarray(k, np.int32)
    r = fn(int(k[0]), memoryview(np.ascontiguousarray(series, F)), k[1], int(k[2]), float(x[8]), float(x[0]), x[1], int(k[3]),
           int(k[4]) * 24 * 60 * 60, int(k[5]), float(x[2]), float(x[3]), float(x[4]), float(x[5]), float(x[6]) * 1.0e6,
           float(x[7]), "")
    return np.array([r[0], r[1], r[2]], dtype=np.float64).astype(F), int(r[3])


# ------------------------------------------------------------------------------------------------------- 1. vectors
def hybrid_branches(obs, time, x, out):
    """which branches a hybrid row takes, recomputed from inputs and recorded outputs (the counts stored with the vectors)"""
    b = {}
    now, prev, put, idx, lp, inflow, rp, area, maxd, oe, h0, ut = [float(v) for v in x]
    if now >= ut:
        d = F(ut) - np.asarray(time, F)
        t_idx = int(np.where(d >= 0, d, np.inf).argmin())
        found = next((i for i in range(t_idx, -1, -1) if not np.isnan(obs[i])), None)
        if found is None:
            b["obs_not_found"] = 1
        elif F(ut) - F(time[found]) > 172800:
            b["obs_outside_window"] = 1
        else:
            b["obs_inside_window"] = 1
    elif now >= put:
        b["tick_below_limit" if idx <= 11 else "tick_above_limit"] = 1
    if np.isnan(out[1]):
        b["nan_persisted"] = 1
    return b


def make_vectors(hyb, rfc, n=3000, seed=11):
    rng = np.random.default_rng(seed)
    ncol = 24
    # ---- hybrid
    H_obs, H_time, H_x, H_out = [], [], [], []
    counts = {k: 0 for k in ("obs_inside_window", "obs_outside_window", "obs_not_found", "tick_below_limit", "tick_above_limit",
                             "nan_persisted", "storage_negative_outflow", "storage_max_reached", "storage_deficit",
                             "storage_final_clamp", "max_storage_override")}
    import logging
    seen = []

    class Tap(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    logging.getLogger("").addHandler(Tap())
    for i in range(n):
        mode = i % 8
        time = np.sort(rng.choice(np.arange(-200, 40), ncol, replace=False)).astype(F) * F(900) + F(rng.choice([0, 0, 0.5, 7]))
        obs = rng.lognormal(1.0, 1.5, ncol).astype(F)
        obs[rng.random(ncol) < (0.9 if mode == 1 else 0.3)] = np.nan
        if mode == 2:
            obs[:] = np.nan
        if mode == 6:
            obs[rng.random(ncol) < 0.3] = F(-rng.lognormal(0, 1))
        area = F(rng.lognormal(0, 1.5))
        oe = F(rng.uniform(100, 400))
        maxd = F(oe + rng.uniform(1, 30))
        h0 = F(oe + rng.uniform(-0.5, 1.05) * (maxd - oe)) if mode != 7 else F(oe + rng.uniform(0, 1e-4))
        rp = F(rng.choice([300, 300, 60, 3600]))
        step = int(rng.integers(1, 600))
        now = F(rp) * F(step)
        ut = F(now + F(rng.choice([-7200, -900, 0, 900, 3600]))) if mode != 3 else F(now + F(900))
        put = F(now + F(rng.choice([-3600, 0, 3600, 86400]))) if mode != 3 else F(now - F(rng.choice([0, 300])))
        idx = F(rng.integers(0, 15))
        prev = F(rng.lognormal(1.0, 1.5)) if rng.random() > 0.15 else F(np.nan)
        if mode == 6 and rng.random() < 0.5:
            prev = F(-rng.lognormal(0, 1))
        lp = F(rng.lognormal(0.5, 1.5))
        inflow = F(rng.lognormal(1.0, 2.0)) if mode != 7 else F(rng.normal(0, 2.0))
        if mode == 5:                                  # a pool near its maximum with a large inflow
            h0 = F(maxd - F(rng.uniform(0, 0.01)))
            inflow = F(rng.lognormal(5.0, 1.0))
            area = F(rng.lognormal(-3, 1))
        x = np.array([now, prev, put, idx, lp, inflow, rp, area, maxd, oe, h0, ut], F)
        del seen[:]
        out = call_hybrid(hyb, obs, time, x)
        for k in hybrid_branches(obs, time, x, out):
            counts[k] += 1
        msgs = " ".join(seen)
        counts["storage_negative_outflow"] += "negative outflow" in msgs
        counts["storage_max_reached"] += "maximum storage exceedance" in msgs
        counts["storage_deficit"] += "storage deficit" in msgs
        # (the final clamp and the override leave no message: seen from the values)
        counts["storage_final_clamp"] += bool("storage deficit" in msgs and inflow < 0 and out[0] == 0)
        counts["max_storage_override"] += bool("maximum storage exceedance" in msgs and out[1] < lp and out[0] == lp and inflow != lp)
        H_obs.append(obs), H_time.append(time), H_x.append(x), H_out.append(out)
    # ---- RFC
    R_s, R_x, R_k, R_out, R_idx = [], [], [], [], []
    rc = {k: 0 for k in ("rfc_index_advance", "rfc_expired", "rfc_negative_recovered", "rfc_negative_not_recovered_type4",
                         "rfc_negative_not_recovered_type5", "rfc_not_used")}
    for i in range(n):
        mode = i % 6
        series = rng.lognormal(1.0, 1.5, ncol).astype(F)
        if mode in (2, 3):
            series[rng.random(ncol) < 0.5] = F(-999.0)
        if mode == 3:
            series[:int(rng.integers(2, ncol))] = F(-999.0)
        typ = 4 if rng.random() < 0.5 else 5
        rp = F(rng.choice([300, 300, 60, 3600]))
        now = F(rp) * F(int(rng.integers(1, 600)))
        ut = F(now + F(rng.choice([-3600, 0, 300, 3600])))
        idx = int(rng.integers(0, ncol - 1))
        total = int(rng.integers(max(idx - 2, 1), ncol))
        days = int(rng.integers(1, 12)) if mode != 4 else 0
        use = 1 if mode != 5 else 0
        maxd = F(rng.uniform(100, 400))
        we = F(maxd - rng.uniform(0, 30)) if rng.random() > 0.1 else F(rng.uniform(0, 0.01))
        inflow = F(rng.lognormal(1.0, 2.0))
        if mode == 3 and typ == 5:
            inflow = F(rng.uniform(0, 50))
        x = np.array([now, ut, inflow, we, F(rng.lognormal(0.5, 1.5)), F(we + rng.normal(0, 0.01)), F(rng.lognormal(-1, 1.5)), maxd, rp], F)
        k = np.array([use, idx, total, int(rng.choice([900, 3600])), days, typ], np.int32)
        out, nidx = call_rfc(rfc, series, x, k)
        live = use and float(now) <= days * 86400
        rc["rfc_not_used"] += not use
        rc["rfc_expired"] += bool(use and not live)
        rc["rfc_index_advance"] += bool(live and nidx != idx)
        if live:
            q = float(series[nidx]) if typ == 4 else float(inflow) + float(series[nidx])
            if q < 0:
                fell_back = out[1] == x[5] and out[0] == (x[4] if typ == 4 else x[2])
                rc["rfc_negative_recovered"] += bool(out[0] >= 0 and not fell_back)
                rc[f"rfc_negative_not_recovered_type{typ}"] += bool(fell_back)
        R_s.append(series), R_x.append(x), R_k.append(k), R_out.append(out), R_idx.append(nidx)
    counts.update(rc)
    for k, v in counts.items():
        assert v > 0, f"branch {k} not covered"
    names = sorted(counts)
    np.savez_compressed(os.path.join(HERE, "reservoir_da_vectors.npz"),
                        hybrid_obs=np.array(H_obs), hybrid_time=np.array(H_time), hybrid_in=np.array(H_x), hybrid_out=np.array(H_out),
                        rfc_series=np.array(R_s), rfc_in=np.array(R_x), rfc_iin=np.array(R_k), rfc_out=np.array(R_out),
                        rfc_idx=np.array(R_idx, np.int32), branch_names=np.array(names), branch_counts=np.array([counts[k] for k in names]))
    print("vectors:", counts)


# ------------------------------------------------------------------------------------------------- 2. network golden
def da_tables(lakes, index_types, rng):
    """reservoir types of the subset's lakes and the tables of a window as compute_nhd_routing_v02 hands them over"""
    lakes = [int(l) for l in lakes]
    types = np.array([index_types[l] for l in lakes], np.int32)
    ones = [k for k, t in enumerate(types) if t == 1]
    fours = [k for k, t in enumerate(types) if t == 4]
    usgs, usace = [ones[1], ones[5]], [ones[8], ones[11]]
    types[usgs], types[usace], types[fours[3]] = 2, 3, 5
    tab = {}
    for name, rows in (("usgs", usgs), ("usace", usace)):
        time = (np.arange(-72 * 4, 24 * 4 + 1) * 900).astype(F)       # 72 h before the window to its end, every 15 minutes
        obs = rng.lognormal(1.5, 1.0, (len(rows), time.size)).astype(F)
        obs[rng.random(obs.shape) < 0.4] = np.nan
        obs[1, (time > -50 * 3600) & (time <= 3 * 3600)] = np.nan         # nothing inside 48 h of lookback until hour 3
        obs[1, : 20] = F(2.5)
        obs[0, (time > 4 * 3600) & (time < 6 * 3600)] = np.nan
        tab[name] = dict(obs=obs, idx=np.array([lakes[k] for k in rows], np.int32), time=time,
                         update_time=np.array([0, 900], F), prev=np.array([np.nan, 3.25], F),
                         put=np.array([1800, 4 * 3600], F), index=np.array([0, 11], F))
    rows = fours                                                      # (the type-5 lake included: looked up like type 4)
    ncol = 40
    series = rng.lognormal(1.0, 1.0, (len(rows), ncol)).astype(F)
    series[rng.random(series.shape) < 0.15] = F(-999.0)
    series[2, :12] = F(-999.0)                                         # nothing to recover for a while
    tab["rfc"] = dict(obs=series, idx=np.array([lakes[k] for k in rows], np.int32), total=np.full(len(rows), ncol - 1, np.int32),
                      use=np.array([1] * (len(rows) - 1) + [0], np.int32), ts_idx=np.full(len(rows), 3, np.int32),
                      update_time=np.full(len(rows), 1800, F), da_dt=np.full(len(rows), 3600, np.int32),
                      days=np.array([11] * (len(rows) - 2) + [0, 11], np.int32))
    return types, tab


def python_loop(hyb, rfc, O, nts, qts, rl, ul, params9, q0, ql, short, res_of_reach, par, h_init, dt, types, lakes, tab, qd0=None):
    """mc_reach.pyx:492-750 (no nudging): fvd [nseg, nts + 1, 3], inflow [nres, nts + 1], final elevations; `tab` is updated
    in place as the loop updates its state arrays.  types None: level pool only."""
    nseg = params9.shape[0]
    fvd = np.zeros((nseg, nts + 1, 3), F)
    for r in rl:
        fvd[r, 0] = q0[r]
    Hs = np.array(h_init, F).copy()
    inflow_out = np.zeros((len(Hs), nts + 1), F)
    dt32 = F(dt)
    pos = {}
    if types is not None:
        for name in ("usgs", "usace", "rfc"):
            pos[name] = {int(l): i for i, l in enumerate(tab[name]["idx"])}
    for t in range(1, nts + 1):
        now = float(dt32 * F(t))
        for ri, (rows, ups) in enumerate(zip(rl, ul)):
            up_c, up_p = F(0), F(0)
            for u in ups:
                up_c = F(up_c + fvd[u, t, 0])
                up_p = F(up_p + fvd[u, t - 1, 0])
            if short:
                up_c = up_p
            k = res_of_reach[ri]
            if k >= 0:
                i = rows[0]
                h_before = Hs[k]
                q, h = O.levelpool(up_c, dt, Hs[k], par[k])
                typ = 1 if types is None else int(types[k])
                if typ in (2, 3):
                    T = tab["usgs" if typ == 2 else "usace"]
                    j = pos["usgs" if typ == 2 else "usace"][int(lakes[k])]
                    a = par[k]
                    x = np.array([now, T["prev"][j], T["put"][j], T["index"][j], q, up_c, dt32, a[0], a[1], a[4], h_before,
                                  T["update_time"][j]], F)
                    o = call_hybrid(hyb, T["obs"][j], T["time"], x)
                    q, h = o[0], o[2]
                    T["prev"][j], T["update_time"][j], T["index"][j], T["put"][j] = o[1], o[3], o[4], o[5]
                elif typ in (4, 5):
                    T = tab["rfc"]
                    j = pos["rfc"][int(lakes[k])]
                    a = par[k]
                    x = np.array([now, T["update_time"][j], up_c, h_before, q, h, a[0], a[1], dt32], F)
                    kk = np.array([T["use"][j], T["ts_idx"][j], T["total"][j], T["da_dt"][j], T["days"][j], typ], np.int32)
                    o, nidx = call_rfc(rfc, T["obs"][j], x, kk)
                    q, h = o[0], o[1]
                    T["update_time"][j], T["ts_idx"][j] = o[2], nidx
                Hs[k] = h
                fvd[i, t] = (q, 0, h)
                inflow_out[k, t] = up_c
                continue
            qup, quc = up_p, up_c
            n = len(rows)
            inp = np.zeros((n, 15), F)
            inp[:, 0] = params9[rows, 0]
            inp[:, 3] = fvd[rows, t - 1, 0]
            inp[:, 4] = ql[rows, (t - 1) // qts]
            inp[:, 5:13] = params9[rows, 1:9]
            inp[:, 14] = fvd[rows, t - 1, 2]
            if short:                                    # qup = the row above's flow of the step before, quc = qup
                inp[0, 1] = qup
                inp[1:, 1] = fvd[rows[:-1], t - 1, 0]
                inp[:, 2] = inp[:, 1]
                fvd[rows, t] = O.segments(inp, det=True)[:, :3]
            else:
                for m in range(n):
                    inp[m, 1], inp[m, 2] = qup, quc
                    o = O.segments(inp[m:m + 1], det=True)[0]
                    fvd[rows[m], t] = o[:3]
                    qup, quc = inp[m, 3], o[0]
    return fvd, inflow_out, Hs


def state_tuples(tab, nts, dt):
    """elements [4], [5], [7] of the loop's return (mc_reach.pyx:820-837)"""
    t_end = float(F(nts) * F(dt))
    out = {}
    for name in ("usgs", "usace"):
        T = tab[name]
        out[name] = (T["idx"], T["update_time"] - t_end, T["prev"], T["index"], T["put"] - t_end)
    T = tab["rfc"]
    out["rfc"] = (T["idx"], T["update_time"] - t_end, T["ts_idx"])
    return out


def make_network(hyb, rfc):
    import copy
    import test_reservoirs as TR
    import helpers as Hh
    from oracle import oracle as O
    from troute_amd import h5
    lc, ids, dv, ql, q0, reaches, net, lakes, wbody_cols, lakeset, _ = TR.reservoir_case()
    with h5.File(os.path.join(REF, "test/LowerColorado_TX/domain/reservoir_index_AnA.nc")) as f:
        index_types = dict(zip(f.read("lake_id").tolist(), f.read("reservoir_type").tolist()))
        assert not np.isin(f.read("usgs_lake_id"), lakes).any() and not np.isin(f.read("usace_lake_id"), lakes).any()
    row = {int(s): i for i, s in enumerate(ids)}
    rl = [np.array([row[s] for s in rr], dtype=np.int64) for rr in reaches]
    ul = [np.array([row[s] for s in net.get(rr[0], [])], dtype=np.int64) for rr in reaches]
    lake_pos = {int(l): k for k, l in enumerate(lakes)}
    res_of_reach = np.array([lake_pos[rr[0]] if rr[0] in lakeset else -1 for rr in reaches], np.int64)
    a = wbody_cols.astype(F)
    par = np.concatenate([a[:, :8], np.full((len(lakes), 1), 10.0, F)], 1)
    h0 = (a[:, 4] + ((a[:, 1] - a[:, 4]).astype(F) * a[:, 8]).astype(F)).astype(F)
    params9 = dv[:, [Hh.DATA_COLS.index(c) for c in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")]]
    types, tab0 = da_tables(lakes, index_types, np.random.default_rng(5))
    lake_rows = np.array([row[int(l)] for l in lakes])
    # rows downstream of lakes: walk the reaches below every lake until ~300 rows are collected
    below = {}
    for rr, ups in zip(reaches, [net.get(rr[0], []) for rr in reaches]):
        for u in ups:
            below[int(u)] = rr
    down = []
    for l in lakes:                                   # ten rows below every lake (through the reaches, lakes left out)
        rr, took = below.get(int(l)), 0
        while rr is not None and took < 10:
            if rr[0] not in lakeset:
                down.extend(row[s] for s in rr[:10 - took])
                took += len(rr[:10 - took])
            rr = below.get(int(rr[-1]))
    full_rows = np.unique(np.concatenate([lake_rows, np.array(down, np.int64)]))
    out = dict(types=types, lakes=np.asarray(lakes, np.int64), full_rows=full_rows, nts=NTS)
    for name in ("usgs", "usace", "rfc"):
        for k, v in tab0[name].items():
            out[f"{name}_{k}"] = v
    for short in (True, False):
        tag = "short" if short else "general"
        # the restated loop proves itself: level pool only == the oracle's C loop
        res = dict(res_of_reach=res_of_reach, par=par, water_elevation=h0.copy(), routing_period=lc.dt)
        want = O.network(24, lc.qts, rl, ul, params9, q0.copy(), ql, short, det=True, res=res)
        got, inflow, Hs = python_loop(hyb, rfc, O, 24, lc.qts, rl, ul, params9, q0, ql, short, res_of_reach, par, h0, lc.dt, None, lakes, None)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "restated loop != oracle.network"
        assert np.array_equal(inflow[:, 1:].view(np.uint32), res["inflow"][:, 1:].view(np.uint32)) and np.array_equal(Hs, res["water_elevation"])
        for label, nts in (("long", NTS),):
            tab = copy.deepcopy(tab0)
            fvd, inflow, Hs = python_loop(hyb, rfc, O, nts, lc.qts, rl, ul, params9, q0, ql, short, res_of_reach, par, h0, lc.dt, types, lakes, tab)
            st = state_tuples(tab, nts, lc.dt)
            key = f"{tag}_{label}"
            out[f"{key}_full"] = fvd[full_rows, 1:]
            out[f"{key}_dec"] = fvd[:, 12::12]
            out[f"{key}_inflow"] = inflow[:, 1:]
            for name in ("usgs", "usace", "rfc"):
                for j, v in enumerate(st[name]):
                    out[f"{key}_state_{name}_{j}"] = np.asarray(v)
            if label == "long":
                lp = python_loop(hyb, rfc, O, 24, lc.qts, rl, ul, params9, q0, ql, short, res_of_reach, par, h0, lc.dt, None, lakes, None)[0]
                da24 = fvd[lake_rows, 1:25, 0]
                assert not np.array_equal(da24, lp[lake_rows, 1:, 0]), "data assimilation changed nothing"
            print(key, "done; lake outflow range", float(fvd[lake_rows, 1:, 0].min()), float(fvd[lake_rows, 1:, 0].max()))
    # (two files, so that each stays under the size a committed file may have: the general mode's results in one of their own)
    general = {k: out.pop(k) for k in list(out) if k.startswith("general_")}
    np.savez_compressed(os.path.join(HERE, "reservoir_da_network.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "reservoir_da_network_general.npz"), **general)


# ------------------------------------------------------------------------------------------------- 3. drop-in helper
def prep_cases():
    """small DataFrames for _prep_reservoir_da_dataframes: (name, kwargs) -- rebuilt by the test"""
    import pandas as pd
    t0 = pd.Timestamp("2021-08-23 13:00:00")
    cols = [t0 + pd.Timedelta(minutes=15 * k) for k in range(-3, 3)]
    e = pd.DataFrame()

    def types():
        return pd.DataFrame({"reservoir_type": [1, 2, 3, 4, 2, 5, 4]}, index=[10, 20, 30, 40, 50, 60, 70])
    usgs = pd.DataFrame(np.arange(18, dtype=float).reshape(3, 6), index=[50, 20, 99], columns=cols)
    usgs_p = pd.DataFrame({"update_time": [0.0, 900.0, 5.0], "prev_persisted_outflow": [1.5, np.nan, 2.0],
                           "persistence_update_time": [0.0, 3600.0, 1.0], "persistence_index": [0.0, 3.0, 1.0]}, index=[50, 20, 99])
    usace = pd.DataFrame(np.arange(6, dtype=float).reshape(1, 6) + 100, index=[30], columns=cols)
    usace_p = pd.DataFrame({"update_time": [300.0], "prev_persisted_outflow": [7.0], "persistence_update_time": [600.0],
                            "persistence_index": [2.0]}, index=[30])
    rfc = pd.DataFrame(np.arange(8, dtype=float).reshape(2, 4), index=[70, 40])
    rfc_p = pd.DataFrame({"totalCounts": [4, 4], "file": ["a", "b"], "use_rfc": [1, 0], "timeseries_idx": [1, 2],
                          "update_time": [1800.0, 0.0], "da_timestep": [3600, 3600], "rfc_persist_days": [11, 5]}, index=[70, 40])
    full = dict(reservoir_usgs_df=usgs, reservoir_usgs_param_df=usgs_p, reservoir_usace_df=usace, reservoir_usace_param_df=usace_p,
                reservoir_rfc_df=rfc, reservoir_rfc_param_df=rfc_p, t0=t0)
    none = dict(reservoir_usgs_df=e, reservoir_usgs_param_df=e, reservoir_usace_df=e, reservoir_usace_param_df=e,
                reservoir_rfc_df=e, reservoir_rfc_param_df=e, t0=t0)
    return [
        ("all_tables", dict(full, waterbody_types_df_sub=types(), from_files=False)),
        ("no_tables_from_files", dict(none, waterbody_types_df_sub=types(), from_files=True)),
        ("no_tables_not_from_files", dict(none, waterbody_types_df_sub=types(), from_files=False)),
        ("usgs_only", dict(none, reservoir_usgs_df=usgs, reservoir_usgs_param_df=usgs_p, waterbody_types_df_sub=types(), from_files=False)),
        ("exclude", dict(full, waterbody_types_df_sub=types(), from_files=False, exclude_segments=[50])),
    ]


def flatten_prep(ret):
    """the helper's returns without the Great Lakes ones (positions 20..25), as arrays"""
    out = {}
    for j in list(range(20)) + [26]:
        v = ret[j]
        if hasattr(v, "index") and hasattr(v, "values"):
            out[f"r{j}_index"] = np.asarray(v.index.values, dtype=np.int64)
            out[f"r{j}_values"] = np.asarray(v.values, dtype=np.float64)
        elif isinstance(v, list):
            out[f"r{j}_list"] = np.asarray(v, dtype="U8")
        else:
            out[f"r{j}_values"] = np.asarray(v, dtype=np.float64)
    return out


def make_prep():
    import pandas as pd
    fn = reference_prep()
    e = pd.DataFrame()
    out = {}
    for name, kw in prep_cases():
        ret = fn(kw["reservoir_usgs_df"], kw["reservoir_usgs_param_df"], kw["reservoir_usace_df"], kw["reservoir_usace_param_df"],
                 kw["reservoir_rfc_df"], kw["reservoir_rfc_param_df"], e, e, e, kw["waterbody_types_df_sub"], kw["t0"],
                 kw["from_files"], kw.get("exclude_segments"))
        for k, v in flatten_prep(ret).items():
            out[f"{name}__{k}"] = v
    np.savez_compressed(os.path.join(HERE, "reservoir_da_prep.npz"), **out)
    print("prep:", len(out), "arrays")


if __name__ == "__main__":
    what = sys.argv[1:] or ["vectors", "prep", "network"]
    hyb, rfc = reference_functions()
    if "vectors" in what:
        make_vectors(hyb, rfc)
    if "prep" in what:
        make_prep()
    if "network" in what:
        make_network(hyb, rfc)
