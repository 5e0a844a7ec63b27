"""THE DROP-IN OVER CONSECUTIVE RUN SETS: compute_nhd_routing_v02 called once per run set with the same caller objects, as the
reference's loop calls it (nwm_routing/__main__.py:195-333, troute_model.py:274-296).  Between two calls the loop makes a new q0
from the results (AbstractNetwork.new_q0, AbstractNetwork.py:177-191), writes it into the same waterbodies_df in place
(update_waterbody_water_elevation, :198), makes a new lastobs_df (new_lastobs, DataAssimilation.py:1506-1550), rebuilds the
reservoir *_param_df frames from the returned state tuples (_set_persistence_reservoir_da_params, DataAssimilation.py:1321-1372;
_set_rfc_reservoir_da_params, :1374-1398) and advances t0 (new_t0, AbstractNetwork.py:200-204) -- restated in run_sets below.

What lies across that loop and keeps things from call to call: _NETWORKS (routing/compute.py), _FlatCache, _PlanCache and its
plan_token shortcut (routing/fast_reach/mc_reach.py), and the plan's row order tuned from the callable's first window.

The reference of every comparison is the oracle's restatement of the reference loop (oracle.network with its level pool and its
simple_da), routed run set by run set with the state handed on, or the recorded long window of the reference loop with reservoir
data assimilation (tests/golden/reservoir_da_network.npz): float32, bit for bit.  Domain: LowerColorado collapsed at its
waterbodies, forcing x 40 (the pools move), 3 run sets of 24 steps."""
import functools

import numpy as np
import pandas as pd
import pytest

import helpers as H
import test_dropin_run_sets_cpu as RS
import test_gpu_stream_reservoir_da as SD
import test_reservoir_da_network as DN
import test_shipped_config as SC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NTS, NSETS = 24, 3
SCALE = [1.0, 0.5, 1.7]                      # every run set has its own forcing
DECAY = 120.0
T0 = pd.Timestamp("2021-08-23 13:00:00")
GAGES_OUT = 3                                # gages observed in run set 1 only: run set 2 decays what run set 1 left
EMPTY = pd.DataFrame()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def frames(gaged=False):
    """the caller's objects of a loop: the lakes-only case of test_dropin_run_sets_cpu, or the shipped configuration's (reaches
    split at the gages as well, tests/test_shipped_config.py) with every run set's observations"""
    if not gaged:
        f = RS.lake_frames(NTS)
    else:
        f = dict(SC.shipped_case(NTS))
        ids, is_lake = f["ids"], f["is_lake"]
        f["param_df"] = pd.DataFrame(f["dv"][~is_lake], index=ids[~is_lake], columns=list(f["lc"].data_cols)).drop(columns=["dt"])
        f["q0_df"] = pd.DataFrame(f["q0"][~is_lake], index=ids[~is_lake], columns=["qu0", "qd0", "h0"])
        f["wb_df"] = pd.DataFrame(f["wbody_cols"], index=f["lakes"], columns=RS.WB_COLS)
        u = SC.GAGES["usgs"]
        sets = [u[:, s * NTS:(s + 1) * NTS + 1].copy() for s in range(NSETS)]      # column k of a run set = its timestep k
        seen = np.flatnonzero(~np.isnan(sets[0][:, NTS // 2:]).all(axis=1) & ~np.isnan(sets[1][:, 1:]).all(axis=1))
        f["out"] = seen[:: max(1, len(seen) // GAGES_OUT)][:GAGES_OUT]
        for later in sets[1:]:
            later[f["out"]] = np.nan
        f["usgs"] = sets
        f["lastobs_df"] = pd.DataFrame({"time_since_lastobs": SC.GAGES["time_since_lastobs"],
                                        "lastobs_discharge": SC.GAGES["lastobs_discharge"]}, index=f["gage_ids"])
    lc, ids = f["lc"], f["ids"]
    assert lc.qlat.shape[1] * lc.qts >= NSETS * NTS and NTS % lc.qts == 0
    nq = NTS // lc.qts
    f["forcing"] = [np.ascontiguousarray(f["ql"][:, s * nq:(s + 1) * nq] * np.float32(SCALE[s])).astype(np.float32) for s in range(NSETS)]
    # the oracle's view of the table: reaches and their upstreams as rows, the reservoir of every reach, level-pool parameters
    row = {int(s): i for i, s in enumerate(ids)}
    f["rl"] = [np.array([row[s] for s in rr], dtype=np.int64) for rr in f["reaches"]]
    f["ul"] = [np.array([row[s] for s in f["net"].get(rr[0], [])], dtype=np.int64) for rr in f["reaches"]]
    lake_pos = {int(l): k for k, l in enumerate(f["lakes"])}
    f["res_of_reach"] = np.array([lake_pos[rr[0]] if rr[0] in f["lakeset"] else -1 for rr in f["reaches"]], np.int64)
    a = f["wbody_cols"].astype(np.float32)
    f["par"] = np.concatenate([a[:, :8], np.full((len(f["lakes"]), 1), 10.0, np.float32)], 1)
    f["h_cold"] = (a[:, 4] + ((a[:, 1] - a[:, 4]).astype(np.float32) * a[:, 8]).astype(np.float32)).astype(np.float32)
    f["params9"] = f["dv"][:, [H.DATA_COLS.index(k) for k in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")]]
    f["lake_rows"] = np.array([row[int(l)] for l in f["lakes"]])
    lake_rows = set(f["lake_rows"].tolist())
    f["below"] = np.array(sorted({int(r[0]) for r, u in zip(f["rl"], f["ul"]) if set(u.tolist()) & lake_rows} - lake_rows), np.int64)
    if gaged:
        reach_of = {r[-1]: i for i, r in enumerate(f["reaches"])}
        f["gage_of_reach"] = np.full(len(f["reaches"]), -1, np.int64)
        for gi, g in enumerate(f["gage_ids"]):
            f["gage_of_reach"][reach_of[g]] = gi
        f["gage_row"] = np.array([row[g] for g in f["gage_ids"]], np.int64)
    return f


# ---- the reference's loop through the drop-in ------------------------------------------------------------------------------------
def new_lastobs(results, time_increment):
    """DataAssimilation.py:1506-1550: the gage tuple of every network -> next run set's lastobs_df, times counted from its start"""
    df = pd.concat([pd.DataFrame(np.array([r[3][1], r[3][2]]).T, index=r[3][0], columns=["time_since_lastobs", "lastobs_discharge"])
                    for r in results], copy=False)
    df["time_since_lastobs"] = df["time_since_lastobs"] - time_increment
    return df


def new_persistence_params(results):
    """_set_persistence_reservoir_da_params, DataAssimilation.py:1321-1372: tuples [4] (USGS) and [5] (USACE) -> the two frames"""
    cols = ["update_time", "prev_persisted_outflow", "persistence_update_time", "persistence_index"]
    out = []
    for j in (4, 5):
        df = pd.DataFrame(data=[], index=[], columns=cols)
        for r in results:
            if len(r[j][0]) > 0:
                tmp = pd.DataFrame(data=r[j][1], index=r[j][0], columns=["update_time"])
                tmp["prev_persisted_outflow"] = r[j][2]
                tmp["persistence_update_time"] = r[j][4]
                tmp["persistence_index"] = r[j][3]
                df = tmp if df.empty else pd.concat([df, tmp])
        out.append(df)
    return out


def new_rfc_params(rfc_param_df, results):
    """_set_rfc_reservoir_da_params, DataAssimilation.py:1374-1398: tuple [7] written into the caller's frame"""
    for r in results:
        if len(r[7][0]) > 0:
            rfc_param_df.loc[r[7][0], "update_time"] = r[7][1]
            rfc_param_df.loc[r[7][0], "timeseries_idx"] = r[7][2]
    return rfc_param_df


def run_sets(f, nsets, short, gaged=False, reservoir_da=None, types_df=None, forcing=None, after_call=None):
    """``nsets`` consecutive calls of compute_nhd_routing_v02 as the reference's loop makes them: the same conn, rconn,
    reaches_bytw, independent_networks, param_df, waterbodies_df and waterbody_types_df objects on every call; q0, lastobs_df and
    the reservoir *_param_df frames from the call before; waterbodies_df updated in place; t0 moved on by nts * dt.
    reservoir_da: None or a dict of the six reservoir frames (the *_p ones are the first run set's; copies are carried on).
    Returns [(the network's result tuple, new_q0 of the results)] per run set."""
    from troute_amd.routing.compute import compute_nhd_routing_v02, new_q0
    lc, ids, is_lake = f["lc"], f["ids"], f["is_lake"]
    forcing = f["forcing"] if forcing is None else forcing
    wb_df = f["wb_df"].copy()                         # (this loop's own: one object for all of its calls)
    types_df = EMPTY if types_df is None else types_df
    q0_df, t0 = f["q0_df"], T0
    lastobs_df = f["lastobs_df"] if gaged else EMPTY
    da = dict(reservoir_da) if reservoir_da else dict(usgs=EMPTY, usgs_p=EMPTY, usace=EMPTY, usace_p=EMPTY, rfc=EMPTY, rfc_p=EMPTY)
    if reservoir_da:
        da["rfc_p"] = da["rfc_p"].copy()
    out = []
    for s in range(nsets):
        ql_df = pd.DataFrame(forcing[s][~is_lake], index=ids[~is_lake])
        usgs_df = pd.DataFrame(f["usgs"][s], index=f["gage_ids"]) if gaged else EMPTY
        results = compute_nhd_routing_v02(
            f["conn_wb"], f["rconn"], f["wbody_map"], f["reaches_bytw"], "V02-structured", "by-network", 10000, 4, t0, lc.dt, NTS,
            lc.qts, f["ind"], f["param_df"], q0_df, ql_df, usgs_df, lastobs_df, da["usgs"], da["usgs_p"], da["usace"], da["usace_p"],
            da["rfc"], da["rfc_p"], EMPTY, EMPTY, EMPTY, {"da_decay_coefficient": DECAY} if gaged else {}, short, False, wb_df, {},
            types_df, reservoir_da is not None, [{}, {}], from_files=False)[0]
        assert len(results) == 1 and np.array_equal(results[0][0], ids)
        if after_call is not None:
            after_call(s)
        q0_df = new_q0(results)                                             # AbstractNetwork.py:177-191
        before = wb_df
        wb_df.update(q0_df)                                                 # AbstractNetwork.py:198
        assert wb_df is before
        if gaged:
            lastobs_df = new_lastobs(results, NTS * lc.dt)
        if reservoir_da:
            da["usgs_p"], da["usace_p"] = new_persistence_params(results)
            da["rfc_p"] = new_rfc_params(da["rfc_p"], results)
        t0 = t0 + pd.Timedelta(seconds=lc.dt * NTS)                         # AbstractNetwork.py:200-204
        out.append((results[0], q0_df))
    return out


# ---- the same loop in the oracle -------------------------------------------------------------------------------------------------
def oracle_set(f, s, short, state, h, lastobs=None):
    """one run set of the oracle from (state [n, 3], pool elevations h[, (lastobs_time, lastobs_val)])"""
    lc = f["lc"]
    res = dict(res_of_reach=f["res_of_reach"], par=f["par"], water_elevation=h, routing_period=lc.dt)
    da = None
    q0 = np.array(state, dtype=np.float32, copy=True)
    if lastobs is not None:
        da = dict(usgs_values=f["usgs"][s], gage_row=f["gage_row"], gage_of_reach=f["gage_of_reach"], decay_coeff=DECAY,
                  routing_period=lc.dt, lastobs_time=lastobs[0], lastobs_val=lastobs[1])
        first = f["usgs"][s][:, 0]                        # initial flow <- first observation (mc_reach.pyx:404-411)
        ok = ~np.isnan(first)
        q0[f["gage_row"][ok], 0] = first[ok]
    want = O.network(NTS, lc.qts, f["rl"], f["ul"], f["params9"], q0, f["forcing"][s], short, det=True, da=da, res=res)
    w = np.ascontiguousarray(want[:, 1:, :])
    assert np.array_equal(bits(w[f["lake_rows"], -1, 2]), bits(res["water_elevation"]))
    o = dict(fvd=w, inflow=res["inflow"][:, 1:].copy(), h=res["water_elevation"].copy(),
             state=np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], axis=1))
    if da is not None:
        o.update(nudge=da["nudge"].copy(), lastobs_time=da["lastobs_time"].copy(), lastobs_val=da["lastobs_val"].copy(),
                 lastobs_in=(np.asarray(lastobs[0], np.float32), np.asarray(lastobs[1], np.float32)))
    return o


@functools.lru_cache(maxsize=None)
def oracle_sets(short, gaged=False):
    """the chained oracle: run set s starts from run set s-1's new_q0, its final pool elevations and its last observations with
    their times counted from the new start"""
    f = frames(gaged)
    state, h = f["q0"], f["h_cold"]
    lastobs = (SC.GAGES["time_since_lastobs"], SC.GAGES["lastobs_discharge"]) if gaged else None
    out = []
    for s in range(NSETS):
        o = oracle_set(f, s, short, state, h, lastobs)
        out.append(o)
        state, h = o["state"], o["h"]
        if gaged:
            lastobs = ((o["lastobs_time"] - np.float32(NTS * f["lc"].dt)).astype(np.float32), o["lastobs_val"])
    return out


def assert_sets_equal_oracle(got, want, f, what):
    n = len(f["ids"])
    assert len(got) == len(want)
    for s, ((r, q0_df), w) in enumerate(zip(got, want)):
        fvd = r[1].reshape(n, NTS, 3)
        for rows, where in ((f["lake_rows"], "lakes"), (f["below"], "below the lakes"), (np.arange(n), "every row")):
            assert np.array_equal(bits(fvd[rows]), bits(w["fvd"][rows])), (what, s, where)
        assert np.array_equal(bits(r[6][f["lake_rows"]]), bits(w["inflow"])), (what, s, "upstream rows of the lakes")
        assert np.array_equal(q0_df.index.values, f["ids"]) and list(q0_df.columns) == ["qu0", "qd0", "h0"]
        assert np.array_equal(bits(q0_df.values.astype(np.float32, copy=False)), bits(w["state"])) and q0_df.values.dtype == np.float32, (what, s, "new_q0")
        if "nudge" in w:
            assert np.array_equal(r[3][0], np.array(f["gage_ids"])), (what, s)
            assert np.array_equal(bits(r[8]), bits(w["nudge"])), (what, s, "nudge")
            assert np.array_equal(bits(r[3][1]), bits(w["lastobs_time"])), (what, s, "lastobs times")
            assert np.array_equal(bits(r[3][2]), bits(w["lastobs_val"])), (what, s, "lastobs values")


def assert_lakes_case_is_not_vacuous(f, want, short):
    """on the oracle alone: the pools move in run set 1, and a run set 2 whose pools restart from run set 1's STARTING outflow and
    elevation (what a frozen copy of the waterbody table gives) is another result at the lakes and below them"""
    assert (want[0]["h"] != f["h_cold"]).any()
    stale_state = want[0]["state"].copy()
    stale_state[f["lake_rows"], 0] = 0.0                 # qd0 of the first run set's table
    stale = oracle_set(f, 1, short, stale_state, f["h_cold"])
    differs = (bits(stale["fvd"]) != bits(want[1]["fvd"])).reshape(len(f["ids"]), -1).any(axis=1)
    assert differs[f["lake_rows"]].any() and f["below"].size and differs[f["below"]].any()
    assert np.abs(want[1]["fvd"][f["lake_rows"], :, 0]).max() > 0


# ---- 1. level-pool lakes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [True, False])
def test_lakes_three_run_sets_against_the_oracle(short):
    f = frames()
    want = oracle_sets(short)
    assert_lakes_case_is_not_vacuous(f, want, short)
    assert_sets_equal_oracle(run_sets(f, NSETS, short), want, f, "lakes")


# ---- 2. the caches change nothing ------------------------------------------------------------------------------------------------
def test_lakes_three_run_sets_without_the_call_and_flat_caches(monkeypatch):
    f = frames()
    want = oracle_sets(True)
    assert_lakes_case_is_not_vacuous(f, want, True)
    cached = run_sets(f, NSETS, True)
    monkeypatch.setenv("TRMC_CALL_CACHE", "0")
    monkeypatch.setenv("TRMC_FLAT_CACHE", "0")
    plain = run_sets(f, NSETS, True)
    assert_sets_equal_oracle(cached, want, f, "caches on")
    assert_sets_equal_oracle(plain, want, f, "caches off")
    for s, ((a, qa), (b, qb)) in enumerate(zip(cached, plain)):
        for j in (1, 6):
            assert a[j].dtype == b[j].dtype and np.array_equal(bits(a[j]), bits(b[j])), (s, j)
        assert np.array_equal(bits(qa.values), bits(qb.values)), s


# ---- 3. lakes and nudged gages together ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [True, False])
def test_lakes_and_gages_three_run_sets_against_the_oracle(short):
    f = frames(True)
    want = oracle_sets(short, True)
    # on the oracle's inputs: gages that are observed in run set 1, bring nothing in run set 2 and decay run set 1's last one
    out = f["out"]
    assert out.size == GAGES_OUT
    for g in out:
        last = np.flatnonzero(~np.isnan(f["usgs"][0][g, :NTS + 1]))[-1]
        assert last >= NTS // 2 and np.isnan(f["usgs"][1][g]).all() and np.isnan(f["usgs"][2][g]).all()
        lt, lv = want[1]["lastobs_in"][0][g], want[1]["lastobs_in"][1][g]
        assert lv == f["usgs"][0][g, last] and lt == np.float32(last * f["lc"].dt) - np.float32(NTS * f["lc"].dt) and lt <= 0
        assert (want[1]["nudge"][g, 1:] != 0).all() and want[1]["lastobs_val"][g] == lv
    others = np.setdiff1d(np.arange(len(f["gage_ids"])), out)
    assert np.count_nonzero(~np.isnan(f["usgs"][1][others, 1:]).all(axis=1)) > 40      # (the rest is observed in run set 2 as well)
    assert (want[0]["h"] != f["h_cold"]).any() and all(np.abs(w["nudge"]).max() > 0 for w in want)
    assert_sets_equal_oracle(run_sets(f, NSETS, short, gaged=True), want, f, "lakes and gages")


# ---- 4. reservoir types 2-5: the recorded long window of the reference loop as three run sets --------------------------------------
def reservoir_da_frames():
    """the fixture's tables as the frames the reference's loop holds before its first run set (tests/test_reservoir_da_prep.py)"""
    g = DN.NET
    da = {}
    for name in ("usgs", "usace"):
        stamps = [T0 + pd.Timedelta(seconds=float(s)) for s in g[f"{name}_time"]]
        idx = g[f"{name}_idx"].astype(np.int64)
        da[name] = pd.DataFrame(g[f"{name}_obs"], index=idx, columns=stamps)
        da[name + "_p"] = pd.DataFrame({"update_time": g[f"{name}_update_time"], "prev_persisted_outflow": g[f"{name}_prev"],
                                        "persistence_update_time": g[f"{name}_put"], "persistence_index": g[f"{name}_index"]}, index=idx)
    idx = g["rfc_idx"].astype(np.int64)
    da["rfc"] = pd.DataFrame(g["rfc_obs"], index=idx)
    da["rfc_p"] = pd.DataFrame({"totalCounts": g["rfc_total"], "file": [""] * len(idx), "use_rfc": g["rfc_use"],
                                "timeseries_idx": g["rfc_ts_idx"], "update_time": g["rfc_update_time"], "da_timestep": g["rfc_da_dt"],
                                "rfc_persist_days": g["rfc_days"]}, index=idx)
    return da


def test_reservoir_types_2_to_5_three_run_sets_equal_the_reference_long_window():
    assert NSETS * NTS == DN.NTS and (SD.NDAYS, SD.NSTEPS) == (NSETS, NTS)
    c = SD.case()
    f = frames()
    assert np.array_equal(c.ids, f["ids"]) and np.array_equal(DN.NET["lakes"], f["lakes"])
    assert set(DN.NET["types"].tolist()) == {1, 2, 3, 4, 5}
    types_df = pd.DataFrame({"reservoir_type": DN.NET["types"].astype(np.int64)}, index=f["lakes"])
    before = types_df.copy()
    got = run_sets(f, NSETS, True, reservoir_da=reservoir_da_frames(), types_df=types_df, forcing=c.days)
    assert types_df.equals(before)                                         # (the caller's types are not demoted behind its back)
    for s, (r, _) in enumerate(got):
        DN.check_against_golden(r, True, s * NTS, (s + 1) * NTS)            # flows, depths and pool elevations, the lakes' inflows
        for j in (4, 5, 7):
            assert len(r[j][0]) > 0
    DN.check_state(got[-1][0], True)
    moved = [np.concatenate([np.asarray(a, np.float64) for a in r[4][1:] + r[5][1:] + r[7][1:]]) for r, _ in got]
    assert not np.array_equal(moved[0], moved[-1], equal_nan=True)          # (the state does move from run set to run set)


# ---- 5. a plan that has been tuned in between ------------------------------------------------------------------------------------
def test_lakes_three_run_sets_on_a_plan_tuned_in_between(monkeypatch):
    from troute_amd.routing.fast_reach import mc_reach as M
    f = frames()
    want = oracle_sets(True)
    assert_lakes_case_is_not_vacuous(f, want, True)
    monkeypatch.setenv("TRMC_PLAN_CACHE", "2")
    monkeypatch.delenv("TRMC_RETUNE", raising=False)
    monkeypatch.delenv("TRMC_ENGINE", raising=False)
    M._PLANS.clear()
    seen = []

    def after_call(s):
        (e,) = M._PLANS._d.values()
        seen.append((e["stage"], e["plan"]))                                # (the plan object is held: its id cannot be taken again)
    try:
        got = run_sets(f, NSETS, True, after_call=after_call)
        # untuned while the costs are collected; rebuilt from them in run set 2; that plan, kept by the callable, in run set 3
        assert [s for s, _ in seen] == [1, 2, 2]
        assert seen[1][1] is not seen[0][1] and seen[2][1] is seen[1][1]
        assert seen[2][1].stats()["nsteps"] == NTS
    finally:
        M._PLANS.clear()
    assert_sets_equal_oracle(got, want, f, "tuned plan")
