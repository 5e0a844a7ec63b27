"""LEVEL-POOL RESERVOIRS AND STREAMFLOW NUDGING IN A STREAM OF DAYS (include/trmc.h trmc_stream_set_gages, trmc_stream_push_day;
csrc/stream.inc): the reservoirs' inflow record and the gages' tables live in the day slots of the ring, a row finds its day's
through its slot (StepArgs::slot_res, slot_da), the pools' elevations and the last observations go from day to day, and a gage
row starts a day from the day's first observation where there is one (mc_reach.pyx:404-411; k_stream_first_obs).

The reference is the oracle's restatement of the reference loop with its level pool and its simple_da, every row its own reach
(oracle.network_by_segment(..., res=, da=)), routed day by day with the state, the pools' elevations and the last observations
handed on: fp32, bit for bit.  The oracle restates reservoirs and nudging for float32 only (as the reference has them), so a
precision-64 stream is held against what CAN be said in double precision: every row that no lake and no gage drains into equals
the plain fp64 oracle bit for bit, and everything -- those rows, the lakes, the gages, the rows below them, both records, the
state -- equals the same days routed as single windows on the same plan (set_reservoirs, set_nudging, route_device)."""
import functools

import numpy as np
import pytest

import helpers as H
import test_gpu_ctile_tables as TT
import test_reservoirs as TR
from oracle import oracle as O
from troute_amd import _lib
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, csr_from_lists, topology_clusters, topology_levels
from troute_amd.routing.fast_reach import simple_da as DA
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu

NSTEPS, QTS, K = 24, 8, 4
DT, DECAY = 300.0, 120.0
GMAX = NSTEPS + 4
OPTIONS = {"cluster_rows": 64, "wide_min_rows": 200, "wide_k": K}
DAY_LEN = np.float32(NSTEPS * DT)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class Case:
    pass


def place(to, up_ptr, up_idx, lag, W, rng, n_random_lakes=4, n_random_gages=7):
    """{name: row} of about a dozen lakes and about twenty gages: lakes inside the slices and inside cluster levels, at a headwater,
    directly below another lake, as a tailwater, below a junction of three rows; gages in both parts, one directly above a lake"""
    n = to.shape[0]
    ups = [up_idx[up_ptr[r]:up_ptr[r + 1]] for r in range(n)]
    cl = lag >= W
    taken, lakes, gages = set(), {}, {}

    def pick(into, name, cond):
        for r in range(n):
            if r not in taken and cond(r):
                into[name] = r
                taken.add(r)
                return r
        raise AssertionError(f"no row for {name}")

    pick(lakes, "lake_headwater", lambda r: ups[r].shape[0] == 0 and to[r] >= 0)
    pick(lakes, "lake_slice_junction", lambda r: 0 < lag[r] < W and ups[r].shape[0] == 2 and to[r] >= 0)
    pick(lakes, "lake_slice_deep", lambda r: min(3, W - 1) <= lag[r] < W and ups[r].shape[0] >= 1 and to[r] >= 0)
    pick(lakes, "lake_junction_of_three", lambda r: ups[r].shape[0] >= 3 and to[r] >= 0)
    pick(lakes, "lake_cluster_head", lambda r: cl[r] and ups[r].shape[0] >= 1 and np.all(lag[ups[r]] < lag[r]) and to[r] >= 0)
    a = pick(lakes, "lake_cluster_interior", lambda r: cl[r] and ups[r].shape[0] >= 1 and np.all(lag[ups[r]] == lag[r]) and to[r] >= 0
             and lag[to[r]] == lag[r] and int(to[r]) not in taken)
    lakes["lake_below_lake"] = int(to[a])
    taken.add(int(to[a]))
    pick(lakes, "lake_cluster_deep", lambda r: cl[r] and lag[r] >= W + 1 and ups[r].shape[0] >= 1 and to[r] >= 0)
    pick(lakes, "lake_tailwater", lambda r: cl[r] and to[r] < 0 and ups[r].shape[0] >= 1)
    free = [int(r) for r in rng.permutation(n) if int(r) not in taken and ups[r].shape[0] >= 1]
    for i, r in enumerate(free[:n_random_lakes]):
        lakes[f"lake_random_{i}"] = r
        taken.add(r)
    for name, lake in (("gage_above_slice_lake", "lake_slice_junction"), ("gage_above_cluster_lake", "lake_cluster_head")):
        g = int(ups[lakes[lake]][0])
        assert g not in taken
        gages[name] = g
        taken.add(g)
    for k in range(4):
        pick(gages, f"gage_slice_{k}", lambda r: lag[r] < W and to[r] >= 0)
        pick(gages, f"gage_cluster_{k}", lambda r: cl[r] and lag[r] == W + k % 2 and to[r] >= 0)
    pick(gages, "gage_slice_feeds_cluster", lambda r: lag[r] < W and to[r] >= 0 and cl[to[r]])
    pick(gages, "gage_modes_012", lambda r: cl[r] and to[r] >= 0)
    pick(gages, "gage_day1_decays_day0_slice", lambda r: 0 < lag[r] < W and to[r] >= 0)
    pick(gages, "gage_day1_decays_day0_cluster", lambda r: cl[r] and to[r] >= 0)
    free = [int(r) for r in rng.permutation(n) if int(r) not in taken]
    for i, r in enumerate(free[:n_random_gages]):
        gages[f"gage_random_{i}"] = r
        taken.add(r)
    return lakes, gages


@functools.lru_cache(maxsize=None)
def case(nseg=5000, seed=77, ndays=3):
    """the network and the days of test_gpu_stream.test_stream_against_the_oracle_day_by_day (wetter: the pools must move), with
    lakes, gages and every day's observations"""
    from test_gpu_parity import synth_inputs
    rng = np.random.default_rng(seed)
    c = Case()
    c.n = nseg
    c.to = H.random_network(rng, nseg)
    _, _, ups = H.reaches_from_to(c.to)
    c.up_ptr, c.up_idx = csr_from_lists(ups)
    c.level = topology_levels(c.up_ptr, c.up_idx)[0]
    c.params, qlat, q0 = synth_inputs(rng, nseg, 3)
    qlat = (qlat * np.float32(40.0)).astype(np.float32)
    scale = [1.0, 0.5, 1.7, 0.8, 1.3]
    c.days = [(qlat * np.float32(scale[d % 5])).astype(np.float32) for d in range(ndays)]
    _, lag, _, c.W, c.C, _ = topology_clusters(c.up_ptr, c.up_idx, wide_min_rows=OPTIONS["wide_min_rows"], cluster_rows=OPTIONS["cluster_rows"])
    c.lag = lag
    lakes, gages = place(c.to, c.up_ptr, c.up_idx, lag, c.W, rng)
    c.lake_names, c.gage_names = list(lakes), list(gages)
    c.lakes = np.array([lakes[k] for k in c.lake_names], np.int64)
    c.gages = np.array([gages[k] for k in c.gage_names], np.int64)
    assert not set(c.lakes.tolist()) & set(c.gages.tolist())
    c.par, c.h0 = TT.lake_parameters(c.lakes.shape[0])
    ng = c.gages.shape[0]
    c.usgs = []
    for d in range(ndays):
        u = rng.lognormal(np.log(0.5), 1.0, (ng, GMAX)).astype(np.float32)
        u[rng.random((ng, GMAX)) < 0.3] = np.nan
        c.usgs.append(u)
    c.lv0 = rng.lognormal(np.log(0.5), 1.0, ng).astype(np.float32)
    c.lt0 = (-rng.integers(0, 7200, ng)).astype(np.float32)
    for i, name in enumerate(c.gage_names):
        if name == "gage_modes_012":                      # nothing known, then observations, then decay; silent afterwards
            for u in c.usgs:
                u[i, :] = np.nan
            c.usgs[0][i, 6:11] = rng.lognormal(0, 1, 5).astype(np.float32)
            c.lv0[i] = c.lt0[i] = np.nan
        elif name.startswith("gage_day1_decays_day0"):    # observed on day 0 only: day 1 decays what day 0 left
            c.usgs[0][i, :] = np.nan
            c.usgs[0][i, 3:15] = rng.lognormal(0, 1, 12).astype(np.float32)
            for u in c.usgs[1:]:
                u[i, :] = np.nan
            c.lv0[i] = c.lt0[i] = np.nan
    q0 = q0.copy()
    q0[c.lakes, 2] = c.h0                                 # the pool's elevation lives in the depth slot
    q0[c.lakes, 1] = 0
    c.q0 = q0
    # rows that no lake and no gage drains into (what the plain oracle can speak for)
    touched = np.zeros(nseg, bool)
    touched[c.lakes] = touched[c.gages] = True
    for r in np.argsort(c.level, kind="stable"):
        if touched[r] and c.to[r] >= 0:
            touched[c.to[r]] = True
    c.untouched = ~touched
    return c


def day_tables(c, ndays):
    """[(mode, a, w)] per day and [(lt_fin, lv_fin)] per day, resolved as the drop-in resolves a window's, the last observations
    handed on as between two calls of the window path (times less the day's length)"""
    lv, lt = c.lv0, c.lt0
    tabs, fins = [], []
    for d in range(ndays):
        mode, a, w, lt_fin, lv_fin = DA.resolve_tables(NSTEPS, DT, DECAY, c.usgs[d], lv, lt)
        tabs.append((mode, a, w))
        fins.append((lt_fin, lv_fin))
        lv, lt = lv_fin, (lt_fin - DAY_LEN).astype(np.float32)
    return tabs, fins


@functools.lru_cache(maxsize=None)
def oracle_days(key=(5000, 77, 3)):
    """the oracle day by day (fp32): [(fvd [n, nsteps, 3], inflow [nres, nsteps], nudge [ngage, nsteps], (lt, lv))]"""
    c = case(*key)
    order = np.argsort(c.level, kind="stable")
    res_of_row = np.full(c.n, -1, np.int64)
    res_of_row[c.lakes] = np.arange(c.lakes.shape[0])
    gage_of_row = np.full(c.n, -1, np.int64)
    gage_of_row[c.gages] = np.arange(c.gages.shape[0])
    state, h, lv, lt = c.q0, c.h0, c.lv0, c.lt0
    out = []
    for d, q in enumerate(c.days):
        res = dict(res_of_reach=res_of_row[order], par=c.par, water_elevation=h, routing_period=DT)
        da = dict(usgs_values=c.usgs[d], gage_row=c.gages, gage_of_reach=gage_of_row[order], decay_coeff=DECAY, routing_period=DT,
                  lastobs_time=lt, lastobs_val=lv)
        want = O.network_by_segment(NSTEPS, QTS, c.up_ptr, c.up_idx, c.level, c.params, state, q, True, det=True, res=res, da=da)
        w = np.ascontiguousarray(want[:, 1:])
        assert np.array_equal(bits(w[c.lakes, -1, 2]), bits(res["water_elevation"]))
        out.append((w, res["inflow"][:, 1:].copy(), da["nudge"][:, 1:].copy(), (da["lastobs_time"].copy(), da["lastobs_val"].copy())))
        state = np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], 1)
        h, lv, lt = res["water_elevation"], da["lastobs_val"], (da["lastobs_time"] - DAY_LEN).astype(np.float32)
    return out


def open_plan(c, precision=32, options=None):
    return RoutingPlan(c.up_ptr, c.up_idx, c.params, assume_short_ts=True, engine="levels", precision=precision,
                       options=dict(OPTIONS, **(options or {})))


def stream_days(p, c, tabs, full_output=True, output_stride=0, slots=0):
    """the case's days through a stream at plan level: [(fvd or None, inflow, nudge, final state)] per day"""
    dt = p.dtype
    ndays = len(c.days)
    p.set_reservoirs(c.lakes, c.par, DT)
    p.stream_set_gages(c.gages)
    p.upload_forcing(NSTEPS, c.days[0].astype(dt), c.q0.astype(dt))
    p.stream_begin(NSTEPS, QTS, slots=slots, full_output=full_output, output_stride=output_stride)
    info = p.stream_info()
    D = info["slots"]
    assert D >= slots
    keep = NSTEPS // output_stride if output_stride else NSTEPS
    want_fvd = full_output or output_stride
    ring = [(_lib.result_empty((c.n, keep, 3), dt, always_pinned=True) if want_fvd else None,
             _lib.result_empty((c.lakes.shape[0], NSTEPS), dt, always_pinned=True),
             _lib.result_empty((c.gages.shape[0], NSTEPS), dt, always_pinned=True),
             _lib.result_empty((c.n, 3), dt, always_pinned=True)) for _ in range(D)]
    got = []

    def take(d):
        p.stream_wait(d)
        got.append(tuple(None if x is None else np.array(x, copy=True) for x in ring[d % D]))
    for d in range(ndays):
        if d >= D:                                        # (the slot's last day leaves before its arrays are reused)
            if p.stream_info()["days_complete"] <= d - D:
                p.stream_flush()
            take(d - D)
        fvd, rin, nud, fin = ring[d % D]
        mode, a, w = tabs[d]
        p.stream_push(pinned_like(c.days[d].astype(dt)), fvd=fvd, q0=fin, nudging=(mode, a.astype(dt), w.astype(dt), c.usgs[d][:, 0]),
                      nudge=nud, reservoir_inflow=rin)
    p.stream_flush()
    for d in range(len(got), ndays):
        take(d)
    p.stream_end()
    return got, info


def window_days(p, c, tabs, stride=0):
    """the same days as single windows on the same plan: set_reservoirs, set_nudging, route_device -- the state through the host,
    a gage row's initial flow replaced by the day's first observation as the drop-in does it (mc_reach.pyx:404-411)"""
    dt = p.dtype
    out = []
    p.set_reservoirs(c.lakes, c.par, DT)
    state = c.q0.astype(dt)
    for d, q in enumerate(c.days):
        ok = ~np.isnan(c.usgs[d][:, 0])
        state = state.copy()
        state[c.gages[ok], 0] = c.usgs[d][ok, 0]
        p.upload_forcing(NSTEPS, q.astype(dt), state)
        mode, a, w = tabs[d]
        p.set_nudging(NSTEPS, c.gages, mode, a.astype(dt), w.astype(dt))
        p.route_device(NSTEPS, QTS, True)
        fvd = p.download_fvd()
        state = p.download_final_state()
        out.append((fvd[:, stride - 1::stride].copy() if stride else fvd, p.download_reservoir_inflow(), p.download_nudge(), state))
    return out


def assert_days_equal(got, want, what, fvd=True):
    assert len(got) == len(want)
    for d, (g, w) in enumerate(zip(got, want)):
        for k, name in enumerate(("fvd", "reservoir_inflow", "nudge", "final_state")):
            if k == 0 and not fvd:
                continue
            assert g[k].shape == w[k].shape, (what, d, name)
            bad = np.flatnonzero((bits(g[k]) != bits(w[k])).reshape(g[k].shape[0], -1).any(axis=1))
            assert bad.size == 0, (what, d, name, bad.size, bad[:16].tolist())


# ---- 1. against the oracle, day by day ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_stream_with_lakes_and_gages_against_the_oracle_day_by_day(precision):
    c = case()
    tabs, fins = day_tables(c, 3)
    modes = np.stack([t[0] for t in tabs])               # [day, gage, step]
    for m in (0, 1, 2):
        assert np.count_nonzero(modes == m) > 0, m
    handed = [i for i, name in enumerate(c.gage_names) if name.startswith("gage_day1_decays_day0")]
    n_handed = sum(int(np.isnan(c.usgs[1][i, 1:NSTEPS + 1]).all() and (modes[1, i] == 2).all() and (modes[0, i] == 1).any()
                       and np.isnan(c.lv0[i])) for i in handed)
    assert n_handed > 0
    assert len(c.lake_names) >= 12 and len(c.gage_names) >= 20
    lake = dict(zip(c.lake_names, c.lakes.tolist()))
    gage = dict(zip(c.gage_names, c.gages.tolist()))
    nup = np.diff(c.up_ptr)
    assert nup[lake["lake_headwater"]] == 0 and nup[lake["lake_junction_of_three"]] >= 3 and c.to[lake["lake_tailwater"]] < 0
    assert c.to[lake["lake_cluster_interior"]] == lake["lake_below_lake"] and c.to[gage["gage_above_cluster_lake"]] == lake["lake_cluster_head"]
    assert np.count_nonzero(c.lag[c.lakes] < c.W) >= 3 and np.count_nonzero(c.lag[c.lakes] >= c.W) >= 5
    assert np.count_nonzero(c.lag[c.gages] < c.W) >= 5 and np.count_nonzero(c.lag[c.gages] >= c.W) >= 5
    want = oracle_days()
    with open_plan(c, precision) as p:
        lag, W, C = p.lags()
        assert np.array_equal(lag, c.lag) and (W, C) == (c.W, c.C)
        got, info = stream_days(p, c, tabs)
        assert info["wide_levels"] > 0 and info["cluster_levels"] > 0
        if precision == 64:
            windows = window_days(p, c, tabs)
    # what the oracle alone says about the case: the pools move and spill, the nudges are not zero
    q, h = np.concatenate([w[0][c.lakes, :, 0] for w in want], 1), np.concatenate([w[0][c.lakes, :, 2] for w in want], 1)
    assert np.all(q.max(axis=1) > 0) and np.all((h != c.h0[:, None]).any(axis=1))
    assert np.count_nonzero(np.abs(np.concatenate([w[2] for w in want], 1)).max(axis=1) > 0) >= c.gages.shape[0] - 1
    if precision == 32:
        assert_days_equal(got, [(w[0], w[1], w[2], np.stack([w[0][:, -1, 0], w[0][:, -1, 0], w[0][:, -1, 2]], 1)) for w in want], "oracle")
        for d in range(3):
            assert np.array_equal(bits(fins[d][0]), bits(want[d][3][0])) and np.array_equal(bits(fins[d][1]), bits(want[d][3][1])), d
            assert not got[d][0][c.lakes, :, 1].any()
        return
    # precision 64 (see the module's docstring): the rows no lake or gage drains into against the plain fp64 oracle ...
    assert 0.3 * c.n < np.count_nonzero(c.untouched) < c.n
    state = c.q0.astype(np.float64)
    for d, ql in enumerate(c.days):
        plain = O.network_by_segment(NSTEPS, QTS, c.up_ptr, c.up_idx, c.level, c.params.astype(np.float64), state, ql.astype(np.float64), True)[:, 1:]
        assert np.array_equal(bits(got[d][0][c.untouched]), bits(np.ascontiguousarray(plain[c.untouched]))), d
        state = got[d][3]
    # ... and everything against the same days as single windows
    assert_days_equal(got, windows, "windows-64")


# ---- 2. stream against windows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["full", "products-stride-8", "tolerance"])
def test_stream_with_lakes_and_gages_equals_its_own_windows(variant):
    c = case()
    tabs, _ = day_tables(c, 3)
    stride = 8 if variant == "products-stride-8" else 0
    with open_plan(c, 32, {"arithmetic": "tolerance"} if variant == "tolerance" else None) as p:
        assert p.arithmetic == ("tolerance" if variant == "tolerance" else "exact")
        windows = window_days(p, c, tabs, stride)
        got, info = stream_days(p, c, tabs, full_output=not stride, output_stride=stride)
        assert info["wide_levels"] > 0 and info["cluster_levels"] > 0
    assert_days_equal(got, windows, variant)
    if variant != "tolerance":
        want = oracle_days()
        for d in range(3):
            assert np.array_equal(bits(got[d][1]), bits(want[d][1])) and np.array_equal(bits(got[d][2]), bits(want[d][2])), d


# ---- 3. LowerColorado with its waterbodies -----------------------------------------------------------------------------------
def test_stream_lowercolorado_with_its_waterbodies_two_days():
    lc, ids, dv, ql, q0, reaches, net, lakes, wbody_cols, lakeset, nts = TR.reservoir_case()
    row = {int(s): i for i, s in enumerate(ids)}
    rl = [np.array([row[s] for s in rr], dtype=np.int64) for rr in reaches]
    ul = [np.array([row[s] for s in net.get(rr[0], [])], dtype=np.int64) for rr in reaches]
    res_of_reach = np.full(len(reaches), -1, np.int64)
    lake_pos = {int(l): k for k, l in enumerate(lakes)}
    for i, rr in enumerate(reaches):
        if rr[0] in lakeset:
            res_of_reach[i] = lake_pos[rr[0]]
    a = wbody_cols.astype(np.float32)
    par = np.concatenate([a[:, :8], np.full((len(lakes), 1), 10.0, np.float32)], 1)
    h0 = (a[:, 4] + ((a[:, 1] - a[:, 4]).astype(np.float32) * a[:, 8]).astype(np.float32)).astype(np.float32)
    # (a lake's channel parameters are NaN in the table, as the drop-in hands them to the plan: they are never read)
    params9 = np.ascontiguousarray(dv[:, [H.DATA_COLS.index(k) for k in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")]])
    lake_rows = np.array([row[int(l)] for l in lakes])
    nseg = len(ids)
    ups = [[] for _ in range(nseg)]
    for r, u in zip(rl, ul):
        ups[r[0]] = u.tolist()
        for x, y in zip(r[1:], r[:-1]):
            ups[x] = [int(y)]
    up_ptr, up_idx = csr_from_lists(ups)
    below = np.array(sorted({int(r[0]) for r, u in zip(rl, ul) if set(u.tolist()) & set(lake_rows.tolist())}), np.int64)
    assert below.size >= 1
    state0 = q0.copy()
    state0[lake_rows, 2] = h0
    days = [ql, (ql * np.float32(0.6)).astype(np.float32)]
    with RoutingPlan(up_ptr, up_idx, params9, assume_short_ts=True, engine="levels", options={"cluster_rows": 128}) as p:
        lag, W, C = p.lags()
        assert W == 0 and C > 0
        p.set_reservoirs(lake_rows, par, lc.dt)
        p.upload_forcing(nts, days[0], state0)
        p.stream_begin(nts, lc.qts, full_output=True)
        D = p.stream_info()["slots"]
        assert D >= 2
        outs = [_lib.result_empty((nseg, nts, 3), np.float32, always_pinned=True) for _ in range(2)]
        rins = [_lib.result_empty((len(lakes), nts), np.float32, always_pinned=True) for _ in range(2)]
        for d, q in enumerate(days):
            p.stream_push(pinned_like(q), fvd=outs[d], reservoir_inflow=rins[d])
        p.stream_flush()
        state, h = q0, h0
        for d, q in enumerate(days):
            p.stream_wait(d)
            res = dict(res_of_reach=res_of_reach, par=par, water_elevation=h, routing_period=lc.dt)
            want = np.ascontiguousarray(O.network(nts, lc.qts, rl, ul, params9, state, q, True, det=True, res=res)[:, 1:])
            for rows, what in ((lake_rows, "lakes"), (below, "below the lakes"), (np.arange(nseg), "every row")):
                assert np.array_equal(bits(outs[d][rows]), bits(want[rows])), (d, what)
            assert np.array_equal(bits(rins[d]), bits(res["inflow"][:, 1:])), d
            assert np.array_equal(bits(outs[d][lake_rows, -1, 2]), bits(res["water_elevation"]))
            state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
            h = res["water_elevation"]
        assert np.abs(outs[1][lake_rows, :, 0]).max() > 0
        p.stream_end()


# ---- 4. RouteStream end to end -----------------------------------------------------------------------------------------------
def test_routestream_with_reservoirs_and_gages_end_to_end():
    key = (3000, 78, 4)
    c = case(*key)
    want = oracle_days(key)
    r = ShardedRouter(c.to, c.params, stream=True, options=OPTIONS, reservoirs=(c.lakes, c.par, DT), gages=c.gages)
    got = {}
    with RouteStream(r, NSTEPS, QTS) as rs:
        for item in rs.route(iter(c.days), c.q0, observations=iter(c.usgs), lastobs=(c.lv0, c.lt0),
                             da_parameters={"da_decay_coefficient": DECAY, "routing_period": DT}):
            assert len(item) == 4 and set(item[3]) == {"reservoir_inflow", "nudge", "lastobs"}
            got[item[0]] = (np.array(item[1]), np.array(item[2]), {k: np.array(v) for k, v in item[3].items()})
        rows = rs.outlet_rows
    assert sorted(got) == [0, 1, 2, 3]
    for d in range(4):
        w = want[d]
        assert np.array_equal(bits(got[d][0]), bits(w[0][rows, :, 0])), d
        assert np.array_equal(bits(got[d][1]), bits(np.stack([w[0][:, -1, 0], w[0][:, -1, 0], w[0][:, -1, 2]], 1))), d
        assert np.array_equal(bits(got[d][2]["reservoir_inflow"]), bits(w[1])), d
        assert np.array_equal(bits(got[d][2]["nudge"]), bits(w[2])), d
        assert np.array_equal(bits(got[d][2]["lastobs"][0]), bits(w[3][0])) and np.array_equal(bits(got[d][2]["lastobs"][1]), bits(w[3][1])), d
    r.close()
    # a router without reservoirs or gages: tuples of the old length
    r = ShardedRouter(c.to, c.params, stream=True, options=OPTIONS)
    with RouteStream(r, NSTEPS, QTS) as rs:
        items = list(rs.route(iter(c.days[:2]), c.q0))
    assert [len(i) for i in items] == [3, 3]
    r.close()


# ---- 5. errors and bookkeeping -----------------------------------------------------------------------------------------------
def test_stream_tables_errors_and_bookkeeping():
    c = case()
    tabs, _ = day_tables(c, 3)
    dt = np.float32
    with open_plan(c) as p:
        # reservoir data assimilation stays per window
        nres = c.lakes.shape[0]
        kind = np.zeros(nres, np.int32)
        kind[0] = 4
        p.set_reservoirs(c.lakes, c.par, DT)
        p.set_reservoir_da(kind, np.zeros(nres, np.int32), rfc=(np.full((1, 6), 1.0e3, np.float32), np.zeros(1, np.float32),
                                                                np.array([[1, 6, 0, 3600, 10]], np.int32)))
        p.upload_forcing(NSTEPS, c.days[0], c.q0)
        with pytest.raises(ValueError, match="types 2-5.*window by window"):
            p.stream_begin(NSTEPS, QTS)
        p.set_reservoirs(c.lakes, c.par, DT)              # (drops the tables)
        with pytest.raises(ValueError, match="gage on a reservoir row"):
            p.stream_set_gages(c.lakes[:1])
        p.stream_set_gages(c.gages)
        p.upload_forcing(NSTEPS, c.days[0], c.q0)
        p.stream_begin(NSTEPS, QTS)
        ql = pinned_like(c.days[0])
        mode, a, w = tabs[0]
        with pytest.raises(ValueError, match="must carry its nudging tables"):
            p.stream_push(ql)
        with pytest.raises(ValueError, match=r"nudging tables of a day must be \[%d\]\[%d\]" % (c.gages.shape[0], NSTEPS)):
            p.stream_push(ql, nudging=(mode[:-1], a[:-1], w[:-1]))
        with pytest.raises(ValueError, match="nudging tables of a day must be"):
            p.stream_push(ql, nudging=(mode[:, :-1], a[:, :-1], w[:, :-1]))
        with pytest.raises(ValueError, match="reservoir-inflow record of a day is"):
            p.stream_push(ql, nudging=tabs[0], reservoir_inflow=np.zeros((nres + 1, NSTEPS), dt))
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.set_reservoirs(c.lakes, c.par, DT)
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.stream_set_gages(c.gages[:3])
        assert p.stream_info()["days_pushed"] == 0        # (a refused push leaves no day behind)
        p.stream_end()
        # a second stream on the same plan with more slots: the same products
        first, info1 = stream_days(p, c, tabs, full_output=False, output_stride=8)
        second, info2 = stream_days(p, c, tabs, full_output=False, output_stride=8, slots=info1["slots"] + 2)
        assert info2["slots"] == info1["slots"] + 2
        assert_days_equal(second, first, "more slots")
        # ... and a stream of more days than its ring has slots: every slot's tables and records are used twice and more
        long = Case()
        long.__dict__.update(c.__dict__)
        ndays = 2 * info1["slots"] + 1
        long.days = [c.days[d % 3] for d in range(ndays)]
        long.usgs = [c.usgs[d % 3] for d in range(ndays)]
        ltabs, _ = day_tables(long, ndays)
        windows = window_days(p, long, ltabs, 8)
        got, info3 = stream_days(p, long, ltabs, full_output=False, output_stride=8)
        assert info3["slots"] == info1["slots"] and len(got) == ndays > info3["slots"]
        assert_days_equal(got, windows, "ring reuse")
    with pytest.raises(NotImplementedError):
        ShardedRouter(c.to, c.params, rank=0, world=2, stream=True, reservoirs=(c.lakes, c.par, DT))
