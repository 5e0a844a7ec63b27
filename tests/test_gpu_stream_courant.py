"""THE COURANT NUMBER OF EVERY ROW OVER A WHOLE STREAM OF DAYS (include/trmc.h trmc_stream_set_courant, trmc_stream_courant;
csrc/k_stream_courant.inc; RoutingPlan.stream_set_courant / stream_courant; ``courant`` of RouteStream): per row the highest
cn = ck dt / dx, the step it was first reached at and the number of steps with cn > limit, the steps counted on over the days.

THE EXPECTED VALUES ARE THE WINDOW'S, never the stream's own: the same days routed as ONE window of days x nsteps steps on the same
plan (or day by day with the state carried, where tables come with every day) and ``window_courant_summary`` at the same limit --
peak, step and count must agree bit for bit over every row.  The fp32 case of every layout is pinned to the ORACLE as well
(tests/stream_courant_cases.py: the reference Fortran's step at the rebuilt inputs of every row-step).  Before anything is compared
the expectation is shown to hold the paths the fold has (``census``): row-steps without flow, rows that go from dry to wet,
over-bank row-steps, cn over the limit at some rows only, a peak on a day's first step, a peak on a later day than the row's first
local maximum.

Shapes: 301 rows (no multiple of 64 or 256, ten rows of fan-in 3), five days of 48 steps at qts 12 and wide_k 16, and days of 36
steps at wide_k 4 -- no multiple of the kernel's eight loads in flight, so its remainder loop runs.  The ring has fewer slots than
days wherever the layout's lag allows (a forest routed as slices alone lags 14 tiles: its ring cannot be shorter than 7)."""
import os

import numpy as np
import pytest

import helpers as H
import stream_courant_cases as SC
from troute_amd import _lib
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

# (tests/test_gpu_stream.py's variants at this forest's size, slices alone, and the slices split over the two streams)
LAYOUTS = {
    "slices": ({"wide_min_rows": 1, "wide_k": 16, "cluster_rows": 64}, 48),
    "clusters-only": ({"wide_min_rows": -1, "wide_k": 16, "cluster_rows": 128}, 48),
    "slices+clusters": ({"wide_min_rows": 30, "wide_k": 16, "cluster_rows": 128}, 48),
    "split": ({"wide_min_rows": 30, "wide_k": 16, "cluster_rows": 128, "stream_split": 1}, 48),
    "k4-small-clusters": ({"wide_min_rows": 30, "wide_k": 4, "cluster_rows": 24}, 36),
}
VARIANTS = {"fp32": (32, {}), "fp64": (64, {}), "tolerance": (32, {"arithmetic": "tolerance"})}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_courant(got, pk, at, over, what, days=None):
    assert list(got) == ["days", "peak_cn", "peak_cn_step", "steps_over"], (what, list(got))
    if days is not None:
        assert got["days"] == days, (what, got["days"], days)
    assert got["peak_cn"].dtype == pk.dtype and got["peak_cn_step"].dtype == np.int64 and got["steps_over"].dtype == np.int64, what
    for name, g, w in (("peak_cn", bits(got["peak_cn"]), bits(pk)), ("peak_cn_step", got["peak_cn_step"], np.asarray(at, np.int64)),
                       ("steps_over", got["steps_over"], np.asarray(over, np.int64))):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def open_plan(layout, variant="fp32", more=None):
    net = SC.network()
    opts, nsteps = LAYOUTS[layout]
    precision, arith = VARIANTS[variant]
    p = RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", precision=precision,
                    options=dict(opts, **arith, **(more or {})))
    return p, nsteps


def window_of(p, days, q0, nsteps, limit):
    """the days as ONE window on plan p: (its summary at `limit`, cn [rows, steps], fvd)"""
    T = nsteps * len(days)
    p.route(T, SC.QTS, True, SC.as_one_window(days), q0)
    s = p.window_courant_summary(limit)
    return s, np.ascontiguousarray(p.window_courant()[:, :, 0]), p.download_fvd()


def stream_of(p, days, q0, nsteps, limit, full_output=False, fetch_between=False):
    """the days as one stream with the Courant number on: (the fetch after the last day, {days complete: fetch} in mid-stream, info)"""
    p.stream_set_courant(limit)
    p.upload_forcing(nsteps, days[0], q0)
    p.stream_begin(nsteps, SC.QTS, full_output=full_output)
    info = p.stream_info()
    between = {}
    for d, day in enumerate(days):
        assert p.stream_push(pinned_like(day)) == d
        done = p.stream_info()["days_complete"]
        if fetch_between and done >= 1 and done not in between:
            between[done] = p.stream_courant()
    p.stream_flush()
    last = p.stream_courant()
    p.stream_end()
    return last, between, info


# ---- 1. every layout, precision and arithmetic, with and without the full result, against the window (fp32: and the oracle) -------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_stream_of_five_days_equals_the_same_days_as_one_window(layout, variant):
    net = SC.network()
    p, nsteps = open_plan(layout, variant)
    with p:
        dt = p.dtype
        assert (p.arithmetic == "tolerance") == (variant == "tolerance") and np.dtype(dt).itemsize * 8 == VARIANTS[variant][0]
        lag, W, C = p.lags()
        assert (W > 0) == (layout != "clusters-only") and (C > 0) == (layout != "slices"), (W, C)
        assert net.to.shape[0] % 64 and net.to.shape[0] % 256 and nsteps % LAYOUTS[layout][0]["wide_k"] == 0 and (nsteps % 8 != 0) == (layout == "k4-small-clusters")
        days, q0 = SC.days_of(nsteps, dtype=dt), net.q0.astype(dt)
        s, cn, fvd = window_of(p, days, q0, nsteps, SC.LIMIT)
        pk, at, over = SC.summary_of(cn, SC.LIMIT)
        # the expected side: the window's summary is its own block's under the rule, and holds every path of the fold
        assert np.array_equal(bits(s["peak_cn"]), bits(pk)) and np.array_equal(s["peak_cn_step"], at) and np.array_equal(s["steps_over"], over)
        SC.census(cn, fvd, q0, nsteps, SC.LIMIT)
        if variant == "fp32":                                   # ... and IS the oracle's
            ocn, ofvd = SC.oracle_cn(nsteps)
            SC.census(ocn, ofvd, net.q0, nsteps, SC.LIMIT)
            assert np.array_equal(bits(cn), bits(ocn)), "the window's cn is not the oracle's"
        for full in (False, True):
            got, between, info = stream_of(p, days, q0, nsteps, SC.LIMIT, full_output=full, fetch_between=True)
            assert (info["slots"] < SC.NDAYS) == (layout != "slices"), info
            assert_courant(got, s["peak_cn"], s["peak_cn_step"], s["steps_over"], (layout, variant, full), SC.NDAYS)
            assert between or layout == "slices", info              # (slices alone: 14 tiles of lag, no day is through before the flush)
            for done, part in between.items():                  # in mid-stream: exactly the days handed over
                assert_courant(part, *SC.summary_of(cn[:, :done * nsteps], SC.LIMIT), (layout, variant, full, "after day", done), done)


# ---- 2. a fetch after day 2 and after day 5; a run over the limit across a day's end ------------------------------------------------
def test_fetches_after_day_two_and_after_day_five_each_equal_the_window_over_that_many_days():
    net = SC.network()
    p, nsteps = open_plan("slices+clusters")
    with p:
        days = SC.days_of(nsteps)
        s2, cn2, _ = window_of(p, days[:2], net.q0, nsteps, SC.LIMIT)
        s5, cn5, _ = window_of(p, days, net.q0, nsteps, SC.LIMIT)
        assert np.array_equal(bits(cn5[:, :2 * nsteps]), bits(cn2))
        over = cn5 > np.float32(SC.LIMIT)
        edges = np.arange(nsteps, SC.NDAYS * nsteps, nsteps)                    # (0-based index of a day's first step)
        across = (over[:, edges - 1] & over[:, edges]).any(axis=1)
        assert across.any()                                                    # a run over the limit across a day's end
        p.stream_set_courant(SC.LIMIT)
        p.upload_forcing(nsteps, days[0], net.q0)
        p.stream_begin(nsteps, SC.QTS)
        for d in (0, 1):
            p.stream_push(pinned_like(days[d]))
        p.stream_flush()
        assert_courant(p.stream_courant(), s2["peak_cn"], s2["peak_cn_step"], s2["steps_over"], "after day 2", 2)
        assert p.stream_courant_kernel_ms() > 0                                 # (the last fold's device time, from events)
        for d in (2, 3, 4):
            p.stream_push(pinned_like(days[d]))
        p.stream_flush()
        got = p.stream_courant()
        assert_courant(got, s5["peak_cn"], s5["peak_cn_step"], s5["steps_over"], "after day 5", 5)
        assert np.array_equal(got["steps_over"][across], over[across].sum(axis=1))             # no gap, no double count
        # any subset of NULL destinations; days_out may be NULL too
        h, n = _lib.lib(), net.to.shape[0]
        pk, st, ov = np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        assert h.trmc_stream_courant(p._h, _lib.ptr(pk), None, None, None) == 0 and np.array_equal(bits(pk), bits(s5["peak_cn"]))
        assert h.trmc_stream_courant(p._h, None, None, _lib.ptr(ov), None) == 0 and np.array_equal(ov, s5["steps_over"])
        assert h.trmc_stream_courant(p._h, _lib.ptr(pk), _lib.ptr(st), None, None) == 0 and np.array_equal(st, s5["peak_cn_step"])
        assert h.trmc_stream_courant(p._h, None, _lib.ptr(st), None, None) == _lib.TRMC_EINVAL
        assert h.trmc_stream_courant(p._h, None, None, None, None) == _lib.TRMC_EINVAL
        p.stream_end()
        again, _, _ = stream_of(p, days, net.q0, nsteps, SC.LIMIT)                             # a second stream starts from zero
        assert_courant(again, s5["peak_cn"], s5["peak_cn_step"], s5["steps_over"], "a second stream", 5)
        other, _, _ = stream_of(p, days, net.q0, nsteps, 0.25)                                 # another limit: the count alone moves
        assert_courant(other, s5["peak_cn"], s5["peak_cn_step"], (cn5 > np.float32(0.25)).sum(axis=1), "limit 0.25", 5)


# ---- 3. the stream's other products do not move --------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_output", [False, True])
def test_the_other_products_are_bit_identical_with_and_without_it(full_output):
    net = SC.network()
    n = net.to.shape[0]
    p, nsteps = open_plan("slices+clusters")
    rows = np.arange(0, n, 7)
    with p:
        days = SC.days_of(nsteps)
        rs = p.rowset(rows)

        def run(courant, stage):
            p.stream_set_courant(SC.LIMIT if courant else None)
            p.stream_set_stage(stage)
            p.stream_set_summary(("peak", "mean"))
            p.upload_forcing(nsteps, days[0], net.q0)
            p.stream_begin(nsteps, SC.QTS, full_output=full_output)
            mk = lambda shape, dt=np.float32: [_lib.result_empty(shape, dt, always_pinned=True) for _ in days]
            hyd, fin, pk, st, mean, stg = mk((rows.size, nsteps)), mk((n, 3)), mk((n,)), mk((n,), np.int32), mk((n,)), mk((rows.size, nsteps))
            fvd = mk((n, nsteps, 3)) if full_output else None
            for d, day in enumerate(days):
                p.stream_push(pinned_like(day), rowset=rs, hyd=hyd[d], q0=fin[d], summary=(pk[d], st[d], mean[d]),
                              **({"stage": stg[d]} if stage else {}), **({"fvd": fvd[d]} if full_output else {}))
            p.stream_flush()
            cou = p.stream_courant() if courant else None
            p.stream_end()
            return {"hyd": hyd, "final": fin, "peak": pk, "step": st, "mean": mean, "stage": stg if stage else None, "fvd": fvd}, cou
        off, _ = run(False, True)
        on, cou = run(True, True)
        lean, cou2 = run(True, False)
        p.stream_set_courant(None)
        p.stream_set_stage(False)
        p.stream_set_summary(None)
        for name in ("hyd", "final", "peak", "step", "mean", "stage", "fvd"):
            if off[name] is None:
                continue
            for d in range(SC.NDAYS):
                assert np.array_equal(bits(on[name][d]), bits(off[name][d])), (name, d)
                if lean[name] is not None:
                    assert np.array_equal(bits(lean[name][d]), bits(off[name][d])), ("without stage", name, d)
        assert off["hyd"][2].max() > 0 and np.abs(off["stage"][2]).max() > 0
        assert_courant(cou2, cou["peak_cn"], cou["peak_cn_step"], cou["steps_over"], "with and without stage", SC.NDAYS)
        s, _, _ = window_of(p, days, net.q0, nsteps, SC.LIMIT)
        assert_courant(cou, s["peak_cn"], s["peak_cn_step"], s["steps_over"], "beside the other products", SC.NDAYS)


# ---- 4. NaN in the forcing -------------------------------------------------------------------------------------------------------------
def test_a_nan_at_the_streams_first_step_stays_and_a_later_one_replaces_nothing():
    import nonfinite_cases as NF
    net = NF.network()[0]
    c = NF.case(NF.DAY * NF.NDAYS, 32, stream=True)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=NF.OPTIONS) as p:
        p.route(c.nsteps, 1, True, np.ascontiguousarray(c.qlat), c.q0)
        s = p.window_courant_summary(SC.LIMIT)
        cn = np.ascontiguousarray(p.window_courant()[:, :, 0])
        pk, at, over = SC.summary_of(cn, SC.LIMIT)
        assert np.array_equal(bits(s["peak_cn"]), bits(pk)) and np.array_equal(s["peak_cn_step"], at) and np.array_equal(s["steps_over"], over)
        nan = np.isnan(cn)
        first = nan[:, 0] & ~nan.all(axis=1)
        later = ~nan[:, 0] & nan.any(axis=1)
        assert first.sum() >= 4 and later.sum() >= 8, (first.sum(), later.sum())
        assert np.isnan(pk[first]).all() and (at[first] == 1).all()                      # a NaN at step 1 stays
        assert not np.isnan(pk[later]).any()                                             # a later one replaces nothing
        behind = later & (nan.argmax(axis=1) < at - 1)
        assert behind.any()                                                              # ... rows that peak BEHIND their NaN
        low = np.float32(np.nanmin(np.where(cn > 0, cn, np.nan)) / 2)                    # a limit every number is over: a NaN is not counted
        days = [c.day(d) for d in range(NF.NDAYS)]
        for limit in (SC.LIMIT, float(low)):
            p.stream_set_courant(limit)
            p.upload_forcing(NF.DAY, days[0], c.q0)
            p.stream_begin(NF.DAY, 1)
            for day in days:
                p.stream_push(pinned_like(day))
            p.stream_flush()
            got = p.stream_courant()
            p.stream_end()
            with np.errstate(invalid="ignore"):
                want_over = (cn > np.float32(limit)).sum(axis=1)
            assert_courant(got, pk, at, want_over, ("NaN", limit), NF.NDAYS)
        assert (want_over[later] < c.nsteps).all() and (want_over[later] > 0).any()


# ---- 5. reservoirs and gages on the golden domain ---------------------------------------------------------------------------------------
def test_lowercolorado_with_its_waterbodies_and_gages_equals_its_windows():
    """reservoir rows (0, 1, 0); a gage row's cn is the un-nudged step's and the row below was fed the nudged flow: what the window's
    block holds, day by day with the state carried and the gage rows started from the day's first observation"""
    import test_reservoirs as TR
    lc, ids, dv, ql, q0, reaches, net, lakes, wbody_cols, lakeset, nts = TR.reservoir_case(48)
    row = {int(s): i for i, s in enumerate(ids)}
    nseg = len(ids)
    ups = [[] for _ in range(nseg)]
    for rr in reaches:
        for k, s in enumerate(rr):
            ups[row[s]] = [row[u] for u in net.get(rr[0], [])] if k == 0 else [row[rr[k - 1]]]
    up_ptr, up_idx = csr_from_lists(ups)
    lake_rows = np.array([row[int(l)] for l in lakes])
    params9 = np.nan_to_num(dv[:, [H.DATA_COLS.index(k) for k in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")]], nan=1.0)
    params9[:, 0] = lc.dt
    a = wbody_cols.astype(np.float32)
    par = np.concatenate([a[:, :8], np.full((len(lakes), 1), 10.0, np.float32)], 1)
    state0 = q0.copy()
    state0[lake_rows, 2] = (a[:, 4] + ((a[:, 1] - a[:, 4]).astype(np.float32) * a[:, 8]).astype(np.float32)).astype(np.float32)
    G = np.load(os.path.join(H.GOLDEN, "lowercolorado_gages.npz"))
    gid = [int(g) for g in G["gage_ids"] if int(g) in row and row[int(g)] not in set(lake_rows.tolist())]
    sel = np.array([G["gage_ids"].tolist().index(g) for g in gid])
    gages = np.array([row[g] for g in gid], np.int64)
    assert gages.size >= 3 and np.unique(gages).size == gages.size
    below = np.array([i for i in range(nseg) if set(ups[i]) & set(gages.tolist())])
    below_lake = np.array([i for i in range(nseg) if set(ups[i]) & set(lake_rows.tolist()) and i not in set(lake_rows.tolist())])
    assert below.size and below_lake.size
    days = [ql, (ql * np.float32(0.6)).astype(np.float32)]
    usgs = G["usgs"][sel].astype(np.float32)

    def tables(d):                                           # the day's observations replace the flow where there is one (mode 1)
        obs = np.ascontiguousarray(usgs[:, 1 + d * nts:1 + (d + 1) * nts])     # (column 0 of a day: its first observation)
        mode = (~np.isnan(obs)).astype(np.uint8)
        return mode, np.nan_to_num(obs, nan=0.0).astype(np.float32), np.zeros_like(obs, dtype=np.float32), np.ascontiguousarray(usgs[:, d * nts])
    with RoutingPlan(up_ptr, up_idx, params9, assume_short_ts=True, engine="levels", options={"cluster_rows": 128}) as p:
        p.set_reservoirs(lake_rows, par, lc.dt)
        state, blocks, nudges = state0, [], []
        for d, q in enumerate(days):                         # the windows, the state through the host
            mode, aa, ww, first = tables(d)
            state = state.copy()
            ok = ~np.isnan(first)
            state[gages[ok], 0] = first[ok]
            p.upload_forcing(nts, q, state)
            p.set_nudging(nts, gages, mode, aa, ww)
            p.route_device(nts, lc.qts, True)
            blocks.append(np.ascontiguousarray(p.window_courant()[:, :, 0]))
            nudges.append(p.download_nudge())
            state = p.download_final_state()
        cn = np.ascontiguousarray(np.concatenate(blocks, axis=1))
        assert np.abs(np.concatenate(nudges, axis=1)).max() > 0                 # something was nudged
        assert not cn[lake_rows].any() and np.nanmax(cn[below]) > 0 and np.nanmax(cn[below_lake]) > 0 and np.nanmax(cn[gages]) > 0
        pk, at, over = SC.summary_of(cn, 0.1)
        assert 0 < np.count_nonzero(over) < nseg
        for full in (False, True):
            p.stream_set_gages(gages)
            p.stream_set_courant(0.1)
            p.upload_forcing(nts, days[0], state0)
            p.stream_begin(nts, lc.qts, full_output=full)
            for d, q in enumerate(days):
                mode, aa, ww, first = tables(d)
                p.stream_push(pinned_like(q), nudging=(mode, aa, ww, first))
            p.stream_flush()
            got = p.stream_courant()
            p.stream_end()
            assert_courant(got, pk, at, over, ("lowercolorado", full), 2)
            assert not got["peak_cn"][lake_rows].any() and (got["peak_cn_step"][lake_rows] == 1).all() and not got["steps_over"][lake_rows].any()


# ---- 6. RouteStream ----------------------------------------------------------------------------------------------------------------------
def test_routestream_courant():
    from troute_amd.distributed import ShardedRouter
    from troute_amd.sequence import RouteStream
    net = SC.network()
    opts, nsteps = LAYOUTS["slices+clusters"]
    days = SC.days_of(nsteps)
    r = ShardedRouter(net.to, net.params, stream=True, options=opts)
    with RouteStream(r, nsteps, SC.QTS, courant=SC.LIMIT) as rs:
        assert rs.courant is None
        seen = []
        for item in rs.route(iter(days), net.q0):
            assert len(item) == 3                                               # (not a product of the day: the tuples do not change)
            c = rs.courant
            seen.append(None if c is None else c["days"])
        got = rs.courant
        assert got["days"] == SC.NDAYS and [s for s in seen if s is not None] == sorted(s for s in seen if s is not None)
    ocn, _ = SC.oracle_cn(nsteps)
    assert_courant(got, *SC.summary_of(ocn, SC.LIMIT), "RouteStream against the oracle", SC.NDAYS)
    with RouteStream(r, nsteps, SC.QTS) as rs:                                   # (an earlier stream's declaration is withdrawn)
        assert len([0 for _ in rs.route(iter(days[:2]), net.q0)]) == 2 and rs.courant is None
    r.close()


# ---- 7. refusals on the device -----------------------------------------------------------------------------------------------------------
def test_refusals():
    net = SC.network()
    h = _lib.lib()
    opts, nsteps = LAYOUTS["slices+clusters"]
    days = SC.days_of(nsteps)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=opts) as p:
        p.stream_set_courant(None)                                              # (withdrawing nothing is no error)
        p.upload_forcing(nsteps, days[0], net.q0)
        p.stream_begin(nsteps, SC.QTS)
        with pytest.raises(RuntimeError, match="begun without the Courant number"):      # a stream begun without it
            p.stream_courant()
        assert h.trmc_stream_courant(p._h, _lib.ptr(np.zeros(net.to.shape[0], np.float32)), None, None, None) == _lib.TRMC_ESTATE
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.stream_set_courant(1.0)
        p.stream_end()
        with pytest.raises(RuntimeError, match="no stream of windows in progress"):
            p.stream_courant()
        p.stream_set_courant(1.0)
        p.upload_forcing(nsteps, days[0], net.q0)
        p.stream_begin(nsteps, SC.QTS)
        assert p.stream_info()["lag_max"] > 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):  # before the first complete day: begun ...
            p.stream_courant()
        with pytest.raises(RuntimeError, match="no day has been folded"):
            p.stream_courant_kernel_ms()
        p.stream_push(pinned_like(days[0]))
        assert p.stream_info()["days_complete"] == 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):  # ... and pushed, its last rows under way
            p.stream_courant()
        assert h.trmc_stream_courant(p._h, _lib.ptr(np.zeros(net.to.shape[0], np.float32)), None, None, None) == _lib.TRMC_ESTATE
        p.stream_flush()
        assert p.stream_courant()["days"] == 1
        p.stream_end()
    # velocity_on_demand = -1: refused without full_output, as stage is; with it the stream runs
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=dict(opts, velocity_on_demand=-1)) as p:
        p.stream_set_courant(1.0)
        p.upload_forcing(nsteps, days[0], net.q0)
        with pytest.raises(NotImplementedError, match="velocity_on_demand"):
            p.stream_begin(nsteps, SC.QTS)
        assert h.trmc_stream_begin(p._h, nsteps, SC.QTS, 0, 0, 0) == _lib.TRMC_EUNSUPPORTED
        p.stream_begin(nsteps, SC.QTS, full_output=True)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        one = p.stream_courant()
        p.stream_end()
        ocn, _ = SC.oracle_cn(nsteps)
        assert_courant(one, *SC.summary_of(ocn[:, :nsteps], 1.0), "velocity_on_demand = -1 with full_output", 1)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="flow") as p:   # the dataflow engine
        assert p.engine == "flow"
        with pytest.raises(ValueError, match="level engine"):
            p.stream_set_courant(1.0)
        assert h.trmc_stream_set_courant(p._h, 1, 1.0) == _lib.TRMC_EINVAL
