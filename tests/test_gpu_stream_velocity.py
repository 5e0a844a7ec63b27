"""PEAK VELOCITY AND VELOCITY-THRESHOLD EXCEEDANCE OF EVERY ROW OVER A WHOLE STREAM OF DAYS (include/trmc.h trmc_stream_set_velocity,
trmc_stream_velocity; csrc/k_stream_velocity.inc; RoutingPlan.stream_set_velocity / stream_velocity; ``velocity`` of RouteStream):
per row the highest velocity and the step it was first reached at and, per level of a threshold table, steps over, first and last
step and longest run, the steps counted on over the days and a run carried over a day's end.

THE EXPECTED VALUES ARE THE WINDOW'S, never the stream's own: the same days routed as ONE window of days x nsteps steps on the same
plan (or day by day with the state carried, where tables come with every day), column 1 of its result, through the numpy rule
(tests/stream_velocity_cases.py ``rule_of``) -- which is first shown equal to ``window_summary(("peak_velocity",))`` and
``window_exceedance("velocity")`` of that window, and for fp32 to the ORACLE's velocity column.  All six figures must agree bit for
bit / integer for integer over every row.  Before anything is compared the expectation is shown to hold the paths the fold has
(``census``).  The thresholds are built from the expected velocities.

Shapes: 301 rows (no multiple of 64 or 256, ten rows of fan-in 3), five days of 48 steps at qts 12 and wide_k 16, and days of 36
steps at wide_k 4 -- no multiple of the kernel's eight loads in flight, so its remainder loop runs.  The ring has fewer slots than
days wherever the layout's lag allows (a forest routed as slices alone lags 14 tiles: its ring cannot be shorter than 7)."""
import os

import numpy as np
import pytest

import helpers as H
import stream_velocity_cases as SV
from troute_amd import _lib
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

# (tests/test_gpu_stream_courant.py's layouts and variants)
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


def assert_velocity(got, want, what, days=None):
    """got: a stream's fetch; want: ``rule_of``'s dict -- the same keys behind "days", in the same order, the same bits"""
    assert list(got) == ["days"] + list(want), (what, list(got), list(want))
    if days is not None:
        assert got["days"] == days, (what, got["days"], days)
    for name, w in want.items():
        g = got[name]
        assert g.dtype == (w.dtype if name == "peak_velocity" else np.int64) and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        g, w = (bits(g), bits(w)) if name == "peak_velocity" else (g, np.asarray(w, np.int64))
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:8].tolist(), g[g != w][:8].tolist(), w[g != w][:8].tolist())


def open_plan(layout, variant="fp32", more=None):
    net = SV.network()
    opts, nsteps = LAYOUTS[layout]
    precision, arith = VARIANTS[variant]
    p = RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", precision=precision,
                    options=dict(opts, **arith, **(more or {})))
    return p, nsteps


def window_of(p, days, q0, nsteps, qts=SV.QTS):
    """the days as ONE window on plan p: its result [rows, steps, 3]"""
    p.route(nsteps * len(days), qts, True, SV.as_one_window(days), q0)
    return p.download_fvd()


def assert_rule_is_the_windows(p, v, th, what):
    """``rule_of`` over the last window's velocities against the window's own products on the device"""
    want = SV.rule_of(v, th)
    s = p.window_summary(("peak_velocity",))
    assert np.array_equal(bits(s["peak_velocity"]), bits(want["peak_velocity"])) and np.array_equal(s["peak_velocity_step"], want["peak_velocity_step"]), what
    p.set_thresholds(th)
    x = p.window_exceedance("velocity")
    p.set_thresholds(None)
    for name in SV.PARTS:
        assert np.array_equal(x[name], want[name]), (what, name)


def stream_of(p, days, q0, nsteps, th, full_output=False, fetch_between=False, qts=SV.QTS):
    """the days as one stream with the velocity on (th None: the peak and its step only): (the fetch after the last day,
    {days complete: fetch} in mid-stream, info)"""
    p.stream_set_velocity(True if th is None else th)
    p.upload_forcing(nsteps, days[0], q0)
    p.stream_begin(nsteps, qts, full_output=full_output)
    info = p.stream_info()
    between = {}
    for d, day in enumerate(days):
        assert p.stream_push(pinned_like(day)) == d
        done = p.stream_info()["days_complete"]
        if fetch_between and done >= 1 and done not in between:
            between[done] = p.stream_velocity()
    p.stream_flush()
    last = p.stream_velocity()
    p.stream_end()
    p.stream_set_velocity(None)
    return last, between, info


# ---- 1. every layout, precision and arithmetic, with and without the full result, K = 0, 1, 4 (and 2), against the window ----------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_stream_of_five_days_equals_the_same_days_as_one_window(layout, variant):
    net = SV.network()
    p, nsteps = open_plan(layout, variant)
    with p:
        dt = p.dtype
        assert (p.arithmetic == "tolerance") == (variant == "tolerance") and np.dtype(dt).itemsize * 8 == VARIANTS[variant][0]
        lag, W, C = p.lags()
        assert (W > 0) == (layout != "clusters-only") and (C > 0) == (layout != "slices"), (W, C)
        assert net.to.shape[0] % 64 and net.to.shape[0] % 256 and (nsteps % 8 != 0) == (layout == "k4-small-clusters")
        days, q0 = SV.days_of(nsteps, dtype=dt), net.q0.astype(dt)
        v = np.ascontiguousarray(window_of(p, days, q0, nsteps)[:, :, 1])
        if variant == "fp32":                                   # the window's velocity IS the oracle's
            assert np.array_equal(bits(v), bits(SV.oracle_cn(nsteps)[1][:, :, 1])), "the window's velocity is not the oracle's"
        tables = {K: SV.thresholds_of(v, K) for K in ((1, 2, 4) if layout == "slices+clusters" else (1, 4))}
        for K, th in tables.items():
            assert th.dtype == dt
            assert_rule_is_the_windows(p, v, th, (layout, variant, K))
            SV.census(v, th, nsteps)
        tables[0] = None
        for full in (False, True):
            for K, th in tables.items():
                got, between, info = stream_of(p, days, q0, nsteps, th, full_output=full, fetch_between=True)
                assert (info["slots"] < SV.NDAYS) == (layout != "slices"), info
                assert_velocity(got, SV.rule_of(v, th), (layout, variant, full, K), SV.NDAYS)
                assert between or layout == "slices", info      # (slices alone: 14 tiles of lag, no day is through before the flush)
                for done, part in between.items():              # in mid-stream: exactly the days handed over
                    assert_velocity(part, SV.rule_of(v[:, :done * nsteps], th), (layout, variant, full, K, "after day", done), done)


# ---- 2. where the full result exists, the fold's velocity is the result's ----------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_folds_peak_equals_the_peak_of_the_streams_own_full_result(variant):
    net = SV.network()
    n = net.to.shape[0]
    p, nsteps = open_plan("slices+clusters", variant)
    with p:
        dt = p.dtype
        days, q0 = SV.days_of(nsteps, dtype=dt), net.q0.astype(dt)
        p.stream_set_velocity(True)
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_begin(nsteps, SV.QTS, full_output=True)
        fvd = [_lib.result_empty((n, nsteps, 3), dt, always_pinned=True) for _ in days]
        for d, day in enumerate(days):
            p.stream_push(pinned_like(day), fvd=fvd[d])
        p.stream_flush()
        got = p.stream_velocity()
        p.stream_end()
        p.stream_set_velocity(None)
        own = np.ascontiguousarray(np.concatenate([f[:, :, 1] for f in fvd], axis=1))
        assert own.max() > 0 and (own == 0).any()
        assert_velocity(got, SV.rule_of(own), ("the stream's own fvd", variant), SV.NDAYS)


# ---- 3. fetches and restarts ------------------------------------------------------------------------------------------------------
def test_fetches_after_day_two_and_after_day_five_and_a_second_stream():
    net = SV.network()
    n = net.to.shape[0]
    p, nsteps = open_plan("slices+clusters")
    with p:
        days = SV.days_of(nsteps)
        v2 = np.ascontiguousarray(window_of(p, days[:2], net.q0, nsteps)[:, :, 1])
        v5 = np.ascontiguousarray(window_of(p, days, net.q0, nsteps)[:, :, 1])
        assert np.array_equal(bits(v5[:, :2 * nsteps]), bits(v2))
        th = SV.thresholds_of(v5, 4)
        w2, w5 = SV.rule_of(v2, th), SV.rule_of(v5, th)
        assert ((w2["peak_velocity"] == 0) & (w2["peak_velocity_step"] == 1)).any()       # rows without flow in two days: (0, 1)
        p.stream_set_velocity(th)
        p.upload_forcing(nsteps, days[0], net.q0)
        p.stream_begin(nsteps, SV.QTS)
        for d in (0, 1):
            p.stream_push(pinned_like(days[d]))
        p.stream_flush()
        assert_velocity(p.stream_velocity(), w2, "after day 2", 2)
        assert p.stream_velocity_kernel_ms() > 0                                # (the last fold's device time, from events)
        for d in (2, 3, 4):
            p.stream_push(pinned_like(days[d]))
        p.stream_flush()
        assert_velocity(p.stream_velocity(), w5, "after day 5", 5)
        # any subset of NULL destinations; days_out may be NULL too
        h = _lib.lib()
        pk, st = np.zeros(n, np.float32), np.zeros(n, np.int64)
        lev = [np.zeros((n, 4), np.int64) for _ in range(4)]
        N = None
        assert h.trmc_stream_velocity(p._h, _lib.ptr(pk), N, N, N, N, N, N) == 0 and np.array_equal(bits(pk), bits(w5["peak_velocity"]))
        assert h.trmc_stream_velocity(p._h, _lib.ptr(pk), _lib.ptr(st), N, N, N, N, N) == 0 and np.array_equal(st, w5["peak_velocity_step"])
        assert h.trmc_stream_velocity(p._h, N, N, N, N, _lib.ptr(lev[2]), N, N) == 0 and np.array_equal(lev[2], w5["last_step"])
        assert h.trmc_stream_velocity(p._h, N, N, *(_lib.ptr(a) for a in lev), N) == 0
        assert all(np.array_equal(a, w5[name]) for a, name in zip(lev, SV.PARTS))
        assert h.trmc_stream_velocity(p._h, N, _lib.ptr(st), N, N, N, N, N) == _lib.TRMC_EINVAL      # a step without its value
        assert h.trmc_stream_velocity(p._h, N, N, N, N, N, N, N) == _lib.TRMC_EINVAL                 # nothing to fetch
        p.stream_end()
        again, _, _ = stream_of(p, days, net.q0, nsteps, th)                     # a second stream starts from zero
        assert_velocity(again, w5, "a second stream", 5)
        th1 = np.ascontiguousarray(th[:, 1::-1] * np.float32(1.5))                # other thresholds: the four figures alone move
        other, _, _ = stream_of(p, days, net.q0, nsteps, th1)
        assert_velocity(other, SV.rule_of(v5, th1), "other thresholds", 5)
        assert np.array_equal(bits(other["peak_velocity"]), bits(again["peak_velocity"])) and not np.array_equal(other["steps_over"], again["steps_over"][:, :2])
        # a stream declared without thresholds holds no exceedance figures
        p.stream_set_velocity(True)
        p.upload_forcing(nsteps, days[0], net.q0)
        p.stream_begin(nsteps, SV.QTS)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        assert h.trmc_stream_velocity(p._h, N, N, _lib.ptr(lev[0]), N, N, N, N) == _lib.TRMC_EINVAL
        assert list(p.stream_velocity()) == ["days", "peak_velocity", "peak_velocity_step"]
        p.stream_end()
        p.stream_set_velocity(None)


# ---- 4. the stream's other products do not move -------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_output", [False, True])
def test_the_other_products_are_bit_identical_with_and_without_it(full_output):
    net = SV.network()
    n = net.to.shape[0]
    p, nsteps = open_plan("slices+clusters")
    rows = np.arange(0, n, 7)
    with p:
        days = SV.days_of(nsteps)
        fvd5 = window_of(p, days, net.q0, nsteps)
        v5 = np.ascontiguousarray(fvd5[:, :, 1])
        th = SV.thresholds_of(v5, 4)
        qth = np.ascontiguousarray(np.quantile(fvd5[:, :, 0], 0.7, axis=1).astype(np.float32))
        dth = np.ascontiguousarray(np.quantile(fvd5[:, :, 2], 0.7, axis=1).astype(np.float32))
        rs = p.rowset(rows)
        p.set_thresholds(qth)

        def run(velocity, others):
            p.stream_set_velocity(th if velocity else None)
            p.stream_set_courant(1.0 if others else None)
            p.stream_set_exceedance("flow" if others else None)
            p.stream_set_depth_exceedance(dth if others else None)
            p.stream_set_stage(True)
            p.stream_set_summary(("peak", "mean"))
            p.upload_forcing(nsteps, days[0], net.q0)
            p.stream_begin(nsteps, SV.QTS, full_output=full_output)
            mk = lambda shape, dt=np.float32: [_lib.result_empty(shape, dt, always_pinned=True) for _ in days]
            hyd, fin, pk, st, mean, stg = mk((rows.size, nsteps)), mk((n, 3)), mk((n,)), mk((n,), np.int32), mk((n,)), mk((rows.size, nsteps))
            fvd = mk((n, nsteps, 3)) if full_output else None
            for d, day in enumerate(days):
                p.stream_push(pinned_like(day), rowset=rs, hyd=hyd[d], q0=fin[d], summary=(pk[d], st[d], mean[d]), stage=stg[d],
                              **({"fvd": fvd[d]} if full_output else {}))
            p.stream_flush()
            acc = {"velocity": p.stream_velocity() if velocity else None}
            if others:
                acc.update(courant=p.stream_courant(), exceedance=p.stream_exceedance(), depth_exceedance=p.stream_depth_exceedance())
            p.stream_end()
            return {"hyd": hyd, "final": fin, "peak": pk, "step": st, "mean": mean, "stage": stg, "fvd": fvd}, acc
        off, _ = run(False, False)
        on, a1 = run(True, False)
        three, a3 = run(False, True)
        four, a4 = run(True, True)                                              # four accumulators in one stream
        for q in ("velocity", "courant", "exceedance", "depth_exceedance"):
            getattr(p, "stream_set_" + q)(None)
        p.stream_set_stage(False)
        p.stream_set_summary(None)
        p.set_thresholds(None)
        for name in ("hyd", "final", "peak", "step", "mean", "stage", "fvd"):
            if off[name] is None:
                continue
            for d in range(SV.NDAYS):
                for other, what in ((on, "velocity"), (three, "the other three"), (four, "all four")):
                    assert np.array_equal(bits(other[name][d]), bits(off[name][d])), (what, name, d)
        assert off["hyd"][2].max() > 0 and np.abs(off["stage"][2]).max() > 0
        want = SV.rule_of(v5, th)
        assert_velocity(a1["velocity"], want, "alone", SV.NDAYS)
        assert_velocity(a4["velocity"], want, "beside the other three", SV.NDAYS)
        for q in ("courant", "exceedance", "depth_exceedance"):                 # ... which do not move either
            assert list(a3[q]) == list(a4[q]) and all(np.array_equal(a3[q][k], a4[q][k]) for k in a3[q]), q
        assert a4["exceedance"]["steps_over"].any() and a4["depth_exceedance"]["steps_over"].any() and a4["courant"]["peak_cn"].max() > 0


# ---- 5. NaN in the forcing ------------------------------------------------------------------------------------------------------------
def test_a_nan_at_the_streams_first_step_stays_and_a_later_one_replaces_nothing():
    import nonfinite_cases as NF
    net = NF.network()[0]
    c = NF.case(NF.DAY * NF.NDAYS, 32, stream=True)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=NF.OPTIONS) as p:
        p.route(c.nsteps, 1, True, np.ascontiguousarray(c.qlat), c.q0)
        v = np.ascontiguousarray(p.download_fvd()[:, :, 1])
        nan = np.isnan(v)
        first = nan[:, 0] & ~nan.all(axis=1)
        later = ~nan[:, 0] & nan.any(axis=1)
        assert first.sum() >= 4 and later.sum() >= 8, (first.sum(), later.sum())
        low = np.float32(np.nanmin(np.where(v > 0, v, np.nan)) / 2)              # a level every positive number is over: a NaN is not counted
        th = np.ascontiguousarray(np.stack([np.full(v.shape[0], low), np.full(v.shape[0], np.float32(np.nanmedian(v[v > 0])))], axis=1).astype(np.float32))
        th[3::4, 1] = np.nan                                                     # ... nor is anything over a NaN threshold
        assert_rule_is_the_windows(p, v, th, "NaN")
        want = SV.rule_of(v, th)
        pk, at = want["peak_velocity"], want["peak_velocity_step"]
        assert np.isnan(pk[first]).all() and (at[first] == 1).all()              # a NaN at step 1 stays
        assert not np.isnan(pk[later]).any()                                     # a later one replaces nothing
        assert (later & (nan.argmax(axis=1) < at - 1)).any()                     # ... rows that peak BEHIND their NaN
        assert (want["steps_over"][later, 0] < c.nsteps).all() and (want["steps_over"][later, 0] > 0).any() and not want["steps_over"][3::4, 1].any()
        days = [c.day(d) for d in range(NF.NDAYS)]
        for full in (False, True):
            got, _, _ = stream_of(p, days, c.q0, NF.DAY, th, full_output=full, qts=1)
            assert_velocity(got, want, ("NaN", full), NF.NDAYS)


# ---- 6. reservoirs and gages on the golden domain ---------------------------------------------------------------------------------------
def test_lowercolorado_with_its_waterbodies_and_gages_equals_its_windows():
    """reservoir rows hand out v = 0: (0, 1) and never over a positive level; a gage row's velocity is the un-nudged step's and the row
    below was fed the nudged flow: what the windows hold, day by day with the state carried and the gage rows started from the day's
    first observation (the construction of tests/test_gpu_stream_courant.py's case 5)"""
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
            blocks.append(np.ascontiguousarray(p.download_fvd()[:, :, 1]))
            nudges.append(p.download_nudge())
            state = p.download_final_state()
        v = np.ascontiguousarray(np.concatenate(blocks, axis=1))
        assert np.abs(np.concatenate(nudges, axis=1)).max() > 0                 # something was nudged
        assert not v[lake_rows].any() and np.nanmax(v[below]) > 0 and np.nanmax(v[below_lake]) > 0 and np.nanmax(v[gages]) > 0
        th = SV.thresholds_of(v, 2)
        th[lake_rows[::2], 0] = np.float32(-1)               # a level below 0: a reservoir row's v = 0 is over it at every step
        want = SV.rule_of(v, th)
        assert 0 < np.count_nonzero(want["steps_over"][:, 0]) < nseg and (want["steps_over"][lake_rows[::2], 0] == 2 * nts).all()
        for full in (False, True):
            p.stream_set_gages(gages)
            p.stream_set_velocity(th)
            p.upload_forcing(nts, days[0], state0)
            p.stream_begin(nts, lc.qts, full_output=full)
            for d, q in enumerate(days):
                mode, aa, ww, first = tables(d)
                p.stream_push(pinned_like(q), nudging=(mode, aa, ww, first))
            p.stream_flush()
            got = p.stream_velocity()
            p.stream_end()
            assert_velocity(got, want, ("lowercolorado", full), 2)
            assert not got["peak_velocity"][lake_rows].any() and (got["peak_velocity_step"][lake_rows] == 1).all()
            for rows in (below, below_lake, gages):
                assert got["peak_velocity"][rows].max() > 0
        p.stream_set_velocity(None)


# ---- 7. RouteStream ----------------------------------------------------------------------------------------------------------------------
def test_routestream_velocity():
    from troute_amd.distributed import ShardedRouter
    from troute_amd.sequence import RouteStream
    net = SV.network()
    opts, nsteps = LAYOUTS["slices+clusters"]
    days = SV.days_of(nsteps)
    ov = np.ascontiguousarray(SV.oracle_cn(nsteps)[1][:, :, 1])
    th = SV.thresholds_of(ov, 3)
    r = ShardedRouter(net.to, net.params, stream=True, options=opts)
    with RouteStream(r, nsteps, SV.QTS) as rs:
        plain = [len(item) for item in rs.route(iter(days), net.q0)]
        assert rs.velocity is None
    for velocity, table in ((th, th), (True, None)):
        with RouteStream(r, nsteps, SV.QTS, velocity=velocity) as rs:
            assert rs.velocity is None
            seen, lens = [], []
            for item in rs.route(iter(days), net.q0):
                lens.append(len(item))
                c = rs.velocity
                seen.append(None if c is None else c["days"])
            got = rs.velocity
            assert lens == plain                                                # (not a product of the day: the tuples do not change)
            assert got["days"] == SV.NDAYS and [s for s in seen if s is not None] == sorted(s for s in seen if s is not None)
        assert_velocity(got, SV.rule_of(ov, table), "RouteStream against the oracle", SV.NDAYS)
    with RouteStream(r, nsteps, SV.QTS) as rs:                                   # (an earlier stream's declaration is withdrawn)
        assert len([0 for _ in rs.route(iter(days[:2]), net.q0)]) == 2 and rs.velocity is None
        assert rs.plan._stream_velocity is None
    r.close()


# ---- 8. refusals on the device -----------------------------------------------------------------------------------------------------------
def test_refusals():
    net = SV.network()
    h = _lib.lib()
    n = net.to.shape[0]
    opts, nsteps = LAYOUTS["slices+clusters"]
    days = SV.days_of(nsteps)
    N = None
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=opts) as p:
        p.stream_set_velocity(None)                                             # (withdrawing nothing is no error)
        assert h.trmc_stream_set_velocity(p._h, 1, 5, _lib.ptr(np.zeros((n, 5), np.float32))) == _lib.TRMC_EINVAL
        assert h.trmc_stream_set_velocity(p._h, 1, -1, N) == _lib.TRMC_EINVAL
        assert h.trmc_stream_set_velocity(p._h, 1, 2, N) == _lib.TRMC_EINVAL
        p.upload_forcing(nsteps, days[0], net.q0)
        p.stream_begin(nsteps, SV.QTS)
        with pytest.raises(RuntimeError, match="begun without the velocity"):    # a stream begun without it
            p.stream_velocity()
        assert h.trmc_stream_velocity(p._h, _lib.ptr(np.zeros(n, np.float32)), N, N, N, N, N, N) == _lib.TRMC_ESTATE
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.stream_set_velocity(True)
        p.stream_end()
        with pytest.raises(RuntimeError, match="no stream of windows in progress"):
            p.stream_velocity()
        p.stream_set_velocity(True)
        p.upload_forcing(nsteps, days[0], net.q0)
        p.stream_begin(nsteps, SV.QTS)
        assert p.stream_info()["lag_max"] > 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):  # before the first complete day: begun ...
            p.stream_velocity()
        with pytest.raises(RuntimeError, match="no day has been folded"):
            p.stream_velocity_kernel_ms()
        p.stream_push(pinned_like(days[0]))
        assert p.stream_info()["days_complete"] == 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):  # ... and pushed, its last rows under way
            p.stream_velocity()
        assert h.trmc_stream_velocity(p._h, _lib.ptr(np.zeros(n, np.float32)), N, N, N, N, N, N) == _lib.TRMC_ESTATE
        p.stream_flush()
        assert p.stream_velocity()["days"] == 1
        p.stream_end()
    # velocity_on_demand = -1: refused without full_output, as stage is; with it the stream runs and equals the oracle
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=dict(opts, velocity_on_demand=-1)) as p:
        p.stream_set_velocity(True)
        p.upload_forcing(nsteps, days[0], net.q0)
        with pytest.raises(NotImplementedError, match="velocity_on_demand"):
            p.stream_begin(nsteps, SV.QTS)
        assert h.trmc_stream_begin(p._h, nsteps, SV.QTS, 0, 0, 0) == _lib.TRMC_EUNSUPPORTED
        p.stream_begin(nsteps, SV.QTS, full_output=True)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        one = p.stream_velocity()
        p.stream_end()
        ov = np.ascontiguousarray(SV.oracle_cn(nsteps)[1][:, :nsteps, 1])
        assert_velocity(one, SV.rule_of(ov), "velocity_on_demand = -1 with full_output", 1)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="flow") as p:   # the dataflow engine
        assert p.engine == "flow"
        with pytest.raises(ValueError, match="level engine"):
            p.stream_set_velocity(True)
        assert h.trmc_stream_set_velocity(p._h, 1, 0, N) == _lib.TRMC_EINVAL
        p.stream_set_velocity(None)                                             # (withdrawing nothing is no error there either)
        assert h.trmc_stream_set_velocity(p._h, 0, 0, N) == 0
