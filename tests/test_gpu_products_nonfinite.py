"""NaN VALUES AND EQUAL PEAKS THROUGH THE ROUTING AND THROUGH EVERY PER-ROW PRODUCT -- needs an MI355X.

Every per-row product is one ordered comparison (include/trmc.h: `if (x[t] > pk)`, `over(t) := x[t] > th`), from which the header
promises that the first of equal peaks wins, that a NaN never replaces a number and that a NaN at step 1 stays.  The rule is
written out separately in k_window_summary, k_stream_summary, the PKD branches of k_mc_tile / k_mc_ctile, k_stream_peak_depth_out,
k_stream_total, k_window_exceed / k_stream_exceed and k_window_courant; `>=`, `!(x <= pk)`, fmax or a peak seeded with 0 in any one
of them passes every other test of the suite.  Here the case of tests/nonfinite_cases.py -- rows whose flow, depth and velocity
hold NaN, zeros and bit-equal positive maxima on the edges of tiles, chunks, groups of eight and days, among the slices and among
the cluster tiles; tests/test_nonfinite_cases_cpu.py shows without a GPU that it holds them -- is routed on every kernel that
steps a row, and every product is compared with numpy over THE ORACLE'S values.

THE COMPARISON (``same``): where the expectation is a NaN the device value must be a NaN -- payload and sign are not compared, x86
and the GPU may propagate different NaN bits -- every other value is compared as bits, every step and count exactly."""
import functools

import numpy as np
import pytest

import helpers as H
import nonfinite_cases as N
import test_gpu_window_courant as WC
from oracle import oracle as O
from test_gpu_window_exceedance import KEYS as X_KEYS, QUANTITIES, exceedance_of
from test_gpu_window_summary import PATHS
from troute_amd import _lib
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu

DAY, NDAYS = N.DAY, N.NDAYS
SUM_KEYS = ("peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step")


def same(got, want, what):
    """THE comparison rule of this module (see above)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind in "iu":
        bad = np.argwhere(got != want)
    else:
        nan = np.isnan(want)
        bad = np.argwhere((np.isnan(got) != nan) | (~nan & (N.bits(got) != N.bits(want))))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:6].tolist(), [got[tuple(b)] for b in bad[:6]], [want[tuple(b)] for b in bad[:6]])


def summary_of(fvd):
    """the seven arrays of a window's summary from (q, v, d) [rows, n, 3]: the header's rule, transcribed (nonfinite_cases)"""
    out = {}
    for kf, ks, col in (("peak_flow", "peak_step", 0), ("peak_depth", "peak_depth_step", 2), ("peak_velocity", "peak_velocity_step", 1)):
        out[kf], out[ks] = N.rule_peak(fvd[:, :, col])
    out["mean_flow"] = N.rule_mean(fvd[:, :, 0])
    return out


def assert_summary(got, fvd, what, rows=None):
    want = summary_of(fvd)
    assert set(got) == set(want), (what, sorted(got))
    for k, g in got.items():
        same(g, want[k] if rows is None else want[k][rows], (what, k))
    return want


def fold_days(days, nsteps):
    """the totals of include/trmc.h over per-day dicts: day 0's values, then `if (pk_D > pk)`; the mean of the means left to right"""
    out = {"days": len(days)}
    for kf, ks in (("peak_flow", "peak_step"), ("peak_depth", "peak_depth_step")):
        pk, st = days[0][kf].copy(), days[0][ks].astype(np.int64)
        with np.errstate(invalid="ignore"):
            for D in range(1, len(days)):
                m = days[D][kf] > pk
                pk[m] = days[D][kf][m]
                st[m] = D * nsteps + days[D][ks][m].astype(np.int64)
        out[kf], out[ks] = pk, st
    s = days[0]["mean_flow"].copy()
    for D in range(1, len(days)):
        s = s + days[D]["mean_flow"]
    out["mean_flow"] = s / s.dtype.type(len(days))
    return out


def window_case(precision, nsteps):
    return N.case(nsteps, RoutingPlan.window_summary_tile(precision)[1])


def tile(precision):
    R, C = RoutingPlan.window_summary_tile(precision)
    return R, C, 16 // (precision // 8)


# ---- a. the routing with NaN in it, on every kernel that steps a row ---------------------------------------------------------
CLUSTER_ENGINES = ("levels-clusters", "levels-slices+clusters")
ENGINES = [(s, e) for s, e in H.TABLE_ENGINES] + [(False, e) for _, e in H.TABLE_ENGINES if e and e not in CLUSTER_ENGINES]
ENGINES = sorted(set(ENGINES), key=lambda se: (str(se[1]), se[0]))       # (both timestep modes; a plan in cluster order is a short one)


@pytest.mark.parametrize("short,engine", ENGINES)
def test_the_routing_on_every_engine(short, engine, monkeypatch):
    """helpers.set_engine: the dataflow engine, k_mc_step, k_mc_tile in one and two tiers, k_mc_ctile without and below slices;
    windows of 24 and 3 C + 1 steps: (q, v, d) of every row and step against the oracle"""
    clusters = H.set_engine(engine, monkeypatch)
    net = N.network()[0]
    C = tile(32)[1]
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=short if clusters else None) as p:
        assert not engine or p.engine == "levels"
        for nsteps in (24, 3 * C + 1):
            c = window_case(32, nsteps)
            got = p.route(nsteps, 1, short, c.qlat, c.q0)
            same(got, c.oracle(short), (engine, short, nsteps))
            stats = p.stats()
            if clusters:
                H.cluster_stats(stats, engine, nsteps)
            elif engine in ("levels-wide", "levels-mid") and short:
                assert stats["wide_levels"] > 0 and stats["wide_segment_steps"] > 0, stats


@pytest.mark.parametrize("short", [True, False])
def test_the_routing_in_double_precision(short):
    net = N.network()[0]
    C = tile(64)[1]
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, precision=64, assume_short_ts=short, options=N.OPTIONS if short else None) as p:
        for nsteps in (24, 3 * C + 1):
            c = window_case(64, nsteps)
            got = p.route(nsteps, 1, short, c.qlat.astype(np.float64), c.q0.astype(np.float64))
            assert got.dtype == np.float64
            same(got, c.oracle(short, 64), ("fp64", short, nsteps))


def test_a_window_that_writes_every_fourth_step_aside():
    """set_output_stride on the plan of OPTIONS: the DEC instances of the tile kernels; the block, the planted rows' hydrographs"""
    net = N.network()[0]
    c = window_case(32, 24)
    want = c.oracle(True)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=N.OPTIONS) as p:
        check_layout(p)
        rs = p.rowset(c.planted)
        p.set_output_stride(N.K)
        p.upload_forcing(24, c.qlat, c.q0)
        p.route_device(24, 1, True)
        p.fetch_begin(rs, True, N.K)
        hyd, state, block = (np.array(x, copy=True) for x in p.fetch_wait())
        same(block, np.ascontiguousarray(want[:, N.K - 1::N.K]), "every fourth step")
        same(hyd, np.ascontiguousarray(want[c.planted, :, 0]), "hydrographs of the planted rows")
        same(state, np.ascontiguousarray(np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)), "final state")
        same(p.download_fvd(), want, "the full result beside it")


def check_layout(p):
    """the device plan of OPTIONS keeps as slices and routes in cluster tiles the rows the census counted there"""
    net = N.network()[0]
    blk, _, nb = p.cluster_blocks()
    lag, W, C = p.lags()
    assert W > 0 and C > 0 and nb > 0 and np.array_equal(blk < 0, net.in_slices)


# ---- b. the window products ----------------------------------------------------------------------------------------------------
def courant_of(c, fvd, short):
    """cn [rows, n] of the oracle's single step at the inputs rebuilt from the oracle's window (test_gpu_window_courant)"""
    net = N.network()[0]
    n, T = fvd.shape[:2]
    x = WC.rebuilt_inputs(fvd, c.q0, np.ascontiguousarray(c.qlat[:, :T]), net.params, net.ups, 1, short)
    o = O.segments(x.reshape(-1, 15), det=fvd.dtype == np.float32).reshape(n, T, 6)
    same(np.ascontiguousarray(o[:, :, [0, 2]]), np.ascontiguousarray(fvd[:, :, [0, 2]]), "reconstruction of the step's inputs")
    return np.ascontiguousarray(o[:, :, 4])


@pytest.mark.parametrize("path", [k for k in PATHS if k != "tolerance"])
def test_window_products_on_every_plan_path(path):
    """per way of routing a window (test_gpu_window_summary.PATHS) two windows, nsteps = 3 C + VE (16-byte loads) and 3 C + 1
    (element-wise): the result, the seven arrays of window_summary -- against the oracle and against the window's own
    download_fvd --, a row set, window_exceedance of the three quantities with K = 4, window_courant_summary"""
    cfg = dict(PATHS[path])
    short, precision = cfg.pop("short"), cfg.get("precision", 32)
    R, C, VE = tile(precision)
    net = N.network()[0]
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=short, **cfg) as p:
        assert p.engine == ("flow" if cfg["engine"] == "flow" else "levels")
        if path == "tiles":
            check_layout(p)
        for nsteps in (3 * C + VE, 3 * C + 1):
            c = window_case(precision, nsteps)
            want = c.oracle(short, precision)
            what = (path, nsteps)
            p.route(nsteps, 1, short, c.qlat.astype(p.dtype), c.q0.astype(p.dtype))
            got = p.window_summary()
            fvd = p.download_fvd()
            same(fvd, want, what)
            w = assert_summary(got, want, what + ("oracle",))
            assert_summary(got, fvd, what + ("own result",))
            planted = w["peak_step"][c.planted]
            assert np.isnan(w["peak_flow"]).any() and np.isnan(w["mean_flow"]).sum() > np.isnan(w["peak_flow"]).sum() and planted.max() > C
            rows = np.concatenate([c.planted[::-1], np.arange(0, N.NSEG, 7)])
            rs = p.rowset(rows)
            assert_summary(p.window_summary(rowset=rs), want, what + ("row set",), rows)
            for quantity in QUANTITIES:
                x = np.ascontiguousarray(want[:, :, QUANTITIES.index(quantity)])
                th = N.thresholds(x)
                p.set_thresholds(th)
                ex = exceedance_of(x, th)
                for k, g in p.window_exceedance(quantity).items():
                    same(g, ex[k], what + (quantity, k))
                for k, g in p.window_exceedance(quantity, rowset=rs).items():
                    same(g, ex[k][rows], what + (quantity, k, "row set"))
            cn = courant_of(c, want, short)
            pk, at = N.rule_peak(cn)
            assert np.isnan(pk).any() and (np.isnan(cn).any(axis=1) & ~np.isnan(pk)).any()        # a NaN that stays, NaN that never win
            for limit in (1.0, 0.01):
                s = p.window_courant_summary(limit)
                same(s["peak_cn"], pk, what + ("peak_cn",))
                same(s["peak_cn_step"], at, what + ("peak_cn_step",))
                with np.errstate(invalid="ignore"):
                    over = (cn > cn.dtype.type(limit)).sum(axis=1).astype(np.int32)
                same(s["steps_over"], over, what + ("steps over", limit))
            assert over.max() > 0
            if path == "tiles":
                assert p.stats()["wide_segment_steps"] == p.stats()["nseg_routed"] * nsteps


def test_window_products_in_the_tolerance_arithmetic():
    """the oracle has no say there: the products are the reductions of that window's own download_fvd, NaN and all"""
    cfg = dict(PATHS["tolerance"])
    short = cfg.pop("short")
    R, C, VE = tile(32)
    net = N.network()[0]
    nsteps = 3 * C + 1
    c = window_case(32, nsteps)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=short, **cfg) as p:
        assert p.arithmetic == "tolerance"
        p.route(nsteps, 1, short, c.qlat, c.q0)
        got = p.window_summary()
        fvd = p.download_fvd()
        assert np.array_equal(np.isnan(fvd), np.isnan(c.oracle(short)))                       # (the NaN are where the oracle's are)
        assert_summary(got, fvd, "tolerance")
        x = np.ascontiguousarray(fvd[:, :, 0])
        th = N.thresholds(x)
        p.set_thresholds(th)
        ex = exceedance_of(x, th)
        for k, g in p.window_exceedance("flow").items():
            same(g, ex[k], ("tolerance", k))


# ---- c. the stream of days -----------------------------------------------------------------------------------------------------
def stream_case():
    return N.case(DAY * NDAYS, 32, stream=True)


def plan_stream(p, c, summary=(), full_output=False, output_stride=0, stage=False, exceedance=False):
    """the three days at plan level -> ([dict of copies per day], the totals or None, the exceedance or None, stream_info)"""
    dt, n = p.dtype, p.nseg
    rows = c.planted
    rs = p.rowset(rows)
    p.stream_set_stage(stage)
    p.stream_set_summary(summary or None)
    p.stream_set_exceedance("flow" if exceedance else None)
    p.upload_forcing(DAY, c.day(0).astype(dt), c.q0.astype(dt))
    p.stream_begin(DAY, 1, slots=NDAYS, full_output=full_output, output_stride=output_stride)
    info = p.stream_info()
    assert info["slots"] >= NDAYS
    keep = DAY // output_stride if output_stride else DAY

    def arr(shape, t=dt, on=True):
        return _lib.result_empty(shape, t, always_pinned=True) if on else None
    pk, mn, pd = "peak" in summary, "mean" in summary, "peak_depth" in summary
    ring = [{"peak_flow": arr((n,), on=pk), "peak_step": arr((n,), np.int32, on=pk), "mean_flow": arr((n,), on=mn),
             "peak_depth": arr((n,), on=pd), "peak_depth_step": arr((n,), np.int32, on=pd),
             "stage": arr((rows.shape[0], DAY), on=stage), "hyd": arr((rows.shape[0], DAY)), "final": arr((n, 3)),
             "fvd": arr((n, keep, 3), on=full_output or output_stride)} for _ in range(NDAYS)]
    for d in range(NDAYS):
        r = ring[d]
        sm = tuple(r[k] for k in SUM_KEYS[:5 if pd else 3]) if summary else None
        assert p.stream_push(pinned_like(c.day(d).astype(dt)), rowset=rs, hyd=r["hyd"], q0=r["final"], fvd=r["fvd"], summary=sm,
                             stage=r["stage"]) == d
    p.stream_flush()
    got = []
    for d in range(NDAYS):
        p.stream_wait(d)
        got.append({k: None if v is None else np.array(v, copy=True) for k, v in ring[d].items()})
    total = p.stream_summary_total() if "total" in summary else None
    exc = p.stream_exceedance() if exceedance else None
    p.stream_end()
    p.stream_set_stage(False)
    p.stream_set_exceedance(None)
    return got, total, exc, info


@functools.lru_cache(maxsize=None)
def expected_days(precision=32):
    """per day the oracle's (fvd, state) and the day's summary by the header's rule; the totals: the fold over those summaries"""
    c = stream_case()
    days = c.oracle_days(precision)
    sums = []
    for fvd, _ in days:
        s = summary_of(fvd)
        sums.append({k: s[k] for k in SUM_KEYS})
    return days, sums, fold_days(sums, DAY)


def assert_days(got, c, what, precision=32, depth=True, stage=False):
    days, sums, _ = expected_days(precision)
    for d in range(NDAYS):
        fvd, state = days[d]
        for k in SUM_KEYS[:5 if depth else 3]:
            if got[d][k] is not None:
                same(got[d][k], sums[d][k], (what, d, k))
        same(got[d]["final"], state, (what, d, "the state handed to the next day"))
        same(got[d]["hyd"], np.ascontiguousarray(fvd[c.planted, :, 0]), (what, d, "hydrographs of the planted rows"))
        if stage:
            same(got[d]["stage"], np.ascontiguousarray(fvd[c.planted, :, 2]), (what, d, "stage of the planted rows"))


def classes(c, *names):
    return np.array([r for r in c.planted if c.intended[r] in names])


def test_stream_days_products_only_and_with_the_full_result():
    """three days on the plan of OPTIONS: a products-only stream -- k_mc_tile_pkd and k_mc_ctile_pkd carry the peak depth from
    launch to launch, k_stream_summary reduces the flow plane, k_stream_total folds --, the same with stage hydrographs, and a
    full_output stream (k_stream_peak_depth_out); each against the oracle day by day, and the two peak depths against each other"""
    net = N.network()[0]
    c = stream_case()
    parts = ("peak", "mean", "peak_depth", "total")
    days, sums, fold = expected_days()
    F, G = classes(c, "F"), classes(c, "G")
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=N.OPTIONS) as p:
        check_layout(p)
        lean, total, _, info = plan_stream(p, c, parts)
        assert info["wide_levels"] > 0 and info["cluster_levels"] > 0 and info["tiles_per_day"] == DAY // N.K    # both carrying kernels ran
        assert_days(lean, c, "products only")
        staged, total_s, _, _ = plan_stream(p, c, parts, stage=True)
        assert_days(staged, c, "with stage", stage=True)
        assert np.isnan(staged[1]["stage"]).any()
        full, total_f, _, _ = plan_stream(p, c, parts, full_output=True)
        assert_days(full, c, "full_output")
        for d in range(NDAYS):
            same(full[d]["fvd"], days[d][0], ("full_output", d, "every (q, v, d)"))
            for k in ("peak_depth", "peak_depth_step"):
                same(lean[d][k], full[d][k], (d, k, "carried against reduced"))
        for name, t in (("products only", total), ("with stage", total_s), ("full_output", total_f)):
            assert t["days"] == NDAYS
            for k in SUM_KEYS:
                same(t[k], fold[k], (name, "total", k))
        # what the classes are there for, on the oracle's fold: F keeps day 0, G stays NaN at step 1, the mean of means is NaN
        for kf, ks in (("peak_flow", "peak_step"), ("peak_depth", "peak_depth_step")):
            assert np.isfinite(fold[kf][F]).all() and np.all(fold[ks][F] <= DAY) and np.array_equal(fold[ks][F], sums[0][ks][F])
            assert np.isnan(fold[kf][G]).all() and np.all(fold[ks][G] == 1)
        any_nan = np.isnan(np.stack([s["mean_flow"] for s in sums])).any(axis=0)
        assert np.array_equal(np.isnan(fold["mean_flow"]), any_nan) and any_nan[F].all() and any_nan[G].all()
        assert (fold["peak_step"] > DAY).any()


def test_stream_days_with_lazily_formed_velocities():
    """a stream that keeps every fourth step and no full result: the LAZYV instances form a velocity at the kept steps only, from
    `it_last > 0` -- the kept (q, v, d) against the oracle, NaN velocities included"""
    net = N.network()[0]
    c = stream_case()
    days = c.oracle_days()
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=N.OPTIONS) as p:
        got, _, _, _ = plan_stream(p, c, ("peak", "peak_depth"), output_stride=N.K)
        assert_days(got, c, "output_stride")
        for d in range(NDAYS):
            kept = np.ascontiguousarray(days[d][0][:, N.K - 1::N.K])
            same(got[d]["fvd"], kept, ("output_stride", d))
        assert np.isnan(np.concatenate([days[d][0][:, N.K - 1::N.K, 1] for d in range(NDAYS)], axis=1)).any()


def test_stream_days_in_double_precision():
    net = N.network()[0]
    c = stream_case()
    _, _, fold = expected_days(64)
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", precision=64, options=N.OPTIONS) as p:
        got, total, _, _ = plan_stream(p, c, ("peak", "mean", "peak_depth", "total"))
        assert_days(got, c, "fp64", precision=64)
        for k in SUM_KEYS:
            same(total[k], fold[k], ("fp64 total", k))


def test_stream_exceedance_with_nan_on_a_days_edge():
    """k_stream_exceed over the three days against the loop of test_gpu_window_exceedance over the oracle's flows in a row: a NaN
    on a day's last step and on the next day's first breaks a run the days would otherwise share"""
    net = N.network()[0]
    c = stream_case()
    x = np.ascontiguousarray(np.concatenate([f[:, :, 0] for f, _ in c.oracle_days()], axis=1))
    th = N.thresholds(x)
    want = exceedance_of(x, th)
    _, _, (last, first) = N.nan_in_runs(x, th, DAY)
    assert last >= 2 and first >= 2
    with RoutingPlan(net.up_ptr, net.up_idx, net.params, assume_short_ts=True, engine="levels", options=N.OPTIONS) as p:
        p.set_thresholds(th)
        _, _, got, _ = plan_stream(p, c, exceedance=True)
    assert got["days"] == NDAYS
    for k in X_KEYS:
        same(got[k], want[k].astype(np.int64), ("stream exceedance", k))


def test_routestream_total_is_the_fold_and_not_numpy_maximum():
    """RouteStream(summary=("peak", "mean", "peak_depth", "total")): the days and the totals against the oracle; rs.total's peak
    differs from np.maximum.reduce of the days' peaks exactly where a day's peak is NaN (np.maximum propagates it, the fold does
    not take it) -- np.fmax or the fold itself is the recipe there"""
    net = N.network()[0]
    c = stream_case()
    days, sums, fold = expected_days()
    r = ShardedRouter(net.to, net.params, stream=True, options=N.OPTIONS)
    items = []
    with RouteStream(r, DAY, 1, summary=("peak", "mean", "peak_depth", "total")) as rs:
        for item in rs.route(iter([c.day(d) for d in range(NDAYS)]), c.q0):
            items.append(tuple({k: np.array(v, copy=True) for k, v in x.items()} if isinstance(x, dict) else
                               (x if x is None or np.isscalar(x) else np.array(x, copy=True)) for x in item))
        total = {k: (v if k == "days" else np.array(v, copy=True)) for k, v in rs.total.items()}
        outlets = np.array(rs.outlet_rows, copy=True)
    r.close()
    assert [i[0] for i in items] == list(range(NDAYS)) and total["days"] == NDAYS
    for d, item in enumerate(items):
        same(item[1], np.ascontiguousarray(days[d][0][outlets, :, 0]), (d, "outlet hydrographs"))
        same(item[2], days[d][1], (d, "final state"))
        for k in SUM_KEYS:
            same(item[3][k], sums[d][k], (d, k))
    for k in SUM_KEYS:
        same(total[k], fold[k], ("rs.total", k))
    pk = np.stack([item[3]["peak_flow"] for item in items])
    recipe = np.maximum.reduce(pk)
    a_day_is_nan = np.isnan(pk).any(axis=0)
    differs = ~((np.isnan(recipe) & np.isnan(total["peak_flow"])) | (N.bits(recipe) == N.bits(total["peak_flow"])))
    keeps_a_number = a_day_is_nan & ~np.isnan(pk[0])                                     # (a NaN on day 0 stays in both)
    assert np.array_equal(recipe != total["peak_flow"], a_day_is_nan)                    # (numpy's !=: a NaN differs from everything)
    assert np.array_equal(differs, keeps_a_number) and differs.sum() >= 8 and not differs[~a_day_is_nan].any()
    same(np.fmax.reduce(pk)[~np.isnan(pk[0])], total["peak_flow"][~np.isnan(pk[0])], "np.fmax where day 0 holds a number")
