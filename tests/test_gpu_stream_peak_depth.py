"""THE PEAK DEPTH OF A DAY AND THE TOTALS OVER THE DAYS OF A STREAM (include/trmc.h TRMC_SUMMARY_PEAK_DEPTH, TRMC_SUMMARY_TOTAL,
trmc_stream_summary_depth_dest, trmc_stream_summary_total; csrc/stream.inc, k_mc_tile_pkd / k_mc_ctile_pkd, k_stream_peak_depth,
k_stream_total).

The depths of a day are out[row][step][2] of its result; a stream that assembles no full result keeps only the depth of a tile's
last step, so the tile kernels carry the row's (peak, step) from tile to tile.  Everything is exact and compares bits:
``peak_of`` is peak_flow's rule (peak = d[1], step = 1, then ``if d[t] > peak``: the first of equal peaks wins), the totals are
folds of the days' arrays (``fold_days``).  Boundary copies of a rank are routed by nobody: (0, 1), what its own full result
holds there.  The NaN rule -- of the carried peak depth, of the reduced one and of the totals' fold -- is tested in
tests/test_gpu_products_nonfinite.py: no depth of the days routed here is a NaN."""
import os
import threading

import numpy as np
import pytest

import test_gpu_stream_summary as SS
from oracle import oracle as O
from troute_amd import _lib
from troute_amd.comm import Comm
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu
bits, copied = SS.bits, SS.copied
NSEG, NSTEPS, QTS, OPTIONS = SS.NSEG, SS.NSTEPS, SS.QTS, SS.OPTIONS
K = OPTIONS["wide_k"]
_serial = [0]


def peak_of(d):
    """(peak, step) of d [rows, nsteps] as include/trmc.h defines them"""
    d = np.ascontiguousarray(d)
    peak, step = d[:, 0].copy(), np.ones(d.shape[0], np.int32)
    for t in range(1, d.shape[1]):
        m = d[:, t] > peak
        peak[m] = d[m, t]
        step[m] = t + 1
    return peak, step


def fold_days(days, nsteps):
    """the totals of include/trmc.h over per-day dicts (peak_flow, peak_step, mean_flow, peak_depth, peak_depth_step; any absent)"""
    out = {"days": len(days)}
    for kf, ks in (("peak_flow", "peak_step"), ("peak_depth", "peak_depth_step")):
        if days[0].get(kf) is None:
            continue
        pk, st = days[0][kf].copy(), days[0][ks].astype(np.int64)
        for D in range(1, len(days)):
            m = days[D][kf] > pk
            pk[m] = days[D][kf][m]
            st[m] = D * nsteps + days[D][ks][m].astype(np.int64)
        out[kf], out[ks] = pk, st
    if days[0].get("mean_flow") is not None:
        s = days[0]["mean_flow"].copy()
        for D in range(1, len(days)):
            s = s + days[D]["mean_flow"]
        out["mean_flow"] = s / s.dtype.type(len(days))
        assert out["mean_flow"].dtype == s.dtype
    return out


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = (got, want) if got.dtype.kind == "i" else (bits(got), bits(want))
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def assert_total(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    assert got["days"] == want["days"], what
    for k in want:
        if k != "days":
            assert got[k].dtype == (np.int64 if k.endswith("step") else want[k].dtype), (what, k)
            assert_same(got[k], want[k], (what, k))


SUM_KEYS = ("peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step")


def plan_stream(p, qlat, q0, ndays, summary, full_output=False, output_stride=0, mid_total=()):
    """the days of a stream at plan level -> [dict of copies per day] (the summary's parts, "final", "fvd"), the stream's info and
    {days pushed: the totals fetched after a flush at that point}; the ring is reused when ndays exceeds the slots"""
    dt = p.dtype
    p.stream_set_summary(summary)
    p.upload_forcing(NSTEPS, SS.day_of(qlat, 0, dt), q0.astype(dt))
    p.stream_begin(NSTEPS, QTS, full_output=full_output, output_stride=output_stride)
    info = p.stream_info()
    D = info["slots"]
    want = set(summary or ())
    keep = NSTEPS // output_stride if output_stride else NSTEPS

    def arr(on, t):
        return _lib.result_empty((NSEG,), t, always_pinned=True) if on else None
    ring = [{"peak_flow": arr("peak" in want, dt), "peak_step": arr("peak" in want, np.int32), "mean_flow": arr("mean" in want, dt),
             "peak_depth": arr("peak_depth" in want, dt), "peak_depth_step": arr("peak_depth" in want, np.int32),
             "final": _lib.result_empty((NSEG, 3), dt, always_pinned=True),
             "fvd": _lib.result_empty((NSEG, keep, 3), dt, always_pinned=True) if (full_output or output_stride) else None} for _ in range(D)]
    got, totals = [], {}

    def take(d):
        p.stream_wait(d)
        got.append(copied(ring[d % D]))
    for d in range(ndays):
        if d >= D:
            if p.stream_info()["days_complete"] <= d - D:
                p.stream_flush()
            take(d - D)
        r = ring[d % D]
        sm = tuple(r[k] for k in SUM_KEYS[:5 if "peak_depth" in want else 3]) if want else None
        assert p.stream_push(pinned_like(SS.day_of(qlat, d, dt)), q0=r["final"], fvd=r["fvd"], summary=sm) == d
        if d + 1 in mid_total:
            p.stream_flush()
            assert p.stream_info()["days_complete"] == d + 1
            totals[d + 1] = p.stream_summary_total()
    p.stream_flush()
    for d in range(len(got), ndays):
        take(d)
    p.stream_end()
    return got, info, totals


# ---- 1. the carry over tiles and over a reused ring ---------------------------------------------------------------------------
def test_peak_depth_against_the_oracle_over_a_reused_ring():
    """a products-only stream of 2 * slots + 1 days whose forcing falls and rises: a slot's day is smaller than its last occupant
    (a carry that was not started over would keep the old peak), rows of two days share a launch, both tile kernels carry"""
    up_ptr, up_idx, params, qlat, q0, dry = SS.plan_case()
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=OPTIONS) as p:
        lvl, _ = p.levels()
        lag, W, C = p.lags()
        p.stream_set_summary(("peak_depth",))
        p.upload_forcing(NSTEPS, SS.day_of(qlat, 0), q0)
        p.stream_begin(NSTEPS, QTS)
        info = p.stream_info()
        p.stream_end()
        assert W > 0 and C > 0 and lag.max() > info["tiles_per_day"] == 6
        ndays = 2 * info["slots"] + 1
        got, _, _ = plan_stream(p, qlat, q0, ndays, ("peak_depth",))
    state, steps = q0, []
    for d in range(ndays):
        want = O.network_by_segment(NSTEPS, QTS, up_ptr, up_idx, lvl, params, state, SS.day_of(qlat, d), True, det=True)[:, 1:, :]
        pk, st = peak_of(want[:, :, 2])
        assert_same(got[d]["peak_depth"], pk, ("oracle", d, "peak_depth"))
        assert_same(got[d]["peak_depth_step"], st, ("oracle", d, "peak_depth_step"))
        state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
        assert_same(got[d]["final"], state, ("oracle", d, "final state"))
        assert not want[dry, :, 2].any()
        assert not got[d]["peak_depth"][dry].any() and np.all(got[d]["peak_depth_step"][dry] == 1)        # no flow: (0, 1)
        steps.append(got[d]["peak_depth_step"])
    steps = np.concatenate(steps)
    assert steps.min() == 1 and steps.max() == NSTEPS and (steps == 1).sum() > len(dry) * ndays
    assert np.any((steps > 1) & (steps <= NSTEPS - K))                  # (inside the day, outside its last tile)
    assert len(set(((steps - 1) // K).tolist())) > 2                    # (not all in one tile)


# ---- 2. precisions, arithmetics, the three kinds of stream -------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fp32", "fp64", "tolerance"])
def test_peak_depth_of_the_full_result_and_of_the_carrying_streams(variant):
    up_ptr, up_idx, params, qlat, q0, dry = SS.plan_case()
    precision = 64 if variant == "fp64" else 32
    opts = dict(OPTIONS, **({"arithmetic": "tolerance"} if variant == "tolerance" else {}))
    ndays, stride = 3, 6
    parts = ("peak", "mean", "peak_depth")
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", precision=precision, options=opts) as p:
        assert np.dtype(p.dtype).itemsize == precision // 8
        full, info, _ = plan_stream(p, qlat, q0, ndays, parts, full_output=True)
        assert info["slots"] >= ndays
        lazy, _, _ = plan_stream(p, qlat, q0, ndays, parts)
        lazy0, _, _ = plan_stream(p, qlat, q0, ndays, parts[:2])
        dec, _, _ = plan_stream(p, qlat, q0, ndays, parts, output_stride=stride)
        dec0, _, _ = plan_stream(p, qlat, q0, ndays, parts[:2], output_stride=stride)
    for d in range(ndays):
        f = full[d]
        assert np.isfinite(f["fvd"]).all() and f["fvd"][:, :, 2].max() > 0
        pk, st = peak_of(f["fvd"][:, :, 2])                              # the stream's own full result
        assert_same(f["peak_depth"], pk, (variant, d, "full"))
        assert_same(f["peak_depth_step"], st, (variant, d, "full step"))
        SS.assert_summary([f[k] for k in SS.KEYS], f["fvd"][:, :, 0], (variant, d))
        for name, run, twin in (("products only", lazy, lazy0), ("output_stride", dec, dec0)):
            assert_same(run[d]["peak_depth"], f["peak_depth"], (variant, d, name))
            assert_same(run[d]["peak_depth_step"], f["peak_depth_step"], (variant, d, name))
            assert twin[d]["peak_depth"] is None
            for k in SS.KEYS + ("final",):                               # the other products: those of a stream without the part
                assert_same(run[d][k], twin[d][k], (variant, d, name, k))
                assert_same(run[d][k], f[k], (variant, d, name, k, "full"))
        assert_same(dec[d]["fvd"], dec0[d]["fvd"], (variant, d, "kept steps"))
        assert_same(dec[d]["fvd"], np.ascontiguousarray(f["fvd"][:, stride - 1::stride]), (variant, d, "kept steps of the full result"))


# ---- 3. reservoirs and gages; reservoir data assimilation is refused ---------------------------------------------------------
def test_peak_depth_with_reservoirs_and_gages():
    """at a reservoir row the pool's water elevation, at a gage row the channel depth (nudging changes the flow only)"""
    import test_gpu_stream_reservoirs_nudging as RN
    c = RN.case(3000, 78, 4)
    r = ShardedRouter(c.to, c.params, stream=True, options=RN.OPTIONS, reservoirs=(c.lakes, c.par, RN.DT), gages=c.gages)
    runs = {}
    for full in (True, False):
        days = []
        with RouteStream(r, RN.NSTEPS, RN.QTS, full_output=full, summary=("peak", "peak_depth")) as rs:
            for item in rs.route(iter(c.days), c.q0, observations=iter(c.usgs), lastobs=(c.lv0, c.lt0),
                                 da_parameters={"da_decay_coefficient": RN.DECAY, "routing_period": RN.DT}):
                assert len(item) == (5 if full else 4)
                assert set(item[-1]) == {"reservoir_inflow", "nudge", "lastobs", "peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step"}
                days.append(copied(item))
        runs[full] = days
    assert len(runs[True]) == len(runs[False]) == len(c.days) == 4
    for w, (f, l) in enumerate(zip(runs[True], runs[False])):
        d = f[3][:, :, 2]
        pk, st = peak_of(d)
        for rows, what in ((slice(None), "all rows"), (c.lakes, "reservoir rows"), (c.gages, "gage rows")):
            for run, name in ((f, "full"), (l, "products only")):
                assert_same(run[-1]["peak_depth"][rows], pk[rows], (w, what, name))
                assert_same(run[-1]["peak_depth_step"][rows], st[rows], (w, what, name, "step"))
        assert np.all(pk[c.lakes] == d[c.lakes].max(axis=1)) and pk[c.lakes].min() > 0        # (the pools' elevations)
        assert np.abs(f[-1]["nudge"]).max() > 0
        assert_same(l[-1]["peak_flow"], f[-1]["peak_flow"], (w, "peak_flow"))
        assert_same(l[2], f[2], (w, "final state"))
    r.close()


def test_peak_depth_is_refused_with_reservoir_data_assimilation():
    import test_gpu_stream_reservoir_da as RD
    c = RD.case()
    with RD.open_plan(c, True, 4) as p:
        RD.declare(p, c)
        p.stream_set_summary(("peak", "peak_depth"))
        p.upload_forcing(RD.NSTEPS, c.days[0], c.q0)
        with pytest.raises(NotImplementedError, match="peak depth.*reservoir data assimilation"):
            p.stream_begin(RD.NSTEPS, c.qts, reservoir_da=True)
        assert p.stream_info()["days_pushed"] == 0
        with pytest.raises(RuntimeError, match="no stream of windows in progress"):           # (no day can be pushed: nothing began)
            p.stream_push(pinned_like(c.days[0]), reservoir_da=RD.day_tables(c, 0))
        p.stream_set_summary(("peak",))                                                       # (the other parts are carried by nobody)
        p.stream_begin(RD.NSTEPS, c.qts, reservoir_da=True)
        p.stream_end()


# ---- 4. the totals -----------------------------------------------------------------------------------------------------------
def route_rs(r, days, q0, nsteps, qts, **kw):
    with RouteStream(r, nsteps, qts, **kw) as rs:
        items = [copied(item) for item in rs.route(iter(days), q0)]
        total = copied(rs.total) if rs.total is not None else None
        if total is not None:
            total["days"] = rs.total["days"]
        rows = np.array(rs.rows, copy=True)
        bnd = np.array(rs.plan.levels()[0]) < 0
    return items, total, rows, bnd


def test_routestream_totals_are_the_fold_of_the_days():
    net, q0, days = SS.rs_case()
    nseg = net["to"].shape[0]
    parts = ("peak", "mean", "peak_depth", "total")
    r = ShardedRouter(net["to"], net["params"], stream=True, options=SS.RS_OPTS)
    items, total, rows, _ = route_rs(r, days, q0, SS.RS_NSTEPS, SS.RS_QTS, summary=parts)
    assert np.array_equal(rows, np.arange(nseg)) and [len(i) for i in items] == [4] * SS.RS_DAYS
    assert all(set(i[3]) == set(SUM_KEYS) for i in items)
    want = fold_days([i[3] for i in items], SS.RS_NSTEPS)
    assert want["days"] == SS.RS_DAYS
    assert_total(total, want, "RouteStream")
    # against everything the days held: a full_output twin, all steps of all days in a row
    full, none, _, _ = route_rs(r, days, q0, SS.RS_NSTEPS, SS.RS_QTS, full_output=True)
    assert none is None
    for c, kf, ks in ((0, "peak_flow", "peak_step"), (2, "peak_depth", "peak_depth_step")):
        x = np.concatenate([f[3][:, :, c] for f in full], axis=1)
        assert np.array_equal(x.argmax(axis=1), total[ks] - 1), kf
        assert_same(total[kf], x.max(axis=1), kf)
    assert np.unique(total["peak_step"] // SS.RS_NSTEPS).size > 1           # (the winning day differs from row to row)
    # the totals alone: the tuples of summary=None, the same totals
    lean, total2, _, _ = route_rs(r, days, q0, SS.RS_NSTEPS, SS.RS_QTS, summary=parts, daily_summary=False)
    assert [len(i) for i in lean] == [3] * SS.RS_DAYS
    assert_total(total2, want, "daily_summary=False")
    for w in range(SS.RS_DAYS):
        assert_same(lean[w][2], items[w][2], (w, "final state"))
        assert_same(lean[w][1], items[w][1], (w, "hydrographs"))
    # the keys of today's summary stay what they were
    three, t3, _, _ = route_rs(r, days[:2], q0, SS.RS_NSTEPS, SS.RS_QTS, summary=("peak", "mean"))
    assert t3 is None and all(set(i[3]) == set(SS.KEYS) for i in three)
    with pytest.raises(ValueError, match="total"):
        RouteStream(r, SS.RS_NSTEPS, SS.RS_QTS, summary=("total",))
    with pytest.raises(ValueError, match="daily_summary"):
        RouteStream(r, SS.RS_NSTEPS, SS.RS_QTS, summary=("peak",), daily_summary=False)
    r.close()


def test_totals_fetched_mid_stream_after_a_flush():
    up_ptr, up_idx, params, qlat, q0, dry = SS.plan_case()
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=OPTIONS) as p:
        got, info, totals = plan_stream(p, qlat, q0, 5, ("peak", "mean", "peak_depth", "total"), mid_total=(2, 5))
    assert sorted(totals) == [2, 5]
    for n, t in totals.items():
        assert t["days"] == n
        assert_total(t, fold_days(got[:n], NSTEPS), ("mid-stream", n))
    assert not np.array_equal(totals[2]["peak_step"], totals[5]["peak_step"])


# ---- 5. two ranks on one GPU -------------------------------------------------------------------------------------------------
def test_peak_depth_and_totals_on_two_ranks():
    """two ranks (threads) on one device over the shared-memory transport: at the rows a rank routes the single-GPU values; at
    its boundary copies -- routed by nobody -- what its own full result holds: no depth, (0, 1)"""
    net, q0, days = SS.rs_case()
    nseg = net["to"].shape[0]
    nsteps, qts, ndays = 32, 16, 4
    days = days[:ndays]
    parts = ("peak", "peak_depth", "total")
    r = ShardedRouter(net["to"], net["params"], stream=True, options=SS.RS_OPTS)
    single, stotal, rows, _ = route_rs(r, days, q0, nsteps, qts, summary=parts)
    r.close()
    assert np.array_equal(rows, np.arange(nseg))
    world = 2
    _serial[0] += 1
    key = f"peakdepth{os.getpid()}_{_serial[0]}"
    results, errors = [None] * world, []

    def run(rank):
        try:
            comm = Comm(rank, world, device=0, backend="shm", key=key)
            rr = ShardedRouter(net["to"], net["params"], rank=rank, world=world, device=0, stream=True, options=SS.RS_OPTS)
            rr.enable_device_exchange(comm)
            lean = route_rs(rr, days, q0, nsteps, qts, summary=parts)
            full = route_rs(rr, days, q0, nsteps, qts, summary=("peak_depth",), full_output=True)
            results[rank] = (lean, full, rr.plan1 is not None)
            rr.close()
            comm.close()
        except Exception as e:                          # pragma: no cover
            import traceback
            traceback.print_exc()
            errors.append(e)
    ts = [threading.Thread(target=run, args=(k,)) for k in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    assert results[0][2] or results[1][2]               # one of them owns a trunk
    nbnd = 0
    for rank in range(world):
        (got, total, srows, bnd), (full, _, frows, fbnd), _ = results[rank]
        assert np.array_equal(srows, frows) and np.array_equal(bnd, fbnd) and bnd.shape == srows.shape
        routed = ~bnd
        nbnd += int(bnd.sum())
        for w in range(ndays):
            sm = got[w][3]
            assert set(sm) == {"peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step"} and sm["mean_flow"] is None
            for k in ("peak_depth", "peak_depth_step", "peak_flow", "peak_step"):
                assert_same(sm[k][routed], single[w][3][k][srows][routed], (rank, w, k))
            fvd = full[w][3][0] if isinstance(full[w][3], tuple) else full[w][3]
            pk, st = peak_of(fvd[:, :, 2])                # the rank's own full result, boundary copies included
            assert_same(sm["peak_depth"], pk, (rank, w, "own full result"))
            assert_same(sm["peak_depth_step"], st, (rank, w, "own full result, step"))
            assert_same(full[w][-1]["peak_depth"], pk, (rank, w, "full_output stream"))
            assert not sm["peak_depth"][bnd].any() and np.all(sm["peak_depth_step"][bnd] == 1)
        assert total["days"] == ndays
        for k in ("peak_depth", "peak_depth_step", "peak_flow", "peak_step"):
            assert_same(total[k][routed], stotal[k][srows][routed], (rank, "total", k))
        assert_total(total, fold_days([g[3] for g in got], nsteps), (rank, "fold"))
    assert nbnd > 0                                     # (the trunk's owner holds boundary copies of the cut rows)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_peak_depth_and_total_refusals():
    up_ptr, up_idx, params, qlat, q0, dry = SS.plan_case()
    day = pinned_like(SS.day_of(qlat, 0))

    def f32():
        return _lib.result_empty((NSEG,), np.float32, always_pinned=True)

    def i32():
        return _lib.result_empty((NSEG,), np.int32, always_pinned=True)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=OPTIONS) as p:
        with pytest.raises(ValueError, match="TRMC_SUMMARY_TOTAL needs at least one"):
            p.stream_set_summary(("total",))
        with pytest.raises(ValueError, match="'peak' and / or 'mean'"):
            p.stream_set_summary(("peak", "velocity"))
        # a stream begun without the bit takes no peak-depth arrays; the refused push leaves nothing behind
        p.stream_set_summary(("peak",))
        p.upload_forcing(NSTEPS, day, q0)
        p.stream_begin(NSTEPS, QTS)
        pk, st = f32(), i32()
        st[...] = -7
        with pytest.raises(RuntimeError, match="begun without TRMC_SUMMARY_PEAK_DEPTH"):
            p.stream_push(day, summary=(pk, st, None, f32(), i32()))
        assert p.stream_info()["days_pushed"] == 0
        with pytest.raises(ValueError, match="peak_depth_step"):
            p.stream_push(day, summary=(pk, st, None, f32(), f32()))
        with pytest.raises(RuntimeError, match="begun without TRMC_SUMMARY_TOTAL"):
            p.stream_summary_total()
        assert p.stream_push(day) == 0                       # (the refused push's arrays do not wait for this day)
        p.stream_flush()
        p.stream_wait(0)
        assert np.all(st == -7)
        p.stream_end()
        with pytest.raises(RuntimeError, match="no stream of windows in progress"):
            p.stream_summary_total()
        # the totals before any day is complete, and an array whose part is off
        p.stream_set_summary(("peak", "total"))
        p.upload_forcing(NSTEPS, day, q0)
        p.stream_begin(NSTEPS, QTS)
        with pytest.raises(RuntimeError, match="no day of the stream is complete"):
            p.stream_summary_total()
        assert p.stream_push(day) == 0 and p.stream_info()["days_complete"] == 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete"):
            p.stream_summary_total()
        p.stream_flush()
        t = p.stream_summary_total()
        assert t["days"] == 1 and set(t) == {"days", "peak_flow", "peak_step"} and t["peak_step"].dtype == np.int64
        x = np.zeros(NSEG, np.float32)
        assert _lib.lib().trmc_stream_summary_total(p._h, None, None, None, _lib.ptr(x), None, None) == _lib.TRMC_EINVAL
        assert _lib.lib().trmc_stream_summary_total(p._h, None, None, _lib.ptr(x), None, None, None) == _lib.TRMC_EINVAL
        p.stream_end()
    # without full_output the part rides in the on-demand-velocity instances: not on a plan that switched them off
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=dict(OPTIONS, velocity_on_demand=-1)) as p:
        p.stream_set_summary(("peak_depth",))
        p.upload_forcing(NSTEPS, day, q0)
        with pytest.raises(NotImplementedError, match="velocity_on_demand"):
            p.stream_begin(NSTEPS, QTS)
        p.stream_begin(NSTEPS, QTS, full_output=True)        # (the full result is reduced instead)
        p.stream_end()
