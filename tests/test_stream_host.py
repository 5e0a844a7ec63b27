"""The host half of a stream of days without a GPU: the parts ``troute_amd.sequence.RouteStream.route`` is made of -- ring
sizing, the gages' last observations, the reservoir-DA state tuples -- on their own, the summary path through the oracle-backed
stand-in for the plan, and when ``latency='low'`` is refused."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from troute_amd import sequence as S                           # noqa: E402
from troute_amd import stream_products as SP                   # noqa: E402
from troute_amd.routing.fast_reach import simple_da            # noqa: E402


# ---- ring sizing: the values the expressions of the single generator gave ------------------------------------------------
@pytest.mark.parametrize("lmax_mine, lmax_all, want_fvd, want", [
    (0, None, False, (0, 1, 3)),
    (0, None, True, (4, 2, 3)),
    (3, None, True, (4, 3, 4)),
    (4, None, True, (5, 3, 4)),
    (5, None, True, (5, 4, 5)),
    (8, 8, False, (5, 3, 4)),
    (2, 8, False, (5, 3, 4)),          # (a rank whose own rows lag less: the furthest rank's lag decides)
    (8, 8, True, (6, 4, 5)),
])
def test_ring_sizes(lmax_mine, lmax_all, want_fvd, want):
    assert S.ring_sizes(lmax_mine, lmax_all, 4, want_fvd, False, 0) == want


def test_ring_sizes_low_latency_and_slots_asked():
    slots, behind, ring = S.ring_sizes(5, None, 4, True, True, 0)
    assert (behind, ring) == (0, 3) and slots == 5
    assert S.ring_sizes(5, None, 4, True, False, 9) == (9, 4, 5)
    assert S.ring_sizes(8, 8, 4, True, False, 9) == (9, 4, 5)
    assert [S.days_spanned(lag, 4) for lag in (0, 1, 4, 5, 8, 9)] == [0, 1, 1, 2, 2, 3]


# ---- the product table ---------------------------------------------------------------------------------------------------
def test_product_table_follows_the_device_table_and_builds_the_push_keywords():
    """one row per enumerator of csrc/stream.inc's P_*, in its order; a slot's arrays go under stream_push's keywords, a summary
    tuple as long as one of the library's two calls takes"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "t-route_amd", "csrc", "stream.inc")).read()
    body = src[src.index("enum : int {"):src.index("P_N\n")]
    enumerators = [ln.split(",")[0].strip() for ln in body.splitlines()[1:] if ln.strip().startswith("P_")]
    assert len(enumerators) == len(SP.PRODUCTS) == 12
    assert [p.name for p in SP.PRODUCTS[:3]] == ["hyd", "q0", "fvd"] and enumerators[:3] == ["P_HYD", "P_Q0", "P_FVD"]
    assert [e for e in enumerators[7:]] == ["P_PEAK", "P_STEP", "P_MEAN", "P_PD", "P_PDS"] and SP.SUMMARY == SP.PRODUCTS[7:]
    a = {p.name: np.zeros(1) for p in SP.PRODUCTS}
    assert set(SP.push_keywords(a)) == {"hyd", "q0", "fvd", "nudge", "reservoir_inflow", "reservoir_da_state", "summary"}
    assert len(SP.push_keywords(a)["summary"]) == 5 and len(SP.push_keywords(a)["reservoir_da_state"]) == 2
    mean_only = SP.push_keywords({"hyd": a["hyd"], "q0": a["q0"], "mean_flow": a["mean_flow"]})
    assert set(mean_only) == {"hyd", "q0", "summary"} and mean_only["summary"] == (None, None, a["mean_flow"])
    peak_only = SP.push_keywords({"peak_flow": a["peak_flow"], "peak_step": a["peak_step"]})["summary"]
    assert peak_only == (a["peak_flow"], a["peak_step"], None)
    depth_only = SP.push_keywords({"peak_depth": a["peak_depth"], "peak_depth_step": a["peak_depth_step"]})["summary"]
    assert depth_only == (None, None, None, a["peak_depth"], a["peak_depth_step"])
    assert [p.name for p in SP.RECORDS] == ["reservoir_inflow", "nudge"]
    assert SP.SUMMARY_WRONG == "summary must be (peak_flow, peak_step, mean_flow[, peak_depth, peak_depth_step]); any may be None"


# ---- reservoir-DA carry --------------------------------------------------------------------------------------------------
def test_reservoir_da_carry():
    """two usgs rows, one usace row, two rfc rows; usgs row 1 and rfc row 0 belong to no reservoir: they pass through, their times
    less the day's length"""
    nsteps, period = 4, 300.0
    day_len = np.float32(1200.0)
    kind = np.array([2, 3, 4, 1], np.int32)                    # (the last reservoir: level pool, no table)
    table_row = np.array([0, 0, 1, 0], np.int32)
    usgs_state = np.array([[100.0, 1.5, 3, 50.0], [7000.25, 2.5, 4, 60.5]], np.float32)
    usace_state = np.array([[300.0, 3.5, 5, 70.0]], np.float32)
    rfc_time = np.array([5000.5, 900.0], np.float32)
    rfc_ipar = np.array([[2, 6, 0, 3600, 10], [3, 6, 0, 3600, 10]], np.int32)
    rda = (kind, table_row, (np.zeros((2, 3), np.float32), np.zeros(3, np.float32), usgs_state),
           (np.zeros((1, 3), np.float32), np.zeros(3, np.float32), usace_state), (np.zeros((2, 6), np.float32), rfc_time, rfc_ipar),
           [np.array([11, 12]), np.array([21]), np.array([31, 32])])
    carry = S.ReservoirDaCarry(rda, nsteps, period)
    state = np.array([[-1100.0, 9.5, 1, -1150.0], [-900.0, 8.5, 2, -950.0], [2400.0, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    tsidx = np.array([0, 0, 7, 0], np.int32)
    usgs, usace, rfc = carry.tuples(state, tsidx)
    assert [x.tolist() for x in (usgs[0], usace[0], rfc[0])] == [[11, 12], [21], [31, 32]]
    # the used rows hold the device's values
    assert [float(x[0]) for x in usgs[1:]] == state[0].tolist() and [float(x[0]) for x in usace[1:]] == state[1].tolist()
    assert float(rfc[1][1]) == 2400.0 and int(rfc[2][1]) == 7
    # the unused rows: the times a day less, in float32; everything else as it was
    assert usgs[1][1] == np.float32(7000.25) - day_len and usgs[4][1] == np.float32(60.5) - day_len
    assert usgs[2][1] == np.float32(2.5) and usgs[3][1] == np.float32(4)
    assert rfc[1][0] == np.float32(5000.5) - day_len and int(rfc[2][0]) == 2
    assert all(x.dtype == np.float32 for x in usgs[1:] + usace[1:] + rfc[1:2]) and rfc[2].dtype == np.int32 and usgs[0].dtype == np.int32
    # what was returned is the caller's: spoiling it changes nothing of the next day, which compounds
    for x in usgs + usace + rfc:
        x[...] = 77
    state2 = state.copy()
    state2[0] = [-1000.0, 9.0, 2, -1050.0]
    usgs2, usace2, rfc2 = carry.tuples(state2, np.array([0, 0, 8, 0], np.int32))
    assert usgs2[0].tolist() == [11, 12] and [float(x[0]) for x in usgs2[1:]] == state2[0].tolist()
    assert usgs2[1][1] == (np.float32(7000.25) - day_len) - day_len and usgs2[4][1] == (np.float32(60.5) - day_len) - day_len
    assert usgs2[2][1] == np.float32(2.5) and usgs2[3][1] == np.float32(4)
    assert rfc2[1][0] == (np.float32(5000.5) - day_len) - day_len and int(rfc2[2][0]) == 2 and int(rfc2[2][1]) == 8
    assert (usgs[1] == 77).all()                                # (... and the first day's arrays are not written again)


# ---- gage carry ----------------------------------------------------------------------------------------------------------
def test_gage_carry():
    ngage, nsteps, period, decay = 3, 6, 300.0, 120.0
    rng = np.random.default_rng(2)
    days = [rng.uniform(1, 9, (ngage, nsteps + 1)).astype(np.float32) for _ in range(2)]
    days[0][1, 0] = np.nan                                      # (a gage without a first observation on day 0 ...)
    days[0][2, 3:] = np.nan                                     # (... and one whose observations end in the day: it decays)
    days[1][2, :] = np.nan                                      # (... into day 1, from the last observation of day 0)
    carry = S.GageCarry(ngage, nsteps, np.float32, 300.0, depth=3)
    nan = np.full(ngage, np.nan, np.float32)
    lv, lt = nan, nan.copy()
    for d, usgs in enumerate(days):
        mode, a, w, lt_fin, lv_fin = simple_da.resolve_tables(nsteps, period, decay, usgs, lv, lt)
        got = carry.nudging(d, usgs)
        assert len(got) == 4 and [x.dtype for x in got] == [np.uint8, np.float32, np.float32, np.float32]
        assert np.array_equal(got[0], mode) and np.array_equal(got[1], a) and np.array_equal(got[2], w)
        assert np.array_equal(got[3], usgs[:, 0], equal_nan=True) and (d == 1 or np.isnan(got[3][1]))
        lv, lt = lv_fin, lt_fin - np.float32(nsteps * period)
        left = carry.lastobs(d)
        assert np.array_equal(left[0], lt_fin, equal_nan=True) and np.array_equal(left[1], lv_fin, equal_nan=True)
        assert carry.lastobs(d) == (None, None)                 # (handed out once)
    assert (mode[2] == 2).all() and np.isfinite(lv[2])           # (day 1's gage 2 did decay from day 0's last observation)
    # the tables of day d and day d + depth are the same ring arrays; the first day's lastobs is taken as given
    assert carry.nudging(3, days[0])[0] is carry.nudging(6, days[0])[0]
    given = (np.array([1.0, 2.0, 3.0]), np.array([-300.0, -600.0, -900.0]))
    first = S.GageCarry(ngage, nsteps, np.float32, 300.0, depth=3, lastobs=given, da_parameters={"da_decay_coefficient": 60.0})
    want = simple_da.resolve_tables(nsteps, 300.0, 60.0, days[1], given[0].astype(np.float32), given[1].astype(np.float32))
    assert np.array_equal(first.nudging(0, days[1])[2], want[2]) and (want[2][2] > 0).all()
    with pytest.raises(ValueError, match="lastobs must be"):
        S.GageCarry(ngage, nsteps, np.float32, 300.0, depth=3, lastobs=(np.zeros(2), np.zeros(3)))


# ---- the summary through the stand-in ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def summary_run():
    """the 64-step, one-process stream of test_distributed_cpu's stride test, with the summary and every step's (q, v, d)"""
    from oracle_plan import OracleStreamPlan
    from troute_amd import synthetic
    from troute_amd.distributed import ShardedRouter
    net = synthetic.generate(nseg=6000, nnet=40, seed=5)
    nseg = net["to"].shape[0]
    rng = np.random.default_rng(4)
    days = [rng.uniform(0, 0.5, (nseg, 8)).astype(np.float32) for _ in range(9)]
    q0 = np.zeros((nseg, 3), np.float32)
    out = {}
    for daily in (True, False):
        router = ShardedRouter(net["to"], net["params"], plan_factory=OracleStreamPlan, stream=True)
        with S.RouteStream(router, 64, 8, output_stride=1, summary=("peak", "mean", "total"), daily_summary=daily) as rs:
            items, copies = [], []
            for it in rs.route(iter(days), q0):                 # (ring arrays: copied as they arrive)
                items.append(it)
                copies.append((np.array(it[3], copy=True), {k: np.array(v, copy=True) for k, v in it[4].items()} if daily else None))
            out[daily] = {"items": items, "copies": copies, "total": rs.total, "slots": rs.last_info["slots"]}
        router.close()
    return out, len(days), nseg


def reductions(q):
    """(peak_flow, peak_step, mean_flow) of flows [rows, nsteps]: include/trmc.h's definitions for finite flows, in float32"""
    at = np.argmax(q, axis=1)
    return q[np.arange(q.shape[0]), at], (at + 1).astype(np.int32), np.cumsum(q, axis=1, dtype=np.float32)[:, -1] / np.float32(q.shape[1])


def test_stream_summary_is_delivered_from_the_ring(summary_run):
    out, ndays, nseg = summary_run
    run = out[True]
    assert [it[0] for it in run["items"]] == list(range(ndays)) and all(len(it) == 5 for it in run["items"])
    for (fvd, sm), it in zip(run["copies"], run["items"]):
        assert list(sm) == ["peak_flow", "peak_step", "mean_flow"] and fvd.shape == (nseg, 64, 3)
        pk, st, mn = reductions(fvd[:, :, 0])
        assert sm["peak_flow"].dtype == np.float32 and sm["peak_step"].dtype == np.int32 and sm["mean_flow"].dtype == np.float32
        assert np.array_equal(sm["peak_flow"], pk) and np.array_equal(sm["peak_step"], st) and np.array_equal(sm["mean_flow"], mn)
    assert len({tuple(sm["peak_step"].tolist()) for _, sm in run["copies"]}) > 1        # (the days differ)
    D = run["slots"]
    assert D < ndays
    for d in range(ndays - D):
        a, b = run["items"][d], run["items"][d + D]
        assert all(a[4][k] is b[4][k] for k in a[4]) and a[3] is b[3] and a[2] is b[2]
        assert a[4]["peak_flow"] is not run["items"][d + 1][4]["peak_flow"]


def test_stream_total_is_the_fold_over_all_days(summary_run):
    out, ndays, nseg = summary_run
    for daily in (True, False):
        total = out[daily]["total"]
        assert set(total) == {"days", "peak_flow", "peak_step", "mean_flow"} and total["days"] == ndays
        pk, st, mn = reductions(out[daily]["copies"][0][0][:, :, 0])
        st = st.astype(np.int64)
        for d in range(1, ndays):
            p, t, m = reductions(out[daily]["copies"][d][0][:, :, 0])
            st, pk, mn = np.where(p > pk, d * 64 + t, st), np.where(p > pk, p, pk), mn + m
        assert np.array_equal(total["peak_flow"], pk) and np.array_equal(total["peak_step"], st) and total["peak_step"].dtype == np.int64
        assert np.array_equal(total["mean_flow"], mn / np.float32(ndays))
        assert st.max() > 64                                    # (some row's peak of the whole stream lies in a later day)


def test_stream_without_daily_summary_yields_no_dict(summary_run):
    out, ndays, _ = summary_run
    assert len(out[False]["items"]) == ndays and all(len(it) == 4 and not isinstance(it[-1], dict) for it in out[False]["items"])
    for (a, _), (b, _) in zip(out[True]["copies"], out[False]["copies"]):
        assert np.array_equal(a, b)


# ---- when latency='low' is refused ---------------------------------------------------------------------------------------
def test_low_latency_with_several_ranks_is_refused_before_the_plan_is_touched():
    calls = []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError(f"{name} reached")

    class Router:
        world, rank, nseg = 2, 0, 10
        plan0 = Recorder()

        def stream_plan(self, late_lag=0):
            calls.append("stream_plan")
            return Recorder()

    rs = S.RouteStream(Router(), 16, 8, latency="low", comm=Recorder())
    with pytest.raises(ValueError, match="^latency='low' is a one-GPU option$"):
        next(rs.route(iter([np.zeros((10, 2), np.float32)])))
    assert calls == []
