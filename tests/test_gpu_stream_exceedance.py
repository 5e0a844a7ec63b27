"""THRESHOLD EXCEEDANCE OVER A WHOLE STREAM OF DAYS (include/trmc.h trmc_stream_set_exceedance, trmc_stream_exceedance;
csrc/k_stream_exceed.inc; RoutingPlan.stream_set_exceedance / stream_exceedance; ``exceedance`` of RouteStream): per row and level
the steps over the threshold, the first and the last of them and the longest run, over every step of every day -- the steps
counted on over the days, a run carried over a day's end.

The definition is exact and its results are integers, so every comparison is ``array_equal`` against the plain numpy loop of
tests/test_gpu_window_exceedance.py (``exceedance_of``) over the days' flows CONCATENATED IN TIME: the oracle's day by day, or the
same stream's own full result where the oracle has no say (double precision, the tolerance arithmetic, reservoirs and gages).

Shapes: those of tests/test_gpu_stream_summary.py (4 000 rows, 24 steps a day at qts 8, slices and cluster tiles, rows that lag
more than a day, its day-to-day forcing scales), and a day of 20 steps at qts 4 -- not a multiple of the kernel's eight loads in
flight.  ``conditions`` keeps the expectation from being vacuous: runs over a day's end, runs longer than any day holds, runs
that end and begin exactly at a day's edge."""
import functools
import os
import threading

import numpy as np
import pytest

import helpers as H
from oracle import oracle as O
from test_gpu_stream_summary import OPTIONS, RS_OPTS, SCALE, copied, rs_case
from test_gpu_window_exceedance import KEYS, exceedance_of
from troute_amd import _lib
from troute_amd.comm import Comm
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu
_serial = [0]

NSEG = 4000
SHAPES = {"24 at qts 8": (24, 8, 3), "20 at qts 4": (20, 4, 5)}      # nsteps, qts, forcing columns
QUANTILES = (0.5, 0.25, 0.9, 0.75)                                   # level k of a row: this quantile of its flows over the stream


def over_the_days(x, th):
    """``exceedance_of`` (the window test's loop) over flows x [rows, days * nsteps], as the stream hands it out: int64"""
    return {k: v.astype(np.int64) for k, v in exceedance_of(x, th).items()}


def thresholds_for(x, dry, K, seed=5):
    """[rows, K] in x's dtype from the flows x [rows, steps] themselves: level k the row's QUANTILES[k]; then, in one level of every
    row of a group (row % 8; the level moves with the row so that every level of every K gets each kind): 0 +inf, 1 -inf, 2 NaN,
    3 a threshold bit-equal to one of the row's own flows; rows 4..7 of eight keep their quantiles; the dry headwaters 0."""
    n = x.shape[0]
    rng = np.random.default_rng(seed)
    th = np.quantile(x.astype(np.float64), QUANTILES[:K], axis=1).T.astype(x.dtype)
    rows = np.arange(n)
    level = (rows // 8) % K
    own = x[rows, rng.integers(0, x.shape[1], n)]
    for kind, value in enumerate((np.inf, -np.inf, np.nan, None)):
        m = rows % 8 == kind
        th[rows[m], level[m]] = own[m] if value is None else value
    th[dry] = 0
    return np.ascontiguousarray(th), level


def conditions(x, th, level, dry, nsteps, want):
    """the expectation `want` (of x against th) holds what the tests are there for -- asserted on the reference's arrays"""
    n, K = th.shape
    ndays = x.shape[1] // nsteps
    total = ndays * nsteps
    rows = np.arange(n)
    kind = np.where(np.isin(rows, dry), -1, rows % 8)
    planted = lambda k, name: want[name][rows[kind == k], level[kind == k]]
    for name in KEYS:
        assert not planted(0, name).any() and not planted(2, name).any(), name              # +inf and a NaN: never over
        assert not want[name][dry].any(), name                                             # no flow against 0: equality is not over
    assert np.all(planted(1, "steps_over") == total) and np.all(planted(1, "first_step") == 1)      # -inf: every step
    assert np.all(planted(1, "last_step") == total) and np.all(planted(1, "longest_run") == total)
    assert np.all(planted(3, "steps_over") < total)                                        # the step the threshold was taken at is not over
    with np.errstate(invalid="ignore"):
        over = x[:, :, None] > th[:, None, :]                                              # [rows, steps, K]
    ends, begins = over[:, nsteps - 1:total - 1:nsteps], over[:, nsteps:total:nsteps]      # a day's last step, the next day's first
    pairs = n * K
    across = (ends & begins).any(axis=1)
    assert across.sum() * 10 >= pairs, (across.sum(), pairs)                               # a run over a day's end: 10 % of the pairs
    in_a_day = np.max([exceedance_of(np.ascontiguousarray(x[:, d * nsteps:(d + 1) * nsteps]), th)["longest_run"] for d in range(ndays)], axis=0)
    longer = want["longest_run"] > in_a_day
    assert longer.sum() * 20 >= pairs, (longer.sum(), pairs)                               # longer than any day holds: 5 %
    assert (ends & ~begins).any() and (~ends & begins).any()                               # a run ends / begins exactly at a day's edge
    assert (want["first_step"] > nsteps).any()
    assert (want["steps_over"] == 0).any()                                               # pairs never over


def assert_equal(got, want, what, days=None):
    if days is not None:
        assert got["days"] == days, (what, got["days"], days)
    assert [k for k in got if k != "days"] == list(KEYS), (what, list(got))
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.dtype == np.int64 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, k, bad.shape[0], bad[:8].tolist(), g[g != w][:8].tolist(), w[g != w][:8].tolist())


@functools.lru_cache(maxsize=None)
def plan_case(nq):
    """the network of tests/test_gpu_stream_summary.py (its seed, its dry headwaters), with nq forcing columns"""
    from test_gpu_parity import synth_inputs
    rng = np.random.default_rng(77)
    to = H.random_network(rng, NSEG)
    _, _, ups = H.reaches_from_to(to)
    up_ptr, up_idx = csr_from_lists(ups)
    params, qlat, q0 = synth_inputs(rng, NSEG, nq)
    dry = np.array([r for r in range(NSEG) if len(ups[r]) == 0][:6])
    qlat[dry] = 0
    q0[dry] = 0
    return up_ptr, up_idx, params, qlat, q0, dry


def day_of(qlat, d, dt=np.float32):
    return (qlat * np.float32(SCALE[d % len(SCALE)])).astype(np.float32).astype(dt)


_reference = {}


def reference(shape, ndays, lvl):
    """the oracle's flows of `ndays` days routed day by day, concatenated in time [rows, ndays * nsteps]: computed once a shape"""
    key = (shape, ndays)
    if key not in _reference:
        nsteps, qts, nq = SHAPES[shape]
        up_ptr, up_idx, params, qlat, q0, dry = plan_case(nq)
        state, flows = q0, []
        for d in range(ndays):
            want = O.network_by_segment(nsteps, qts, up_ptr, up_idx, lvl, params, state, day_of(qlat, d), True, det=True)[:, 1:, :]
            flows.append(want[:, :, 0])
            state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
        x = np.ascontiguousarray(np.concatenate(flows, axis=1))
        x.setflags(write=False)
        _reference[key] = x
    return _reference[key]


def stream_days(p, nsteps, qts, days, q0, fetch_after_each=False, **begin):
    """one stream of `days` on plan p (the exceedance declared by the caller); returns (the fetch after the last day, the fetches
    made after every push that found a day complete, the days' full results where begun with full_output)"""
    p.upload_forcing(nsteps, days[0], q0)
    p.stream_begin(nsteps, qts, **begin)
    outs = [_lib.result_empty((p.nseg, nsteps, 3), p.dtype, always_pinned=True) for _ in days] if begin.get("full_output") else None
    between = []
    for d, day in enumerate(days):
        assert p.stream_push(pinned_like(day), **({"fvd": outs[d]} if outs else {})) == d
        done = p.stream_info()["days_complete"]
        if fetch_after_each and done >= 1:
            between.append((done, p.stream_exceedance()))
    p.stream_flush()
    last = p.stream_exceedance()
    p.stream_end()                                              # (waits for everything: every day's full result is on the host)
    return last, between, outs


# ---- 1. the oracle over a reused ring; 5. a fetch in mid-stream; 6. a second stream on the same plan ---------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exceedance_against_the_oracle_over_a_reused_ring(shape):
    """products-only fp32 streams of 2 * slots + 1 days, K = 1, 2, 3 and 4 one after the other on ONE plan (each starts from
    zero), against the oracle's flows routed day by day; with K = 4 a fetch after every push: the days folded so far, no more."""
    nsteps, qts, nq = SHAPES[shape]
    up_ptr, up_idx, params, qlat, q0, dry = plan_case(nq)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=OPTIONS) as p:
        lvl, _ = p.levels()
        lag, W, C = p.lags()
        p.upload_forcing(nsteps, day_of(qlat, 0), q0)
        p.stream_begin(nsteps, qts)
        info = p.stream_info()
        p.stream_end()
        ndays = 2 * info["slots"] + 1
        assert lag.max() > info["tiles_per_day"] and W > 0 and C > 0 and nsteps % 8 == (0 if shape == "24 at qts 8" else 4)
        x = reference(shape, ndays, lvl)
        days = [day_of(qlat, d) for d in range(ndays)]
        for K in (4, 1, 2, 3):
            th, level = thresholds_for(x, dry, K)
            want = over_the_days(x, th)
            conditions(x, th, level, dry, nsteps, want)
            p.set_thresholds(th[:, 0] if K == 1 else th)
            p.stream_set_exceedance("flow")
            got, between, _ = stream_days(p, nsteps, qts, days, q0, fetch_after_each=K == 4)
            assert_equal(got, want, (shape, K), ndays)
            assert all(v.shape == (NSEG, K) for k, v in got.items() if k != "days")
            if K == 4:                                              # (5.) in mid-stream: exactly the days handed over
                seen = [done for done, _ in between]
                assert seen and seen == sorted(seen) and 1 <= seen[0] < seen[-1] < ndays, seen
                for done, part in between[:: max(1, len(between) // 4)]:
                    assert_equal(part, over_the_days(np.ascontiguousarray(x[:, :done * nsteps]), th), (shape, "after day", done), done)
                again, _, _ = stream_days(p, nsteps, qts, days, q0)     # (6.) the same days again on this plan: not twice the counts
                assert_equal(again, want, (shape, "a second stream"), ndays)
        # parts: the arrays asked for only
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_begin(nsteps, qts)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        some = p.stream_exceedance(("longest_run", "first_step"))
        assert list(some) == ["days", "first_step", "longest_run"] and some["days"] == 1
        w1 = over_the_days(np.ascontiguousarray(x[:, :nsteps]), th)
        assert np.array_equal(some["first_step"], w1["first_step"]) and np.array_equal(some["longest_run"], w1["longest_run"])
        p.stream_end()


# ---- 2. the same stream's full result -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fp32", "fp64", "tolerance"])
def test_exceedance_and_full_result_of_the_same_stream(variant):
    """one stream with full_output AND the exceedance: the numpy loop over that stream's own fvd[:, :, 0]; a products-only stream
    of the same days gives the same arrays"""
    nsteps, qts, nq = SHAPES["24 at qts 8"]
    up_ptr, up_idx, params, qlat, q0, dry = plan_case(nq)
    precision = 64 if variant == "fp64" else 32
    opts = dict(OPTIONS, **({"arithmetic": "tolerance"} if variant == "tolerance" else {}))
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", precision=precision, options=opts) as p:
        dt = p.dtype
        assert np.dtype(dt).itemsize == precision // 8
        ndays = 5
        days = [day_of(qlat, d, dt) for d in range(ndays)]
        p.upload_forcing(nsteps, days[0], q0.astype(dt))
        p.stream_begin(nsteps, qts, full_output=True)
        outs = [_lib.result_empty((NSEG, nsteps, 3), dt, always_pinned=True) for _ in range(ndays)]
        for d in range(ndays):                                      # (thresholds come from the flows: a first stream without them)
            p.stream_push(pinned_like(days[d]), fvd=outs[d])
        p.stream_end()                                              # (flushes and waits for everything: more days than slots)
        x = np.ascontiguousarray(np.concatenate([o[:, :, 0] for o in outs], axis=1))
        assert x.dtype == dt and np.isfinite(x).all() and x.max() > 0
        th, level = thresholds_for(x, dry, 4)
        want = over_the_days(x, th)
        conditions(x, th, level, dry, nsteps, want)
        p.set_thresholds(th)
        p.stream_set_exceedance("flow")
        got, _, outs2 = stream_days(p, nsteps, qts, days, q0.astype(dt), full_output=True)
        assert all(np.array_equal(a, b) for a, b in zip(outs, outs2))          # (the exceedance changes nothing of the result)
        assert_equal(got, want, (variant, "full_output"), ndays)
        lean, _, _ = stream_days(p, nsteps, qts, days, q0.astype(dt))
        assert_equal(lean, want, (variant, "products only"), ndays)
        p.stream_set_exceedance(None)                                          # withdrawn: the next stream has none
        p.upload_forcing(nsteps, days[0], q0.astype(dt))
        p.stream_begin(nsteps, qts)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        with pytest.raises(RuntimeError, match="begun without an exceedance"):
            p.stream_exceedance()
        p.stream_end()


# ---- 3. reservoirs and gages --------------------------------------------------------------------------------------------------
def test_exceedance_with_reservoirs_and_gages():
    """at gage rows the flow after nudging, at reservoir rows the pool's outflow: what the stream's own fvd[:, :, 0] holds"""
    import test_gpu_stream_reservoirs_nudging as RN
    c = RN.case(3000, 78, 4)
    r = ShardedRouter(c.to, c.params, stream=True, options=RN.OPTIONS, reservoirs=(c.lakes, c.par, RN.DT), gages=c.gages)

    def route(**kw):
        with RouteStream(r, RN.NSTEPS, RN.QTS, full_output=True, **kw) as rs:
            flows = [np.array(item[3][:, :, 0]) for item in rs.route(iter(c.days), c.q0, observations=iter(c.usgs), lastobs=(c.lv0, c.lt0),
                                                                     da_parameters={"da_decay_coefficient": RN.DECAY, "routing_period": RN.DT})]
            return np.ascontiguousarray(np.concatenate(flows, axis=1)), rs.exceedance
    x, none = route()
    assert none is None and x.shape == (c.to.shape[0], 4 * RN.NSTEPS)
    th, _ = thresholds_for(x, np.zeros(0, np.int64), 3)
    x2, got = route(exceedance=("flow", th))
    assert np.array_equal(x, x2)
    want = over_the_days(x, th)
    assert_equal(got, want, "lakes and gages", 4)
    for rows, what in ((c.gages, "gage rows"), (c.lakes, "reservoir rows")):
        part = {k: (v if k == "days" else v[rows]) for k, v in got.items()}
        assert_equal(part, over_the_days(np.ascontiguousarray(x[rows]), th[rows]), what, 4)
        partly = want["steps_over"][rows]
        assert np.any((partly > 0) & (partly < x.shape[1])), what               # (these rows cross their thresholds)
    r.close()


# ---- 4. one day against a window ----------------------------------------------------------------------------------------------
def test_a_one_day_stream_equals_the_window_call():
    nsteps, qts, nq = SHAPES["20 at qts 4"]
    up_ptr, up_idx, params, qlat, q0, dry = plan_case(nq)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=OPTIONS) as p:
        fvd = p.route(nsteps, qts, True, qlat, q0)
        th, _ = thresholds_for(np.ascontiguousarray(fvd[:, :, 0]), dry, 4)
        p.set_thresholds(th)
        window = p.window_exceedance("flow")
        assert window["steps_over"].dtype == np.int32 and 0 < np.count_nonzero(window["steps_over"]) < window["steps_over"].size
        p.stream_set_exceedance("flow")
        got, _, _ = stream_days(p, nsteps, qts, [qlat], q0)
        assert_equal(got, {k: v.astype(np.int64) for k, v in window.items()}, "one day", 1)
        assert_equal(got, over_the_days(np.ascontiguousarray(fvd[:, :, 0]), th), "one day, numpy", 1)


# ---- 7. RouteStream: one rank, and two ranks on one device --------------------------------------------------------------------
RS_NSTEPS, RS_QTS = 32, 16


def test_routestream_exceedance_on_one_rank_and_on_two():
    """``RouteStream(..., exceedance=("flow", thresholds))``: ``rs.exceedance`` once ``route()`` has yielded its last day, next to
    ``rs.total``, over the rank's ``rows`` -- on two ranks (threads, the shared-memory transport) the trunk's rows where a rank owns
    them and its boundary copies of the cut rows, each against the threshold of the row it is"""
    net, q0, days = rs_case()
    nseg = net["to"].shape[0]
    r = ShardedRouter(net["to"], net["params"], stream=True, options=RS_OPTS)
    with RouteStream(r, RS_NSTEPS, RS_QTS, full_output=True) as rs:
        x = np.ascontiguousarray(np.concatenate([np.array(item[3][:, :, 0]) for item in rs.route(iter(days), q0)], axis=1))
        assert rs.exceedance is None and np.array_equal(rs.rows, np.arange(nseg))
    th, _ = thresholds_for(x, np.zeros(0, np.int64), 2)
    want = over_the_days(x, th)
    assert (want["longest_run"] > RS_NSTEPS).any() and (want["first_step"] > RS_NSTEPS).any() and (want["steps_over"] == 0).any()
    with RouteStream(r, RS_NSTEPS, RS_QTS, exceedance=("flow", th), summary=("peak", "total"), daily_summary=False) as rs:
        items = [copied(item) for item in rs.route(iter(days), q0)]
        assert [len(i) for i in items] == [3] * len(days)                       # (not a product of the day: the tuples do not change)
        assert_equal(rs.exceedance, want, "one rank", len(days))
        assert rs.total["days"] == len(days) and np.array_equal(rs.total["peak_flow"], x.max(axis=1))
        assert np.array_equal(want["first_step"][:, 0] > 0, want["steps_over"][:, 0] > 0)
    with RouteStream(r, RS_NSTEPS, RS_QTS) as rs:                              # (an earlier stream's declaration is withdrawn)
        assert len([0 for _ in rs.route(iter(days[:2]), q0)]) == 2 and rs.exceedance is None
    r.close()
    world = 2
    _serial[0] += 1
    key = f"exceed{os.getpid()}_{_serial[0]}"
    results, errors = [None] * world, []

    def run(rank):
        try:
            comm = Comm(rank, world, device=0, backend="shm", key=key)
            rr = ShardedRouter(net["to"], net["params"], rank=rank, world=world, device=0, stream=True, options=RS_OPTS)
            rr.enable_device_exchange(comm)
            with RouteStream(rr, RS_NSTEPS, RS_QTS, exceedance=("flow", th)) as rs:
                n = len([0 for _ in rs.route(days, q0)])
                results[rank] = (copied(rs.exceedance), np.array(rs.rows, copy=True), rr.plan1 is not None, n)
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
    assert sum(res[1].shape[0] for res in results) >= nseg
    for rank in range(world):
        got, srows, _, n = results[rank]
        assert n == len(days)
        got = dict(got, days=int(got["days"]))
        assert_equal(got, {k: v[srows] for k, v in want.items()}, ("rank", rank), len(days))


# ---- 8. refusals on the device ------------------------------------------------------------------------------------------------
def test_refusals():
    from test_gpu_window_summary import inputs
    nseg, nq, nsteps = 50, 2, 8
    ups, params, qlat, q0 = inputs(4, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    th = np.full((nseg, 2), 0.5, np.float32)
    h = _lib.lib()
    a = np.zeros((nseg, 2), np.int64)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={"cluster_rows": 8, "wide_min_rows": 3, "wide_k": 4}) as p:
        with pytest.raises(RuntimeError, match="no thresholds"):           # a declaration without thresholds
            p.stream_set_exceedance("flow")
        p.stream_set_exceedance(None)                                       # (withdrawing nothing is no error)
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4)
        with pytest.raises(RuntimeError, match="begun without an exceedance"):   # a fetch with no declaration
            p.stream_exceedance()
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.stream_set_exceedance("flow")
        p.stream_end()
        p.set_thresholds(th)
        assert h.trmc_stream_set_exceedance(p._h, _lib.TRMC_X_DEPTH) == _lib.TRMC_EUNSUPPORTED
        assert h.trmc_stream_set_exceedance(p._h, _lib.TRMC_X_VELOCITY) == _lib.TRMC_EUNSUPPORTED
        assert b"window" in h.trmc_last_error() and b"flow planes" in h.trmc_last_error()
        assert h.trmc_stream_set_exceedance(p._h, 3) == _lib.TRMC_EINVAL
        assert h.trmc_stream_set_exceedance(p._h, -2) == _lib.TRMC_EINVAL
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4)                                           # (the refused declarations declared nothing)
        with pytest.raises(RuntimeError, match="begun without an exceedance"):
            p.stream_exceedance()
        p.stream_end()
        p.stream_set_exceedance("flow")
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4)
        lag_max = p.stream_info()["lag_max"]
        assert lag_max > 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):   # before a day is complete: begun ...
            p.stream_exceedance()
        p.stream_push(pinned_like(qlat))
        assert p.stream_info()["days_complete"] == 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):   # ... and pushed, its last rows under way
            p.stream_exceedance()
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.set_thresholds(th)
        p.stream_flush()
        assert h.trmc_stream_exceedance(p._h, None, None, _lib.ptr(a), None, None) == 0     # (any array may be NULL, days_out too)
        got = p.stream_exceedance()
        assert got["days"] == 1 and np.array_equal(got["last_step"], a) and a.max() > 0
        p.stream_end()
        with pytest.raises(RuntimeError, match="no stream of windows in progress"):
            p.stream_exceedance()
        # the declaration outlives the stream; thresholds cleared under it: the next stream is refused, not begun without them
        p.set_thresholds(None)
        p.upload_forcing(nsteps, qlat, q0)
        with pytest.raises(RuntimeError, match="thresholds have been cleared"):
            p.stream_begin(nsteps, 4)
        p.set_thresholds(th[:, 0])
        p.stream_begin(nsteps, 4)
        p.stream_push(pinned_like(qlat))
        p.stream_flush()
        one = p.stream_exceedance()
        assert one["steps_over"].shape == (nseg, 1) and np.array_equal(one["last_step"][:, 0], a[:, 0])
        p.stream_end()
        with p.clone() as c:                                                # a clone starts without a threshold table
            with pytest.raises(RuntimeError, match="no thresholds"):
                c.stream_set_exceedance("flow")
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="flow") as p:   # a declaration on a dataflow plan
        assert p.engine == "flow"
        p.set_thresholds(th)
        with pytest.raises(ValueError, match="level engine"):
            p.stream_set_exceedance("flow")
