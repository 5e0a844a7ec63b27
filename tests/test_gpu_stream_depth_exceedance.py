"""OUT-OF-BANK AND STAGE-THRESHOLD EXCEEDANCE OVER A WHOLE STREAM OF DAYS (include/trmc.h trmc_stream_set_depth_exceedance,
trmc_stream_depth_exceedance; csrc/k_stream_exceed_depth.inc; RoutingPlan.stream_set_depth_exceedance / stream_depth_exceedance;
``depth_exceedance`` of RouteStream): per row and level the steps the DEPTH is over the threshold, the first and the last of them
and the longest run, over every step of every day -- the steps counted on over the days, a run carried over a day's end.

The definition is exact and its results are integers, so every comparison is ``array_equal`` on int64 against the plain numpy loop
(``over_the_days`` of tests/test_gpu_stream_exceedance.py) over the days' depths CONCATENATED IN TIME: the oracle's column 2 day by
day, or the same stream's own full result where the oracle has no say (double precision, the tolerance arithmetic, reservoirs and
gages).  Shapes, thresholds and the conditions that keep the expectation from being vacuous are the flow tests': 4 000 rows, slices
and cluster tiles, rows that lag more than a day, 24 steps a day at qts 8 and 20 at qts 4 (not a multiple of the kernel's eight
loads in flight), a ring that is reused; ``conditions`` was checked on the oracle's depth arrays without a GPU for 7 to 13 days of
either shape and K = 1..4."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import helpers as H  # noqa: F401
from oracle import oracle as O
from test_gpu_stream_exceedance import NSEG, SHAPES, assert_equal, conditions, day_of, over_the_days, plan_case, thresholds_for
from test_gpu_stream_summary import OPTIONS, RS_OPTS, copied, rs_case
from test_gpu_window_exceedance import bankfull_of
from troute_amd import _lib
from troute_amd.comm import Comm
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu
_serial = [0]
_reference = {}


def reference(shape, ndays, lvl, scale=1.0):
    """the oracle's (flows, depths) of `ndays` days routed day by day, each concatenated in time [rows, ndays * nsteps]: computed
    once a shape and forcing scale, never written to"""
    key = (shape, ndays, scale)
    if key not in _reference:
        nsteps, qts, nq = SHAPES[shape]
        up_ptr, up_idx, params, qlat, q0, dry = plan_case(nq)
        state, flows, depths = q0, [], []
        for d in range(ndays):
            want = O.network_by_segment(nsteps, qts, up_ptr, up_idx, lvl, params, state, scaled(day_of(qlat, d), scale), True, det=True)[:, 1:, :]
            flows.append(want[:, :, 0])
            depths.append(want[:, :, 2])
            state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
        both = tuple(np.ascontiguousarray(np.concatenate(a, axis=1)) for a in (flows, depths))
        for a in both:
            a.setflags(write=False)
        _reference[key] = both
    return _reference[key]


def scaled(day, scale):
    return day if scale == 1.0 else (day * np.float32(scale)).astype(np.float32)


def open_plan(nq, **kw):
    up_ptr, up_idx, params, _, _, _ = plan_case(nq)
    options = dict(OPTIONS, **kw.pop("options", {}))
    return RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=options, **kw)


def ring_of(p, nsteps, qts, day, q0):
    """(slots, tiles a day) of a stream on p, which has slices and cluster tiles and rows that lag more than a day"""
    lag, W, C = p.lags()
    p.upload_forcing(nsteps, day, q0)
    p.stream_begin(nsteps, qts)
    info = p.stream_info()
    p.stream_end()
    assert info["wide_levels"] > 0 and info["cluster_levels"] > 0 and W > 0 and C > 0
    assert lag.max() > info["tiles_per_day"]
    return info["slots"], info["tiles_per_day"]


def stream_days(p, nsteps, qts, days, q0, fetch_after_each=False, flow=False, **begin):
    """one stream of `days` on plan p (the declarations are the caller's); returns (the depth exceedance fetched after the last
    day, the fetches made after every push that found a day complete, the days' full results where begun with full_output, the
    flow exceedance after the last day where asked for)"""
    p.upload_forcing(nsteps, days[0], q0)
    p.stream_begin(nsteps, qts, **begin)
    outs = [_lib.result_empty((p.nseg, nsteps, 3), p.dtype, always_pinned=True) for _ in days] if begin.get("full_output") else None
    between = []
    for d, day in enumerate(days):
        assert p.stream_push(pinned_like(day), **({"fvd": outs[d]} if outs else {})) == d
        done = p.stream_info()["days_complete"]
        if fetch_after_each and done >= 1:
            between.append((done, p.stream_depth_exceedance()))
    p.stream_flush()
    last = p.stream_depth_exceedance()
    q = p.stream_exceedance() if flow else None
    p.stream_end()                                              # (waits for everything: every day's full result is on the host)
    return last, between, outs, q


# ---- 1. the oracle over a reused ring, a fetch after every day ----------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_depth_exceedance_against_the_oracle_over_a_reused_ring(shape):
    """products-only fp32 streams of 2 * slots + 1 days, K = 4, 1, 2 and 3 one after the other on ONE plan (each starts from zero),
    against the oracle's depths routed day by day; a fetch after every push: the days folded so far, no more"""
    nsteps, qts, nq = SHAPES[shape]
    _, _, _, qlat, q0, dry = plan_case(nq)
    with open_plan(nq) as p:
        lvl, _ = p.levels()
        slots, tpd = ring_of(p, nsteps, qts, day_of(qlat, 0), q0)
        ndays = 2 * slots + 1
        assert nsteps % 8 == (0 if shape == "24 at qts 8" else 4)
        _, x = reference(shape, ndays, lvl)
        assert x.dtype == np.float32 and np.isfinite(x).all() and x.max() > 0
        days = [day_of(qlat, d) for d in range(ndays)]
        for K in (4, 1, 2, 3):
            th, level = thresholds_for(x, dry, K)
            want = over_the_days(x, th)
            conditions(x, th, level, dry, nsteps, want)
            p.stream_set_depth_exceedance(th[:, 0] if K == 1 else th)
            got, between, _, _ = stream_days(p, nsteps, qts, days, q0, fetch_after_each=True)
            assert_equal(got, want, (shape, K), ndays)
            assert all(v.shape == (NSEG, K) for k, v in got.items() if k != "days")
            seen = [done for done, _ in between]
            assert seen and seen == sorted(seen) and 1 <= seen[0] < seen[-1] < ndays, seen
            for done, part in between[:: max(1, len(between) // 3)]:
                assert_equal(part, over_the_days(np.ascontiguousarray(x[:, :done * nsteps]), th), (shape, K, "after day", done), done)
        again, _, _, _ = stream_days(p, nsteps, qts, days, q0)          # the same days again on this plan: not twice the counts
        assert_equal(again, want, (shape, "a second stream"), ndays)
        # parts: the arrays asked for only
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_begin(nsteps, qts)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        some = p.stream_depth_exceedance(("longest_run", "first_step"))
        assert list(some) == ["days", "first_step", "longest_run"] and some["days"] == 1
        w1 = over_the_days(np.ascontiguousarray(x[:, :nsteps]), th)
        assert np.array_equal(some["first_step"], w1["first_step"]) and np.array_equal(some["longest_run"], w1["longest_run"])
        assert p.stream_depth_exceedance_kernel_ms() > 0
        p.stream_end()


# ---- 2. the depth plane and the full result of the same days ------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fp32", "fp64", "tolerance"])
def test_plane_source_and_full_result_source_give_the_same_arrays(variant):
    """a stream with full_output folds the day's out[row][step][2], one without it the slot's depth plane: each against the numpy
    loop over that stream's own full result, and the same arrays from both"""
    nsteps, qts, nq = SHAPES["20 at qts 4"]
    _, _, _, qlat, q0, dry = plan_case(nq)
    precision = 64 if variant == "fp64" else 32
    with open_plan(nq, precision=precision, options={"arithmetic": "tolerance"} if variant == "tolerance" else {}) as p:
        dt = p.dtype
        assert np.dtype(dt).itemsize == precision // 8
        ndays = 5
        days = [day_of(qlat, d, dt) for d in range(ndays)]
        p.upload_forcing(nsteps, days[0], q0.astype(dt))
        p.stream_begin(nsteps, qts, full_output=True)
        outs = [_lib.result_empty((NSEG, nsteps, 3), dt, always_pinned=True) for _ in range(ndays)]
        for d in range(ndays):                                      # (thresholds come from the depths: a first stream without them)
            p.stream_push(pinned_like(days[d]), fvd=outs[d])
        p.stream_end()                                              # (flushes and waits for everything: more days than slots)
        x = np.ascontiguousarray(np.concatenate([o[:, :, 2] for o in outs], axis=1))
        assert x.dtype == dt and np.isfinite(x).all() and x.max() > 0
        th, level = thresholds_for(x, dry, 4)
        want = over_the_days(x, th)
        conditions(x, th, level, dry, nsteps, want)
        p.stream_set_depth_exceedance(th)
        full, _, outs2, _ = stream_days(p, nsteps, qts, days, q0.astype(dt), full_output=True)
        assert all(np.array_equal(a, b) for a, b in zip(outs, outs2))          # (the fold changes nothing of the result)
        assert_equal(full, want, (variant, "full_output"), ndays)
        lean, _, _, _ = stream_days(p, nsteps, qts, days, q0.astype(dt))
        assert_equal(lean, want, (variant, "the depth plane"), ndays)
        assert_equal(lean, full, (variant, "plane against full result"), ndays)
        p.stream_set_depth_exceedance(th[:, :3])                                 # three levels in a table four wide, from the full result
        three, _, _, _ = stream_days(p, nsteps, qts, days, q0.astype(dt), full_output=True)
        assert_equal(three, {k: v[:, :3] for k, v in want.items()}, (variant, "K = 3, full_output"), ndays)
        p.stream_set_depth_exceedance(None)                                      # withdrawn: the next stream has none
        p.upload_forcing(nsteps, days[0], q0.astype(dt))
        p.stream_begin(nsteps, qts)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        with pytest.raises(RuntimeError, match="begun without a depth exceedance"):
            p.stream_depth_exceedance()
        p.stream_end()


# ---- 3. reservoirs and gages --------------------------------------------------------------------------------------------------
def test_depth_exceedance_with_reservoirs_and_gages():
    """at reservoir rows the pool's water elevation, at gage rows the step's own depth (nudging changes the flow only): what the
    stream's own fvd[:, :, 2] holds, from the full result and from the depth plane"""
    import test_gpu_stream_reservoirs_nudging as RN
    c = RN.case(3000, 78, 4)
    r = ShardedRouter(c.to, c.params, stream=True, options=RN.OPTIONS, reservoirs=(c.lakes, c.par, RN.DT), gages=c.gages)

    def route(full=True, **kw):
        with RouteStream(r, RN.NSTEPS, RN.QTS, full_output=full, **kw) as rs:
            items = [copied(item) for item in rs.route(iter(c.days), c.q0, observations=iter(c.usgs), lastobs=(c.lv0, c.lt0),
                                                       da_parameters={"da_decay_coefficient": RN.DECAY, "routing_period": RN.DT})]
            depths = np.ascontiguousarray(np.concatenate([i[3][:, :, 2] for i in items], axis=1)) if full else None
            nudged = max(float(np.abs(i[-1]["nudge"]).max()) for i in items)
            return depths, nudged, rs.depth_exceedance
    x, nudged, none = route()
    assert none is None and x.shape == (c.to.shape[0], 4 * RN.NSTEPS) and nudged > 0      # (the gages were nudged)
    assert x[c.lakes].min() > 0                                                          # (the pools hold water: an elevation)
    th, _ = thresholds_for(x, np.zeros(0, np.int64), 3)
    x2, _, got = route(depth_exceedance=th)
    assert np.array_equal(x, x2)
    want = over_the_days(x, th)
    assert_equal(got, want, "lakes and gages, full result", 4)
    _, nudged, lean = route(full=False, depth_exceedance=th)
    assert nudged > 0
    assert_equal(lean, want, "lakes and gages, depth plane", 4)
    for rows, what in ((c.gages, "gage rows"), (c.lakes, "reservoir rows")):
        for res, src in ((got, "full result"), (lean, "depth plane")):
            part = {k: (v if k == "days" else v[rows]) for k, v in res.items()}
            assert_equal(part, over_the_days(np.ascontiguousarray(x[rows]), th[rows]), (what, src), 4)
        partly = want["steps_over"][rows]
        assert np.any((partly > 0) & (partly < x.shape[1])), what               # (these rows cross their thresholds)
    r.close()


# ---- 4. one day against a window ----------------------------------------------------------------------------------------------
def test_a_one_day_stream_equals_the_window_call_on_depth():
    nsteps, qts, nq = SHAPES["20 at qts 4"]
    _, _, _, qlat, q0, dry = plan_case(nq)
    with open_plan(nq) as p:
        fvd = p.route(nsteps, qts, True, qlat, q0)
        depth = np.ascontiguousarray(fvd[:, :, 2])
        th, _ = thresholds_for(depth, dry, 4)
        p.set_thresholds(th)
        window = p.window_exceedance("depth")
        assert window["steps_over"].dtype == np.int32 and 0 < np.count_nonzero(window["steps_over"]) < window["steps_over"].size
        p.set_thresholds(None)                                      # (the stream's table is its own)
        p.stream_set_depth_exceedance(th)
        got, _, _, _ = stream_days(p, nsteps, qts, [qlat], q0)
        assert_equal(got, {k: v.astype(np.int64) for k, v in window.items()}, "one day", 1)
        assert_equal(got, over_the_days(depth, th), "one day, numpy", 1)


# ---- 5. out of bank -----------------------------------------------------------------------------------------------------------
BANK_SCALE = 16.0   # (the oracle, without a GPU: 1 252 of the 4 000 rows leave their banks in five days at this scale, 2 748 never do)


def test_bankfull_is_the_depth_against_the_plans_bankfull_depth():
    shape = "24 at qts 8"
    nsteps, qts, nq = SHAPES[shape]
    _, _, params, qlat, q0, dry = plan_case(nq)
    ndays = 5
    with open_plan(nq) as p:
        lvl, _ = p.levels()
        _, x = reference(shape, ndays, lvl, BANK_SCALE)
        bfd = p.bankfull_depth()
        assert np.array_equal(bfd.view(np.uint32), bankfull_of(params, np.float32).view(np.uint32))
        want = over_the_days(x, np.ascontiguousarray(bfd[:, None]))
        out = want["steps_over"][:, 0]
        assert np.count_nonzero(out) >= 100 and np.count_nonzero(out == 0) >= 100          # rows that go out of bank, rows that never do
        assert np.count_nonzero((out > 0) & (out < x.shape[1])) >= 100 and (want["longest_run"] > nsteps).any()
        p.stream_set_depth_exceedance("bankfull")
        days = [scaled(day_of(qlat, d), BANK_SCALE) for d in range(ndays)]
        got, _, _, _ = stream_days(p, nsteps, qts, days, q0)
        assert_equal(got, want, "bankfull", ndays)
        assert got["steps_over"].shape == (NSEG, 1)


# ---- 6. flow and depth in one stream ------------------------------------------------------------------------------------------
def test_flow_and_depth_exceedance_in_one_stream():
    shape = "24 at qts 8"
    nsteps, qts, nq = SHAPES[shape]
    _, _, _, qlat, q0, dry = plan_case(nq)
    h = _lib.lib()
    with open_plan(nq) as p:
        lvl, _ = p.levels()
        slots, _ = ring_of(p, nsteps, qts, day_of(qlat, 0), q0)
        ndays = slots + 2
        xq, xd = reference(shape, ndays, lvl)
        days = [day_of(qlat, d) for d in range(ndays)]
        thq, _ = thresholds_for(xq, dry, 3)
        thd, _ = thresholds_for(xd, dry, 2, seed=6)
        wantq, wantd = over_the_days(xq, thq), over_the_days(xd, thd)
        p.set_thresholds(thq)
        p.stream_set_exceedance("flow")
        p.stream_set_depth_exceedance(thd)
        d_both, _, _, q_both = stream_days(p, nsteps, qts, days, q0, flow=True)
        assert_equal(d_both, wantd, "depth, with flow", ndays)
        assert_equal(q_both, wantq, "flow, with depth", ndays)
        p.stream_set_exceedance(None)
        d_alone, _, _, _ = stream_days(p, nsteps, qts, days, q0)
        assert_equal(d_alone, d_both, "depth alone", ndays)
        p.stream_set_depth_exceedance(None)
        p.stream_set_exceedance("flow")
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_begin(nsteps, qts)
        for day in days:
            p.stream_push(pinned_like(day))
        p.stream_flush()
        q_alone = p.stream_exceedance()
        with pytest.raises(RuntimeError, match="begun without a depth exceedance"):
            p.stream_depth_exceedance()
        p.stream_end()
        assert_equal(q_alone, q_both, "flow alone", ndays)
        # a stream with neither, after one with both on the same plan, holds no accumulator
        p.stream_set_depth_exceedance(thd)
        both_again = stream_days(p, nsteps, qts, days[:2], q0, flow=True)
        assert both_again[0]["days"] == 2 and both_again[3]["days"] == 2
        p.stream_set_exceedance(None)
        p.stream_set_depth_exceedance(None)
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_begin(nsteps, qts)
        p.stream_push(pinned_like(days[0]))
        p.stream_flush()
        a = np.zeros((NSEG, 2), np.int64)
        days_out, ms = C.c_int64(-3), C.c_double(-1.0)
        assert h.trmc_stream_depth_exceedance(p._h, _lib.ptr(a), None, None, None, C.byref(days_out)) == _lib.TRMC_ESTATE
        assert h.trmc_stream_exceedance(p._h, _lib.ptr(a), None, None, None, None) == _lib.TRMC_ESTATE
        assert h.trmc_stream_depth_exceedance_kernel_ms(p._h, C.byref(ms)) == _lib.TRMC_ESTATE
        assert not a.any() and days_out.value == -3 and ms.value == -1.0
        p.stream_end()


# ---- 7. RouteStream: one rank, and two ranks on one device --------------------------------------------------------------------
RS_NSTEPS, RS_QTS = 32, 16


def test_routestream_depth_exceedance_on_one_rank_and_on_two():
    """``RouteStream(..., depth_exceedance=thresholds)``: ``rs.depth_exceedance`` once ``route()`` has yielded its last day, next
    to ``rs.exceedance``, over the rank's ``rows`` -- on two ranks (threads, the shared-memory transport) every row a rank routes
    equals the one-rank result, and its boundary copies of the cut rows, which nobody routes, report what a depth of 0 gives
    against the threshold of the row they are"""
    net, q0, days = rs_case()
    nseg = net["to"].shape[0]
    r = ShardedRouter(net["to"], net["params"], stream=True, options=RS_OPTS)
    with RouteStream(r, RS_NSTEPS, RS_QTS, full_output=True) as rs:
        blocks = [copied(item[3]) for item in rs.route(iter(days), q0)]
        assert rs.depth_exceedance is None and np.array_equal(rs.rows, np.arange(nseg))
    xq, x = (np.ascontiguousarray(np.concatenate([b[:, :, c] for b in blocks], axis=1)) for c in (0, 2))
    th, _ = thresholds_for(x, np.zeros(0, np.int64), 3)
    th[:, 2] = -np.inf                                  # (a level every depth is over, the 0 of a boundary copy too)
    thq, _ = thresholds_for(xq, np.zeros(0, np.int64), 1)
    want, wantq = over_the_days(x, th), over_the_days(xq, thq)
    assert (want["longest_run"] > RS_NSTEPS).any() and (want["first_step"] > RS_NSTEPS).any() and (want["steps_over"] == 0).any()
    with RouteStream(r, RS_NSTEPS, RS_QTS, depth_exceedance=th, exceedance=("flow", thq)) as rs:
        items = [copied(item) for item in rs.route(iter(days), q0)]
        assert [len(i) for i in items] == [3] * len(days)                       # (not a product of the day: the tuples do not change)
        assert_equal(rs.depth_exceedance, want, "one rank", len(days))
        assert_equal(rs.exceedance, wantq, "one rank, flow beside it", len(days))
    with RouteStream(r, RS_NSTEPS, RS_QTS) as rs:                              # (an earlier stream's declaration is withdrawn)
        assert len([0 for _ in rs.route(iter(days[:2]), q0)]) == 2 and rs.depth_exceedance is None and rs.exceedance is None
        assert getattr(rs.plan, "_stream_depth_levels", 0) == 0
    r.close()
    world = 2
    _serial[0] += 1
    key = f"dexceed{os.getpid()}_{_serial[0]}"
    results, errors = [None] * world, []

    def run(rank):
        try:
            comm = Comm(rank, world, device=0, backend="shm", key=key)
            rr = ShardedRouter(net["to"], net["params"], rank=rank, world=world, device=0, stream=True, options=RS_OPTS)
            rr.enable_device_exchange(comm)
            with RouteStream(rr, RS_NSTEPS, RS_QTS, depth_exceedance=th) as rs:
                n = len([0 for _ in rs.route(days, q0)])
                copies = np.zeros(rs.rows.shape[0], bool)                       # the rank's boundary copies of the cut rows
                if rr.plan1 is not None:
                    copies[rr.rows0.shape[0]:] = np.asarray(rr.boundary1, bool)
                results[rank] = (copied(rs.depth_exceedance), np.array(rs.rows, copy=True), rr.plan1 is not None, n, copies)
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
    assert sum(int(res[4].sum()) for res in results) > 0            # ... and holds boundary copies
    for rank in range(world):
        got, srows, _, n, copies = results[rank]
        assert n == len(days) and int(got["days"]) == len(days)
        routed = {k: np.ascontiguousarray(v[~copies]) for k, v in got.items() if k != "days"}
        assert_equal(routed, {k: v[srows[~copies]] for k, v in want.items()}, ("rank", rank, "routed rows"))
        if copies.any():
            zero = over_the_days(np.zeros((int(copies.sum()), x.shape[1]), np.float32), np.ascontiguousarray(th[srows[copies]]))
            assert_equal({k: np.ascontiguousarray(v[copies]) for k, v in got.items() if k != "days"}, zero, ("rank", rank, "boundary copies"))
            assert np.all(zero["steps_over"][:, 2] == x.shape[1]) and not zero["steps_over"][:, :2].all()


# ---- 8. refusals on the device ------------------------------------------------------------------------------------------------
def test_refusals():
    from test_gpu_window_summary import inputs
    from troute_amd.plan import csr_from_lists
    nseg, nq, nsteps = 50, 2, 8
    ups, params, qlat, q0 = inputs(4, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    th = np.tile(np.array([0.0, 0.05], np.float32), (nseg, 1))          # (level 0: over wherever there is water)
    h = _lib.lib()
    a = np.zeros((nseg, 2), np.int64)
    opts = {"cluster_rows": 8, "wide_min_rows": 3, "wide_k": 4}
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=opts) as p:
        p.stream_set_depth_exceedance(None)                                 # (withdrawing nothing is no error)
        assert h.trmc_stream_set_depth_exceedance(p._h, 5, _lib.ptr(th)) == _lib.TRMC_EINVAL
        assert h.trmc_stream_set_depth_exceedance(p._h, -1, _lib.ptr(th)) == _lib.TRMC_EINVAL
        assert h.trmc_stream_set_depth_exceedance(p._h, 2, None) == _lib.TRMC_EINVAL
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4)                                           # (the refused declarations declared nothing)
        with pytest.raises(RuntimeError, match="begun without a depth exceedance"):   # a fetch with no declaration
            p.stream_depth_exceedance()
        with pytest.raises(RuntimeError, match="begun without a depth exceedance|no day has been folded"):
            p.stream_depth_exceedance_kernel_ms()
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.stream_set_depth_exceedance(th)
        p.stream_end()
        p.stream_set_depth_exceedance(th)
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4)
        assert p.stream_info()["lag_max"] > 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):   # before a day is complete: begun ...
            p.stream_depth_exceedance()
        p.stream_push(pinned_like(qlat))
        assert p.stream_info()["days_complete"] == 0
        with pytest.raises(RuntimeError, match="no day of the stream is complete yet"):   # ... and pushed, its last rows under way
            p.stream_depth_exceedance()
        assert h.trmc_stream_depth_exceedance(p._h, _lib.ptr(a), None, None, None, None) == _lib.TRMC_ESTATE and not a.any()
        with pytest.raises(RuntimeError, match="no day has been folded"):
            p.stream_depth_exceedance_kernel_ms()
        p.stream_flush()
        assert h.trmc_stream_depth_exceedance(p._h, None, None, _lib.ptr(a), None, None) == 0   # (any array may be NULL, days_out too)
        got = p.stream_depth_exceedance()
        assert got["days"] == 1 and np.array_equal(got["last_step"], a) and a.max() > 0
        assert p.stream_depth_exceedance_kernel_ms() > 0
        p.stream_end()
        with pytest.raises(RuntimeError, match="no stream of windows in progress"):
            p.stream_depth_exceedance()
        # the declaration outlives the stream, and is no threshold of the plan's
        with pytest.raises(RuntimeError, match="no thresholds"):
            p.stream_set_exceedance("flow")
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4, full_output=True)
        p.stream_push(pinned_like(qlat))
        p.stream_flush()
        again = p.stream_depth_exceedance()
        assert_equal(again, got, "the declaration stays; the full result's depths", 1)
        p.stream_end()
    # without full_output the depths ride in the on-demand-velocity instances: not on a plan that switched them off
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=dict(opts, velocity_on_demand=-1)) as p:
        p.stream_set_depth_exceedance(th)
        p.upload_forcing(nsteps, qlat, q0)
        with pytest.raises(NotImplementedError, match="velocity_on_demand"):
            p.stream_begin(nsteps, 4)
        assert h.trmc_stream_begin(p._h, nsteps, 4, 0, 0, 0) == _lib.TRMC_EUNSUPPORTED
        with pytest.raises(RuntimeError, match="no stream of windows in progress"):     # (the refused calls began nothing)
            p.stream_depth_exceedance()
        p.stream_begin(nsteps, 4, full_output=True)                         # (the full result is read instead)
        p.stream_push(pinned_like(qlat))
        p.stream_flush()
        assert_equal(p.stream_depth_exceedance(), got, "velocity_on_demand = -1 with full_output", 1)
        p.stream_end()
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="flow") as p:   # a declaration on a dataflow plan
        assert p.engine == "flow"
        assert h.trmc_stream_set_depth_exceedance(p._h, 2, _lib.ptr(th)) == _lib.TRMC_EINVAL
        with pytest.raises(ValueError, match="level engine"):
            p.stream_set_depth_exceedance(th)


def test_depth_exceedance_is_refused_with_reservoir_data_assimilation():
    import test_gpu_stream_reservoir_da as RD
    c = RD.case()
    with RD.open_plan(c, True, 4) as p:
        RD.declare(p, c)
        p.stream_set_depth_exceedance(np.full(p.nseg, 1.0, np.float32))
        p.upload_forcing(RD.NSTEPS, c.days[0], c.q0)
        with pytest.raises(NotImplementedError, match="(?s)depth exceedance.*reservoir data assimilation"):
            p.stream_begin(RD.NSTEPS, c.qts, reservoir_da=True)
        assert p.stream_info()["days_pushed"] == 0
        p.stream_set_depth_exceedance(None)
        p.stream_begin(RD.NSTEPS, c.qts, reservoir_da=True)                      # (without it: as before)
        p.stream_end()
