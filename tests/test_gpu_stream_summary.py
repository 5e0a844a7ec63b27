"""THE PER-ROW SUMMARY OF A DAY IN A STREAM OF DAYS (include/trmc.h trmc_stream_set_summary, trmc_stream_summary_dest;
csrc/stream.inc, k_stream_summary): peak flow, the 1-based step of the peak and the mean flow of every row, formed on the device
from all nsteps flows of the day when the day is handed over.

The definition is exact, so everything here compares bits (``summary_of``): peak = q[1], step = 1, then in order
``if q[t] > peak: peak, step = q[t], t`` (the first of equal peaks wins); mean = the left-to-right sum in the plan's precision over
nsteps (np.cumsum).  The flows are those of the day's result, fvd[:, :, 0] -- the oracle's day by day at plan level, and the same
stream's own full result where the oracle has no say (double precision with reservoirs, the tolerance arithmetic).

The NaN rule (a NaN never replaces a number, a NaN at step 1 stays) and ties between positive peaks are not tested here -- no flow
of these days is a NaN -- but in tests/test_gpu_products_nonfinite.py, on a network whose forcing carries NaN."""
import functools
import os
import threading

import numpy as np
import pytest

import helpers as H
from oracle import oracle as O
from troute_amd import _lib, synthetic
from troute_amd.comm import Comm
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu
_serial = [0]

KEYS = ("peak_flow", "peak_step", "mean_flow")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def summary_of(q):
    """(peak_flow, peak_step, mean_flow) of flows q [rows, nsteps] as include/trmc.h defines them"""
    q = np.ascontiguousarray(q)
    n, nsteps = q.shape
    peak, step = q[:, 0].copy(), np.ones(n, np.int32)
    for t in range(1, nsteps):
        m = q[:, t] > peak
        peak[m] = q[m, t]
        step[m] = t + 1
    mean = np.cumsum(q, axis=1, dtype=q.dtype)[:, -1] / q.dtype.type(nsteps)
    assert peak.dtype == q.dtype and mean.dtype == q.dtype
    return peak, step, mean


def assert_summary(got, q, what):
    want = summary_of(q)
    for k, g, w in zip(KEYS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape)
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, (what, k, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def summary_ring(p, n):
    return (_lib.result_empty((n,), p.dtype, always_pinned=True), _lib.result_empty((n,), np.int32, always_pinned=True),
            _lib.result_empty((n,), p.dtype, always_pinned=True))


# ---- 1. + 2. plan level ------------------------------------------------------------------------------------------------------
NSEG, NSTEPS, QTS = 4000, 24, 8
OPTIONS = {"cluster_rows": 64, "wide_min_rows": 200, "wide_k": 4}
SCALE = [1.0, 0.2, 3.0, 0.5, 2.0]                          # (the forcing falls and rises from day to day)


@functools.lru_cache(maxsize=None)
def plan_case():
    from test_gpu_parity import synth_inputs
    rng = np.random.default_rng(77)
    to = H.random_network(rng, NSEG)
    _, _, ups = H.reaches_from_to(to)
    up_ptr, up_idx = csr_from_lists(ups)
    params, qlat, q0 = synth_inputs(rng, NSEG, 3)
    dry = np.array([r for r in range(NSEG) if len(ups[r]) == 0][:6])   # headwaters without water: no flow on any day
    qlat[dry] = 0
    q0[dry] = 0
    return up_ptr, up_idx, params, qlat, q0, dry


def day_of(qlat, d, dt=np.float32):
    return (qlat * np.float32(SCALE[d % len(SCALE)])).astype(np.float32).astype(dt)


def test_summary_against_the_oracle_over_a_reused_ring():
    """a products-only stream (no full result, no decimated one) of 2 * slots + 1 days: every slot's summary buffers are used more
    than once, rows finish a day while others are in the next, both tile kernels feed the flow plane"""
    up_ptr, up_idx, params, qlat, q0, dry = plan_case()
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=OPTIONS) as p:
        lvl, _ = p.levels()
        lag, W, C = p.lags()
        p.stream_set_summary(("peak", "mean"))
        p.upload_forcing(NSTEPS, day_of(qlat, 0), q0)
        p.stream_begin(NSTEPS, QTS)
        info = p.stream_info()
        D = info["slots"]
        ndays = 2 * D + 1
        assert lag.max() > info["tiles_per_day"] and W > 0 and C > 0
        ring = [summary_ring(p, NSEG) + (_lib.result_empty((NSEG, 3), np.float32, always_pinned=True),) for _ in range(D)]
        got = []

        def take(d):
            p.stream_wait(d)
            got.append(tuple(np.array(x, copy=True) for x in ring[d % D]))
        for d in range(ndays):
            if d >= D:                                        # (the slot's last day leaves before its arrays are reused)
                if p.stream_info()["days_complete"] <= d - D:
                    p.stream_flush()
                take(d - D)
            pk, st, mn, fin = ring[d % D]
            assert p.stream_push(pinned_like(day_of(qlat, d)), q0=fin, summary=(pk, st, mn)) == d
        p.stream_flush()
        for d in range(len(got), ndays):
            take(d)
        p.stream_end()
    state, steps = q0, []
    for d in range(ndays):
        want = O.network_by_segment(NSTEPS, QTS, up_ptr, up_idx, lvl, params, state, day_of(qlat, d), True, det=True)[:, 1:, :]
        assert_summary(got[d][:3], want[:, :, 0], ("oracle", d))
        state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
        assert np.array_equal(bits(got[d][3]), bits(state)), d
        assert not want[dry, :, 0].any()
        assert not got[d][0][dry].any() and np.all(got[d][1][dry] == 1) and not got[d][2][dry].any()   # no flow: (0, 1, 0)
        steps.append(got[d][1])
    steps = np.concatenate(steps)
    assert steps.min() == 1 and steps.max() == NSTEPS and (steps == 1).sum() > len(dry) * ndays
    assert np.any((steps > 1) & (steps < NSTEPS))


@pytest.mark.parametrize("variant", ["fp32", "fp64", "tolerance"])
def test_summary_and_full_result_of_the_same_stream(variant):
    """one stream with full_output AND the summary: the summary is the reduction of that stream's own fvd[:, :, 0]"""
    up_ptr, up_idx, params, qlat, q0, dry = plan_case()
    precision = 64 if variant == "fp64" else 32
    opts = dict(OPTIONS, **({"arithmetic": "tolerance"} if variant == "tolerance" else {}))
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", precision=precision, options=opts) as p:
        dt = p.dtype
        assert np.dtype(dt).itemsize == precision // 8
        p.stream_set_summary(["mean", "peak"])
        p.upload_forcing(NSTEPS, day_of(qlat, 0, dt), q0.astype(dt))
        p.stream_begin(NSTEPS, QTS, full_output=True)
        D = p.stream_info()["slots"]
        ndays = 3
        assert D >= ndays
        outs = [_lib.result_empty((NSEG, NSTEPS, 3), dt, always_pinned=True) for _ in range(ndays)]
        sums = [summary_ring(p, NSEG) for _ in range(ndays)]
        for d in range(ndays):
            p.stream_push(pinned_like(day_of(qlat, d, dt)), fvd=outs[d], summary=sums[d])
        p.stream_flush()
        for d in range(ndays):
            p.stream_wait(d)
            assert np.isfinite(outs[d]).all() and outs[d][:, :, 0].max() > 0
            assert_summary(sums[d], outs[d][:, :, 0], (variant, d))
        p.stream_end()


# ---- 3. RouteStream ----------------------------------------------------------------------------------------------------------
RS_NSTEPS, RS_QTS, RS_DAYS = 48, 16, 6
RS_OPTS = {"wide_min_rows": 64, "wide_k": 8}


@functools.lru_cache(maxsize=None)
def rs_case(seed=11):
    net = synthetic.generate(nseg=20000, nnet=60, seed=seed, nq=3)
    nseg = net["to"].shape[0]
    q0 = np.random.default_rng(1).uniform(0, 1, (nseg, 3)).astype(np.float32)
    rng = np.random.default_rng(3)
    base = [rng.uniform(0, 0.6, net["qlat"].shape).astype(np.float32) for _ in range(3)]
    days = [(base[w % 3] * np.float32(SCALE[w % 5])).astype(np.float32) for w in range(RS_DAYS)]
    return net, q0, days


def copied(x):
    if isinstance(x, dict):
        return {k: copied(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(copied(v) for v in x)
    return None if x is None else np.array(x, copy=True)


def route_all(r, days, q0, nsteps=RS_NSTEPS, qts=RS_QTS, **kw):
    with RouteStream(r, nsteps, qts, **kw) as rs:
        items = [copied(item) for item in rs.route(iter(days), q0)]
        rows = np.array(rs.rows, copy=True)
    assert [i[0] for i in items] == list(range(len(days)))
    return items, rows


def test_routestream_summary_equals_the_reduction_of_the_full_result():
    net, q0, days = rs_case()
    nseg = net["to"].shape[0]
    r = ShardedRouter(net["to"], net["params"], stream=True, options=RS_OPTS)
    full, rows = route_all(r, days, q0, full_output=True)               # (no summary: today's tuples)
    assert [len(i) for i in full] == [4] * RS_DAYS and np.array_equal(rows, np.arange(nseg))
    summ, _ = route_all(r, days, q0, summary=("peak", "mean"))          # (the summary and no other per-row output)
    for w in range(RS_DAYS):
        assert len(summ[w]) == 4 and set(summ[w][3]) == set(KEYS)
        assert_summary([summ[w][3][k] for k in KEYS], full[w][3][:, :, 0], ("RouteStream", w))
        # the other products of the summarising stream: the bits of a stream without a summary
        assert np.array_equal(bits(summ[w][1]), bits(full[w][1])) and np.array_equal(bits(summ[w][2]), bits(full[w][2])), w
    peak_only, _ = route_all(r, days[:3], q0, summary=("peak",))
    for w in range(3):
        sm = peak_only[w][3]
        assert set(sm) == set(KEYS) and sm["mean_flow"] is None
        assert np.array_equal(bits(sm["peak_flow"]), bits(summ[w][3]["peak_flow"])) and np.array_equal(sm["peak_step"], summ[w][3]["peak_step"])
    mean_stride, _ = route_all(r, days[:3], q0, summary="mean", output_stride=12)
    for w in range(3):
        assert len(mean_stride[w]) == 5 and mean_stride[w][4]["peak_flow"] is None and mean_stride[w][4]["peak_step"] is None
        assert np.array_equal(bits(mean_stride[w][4]["mean_flow"]), bits(summ[w][3]["mean_flow"]))
        assert np.array_equal(bits(mean_stride[w][3]), bits(full[w][3][:, 11::12]))
    plain, _ = route_all(r, days[:2], q0, summary=None)
    assert [len(i) for i in plain] == [3, 3]
    # a forecast's maximum from the days' summaries: the larger peak, the time from the winning day's step
    pk = np.stack([summ[w][3]["peak_flow"] for w in range(RS_DAYS)])
    st = np.stack([summ[w][3]["peak_step"] for w in range(RS_DAYS)])
    q_all = np.concatenate([full[w][3][:, :, 0] for w in range(RS_DAYS)], axis=1)
    day = pk.argmax(axis=0)
    assert np.array_equal(bits(np.maximum.reduce(pk)), bits(q_all.max(axis=1)))
    assert np.array_equal(day * RS_NSTEPS + st[day, np.arange(nseg)] - 1, q_all.argmax(axis=1))
    with pytest.raises(ValueError, match="summary"):
        RouteStream(r, RS_NSTEPS, RS_QTS, summary=("depth",))
    r.close()


# ---- 4. reservoirs and gages -------------------------------------------------------------------------------------------------
def test_routestream_summary_with_reservoirs_and_gages():
    """at gage rows the flow after nudging, at reservoir rows the pool's outflow: what the day's fvd[:, :, 0] holds"""
    import test_gpu_stream_reservoirs_nudging as RN
    key = (3000, 78, 4)
    c = RN.case(*key)
    r = ShardedRouter(c.to, c.params, stream=True, options=RN.OPTIONS, reservoirs=(c.lakes, c.par, RN.DT), gages=c.gages)
    n = 0
    with RouteStream(r, RN.NSTEPS, RN.QTS, full_output=True, summary=("peak", "mean")) as rs:
        for item in rs.route(iter(c.days), c.q0, observations=iter(c.usgs), lastobs=(c.lv0, c.lt0),
                             da_parameters={"da_decay_coefficient": RN.DECAY, "routing_period": RN.DT}):
            assert len(item) == 5 and set(item[4]) == {"reservoir_inflow", "nudge", "lastobs"} | set(KEYS)
            q = np.array(item[3][:, :, 0])
            got = [np.array(item[4][k]) for k in KEYS]
            assert_summary(got, q, ("lakes and gages", item[0]))
            assert_summary([g[c.gages] for g in got], q[c.gages], ("gage rows", item[0]))
            assert_summary([g[c.lakes] for g in got], q[c.lakes], ("reservoir rows", item[0]))
            assert np.abs(np.array(item[4]["nudge"])).max() > 0 and item[4]["reservoir_inflow"].shape == (c.lakes.shape[0], RN.NSTEPS)
            n += 1
    assert n == len(c.days) == 4
    r.close()


# ---- 5. two ranks on one GPU -------------------------------------------------------------------------------------------------
def test_summary_on_two_ranks_equals_the_single_gpu_summary_at_their_rows():
    """two ranks (threads) on one device over the shared-memory transport: every rank gets the summary of its own rows -- the
    trunk's where it owns them, the boundary copies of the cut rows (whose flow is the exchanged one) included"""
    net, q0, days = rs_case()
    nseg = net["to"].shape[0]
    nsteps, qts, ndays = 32, 16, RS_DAYS
    r = ShardedRouter(net["to"], net["params"], stream=True, options=RS_OPTS)
    single, rows = route_all(r, days, q0, nsteps, qts, summary=("peak", "mean"))
    r.close()
    assert np.array_equal(rows, np.arange(nseg))
    world = 2
    _serial[0] += 1
    key = f"summary{os.getpid()}_{_serial[0]}"
    results, errors = [None] * world, []

    def run(rank):
        try:
            comm = Comm(rank, world, device=0, backend="shm", key=key)
            rr = ShardedRouter(net["to"], net["params"], rank=rank, world=world, device=0, stream=True, options=RS_OPTS)
            rr.enable_device_exchange(comm)
            with RouteStream(rr, nsteps, qts, summary=("peak", "mean")) as rs:
                got = [copied(item) for item in rs.route(days, q0)]
                srows = np.array(rs.rows, copy=True)
            results[rank] = (got, srows, rr.plan1 is not None)
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
        got, srows, _ = results[rank]
        assert [g[0] for g in got] == list(range(ndays))
        for w in range(ndays):
            assert len(got[w]) == 4 and set(got[w][3]) == set(KEYS)
            for k in KEYS:
                g, want = got[w][3][k], single[w][3][k][srows]
                assert g.shape == (srows.shape[0],) and g.dtype == want.dtype
                assert np.array_equal(bits(g), bits(want)), (rank, w, k)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_summary_refusals_and_bookkeeping():
    net = synthetic.generate(nseg=3000, nnet=9, seed=5, nq=3)
    nseg = net["to"].shape[0]
    up_ptr, up_idx = synthetic.upstream_csr(net["to"])
    q0 = np.zeros((nseg, 3), np.float32)
    day = pinned_like(np.full((nseg, 3), 0.1, np.float32))
    with RoutingPlan(up_ptr, up_idx, net["params"], assume_short_ts=True, engine="levels", options={"cluster_rows": 128, "wide_k": 8}) as p:
        pk, st, mn = summary_ring(p, nseg)
        with pytest.raises(ValueError, match="'peak' and / or 'mean'"):
            p.stream_set_summary(("depth",))
        p.stream_set_summary(("peak",))
        p.upload_forcing(32, day, q0)
        p.stream_begin(32, 16)
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.stream_set_summary(None)
        with pytest.raises(ValueError, match="peak_flow"):
            p.stream_push(day, summary=(np.zeros(nseg - 1, np.float32), st, None))
        with pytest.raises(ValueError, match="peak_flow"):
            p.stream_push(day, summary=(np.zeros(nseg, np.int32), st, None))
        with pytest.raises(ValueError, match="peak_step"):
            p.stream_push(day, summary=(pk, np.zeros(nseg, np.float32), None))
        with pytest.raises(ValueError, match="peak_flow, peak_step, mean_flow"):
            p.stream_push(day, summary=(pk, st))
        with pytest.raises(ValueError, match="TRMC_SUMMARY_MEAN"):          # (an array whose part of the mask is off)
            p.stream_push(day, summary=(pk, st, mn))
        with pytest.raises(ValueError, match="forcing columns"):            # (a push refused AFTER its arrays were named ...)
            p.stream_push(pinned_like(np.zeros((nseg, 2), np.float32)), summary=(pk, st, None))
        assert p.stream_info()["days_pushed"] == 0                          # (a refused push leaves no day behind)
        st[...] = -7
        fvd_none = p.stream_push(day)                                       # (... which do not wait for another day)
        assert fvd_none == 0 and p.stream_push(day, summary=(pk, None, None)) == 1
        p.stream_flush()
        p.stream_wait(1)
        assert np.all(st == -7) and pk.max() > 0
        p.stream_end()
        # the declaration outlives the stream; switched off, a stream takes no summary arrays
        p.upload_forcing(32, day, q0)
        p.stream_begin(32, 16)
        assert p.stream_push(day, summary=(pk, st, None)) == 0
        p.stream_end()
        assert st.min() >= 1 and st.max() <= 32
        p.stream_set_summary(None)
        p.upload_forcing(32, day, q0)
        p.stream_begin(32, 16)
        with pytest.raises(RuntimeError, match="begun without a summary"):
            p.stream_push(day, summary=(pk, st, None))
        assert p.stream_info()["days_pushed"] == 0
        assert p.stream_push(day) == 0
        p.stream_end()
