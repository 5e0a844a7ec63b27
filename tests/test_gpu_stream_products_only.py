"""A stream begun without full_output forms a step's VELOCITY only where somebody is handed it (stream_args: the kept steps of
output_stride, nowhere for hydrographs and final states) -- the library's default, decided when the stream begins.  The velocity
feeds nothing (MCsingleSegStime_f2py_NOLOOP.f90:163-169 forms it from the final depth; the next step does not read it), so every
product keeps its bits: against a plan that forces every step to form it (trmc_plan_options.velocity_on_demand < 0), against
the decimated block cut out of a full result, and -- where a full result is asked for -- every velocity against the oracle."""
import numpy as np
import pytest

import helpers as H
from oracle import oracle as O
from troute_amd import _lib, synthetic
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu

NSTEPS, QTS, NDAYS = 48, 16, 6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def conus_like():
    """a CONUS-shaped synthetic network at test size, its starting state and a sequence of distinct days"""
    net = synthetic.generate(nseg=20000, nnet=60, seed=21, nq=3)
    nseg = net["to"].shape[0]
    q0 = np.random.default_rng(4).uniform(0, 1, (nseg, 3)).astype(np.float32)
    rng = np.random.default_rng(5)
    days = [rng.uniform(0, 0.6, net["qlat"].shape).astype(np.float32) for _ in range(NDAYS)]
    return net, q0, days


def stream_days(r, days, q0, **kw):
    got = {}
    with RouteStream(r, NSTEPS, QTS, **kw) as rs:
        for item in rs.route(iter(days), q0):
            got[item[0]] = tuple(None if x is None else np.array(x, copy=True) for x in item[1:])
        rows = np.array(rs.outlet_rows, copy=True)
    assert sorted(got) == list(range(len(days)))
    return rows, got


# slices + clusters, as the timed configuration streams the CONUS network
OPTS = {"wide_min_rows": 64, "wide_k": 8}


@pytest.mark.parametrize("stride", [None, 12])
def test_products_only_default_equals_every_velocity_formed(stride):
    """outlet hydrographs, final states (and the hourly block) of the default plan are bit-identical to those of a plan that
    forms every step's velocity"""
    net, q0, days = conus_like()
    got = []
    for opts in (OPTS, dict(OPTS, velocity_on_demand=-1)):
        r = ShardedRouter(net["to"], net["params"], stream=True, options=opts)
        lag, W, C = r.plan0.lags()
        assert W > 0 and C > 0
        got.append(stream_days(r, days, q0, output_stride=stride))
        r.close()
    (rows_a, a), (rows_b, b) = got
    assert np.array_equal(rows_a, rows_b)
    for w in range(NDAYS):
        assert np.array_equal(bits(a[w][0]), bits(b[w][0])), w
        assert np.array_equal(bits(a[w][1]), bits(b[w][1])), w
        if stride:
            assert np.array_equal(bits(a[w][2]), bits(b[w][2])), w
            assert np.any(a[w][2][:, :, 1] != 0), w      # (the kept steps' velocities are formed)


def test_decimated_stream_equals_the_full_result_sliced():
    """the kept (q, v, d) of an output_stride stream -- velocities formed at the kept steps only -- equal every output_stride-th
    step of a full_output stream of the same days on the same plan"""
    net, q0, days = conus_like()
    stride = 12
    r = ShardedRouter(net["to"], net["params"], stream=True, options=OPTS)
    rows_f, full = stream_days(r, days, q0, full_output=True)
    rows_d, dec = stream_days(r, days, q0, output_stride=stride)
    r.close()
    assert np.array_equal(rows_f, rows_d)
    for w in range(NDAYS):
        want = np.ascontiguousarray(full[w][2][:, stride - 1::stride])
        assert dec[w][2].shape == want.shape and np.array_equal(bits(dec[w][2]), bits(want)), w
        assert np.array_equal(bits(dec[w][0]), bits(full[w][0])), w
        assert np.array_equal(bits(dec[w][1]), bits(full[w][1])), w


def test_full_output_stream_velocities_equal_the_oracle():
    """a full_output stream on a default plan still forms every step's velocity: every (q, v, d), the velocity plane named on
    its own, against the CPU restatement of the reference loop"""
    rng = np.random.default_rng(31)
    nseg, nsteps, qts = 4000, 24, 8
    to = H.random_network(rng, nseg)
    _, _, ups = H.reaches_from_to(to)
    up_ptr, up_idx = csr_from_lists(ups)
    from test_gpu_parity import synth_inputs
    params, qlat, q0 = synth_inputs(rng, nseg, 3)
    days = [qlat, (qlat * 0.4).astype(np.float32)]
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels",
                     options={"cluster_rows": 64, "wide_min_rows": 200, "wide_k": 4}) as p:
        lvl, _ = p.levels()
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_begin(nsteps, qts, full_output=True)
        D = p.stream_info()["slots"]
        outs = [_lib.result_empty((nseg, nsteps, 3), np.float32, always_pinned=True) for _ in range(D)]
        for d, q in enumerate(days):
            p.stream_push(pinned_like(q), fvd=outs[d % D])
        p.stream_flush()
        state = q0
        for d, q in enumerate(days):
            p.stream_wait(d)
            want = O.network_by_segment(nsteps, qts, up_ptr, up_idx, lvl, params, state, q, True, det=True)[:, 1:, :]
            got = outs[d % D]
            assert np.any(want[:, :, 1] != 0), d
            assert np.array_equal(bits(got[:, :, 1]), bits(want[:, :, 1])), d
            assert np.array_equal(bits(got), bits(want)), d
            state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
        p.stream_end()
