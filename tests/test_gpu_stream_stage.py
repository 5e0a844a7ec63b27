"""STAGE HYDROGRAPHS OF A STREAM DAY (include/trmc.h trmc_stream_set_stage, trmc_stream_stage_dest; csrc/stream.inc P_STAGE;
k_mc_tile_dpl / k_mc_ctile_dpl, which write a slot's depth plane at EVERY step instead of at a tile's last one): the depth of every
step at the rows of the day's row set.

Everything is exact and compares bits.  The reference is column 2 of the same days routed one by one as single windows with the
full result on the same plan (the state through the host), which other tests hold against the oracle and the reference Fortran;
LowerColorado is held against the reference Fortran directly.  Three days of three tiles (nsteps 48, 16 steps per launch) put
a row's store at a tile's first and last step, at a day's end and at the hand-over into the next slot; the row sets hold rows of the
first and last slice level, of the first and last cluster level, the first and last plan position, and the one row of a cluster
block that is alone in its wavefront (``case``: a chain appended to the network is cut so that its last row is a cluster level of its
own)."""
import functools

import numpy as np
import pytest

import helpers as H
from troute_amd import _lib, synthetic
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, topology_clusters
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu

NSTEPS, QTS, NDAYS = 48, 16, 3
LAYOUTS = {
    "slices+clusters": {"wide_min_rows": 64, "wide_k": 16, "cluster_rows": 128},
    "clusters-only": {"wide_min_rows": -1, "wide_k": 16, "cluster_rows": 128},
    "k4-small-clusters": {"wide_min_rows": 300, "wide_k": 4, "cluster_rows": 24},
}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:8].tolist(), [got[tuple(i)] for i in bad[:4]], [want[tuple(i)] for i in bad[:4]])


@functools.lru_cache(maxsize=None)
def case(layout):
    """a synthetic network of about 5000 rows and, as one more network, an unbranched chain whose length is the layout's slices
    plus one more cluster level than the network has, plus ONE row: that row is the only row of the last cluster level -- a cluster
    block of one row, alone in its wavefront -- and the plan's last position.  -> (to, up_ptr, up_idx, params, days, q0, rows)"""
    opt = LAYOUTS[layout]
    net = synthetic.generate(nseg=5000, nnet=14, seed=21, nq=3)
    to0, n0 = np.asarray(net["to"], np.int64), net["to"].shape[0]
    _, _, _, W, C, _ = topology_clusters(*synthetic.upstream_csr(to0), wide_min_rows=opt["wide_min_rows"], cluster_rows=opt["cluster_rows"])
    L = W + opt["cluster_rows"] * C + 1
    chain = n0 + np.arange(1, L + 1, dtype=np.int64)
    chain[-1] = -1
    to = np.concatenate([to0, chain])
    n = to.shape[0]
    up_ptr, up_idx = synthetic.upstream_csr(to)
    pos, lag, blk, W2, C2, _ = topology_clusters(up_ptr, up_idx, wide_min_rows=opt["wide_min_rows"], cluster_rows=opt["cluster_rows"])
    assert (W2, C2) == (W, C + 1) and C > 0 and (W > 0) == (layout != "clusters-only")
    last = np.flatnonzero(lag == W + C2 - 1)
    assert last.tolist() == [n - 1] and pos[n - 1] == pos.max()          # alone in its level, hence in its block and wavefront
    rng = np.random.default_rng(5)
    pick = np.r_[0:n0, rng.integers(0, n0, L)]
    params = np.ascontiguousarray(net["params"][pick])
    days = [np.ascontiguousarray((rng.uniform(0, 0.6, (n, 3)) * s).astype(np.float32)) for s in (1.0, 0.3, 2.0)]
    q0 = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    sets = [np.flatnonzero(lag == W)[:3], np.flatnonzero(lag == W + C2 - 2)[:3], last, [int(np.argmin(pos)), int(np.argmax(pos))],
            rng.integers(0, n, 40)]
    if W > 0:
        sets += [np.flatnonzero(lag == 0)[:3], np.flatnonzero(lag == W - 1)[:3]]
    rows = np.unique(np.concatenate([np.asarray(s, np.int64) for s in sets]))
    for lv in ([0, W - 1] if W > 0 else []) + [W, W + C2 - 1]:
        assert np.any(lag[rows] == lv), (layout, lv)
    return to, up_ptr, up_idx, params, days, q0, rows


def window_days(p, days, q0):
    """the days one by one as single windows with the full result on the plan itself: [(fvd [n, nsteps, 3], final state)]"""
    out, state = [], q0.astype(p.dtype)
    for q in days:
        p.upload_forcing(NSTEPS, q.astype(p.dtype), state)
        p.route_device(NSTEPS, QTS, True)
        fvd, state = p.download_fvd().copy(), p.download_final_state()
        out.append((fvd, state))
    return out


def stream_days(p, days, q0, rows, stage=True, full_output=False, output_stride=0, summary=None, nsteps=NSTEPS, qts=QTS):
    """the days as one stream at plan level, the row set ``rows``: [dict of copies per day] -- "stage", "hyd", "final", "fvd", the
    summary's parts"""
    dt, n = p.dtype, p.nseg
    rs = p.rowset(rows)
    p.stream_set_stage(stage)
    p.stream_set_summary(summary)
    p.upload_forcing(nsteps, days[0].astype(dt), q0.astype(dt))
    p.stream_begin(nsteps, qts, slots=len(days), full_output=full_output, output_stride=output_stride)
    D = p.stream_info()["slots"]
    assert D >= len(days)
    keep = nsteps // output_stride if output_stride else nsteps

    def arr(shape, t=dt, on=True):
        return _lib.result_empty(shape, t, always_pinned=True) if on else None
    pd = bool(summary) and "peak_depth" in summary
    ring = [{"stage": arr((rows.shape[0], nsteps), on=stage), "hyd": arr((rows.shape[0], nsteps)), "final": arr((n, 3)),
             "fvd": arr((n, keep, 3), on=full_output or output_stride), "peak_depth": arr((n,), on=pd),
             "peak_depth_step": arr((n,), np.int32, on=pd)} for _ in days]
    for r in ring:
        if r["stage"] is not None:
            r["stage"][...] = -1
    for d, q in enumerate(days):
        r = ring[d]
        sm = (None, None, None, r["peak_depth"], r["peak_depth_step"]) if pd else None
        assert p.stream_push(pinned_like(q.astype(dt)), rowset=rs, hyd=r["hyd"], q0=r["final"], fvd=r["fvd"], summary=sm, stage=r["stage"]) == d
    p.stream_flush()
    got = []
    for d in range(len(days)):
        p.stream_wait(d)
        got.append({k: None if v is None else np.array(v, copy=True) for k, v in ring[d].items()})
    p.stream_end()
    return got


def open_plan(layout, precision=32, **more):
    to, up_ptr, up_idx, params, days, q0, rows = case(layout)
    return RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", precision=precision, options=dict(LAYOUTS[layout], **more))


# ---- 1. against single windows, in three layouts -----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_stage_equals_the_depths_of_the_days_routed_as_windows(layout):
    to, up_ptr, up_idx, params, days, q0, rows = case(layout)
    with open_plan(layout) as p:
        lag, W, C = p.lags()
        assert C > 0 and (W > 0) == (layout != "clusters-only") and np.count_nonzero(lag == W + C - 1) == 1
        want = window_days(p, days, q0)
        got = stream_days(p, days, q0, rows)
        off = stream_days(p, days, q0, rows, stage=False)
    for d in range(NDAYS):
        assert_same(got[d]["stage"], np.ascontiguousarray(want[d][0][rows, :, 2]), (layout, d, "stage"))
        assert_same(got[d]["hyd"], np.ascontiguousarray(want[d][0][rows, :, 0]), (layout, d, "hydrographs"))
        assert_same(got[d]["final"], want[d][1], (layout, d, "final state"))
        assert_same(off[d]["hyd"], got[d]["hyd"], (layout, d, "hydrographs of a stream without stage"))
        assert_same(off[d]["final"], got[d]["final"], (layout, d, "final state of a stream without stage"))
        assert got[d]["stage"].max() > 0 and np.isfinite(got[d]["stage"]).all()
    assert not np.array_equal(got[0]["stage"], got[1]["stage"])


# ---- 2. precisions and arithmetics -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fp64", "tolerance"])
def test_stage_in_double_precision_and_in_the_tolerance_arithmetic(variant):
    """(fp32 exact: test 1.)  The tolerance arithmetic against the stream's own windows in that arithmetic."""
    layout = "slices+clusters"
    to, up_ptr, up_idx, params, days, q0, rows = case(layout)
    more = {"arithmetic": "tolerance"} if variant == "tolerance" else {}
    with open_plan(layout, 64 if variant == "fp64" else 32, **more) as p:
        assert np.dtype(p.dtype).itemsize == (8 if variant == "fp64" else 4)
        want = window_days(p, days, q0)
        got = stream_days(p, days, q0, rows)
    for d in range(NDAYS):
        assert_same(got[d]["stage"], np.ascontiguousarray(want[d][0][rows, :, 2]), (variant, d, "stage"))
        assert_same(got[d]["final"], want[d][1], (variant, d, "final state"))


# ---- 3. with the other products ----------------------------------------------------------------------------------------------
def test_stage_with_output_stride_full_output_and_peak_depth():
    layout, stride = "slices+clusters", 12
    to, up_ptr, up_idx, params, days, q0, rows = case(layout)
    with open_plan(layout) as p:
        want = window_days(p, days, q0)
        dec = stream_days(p, days, q0, rows, output_stride=stride)
        full = stream_days(p, days, q0, rows, full_output=True)
        pkd = stream_days(p, days, q0, rows, summary=("peak_depth",))
        both = stream_days(p, days, q0, rows, summary=("peak_depth",), output_stride=stride)
    for d in range(NDAYS):
        ref = np.ascontiguousarray(want[d][0][rows, :, 2])
        for name, run in (("output_stride", dec), ("full_output", full), ("peak_depth", pkd), ("peak_depth + output_stride", both)):
            assert_same(run[d]["stage"], ref, (name, d, "stage"))
            assert_same(run[d]["final"], want[d][1], (name, d, "final state"))
        for run in (dec, both):                                            # every kept step of the hourly block
            assert run[d]["fvd"].shape == (to.shape[0], NSTEPS // stride, 3)
            assert_same(np.ascontiguousarray(run[d]["fvd"][rows, :, 2]), np.ascontiguousarray(run[d]["stage"][:, stride - 1::stride]), (d, "kept steps"))
            assert_same(run[d]["fvd"], np.ascontiguousarray(want[d][0][:, stride - 1::stride]), (d, "hourly block"))
        assert_same(np.ascontiguousarray(full[d]["fvd"][rows, :, 2]), full[d]["stage"], (d, "out[row][:, 2]"))
        for run in (pkd, both):
            st = run[d]["stage"]
            assert_same(st.max(axis=1), run[d]["peak_depth"][rows], (d, "peak depth"))
            assert np.array_equal(st.argmax(axis=1) + 1, run[d]["peak_depth_step"][rows]), (d, "step of the peak depth")


# ---- 4. reservoirs and gages -------------------------------------------------------------------------------------------------
def test_stage_at_reservoir_and_gage_rows():
    """a reservoir row's stage is its pool's elevation, a gage row's the step's own depth (the nudge changes the flow only): the
    same days as windows on the same plan (set_reservoirs, set_nudging); then end to end through ShardedRouter / RouteStream"""
    import test_gpu_stream_reservoirs_nudging as RN
    c = RN.case(3000, 78, 4)
    tabs, _ = RN.day_tables(c, len(c.days))
    rows = np.unique(np.concatenate([c.lakes, c.gages, np.arange(0, c.n, 97)]))
    lake_at, gage_at = np.searchsorted(rows, c.lakes), np.searchsorted(rows, c.gages)
    with RN.open_plan(c) as p:
        want = RN.window_days(p, c, tabs)
        rs = p.rowset(rows)
        p.stream_set_stage(True)
        p.set_reservoirs(c.lakes, c.par, RN.DT)
        p.stream_set_gages(c.gages)
        p.upload_forcing(RN.NSTEPS, c.days[0], c.q0)
        p.stream_begin(RN.NSTEPS, RN.QTS, slots=len(c.days))       # (a slot per day: every array is read after the flush)
        assert p.stream_info()["slots"] >= len(c.days)
        stg = [_lib.result_empty((rows.shape[0], RN.NSTEPS), np.float32, always_pinned=True) for _ in c.days]
        nud = [_lib.result_empty((c.gages.shape[0], RN.NSTEPS), np.float32, always_pinned=True) for _ in c.days]
        for d, q in enumerate(c.days):
            mode, a, w = tabs[d]
            p.stream_push(pinned_like(q), rowset=rs, nudging=(mode, a, w, c.usgs[d][:, 0]), nudge=nud[d], stage=stg[d])
        p.stream_flush()
        for d in range(len(c.days)):
            p.stream_wait(d)
            fvd = want[d][0]
            assert_same(stg[d][lake_at], np.ascontiguousarray(fvd[c.lakes, :, 2]), (d, "pool elevations"))
            assert_same(stg[d][gage_at], np.ascontiguousarray(fvd[c.gages, :, 2]), (d, "gage rows"))
            assert_same(np.array(stg[d]), np.ascontiguousarray(fvd[rows, :, 2]), (d, "every row of the set"))
            assert_same(np.array(nud[d]), want[d][2], (d, "nudge record"))
            assert np.abs(nud[d]).max() > 0 and stg[d][lake_at].min() > 0        # (the gages were nudged; the pools hold water)
        p.stream_end()
        p.stream_set_stage(False)
    r = ShardedRouter(c.to, c.params, stream=True, options=RN.OPTIONS, reservoirs=(c.lakes, c.par, RN.DT), gages=c.gages)
    runs = {}
    for full in (True, False):
        with RouteStream(r, RN.NSTEPS, RN.QTS, full_output=full, stage=True) as rs_:
            items = []
            for item in rs_.route(iter(c.days), c.q0, observations=iter(c.usgs), lastobs=(c.lv0, c.lt0),
                                  da_parameters={"da_decay_coefficient": RN.DECAY, "routing_period": RN.DT}):
                assert set(item[-1]) == {"reservoir_inflow", "nudge", "lastobs", "stage"}
                items.append(tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in item[:-1]) + ({k: np.array(v, copy=True) for k, v in item[-1].items() if k != "lastobs"},))
            out_rows = np.array(rs_.outlet_rows)
        runs[full] = items
    with RouteStream(r, RN.NSTEPS, RN.QTS) as rs_:                          # (off again: the dict of a router with reservoirs and gages)
        for item in rs_.route(iter(c.days[:1]), c.q0, observations=iter(c.usgs), lastobs=(c.lv0, c.lt0)):
            assert set(item[-1]) == {"reservoir_inflow", "nudge", "lastobs"}
    r.close()
    for d in range(len(c.days)):
        f, l = runs[True][d], runs[False][d]
        assert f[-1]["stage"].shape == (out_rows.shape[0], RN.NSTEPS)
        assert_same(f[-1]["stage"], np.ascontiguousarray(f[3][out_rows, :, 2]), (d, "RouteStream, full_output"))
        assert_same(l[-1]["stage"], f[-1]["stage"], (d, "RouteStream, products only"))
        assert_same(l[-1]["stage"], np.ascontiguousarray(want[d][0][out_rows, :, 2]), (d, "RouteStream against the windows"))
        assert_same(l[1], f[1], (d, "hydrographs"))


# ---- 5. against the reference ------------------------------------------------------------------------------------------------
def test_stage_of_lowercolorado_equals_the_reference_fortran():
    """LowerColorado (11 248 rows, 288 steps of 300 s) as a stream of one day, stage at 250 rows: the golden's 100 probe rows, the
    outlet, 149 more.  Every step of every row of the set against the reference Fortran's depth, bit for bit:
    tests/golden/lowercolorado_stage_rows.npz holds it -- the reference Fortran kernel driven through the restated loop
    (oracle.network(..., ref_name="libmc_ref_qj0_f32.so")), as tests/golden/lowercolorado_golden.npz was made, which it equals at
    that file's probe rows and time slices; both are compared."""
    import os
    lc = H.LowerColorado()
    g = lc.golden()
    fx = np.load(os.path.join(H.GOLDEN, "lowercolorado_stage_rows.npz"))
    rows, depth = np.asarray(fx["rows"], np.int64), fx["depth"]
    up_ptr, up_idx = lc.csr()
    n = lc.nseg
    has_down = np.zeros(n, bool)
    has_down[up_idx] = True
    outlets = np.flatnonzero(~has_down)
    probes = np.asarray(g["probes"], np.int64)
    assert rows.shape[0] >= 200 and depth.shape == (rows.shape[0], lc.nts) and depth.dtype == np.float32
    assert np.isin(outlets, rows).all() and np.isin(probes, rows).all() and np.all(np.diff(rows) > 0)
    at = np.searchsorted(rows, probes)
    assert_same(depth[at], np.ascontiguousarray(g["shortts_f32_probes"][:, 1:, 2]), "the fixture against the golden's probe rows")
    assert_same(np.ascontiguousarray(depth[:, g["tsel"] - 1]), np.ascontiguousarray(g["shortts_f32_tsel"][rows, :, 2]), "the fixture against the golden's time slices")
    with RoutingPlan(up_ptr, up_idx, lc.params9, assume_short_ts=True, engine="levels", options={"cluster_rows": 128}) as p:
        got = stream_days(p, [lc.qlat], lc.q0, rows, nsteps=lc.nts, qts=lc.qts)[0]
    assert_same(got["stage"], depth, "stage at every step of every row of the set")
    assert_same(got["hyd"][at], np.ascontiguousarray(g["shortts_f32_probes"][:, 1:, 0]), "probe rows, flows")
    assert got["stage"][np.searchsorted(rows, outlets)].max() > 0


def test_stage_of_a_boundary_row_is_zero():
    """a plan with boundary rows (prescribed hydrographs, routed by nobody): their stage is 0, as column 2 of a full result is,
    and the rows below them have the depths of the same stream with the full result"""
    from troute_amd import comm as X
    layout = "slices+clusters"
    to, up_ptr, up_idx, params, days, q0, rows = case(layout)
    heads = np.flatnonzero((np.diff(up_ptr) == 0) & (to >= 0))[:3]
    boundary = np.zeros(to.shape[0], np.uint8)
    boundary[heads] = 1
    below = to[heads]
    rows = np.unique(np.concatenate([rows, heads, below, to[below][to[below] >= 0]]))
    at = np.searchsorted(rows, heads)
    flows = np.tile(np.linspace(0.5, 3.0, NSTEPS, dtype=np.float32), (3, 1))       # (the same for each: their order does not matter)
    runs = {}
    with RoutingPlan(up_ptr, up_idx, params, boundary=boundary, assume_short_ts=True, engine="levels", options=LAYOUTS[layout]) as p:
        assert p.nboundary == 3
        buf = X.DeviceBuffer.from_array(p.info()["device"], flows)
        rs = p.rowset(rows)
        p.stream_set_stage(True)
        for full in (False, True):
            p.upload_forcing(NSTEPS, days[0], q0)
            p.stream_begin(NSTEPS, QTS, slots=NDAYS, full_output=full)
            stg = [_lib.result_empty((rows.shape[0], NSTEPS), np.float32, always_pinned=True) for _ in days]
            fvd = [_lib.result_empty((to.shape[0], NSTEPS, 3), np.float32, always_pinned=True) if full else None for _ in days]
            for d, q in enumerate(days):
                stg[d][...] = -1
                p.stream_push(pinned_like(q), boundary_q_ptr=buf.ptr, rowset=rs, fvd=fvd[d], stage=stg[d])
            p.stream_flush()
            for d in range(NDAYS):
                p.stream_wait(d)
            runs[full] = ([np.array(x) for x in stg], [None if x is None else np.array(x) for x in fvd])
            p.stream_end()
        p.stream_set_stage(False)
    for d in range(NDAYS):
        lean, (full, fvd) = runs[False][0][d], (runs[True][0][d], runs[True][1][d])
        assert not lean[at].any() and not full[at].any(), d
        assert_same(full, np.ascontiguousarray(fvd[rows, :, 2]), (d, "full_output: out[row][:, 2]"))
        assert_same(lean, full, (d, "the depth plane against the full result"))
        assert lean[np.searchsorted(rows, below)].min() > 0 and np.all(fvd[below, :, 0] > 0)


# ---- 6. errors and off -------------------------------------------------------------------------------------------------------
def test_stage_refusals_and_a_stream_without_it():
    layout = "slices+clusters"
    to, up_ptr, up_idx, params, days, q0, rows = case(layout)
    day = pinned_like(days[0])
    lib = _lib.lib()
    with open_plan(layout) as p:
        rs = p.rowset(rows)
        good = _lib.result_empty((rows.shape[0], NSTEPS), np.float32, always_pinned=True)
        good[...] = -7
        # a stream begun without stage hands no such array over, and asking for one is TRMC_ESTATE
        p.upload_forcing(NSTEPS, day, q0)
        p.stream_begin(NSTEPS, QTS)
        assert lib.trmc_stream_stage_dest(p._h, _lib.ptr(good)) == _lib.TRMC_ESTATE
        with pytest.raises(RuntimeError, match="begun without stage"):
            p.stream_push(day, rowset=rs, stage=good)
        assert lib.trmc_stream_set_stage(p._h, 1) == _lib.TRMC_ESTATE           # (a stream is in progress)
        assert p.stream_info()["days_pushed"] == 0
        assert p.stream_push(day, rowset=rs) == 0
        p.stream_flush()
        p.stream_wait(0)
        assert np.all(good == -7)
        p.stream_end()
        assert lib.trmc_stream_stage_dest(p._h, _lib.ptr(good)) == _lib.TRMC_ESTATE  # (no stream in progress)
        # with stage: a day with no row set is TRMC_EINVAL, and the refused push leaves nothing behind
        p.stream_set_stage(True)
        p.upload_forcing(NSTEPS, day, q0)
        p.stream_begin(NSTEPS, QTS)
        assert lib.trmc_stream_stage_dest(p._h, _lib.ptr(good)) == _lib.TRMC_OK
        assert lib.trmc_stream_push(p._h, _lib.ptr(day), day.shape[1], None, -1, None, None, None) == _lib.TRMC_EINVAL
        assert lib.trmc_stream_stage_dest(p._h, None) == _lib.TRMC_OK
        with pytest.raises(ValueError, match="rowset is required"):
            p.stream_push(day, stage=good)
        assert p.stream_info()["days_pushed"] == 0
        assert p.stream_push(day, rowset=rs) == 0                                # (a day that hands none over)
        assert p.stream_push(day, rowset=rs, stage=good) == 1
        p.stream_flush()
        p.stream_wait(1)
        assert good.min() >= 0
        p.stream_end()
        p.stream_set_stage(False)
    # without full_output the store rides in the on-demand-velocity instances: not on a plan that switched them off
    with open_plan(layout, velocity_on_demand=-1) as p:
        p.stream_set_stage(True)
        p.upload_forcing(NSTEPS, day, q0)
        with pytest.raises(NotImplementedError, match="velocity_on_demand"):
            p.stream_begin(NSTEPS, QTS)
        p.stream_begin(NSTEPS, QTS, full_output=True)                            # (the full result is gathered instead)
        p.stream_end()
    # the dataflow engine runs no stream
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="flow") as p:
        assert lib.trmc_stream_set_stage(p._h, 1) == _lib.TRMC_EINVAL
        with pytest.raises(ValueError, match="level engine"):
            p.stream_set_stage(True)


def test_stage_is_refused_with_reservoir_data_assimilation():
    import test_gpu_stream_reservoir_da as RD
    c = RD.case()
    with RD.open_plan(c, True, 4) as p:
        RD.declare(p, c)
        p.stream_set_stage(True)
        p.upload_forcing(RD.NSTEPS, c.days[0], c.q0)
        with pytest.raises(NotImplementedError, match="(?s)stage.*reservoir data assimilation"):
            p.stream_begin(RD.NSTEPS, c.qts, reservoir_da=True)
        assert p.stream_info()["days_pushed"] == 0
        p.stream_set_stage(False)
        p.stream_begin(RD.NSTEPS, c.qts, reservoir_da=True)                      # (without it: as before)
        p.stream_end()
