"""WINDOWS AND STREAMS OF DAYS TAKING TURNS ON ONE PLAN.  The tiles of a window (route_advance_t) and of a stream of days
(stream.inc) are set up by one helper (tile_setup, host_levels.inc) on the plan's ONE set of buffers: the class every wide row
showed in its last tile (the in-block partition's history), the three hot lists with their marks, and the count of the launches
that carried them -- which of the lists a launch reads.  Whatever routes next on the plan picks all of that up where the piece
before left it.

The network, inputs and options of test_gpu_tile_lean_loop (1 200 rows: three slices of 300 over a tail in clusters, 32 steps, K = 8)
on one fp32 plan in the exact arithmetic: a window, a products-only stream of two days, a window, a stream of two days with
output_stride = 4, a window -- every piece from the state the piece before left on the device.  Bit for bit against the oracle
chained as oracle_days() chains it: every window's full result, every stream day's hydrographs of all rows and final state, the
kept steps of the strided stream.  Then the same schedule with the hot rows off, and with the partition off.

The fp64 instances of the tile kernels take such turns too, on a precision-64 plan against the fp64 oracle: a window (k_mc_tile /
k_mc_ctile <double, false, false, false>), a window that decimates as it goes (DEC), a products-only stream (LAZYV), a strided
one (DEC and LAZYV).

The step kernels of rows with a lag (trmc_plan_set_lag) in the other arithmetics -- k_mc_step <float, SHORT, LAG, TOL>,
<double, SHORT, LAG> and k_mc_step_rda <SHORT, LAG> -- on the lagged chain of test_gpu_window_api.

Tiles that are no whole number of stages (K = 12: runs of 8 + 4 steps, a last tile of 4 or 6): what both tile kernels stage, write
as runs and keep of a window, in the float4 and in the scalar form."""
import functools

import numpy as np
import pytest

import test_gpu_ctile_tables as CT
import test_gpu_tile_lean_loop as LL
from oracle import oracle as O
from troute_amd import _lib
from troute_amd.comm import DeviceBuffer
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

NSTEPS, QTS = LL.NSTEPS, LL.QTS
# (piece, days, output_stride): seven days in all
SCHEDULE = [("window", 1, 0), ("stream", 2, 0), ("window", 1, 0), ("stream", 2, 4), ("window", 1, 0)]
NDAYS = sum(p[1] for p in SCHEDULE)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def forcing(i, dtype=np.float32):
    """day i of the schedule: the two days of the lean-loop test in turn"""
    return LL.inputs()[4][i % 2].astype(dtype)


@functools.lru_cache(maxsize=None)
def oracle_chain(dtype=np.float32):
    """the seven days by the CPU restatement of the reference loop (fp32: with the deterministic power, as oracle_days() has it),
    the state handed on as new_q0 does: [n, NSTEPS, 3] each"""
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    state, out = q0.astype(dtype), []
    for i in range(NDAYS):
        w = O.network_by_segment(NSTEPS, QTS, up_ptr, up_idx, level, params.astype(dtype), state, forcing(i, dtype), True,
                                 **({"det": True} if dtype == np.float32 else {}))[:, 1:, :]
        w.setflags(write=False)
        out.append(w)
        state = np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], 1)
    return out


def stream_days(plan, rs, first, ndays, output_stride):
    """days first .. first + ndays - 1 as one stream from the state on the device; per day (hydrographs, final state, kept block)"""
    n, dt = plan.nseg, plan.dtype
    plan.upload_forcing(NSTEPS, forcing(first, dt), None)
    plan.stream_begin(NSTEPS, QTS, output_stride=output_stride)
    keep, out = [pinned_like(forcing(first + d, dt)) for d in range(ndays)], []
    for q in keep:
        hyd = _lib.result_empty((n, NSTEPS), dt, always_pinned=True)
        st = _lib.result_empty((n, 3), dt, always_pinned=True)
        blk = _lib.result_empty((n, NSTEPS // output_stride, 3), dt, always_pinned=True) if output_stride else None
        plan.stream_push(q, rowset=rs, hyd=hyd, q0=st, fvd=blk)
        out.append((hyd, st, blk))
    plan.stream_flush()
    for d in range(ndays):
        plan.stream_wait(d)
    info = plan.stream_info()
    plan.stream_end()
    assert info["wide_levels"] == 3 and info["cluster_levels"] >= 2, info
    return out


def check_stream(got, want, first, stride):
    for d, (hyd, st, blk) in enumerate(got):
        w = want[first + d]
        assert hyd.dtype == w.dtype and np.array_equal(bits(hyd), bits(w[:, :, 0])), first + d
        assert np.array_equal(bits(st), bits(np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], 1))), first + d
        if stride:
            kept = np.ascontiguousarray(w[:, stride - 1::stride])
            assert blk.shape == kept.shape and np.any(kept[:, :, 1] != 0)
            assert np.array_equal(bits(blk), bits(kept)), first + d


# (trmc_plan_options: 0 is the default and < 0 is off -- the plan's own hot_rows = 0 and tile_perm_group = 0)
@pytest.mark.parametrize("extra", [{}, {"hot_rows": -1}, {"tile_perm_group": -1}], ids=["defaults", "hot_rows_off", "partition_off"])
def test_windows_and_streams_hand_the_tiles_state_on(extra):
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    want = oracle_chain()
    n = params.shape[0]
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={**LL.OPTS, **extra}) as plan:
        assert plan.precision == 32 and plan.arithmetic == "exact"
        rs = plan.rowset(np.arange(n))
        day = 0
        for piece, ndays, stride in SCHEDULE:
            if piece == "window":
                plan.upload_forcing(NSTEPS, forcing(day), q0 if day == 0 else None)
                stats = plan.route_device(NSTEPS, QTS, True)
                assert stats["wide_levels"] == 3 and stats["wide_segment_steps"] == n * NSTEPS, stats
                assert np.array_equal(bits(plan.download_fvd()), bits(want[day])), (piece, day)
            else:
                check_stream(stream_days(plan, rs, day, ndays, stride), want, day, stride)
            day += ndays
        assert day == NDAYS
        # (the lists were in use where they are on -- rows over bank and rows of many iterations are among the slices' -- and
        # only there: they go with the partition)
        assert (plan.hot_rows() > 0) == (not extra), plan.hot_rows()


def test_an_fp64_plan_takes_such_turns_too():
    """window, window that decimates as it goes (trmc_plan_set_output_stride: the kept steps of every row), products-only
    stream, strided stream: between them every <double, ...> instance of k_mc_tile and k_mc_ctile, against the fp64 oracle"""
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    want = oracle_chain(np.float64)
    n = params.shape[0]
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=LL.OPTS, precision=64) as plan:
        assert plan.dtype == np.float64
        rs = plan.rowset(np.arange(n))
        for day, stride in enumerate((0, 4)):
            plan.set_output_stride(stride)
            plan.upload_forcing(NSTEPS, forcing(day, np.float64), q0.astype(np.float64) if day == 0 else None)
            stats = plan.route_device(NSTEPS, QTS, True)
            assert stats["wide_levels"] == 3 and stats["wide_segment_steps"] == n * NSTEPS, stats
            assert np.array_equal(bits(plan.download_fvd()), bits(want[day])), day
            if stride:
                plan.fetch_begin(rs, True, stride)
                kept = np.ascontiguousarray(want[day][:, stride - 1::stride])
                assert np.array_equal(bits(plan.fetch_wait()[2]), bits(kept)), day
        plan.set_output_stride(0)
        check_stream(stream_days(plan, rs, 2, 2, 0), want, 2, 0)
        check_stream(stream_days(plan, rs, 4, 2, 4), want, 4, 4)


def test_a_tolerance_window_that_decimates_as_it_goes():
    """k_mc_tile / k_mc_ctile <float, TOL, DEC> without LAZYV -- a window of a tolerance-arithmetic plan that writes the kept steps
    aside: the same full result as the window that does not (<float, TOL>), bit for bit, and the kept steps are its slices"""
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    n = params.shape[0]
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={**LL.OPTS, "arithmetic": "tolerance"}) as plan:
        assert plan.arithmetic == "tolerance"
        rs = plan.rowset(np.arange(n))
        full = []
        for stride in (0, 4):
            plan.set_output_stride(stride)
            plan.upload_forcing(NSTEPS, forcing(0), q0)
            stats = plan.route_device(NSTEPS, QTS, True)
            assert stats["wide_levels"] == 3 and stats["wide_segment_steps"] == n * NSTEPS, stats
            full.append(plan.download_fvd())
        plan.fetch_begin(rs, True, 4)
        kept = plan.fetch_wait()[2]
        assert np.array_equal(bits(full[0]), bits(full[1])) and np.all(np.isfinite(full[0]))
        assert np.array_equal(bits(kept), bits(np.ascontiguousarray(full[1][:, 3::4])))


@pytest.mark.parametrize("variant", ["tolerance", "fp64", "reservoir_da"])
def test_lagged_rows_in_the_other_arithmetics_equal_two_phase_routing(variant):
    """The chain of test_gpu_window_api.test_time_skewed_rows_equal_two_phase_routing -- rows 0..9 feeding, through a cut, rows
    10..19 that run 2 K launches behind and get their boundary values chunk by chunk -- on the level engine: a plan in the
    tolerance arithmetic, a precision-64 plan, and a plan whose reservoirs carry data-assimilation tables (one lake in either
    chain, RFC lakes whose use_forecast is 0: the _rda instances route the window, test_gpu_ctile_tables).  Bit for bit the whole
    chain routed by one ordinary plan of the same kind (the LAG = false instance of the same arithmetic)."""
    n = 10
    rng = np.random.default_rng(7)
    p = np.stack([np.full(2 * n, 300.0), rng.uniform(300, 3000, 2 * n), rng.uniform(1, 9, 2 * n), np.zeros(2 * n),
                  np.zeros(2 * n), np.full(2 * n, 0.06), np.full(2 * n, 0.12), rng.uniform(0.2, 1.5, 2 * n),
                  rng.uniform(1e-3, 2e-2, 2 * n)], 1)
    p[:, 3] = p[:, 2] * 5 / 3
    p[:, 4] = 3 * p[:, 3]
    p = p.astype(np.float32)
    dt = np.float64 if variant == "fp64" else np.float32
    qlat = rng.uniform(0, 0.4, (2 * n, 3)).astype(dt)
    q0 = rng.uniform(0, 1, (2 * n, 3)).astype(dt)
    nsteps, qts, K = 30, 12, 4
    kw = dict(assume_short_ts=True, engine="levels", precision=64 if variant == "fp64" else 32,
              options={"arithmetic": "tolerance"} if variant == "tolerance" else None)
    lakes = np.array([4, n + 4], np.int64)                    # (rows of the whole chain: one lake above the cut, one below)
    par, h0 = CT.lake_parameters(2)
    if variant == "reservoir_da":
        q0[lakes, 2] = h0
        q0[lakes, 1] = 0

    def tables(plan, rows):
        if variant != "reservoir_da":
            return
        plan.set_reservoirs(rows, par, CT.DT)
        plan.set_reservoir_da(np.full(2, 4, np.int32), np.arange(2, dtype=np.int32),
                              rfc=(np.full((2, 6), 1.0e3, np.float32), np.zeros(2, np.float32),
                                   np.tile(np.array([1, 6, 0, 3600, 10], np.int32), (2, 1))))

    ups = [[]] + [[i - 1] for i in range(1, 2 * n)]
    with RoutingPlan(*csr_from_lists(ups), p, **kw) as plan:
        tables(plan, lakes)
        want = plan.route(nsteps, qts, True, qlat, q0)
        assert want.dtype == dt and plan.arithmetic == ("tolerance" if variant == "tolerance" else "exact")
        assert plan.stats()["main_launches"] == nsteps       # (one step per launch: the step kernels)
    # merged table: rows 0..9 upper chain, row 10 = boundary copy of row 9, rows 11..20 = lower chain (lag 2K)
    ups_m = [[]] + [[i - 1] for i in range(1, n)] + [[]] + [[n]] + [[i - 1] for i in range(n + 2, 2 * n + 1)]
    sel = list(range(n)) + [n - 1] + list(range(n, 2 * n))
    boundary = np.zeros(2 * n + 1, np.uint8)
    boundary[n] = 1
    lag = np.zeros(2 * n + 1, np.int32)
    lag[n + 1:] = 2 * K
    esz = np.dtype(dt).itemsize
    with RoutingPlan(*csr_from_lists(ups_m), p[sel], boundary, **kw) as plan:
        plan.set_lag(lag)
        tables(plan, np.where(lakes >= n, lakes + 1, lakes))
        plan.upload_forcing(nsteps, qlat[sel], q0[sel], None)
        plan.route_begin(nsteps, qts, True)
        rs = plan.rowset(np.array([n - 1], np.int64))
        last = nsteps + 2 * K
        bufs = []
        for c in range(-(-last // K)):
            plan.route_advance(min((c + 1) * K, last))
            tb, te = c * K, min(nsteps, (c + 1) * K)
            if te > tb:
                b = DeviceBuffer(0, (te - tb) * esz)
                plan.gather_flow_range(rs, tb, te, b.ptr, te - tb)
                plan.set_boundary_flow_range(tb, te, b.ptr, te - tb)
                bufs.append(b)
        st = plan.route_end()
        assert st["main_launches"] == last and st["wide_levels"] == 0, st
        got = plan.download_fvd()
    assert np.all(np.isfinite(want)) and np.all(want[:, -1, 0] > 0)
    assert np.array_equal(bits(got[:n]), bits(want[:n]))
    assert np.array_equal(bits(got[n + 1:]), bits(want[n:]))


@functools.lru_cache(maxsize=None)
def oracle_window(nsteps, qts):
    """one window of nsteps steps from the lean-loop test's first day (its first nsteps / qts forcing columns): [n, nsteps, 3]"""
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    ql = np.ascontiguousarray(days[0][:, :nsteps // qts])
    w = O.network_by_segment(nsteps, qts, up_ptr, up_idx, level, params, q0, ql, True, det=True)[:, 1:, :]
    w.setflags(write=False)
    return ql, w


@pytest.mark.parametrize("stride", [0, 5], ids=["full", "stride5"])
@pytest.mark.parametrize("nsteps,qts", [(28, 4), (30, 5)], ids=["float4_runs", "scalar_runs"])
def test_tiles_that_are_no_whole_number_of_stages(nsteps, qts, stride):
    """K = 12 against stages of 8 steps: a tile is staged and written as a run of 8 steps and one of 4, the window's last tile
    (4 steps of 28; 6 of 30) as one short run.  28 steps, qts = 4: nsteps and K are multiples of 4, every run goes out as
    16-byte pieces; 30 steps, qts = 5: the scalar form, and a last run of 6 steps -- no multiple of 4.  With output_stride = 5
    the kept steps 5, 10 | 15, 20 | 25 (, 30) lie in the first and in the second run of a tile and in every tile: the block
    kept aside is those steps of the full result.  Slices (k_mc_tile) and clusters (k_mc_ctile), bit for bit against the oracle."""
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    ql, want = oracle_window(nsteps, qts)
    n = params.shape[0]
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={**LL.OPTS, "wide_k": 12}) as plan:
        LL.check_paths(plan)
        plan.set_output_stride(stride)
        plan.upload_forcing(nsteps, ql, q0)
        stats = plan.route_device(nsteps, qts, True)
        assert stats["wide_levels"] == 3 and stats["wide_segment_steps"] == n * nsteps, stats
        got = plan.download_fvd()
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
        if stride:
            plan.fetch_begin(plan.rowset(np.arange(n)), True, stride)
            kept = np.ascontiguousarray(want[:, stride - 1::stride])
            blk = plan.fetch_wait()[2]
            assert kept.shape == (n, nsteps // stride, 3) and np.any(kept[:, :, 1] != 0)
            assert blk.shape == kept.shape and np.array_equal(bits(blk), bits(kept))
