"""THRESHOLD EXCEEDANCE PER ROW OF ONE ROUTING WINDOW (include/trmc.h trmc_plan_set_thresholds, trmc_window_exceedance,
trmc_plan_bankfull_depth; csrc/k_window_exceed.inc; RoutingPlan.set_thresholds / window_exceedance / bankfull_depth; the
``exceedance`` keyword of the drop-in): per row and level the number of steps over the threshold, the first and the last of
them and the longest run of consecutive ones.

The definition is exact and its results are integers, so everything here is compared for equality.  Expected values are ALWAYS
numpy over ``plan.download_fvd()`` of the same window (``exceedance_of``: a plain loop over t that states the definition).  The
kernel stages tiles of R rows x C steps (``RoutingPlan.window_exceedance_tile``) and walks VE = 16 / itemsize steps at a time: the
shapes sit on those edges.  Thresholds are taken from the window's own values (``edge_thresholds``) so that equality, a NaN, -inf
and +inf all occur."""

import numpy as np
import pandas as pd
import pytest

import helpers as H
from test_gpu_window_summary import PATHS, inputs, qts_for, summary_of
from troute_amd import _lib, nhd_network as nn
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

KEYS = ("steps_over", "first_step", "last_step", "longest_run")
QUANTITIES = ("flow", "velocity", "depth")


def exceedance_of(x, th):
    """the four arrays [rows, K] of a series x [rows, nsteps] against thresholds th [rows, K] of the same dtype, as
    include/trmc.h defines them: over(t) := x[t] > th (false with a NaN on either side; equality is not over), t = 1..nsteps"""
    x, th = np.ascontiguousarray(x), np.ascontiguousarray(th)
    assert x.dtype == th.dtype and x.ndim == 2 and th.ndim == 2 and x.shape[0] == th.shape[0]
    shape = th.shape
    count, first, last, longest, run = (np.zeros(shape, np.int64) for _ in range(5))
    with np.errstate(invalid="ignore"):
        for t in range(1, x.shape[1] + 1):
            over = x[:, t - 1][:, None] > th
            count = count + over
            first = np.where(over & (first == 0), t, first)
            last = np.where(over, t, last)
            run = np.where(over, run + 1, 0)
            longest = np.maximum(longest, run)
    return {k: v.astype(np.int32) for k, v in zip(KEYS, (count, first, last, longest))}


def edge_thresholds(x, rng, nlevels=4):
    """level 0: the row's own value at a random step (equality occurs: not over); level 1: the row's median over t; level 2: -inf
    on even rows (always over), NaN on odd rows (never); level 3: +inf (never).  The first `nlevels` of them."""
    n, nsteps = x.shape
    th = np.empty((n, 4), x.dtype)
    th[:, 0] = x[np.arange(n), rng.integers(0, nsteps, n)]
    th[:, 1] = np.median(x, axis=1).astype(x.dtype)
    th[0::2, 2] = -np.inf
    th[1::2, 2] = np.nan
    th[:, 3] = np.inf
    return np.ascontiguousarray(th[:, :nlevels])


def assert_exceedance(got, x, th, what, parts=KEYS):
    want = exceedance_of(x, th)
    assert list(got) == [k for k in KEYS if k in parts], (what, list(got))
    for k, g in got.items():
        w = want[k]
        assert g.dtype == np.int32 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, k, bad.shape[0], bad[:8].tolist(), g[g != w][:8].tolist(), w[g != w][:8].tolist())
    return want


def assert_the_edges_are_in(want, th, nsteps):
    """the expected arrays of ``edge_thresholds`` with four levels really hold what the levels are there for"""
    even, odd = slice(0, None, 2), slice(1, None, 2)
    for k, always in zip(KEYS, (nsteps, 1, nsteps, nsteps)):
        assert np.all(want[k][even, 2] == always), k             # -inf: (nsteps, 1, nsteps, nsteps)
        assert not want[k][odd, 2].any() and not want[k][:, 3].any(), k   # a NaN and +inf: never over
    assert np.all(want["steps_over"][:, 0] < nsteps)             # the step the threshold was taken at is not over
    pairs = want["steps_over"][:, :2]
    partly = np.count_nonzero((pairs > 0) & (pairs < nsteps))
    assert 4 * partly >= pairs.size, (partly, pairs.size)        # a quarter of (row, level 0..1) neither never nor always over
    again = np.count_nonzero(want["longest_run"][:, :2] < pairs)
    assert again >= 20, again                                    # two or more separate excursions


def flashy(qlat):
    """hourly columns alternately high and low: hydrographs that cross a row's median more than once"""
    q = qlat.copy()
    q[:, 0::2] *= np.float32(8.0)
    q[:, 1::2] *= np.float32(0.125)
    return q


def tile(precision):
    R, C = RoutingPlan.window_exceedance_tile(precision)
    return R, C, 16 // (precision // 8)          # rows, steps, steps of one 16-byte group of the walk


def column(fvd, quantity):
    return np.ascontiguousarray(fvd[:, :, QUANTITIES.index(quantity)])


# ---- 1. every way of routing a window ---------------------------------------------------------------------------------------
def case_of_path(path):
    cfg = dict(PATHS[path])
    short, precision = cfg.pop("short"), cfg.get("precision", 32)
    R, C, VE = tile(precision)
    nseg, nq = (4000 if path == "tiles" else 4 * R + 37), 5     # ("tiles": the plan of test_gpu_stream_summary, slices and cluster tiles)
    ups, params, qlat, q0 = inputs(21, nseg, nq)
    return cfg, short, precision, nseg, nq, ups, params, flashy(qlat), q0, (3 * C + VE, 3 * C + 1)


@pytest.mark.parametrize("path", list(PATHS))
def test_every_output_equals_numpy_on_the_full_block(path):
    """One plan per way of routing, two windows on it: nsteps = 3 C + one 16-byte group (wide loads, a short last chunk) and
    3 C + 1 (element-wise loads); more rows than four blocks; K = 4, the three quantities, the four outputs.

    That the expectation is not vacuous -- ``assert_the_edges_are_in``: a quarter of the (row, level 0..1) pairs partly over,
    twenty or more pairs with separate excursions -- was checked without a GPU for every fp32 shape used here (293 and 4000 rows,
    100 and 97 steps, both timestep modes, the three quantities) with the oracle plan of tests/oracle_plan.py routing the same
    inputs, and for the fp64 shapes (293 rows, 50 and 49 steps) with the same plan's fp32 values cast to double: the smallest
    share of partly-over pairs was 0.988 and the smallest number of pairs with separate excursions 320."""
    cfg, short, precision, nseg, nq, ups, params, qlat, q0, windows = case_of_path(path)
    up_ptr, up_idx = csr_from_lists(ups)
    rng = np.random.default_rng(3)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=short, **cfg) as p:
        assert p.engine == ("flow" if cfg["engine"] == "flow" else "levels") and p.arithmetic == ("tolerance" if path == "tolerance" else "exact")
        for nsteps in windows:
            p.route(nsteps, qts_for(nsteps, nq), short, qlat.astype(p.dtype), q0.astype(p.dtype))
            fvd = p.download_fvd()
            assert fvd.dtype == p.dtype and fvd.shape == (nseg, nsteps, 3) and np.isfinite(fvd).all() and fvd[:, :, 0].max() > 0
            for quantity in QUANTITIES:
                x = column(fvd, quantity)
                th = edge_thresholds(x, rng)
                p.set_thresholds(th)
                want = assert_exceedance(p.window_exceedance(quantity), x, th, (path, nsteps, quantity))
                assert_the_edges_are_in(want, th, nsteps)
        assert p.window_exceedance_kernel_ms() >= 0


# ---- 2. the tile's edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("rows", ["1", "R-1", "R", "R+1"])
def test_shapes_on_the_edges_of_the_tile(rows, precision):
    """nseg in {1, R - 1, R, R + 1} x nsteps in {1, C - 1, C, C + 1} x K in {1, 2, 3}, every row and a row set that is a permuted
    subset, all four parts and subsets of them (NULL destinations); at R + 1 rows also nsteps in {VE, C + VE}: the wide loads
    (every row's record 16-byte aligned) with a first chunk shorter than C, and with a short last chunk behind a whole one"""
    R, C, VE = tile(precision)
    nseg = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1}[rows]
    nq = 3
    ups, params, qlat, q0 = inputs(2000 + nseg, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    q0[:, :] = np.maximum(q0, 0.01)                             # (a single row, too, carries water)
    rng = np.random.default_rng(nseg)
    subset = rng.permutation(nseg)[:max(1, (2 * nseg) // 3)]
    part_sets = [KEYS, ("steps_over",), ("first_step", "last_step"), ("longest_run",), ("last_step", "steps_over"), KEYS[1:]]
    turn = 0
    with RoutingPlan(up_ptr, up_idx, params, precision=precision) as p:
        rs = p.rowset(subset)
        for nsteps in (1, C - 1, C, C + 1) + ((VE, C + VE) if rows == "R+1" else ()):
            p.route(nsteps, qts_for(nsteps, nq), False, flashy(qlat).astype(p.dtype), q0.astype(p.dtype))
            fvd = p.download_fvd()
            assert fvd.shape == (nseg, nsteps, 3) and fvd[:, :, 0].max() > 0
            for K in (1, 2, 3):
                quantity, parts = QUANTITIES[turn % 3], part_sets[turn % len(part_sets)]
                turn += 1
                x = column(fvd, quantity)
                th = edge_thresholds(x, rng, K)
                p.set_thresholds(th[:, 0] if K == 1 and nsteps % 2 else th)       # ([nseg] is one level)
                what = (rows, precision, nsteps, K, quantity)
                everything = assert_exceedance(p.window_exceedance(quantity), x, th, what)
                assert all(v.shape == (nseg, K) for v in everything.values())
                assert_exceedance(p.window_exceedance(quantity, parts), x, th, what + (parts,), parts)
                assert_exceedance(p.window_exceedance(quantity, rowset=rs), x[subset], th[subset], what + ("row set",))
                assert_exceedance(p.window_exceedance(quantity, parts, rowset=rs), x[subset], th[subset], what + ("row set", parts), parts)


# ---- 3. the thresholds' lifetime ----------------------------------------------------------------------------------------------
def test_thresholds_stay_are_replaced_are_cleared_and_belong_to_one_handle():
    R, C, VE = tile(32)
    nseg, nq, nsteps = R + 9, 3, C + VE
    ups, params, qlat, q0 = inputs(31, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    rng = np.random.default_rng(4)
    with RoutingPlan(up_ptr, up_idx, params) as p:
        p.route(nsteps, qts_for(nsteps, nq), False, flashy(qlat), q0)
        fvd1 = p.download_fvd()
        th4 = edge_thresholds(column(fvd1, "flow"), rng)
        p.set_thresholds(th4)
        assert_exceedance(p.window_exceedance("flow"), column(fvd1, "flow"), th4, "window 1")
        # set once, they serve a second window (another forcing, another length)
        p.route(nsteps + 1, qts_for(nsteps + 1, nq), False, (flashy(qlat) * np.float32(0.5)), q0)
        fvd2 = p.download_fvd()
        assert not np.array_equal(fvd1[:, :8], fvd2[:, :8])
        for quantity in QUANTITIES:
            assert_exceedance(p.window_exceedance(quantity), column(fvd2, quantity), th4, ("window 2", quantity))
        # another K replaces them
        th2 = edge_thresholds(column(fvd2, "depth"), rng, 2)
        p.set_thresholds(th2)
        got = assert_exceedance(p.window_exceedance("depth"), column(fvd2, "depth"), th2, "replaced")
        assert got["steps_over"].shape == (nseg, 2)
        # a clone has none until they are set on it, and setting them there leaves the original's alone
        with p.clone() as c:
            c.route(nsteps, qts_for(nsteps, nq), False, flashy(qlat), q0)
            with pytest.raises(RuntimeError, match="no thresholds"):
                c.window_exceedance("flow")
            th1 = edge_thresholds(column(fvd1, "velocity"), rng, 1)
            c.set_thresholds(th1)
            assert_exceedance(c.window_exceedance("velocity"), column(c.download_fvd(), "velocity"), th1, "clone")
            assert_exceedance(p.window_exceedance("depth"), column(fvd2, "depth"), th2, "the original beside its clone")
        # None clears them: the call is refused again
        p.set_thresholds(None)
        with pytest.raises(RuntimeError, match="no thresholds"):
            p.window_exceedance("depth")
        p.set_thresholds(th4)
        assert_exceedance(p.window_exceedance("flow"), column(fvd2, "flow"), th4, "set again")


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    nseg, nq, nsteps = 50, 2, 8
    ups, params, qlat, q0 = inputs(4, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    th = np.full((nseg, 2), 0.5, np.float32)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={"cluster_rows": 8, "wide_min_rows": 3, "wide_k": 4}) as p:
        p.set_thresholds(th)
        with pytest.raises(RuntimeError, match="nothing routed"):          # before any window
            p.window_exceedance()
        p.set_thresholds(None)
        p.route(nsteps, 4, True, qlat, q0)
        fvd = p.download_fvd()
        with pytest.raises(RuntimeError, match="no thresholds"):           # without thresholds
            p.window_exceedance()
        p.set_thresholds(th)
        assert_exceedance(p.window_exceedance("flow"), column(fvd, "flow"), th, "after the window")
        h = _lib.lib()
        a = np.zeros((nseg, 2), np.int32)
        assert h.trmc_window_exceedance(p._h, -1, _lib.TRMC_X_FLOW, None, None, None, None) == _lib.TRMC_EINVAL      # nothing asked for
        assert h.trmc_window_exceedance(p._h, -1, 3, _lib.ptr(a), None, None, None) == _lib.TRMC_EINVAL              # no such quantity
        assert h.trmc_window_exceedance(p._h, -1, -1, _lib.ptr(a), None, None, None) == _lib.TRMC_EINVAL
        assert h.trmc_window_exceedance(p._h, 7, _lib.TRMC_X_FLOW, _lib.ptr(a), None, None, None) == _lib.TRMC_EINVAL  # no such row set
        assert h.trmc_plan_set_thresholds(p._h, 5, _lib.ptr(th)) == _lib.TRMC_EINVAL
        assert h.trmc_plan_set_thresholds(p._h, -1, _lib.ptr(th)) == _lib.TRMC_EINVAL
        assert h.trmc_window_exceedance(p._h, -1, _lib.TRMC_X_DEPTH, None, None, _lib.ptr(a), None) == 0             # (the refused calls changed nothing)
        assert np.array_equal(a, exceedance_of(column(fvd, "depth"), th)["last_step"])
        p.route_begin(nsteps, 4, True)                                       # a window in progress
        with pytest.raises(RuntimeError, match="window is in progress"):
            p.window_exceedance()
        with pytest.raises(RuntimeError, match="window is in progress"):
            p.set_thresholds(th)
        p.route_advance(nsteps)
        p.route_end()
        assert_exceedance(p.window_exceedance("velocity"), column(fvd, "velocity"), th, "the same forcing again")
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4)
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.window_exceedance()
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.set_thresholds(th)
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.set_thresholds(None)
        p.stream_push(pinned_like(qlat))
        p.stream_flush()
        p.stream_end()
        with pytest.raises(RuntimeError, match="nothing routed"):          # a stream leaves no window result behind
            p.window_exceedance()


# ---- 5. the plan's scratch block is shared with the summary and the Courant summary -------------------------------------------
def test_the_three_reductions_of_one_window_in_any_order():
    from test_gpu_window_summary import assert_summary, bits, peak_of
    R, C, VE = tile(32)
    nseg, nq, nsteps = 2 * R + 11, 4, C + VE
    ups, params, qlat, q0 = inputs(9, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    with RoutingPlan(up_ptr, up_idx, params) as p:
        p.route(nsteps, qts_for(nsteps, nq), False, flashy(qlat), q0)
        fvd = p.download_fvd()
        th = edge_thresholds(column(fvd, "flow"), np.random.default_rng(6))
        p.set_thresholds(th)
        cn = p.window_courant()[:, :, 0]
        with np.errstate(invalid="ignore"):
            over_cn = (cn > np.float32(1)).sum(1).astype(np.int32)
        peak_cn, peak_cn_step = peak_of(cn)                      # (trmc_window_courant_summary's rule is the summary's)
        assert summary_of(fvd)["peak_step"].max() > 1

        def exceedance():
            assert_exceedance(p.window_exceedance("flow"), column(fvd, "flow"), th, "exceedance")

        def summary():
            assert_summary(p.window_summary(), fvd, "summary")

        def courant():
            got = p.window_courant_summary(1.0)
            assert np.array_equal(got["steps_over"], over_cn) and np.array_equal(got["peak_cn_step"], peak_cn_step)
            assert np.array_equal(bits(got["peak_cn"]), bits(peak_cn))

        for order in ((exceedance, summary, courant), (courant, summary, exceedance), (summary, exceedance, courant, exceedance, summary)):
            for call in order:
                call()


# ---- 6. the bankfull depth ------------------------------------------------------------------------------------------------------
def bankfull_of(params, dtype):
    """MUSKINGCUNGE f90:55-61 in `dtype` on the plan's parameter table [nseg, 9] (float32, cast as the plan casts it)"""
    p = params.astype(dtype)
    bw, tw, cs = p[:, _lib.PARAM_COLS.index("bw")], p[:, _lib.PARAM_COLS.index("tw")], p[:, _lib.PARAM_COLS.index("cs")]
    one, two = dtype(1), dtype(2)
    with np.errstate(divide="ignore"):
        z = np.where(cs == 0, one, one / cs).astype(dtype)
    return np.where(bw > tw, bw / dtype(0.00001), np.where(bw == tw, bw / (two * z), (tw - bw) / (two * z))).astype(dtype)


@pytest.mark.parametrize("precision", [32, 64])
def test_bankfull_depth_is_the_step_kernels_own(precision):
    R, C, VE = tile(precision)
    nseg = 2 * R + 5
    ups, params, _, _ = inputs(12, nseg, 1)
    bw, tw, cs = (_lib.PARAM_COLS.index(k) for k in ("bw", "tw", "cs"))
    params[0::7, tw] = params[0::7, bw] * np.float32(0.5)       # bw > tw
    params[1::7, tw] = params[1::7, bw]                         # bw == tw
    params[2::7, cs] = 0                                        # cs == 0: z = 1
    params[3::7, cs], params[3::7, tw] = 0, params[3::7, bw]
    assert (params[:, bw] > params[:, tw]).any() and (params[:, bw] == params[:, tw]).any() and (params[:, cs] == 0).any()
    assert (params[:, bw] < params[:, tw]).sum() > nseg // 2
    dtype = np.float32 if precision == 32 else np.float64
    want = bankfull_of(params, dtype)
    assert np.isfinite(want).all() and (want > 0).all()
    boundary = np.zeros(nseg, np.uint8)
    heads = [r for r in range(nseg) if not ups[r]]
    boundary[heads[:3]] = 1
    up_ptr, up_idx = csr_from_lists(ups)
    view = {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
    with RoutingPlan(up_ptr, up_idx, params, precision=precision) as p:
        got = p.bankfull_depth()
        assert got.dtype == dtype and got.shape == (nseg,)
        assert np.array_equal(got.view(view), want.view(view))
        # rows declared as reservoirs route no Muskingum-Cunge step: +inf while they are declared
        lakes = np.array([r for r in range(nseg) if r not in heads][:4], dtype=np.int64)
        par = np.tile(np.array([2.0e5, 12.0, 1.0, 0.6, 5.0, 0.4, 10.0, 20.0, 10.0], dtype), (lakes.size, 1))
        p.set_reservoirs(lakes, par, 300.0)
        got = p.bankfull_depth()
        assert np.all(np.isposinf(got[lakes]))
        rest = np.setdiff1d(np.arange(nseg), lakes)
        assert np.array_equal(got[rest].view(view), want[rest].view(view))
    with RoutingPlan(up_ptr, up_idx, params, boundary=boundary, precision=precision) as p:
        got = p.bankfull_depth()                                # boundary rows carry a prescribed hydrograph: +inf
        assert np.all(np.isposinf(got[heads[:3]]))
        rest = np.setdiff1d(np.arange(nseg), heads[:3])
        assert np.array_equal(got[rest].view(view), want[rest].view(view))


def flood_args(nts, scale=np.float32(400.0)):
    from troute_amd.routing.fast_reach.mc_reach import mc_only_args
    lc = H.LowerColorado()
    qlat = (lc.qlat * scale).astype(np.float32)
    return lc, mc_only_args(nts, lc.dt, lc.qts, lc.reaches, lc.rconn, lc.ids, lc.data_cols, lc.data_values, lc.q0, qlat, None, False)


def test_out_of_bank_is_the_depth_against_the_bankfull_depth():
    """``exceedance=("depth", "bankfull")`` with nothing supplied by the caller; the forcing is the golden domain's times 400, under
    which (checked with the oracle on the CPU) hundreds of rows leave their banks for part of the window"""
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    nts = 48
    lc, args = flood_args(nts)
    got = compute_network_structured(*args, exceedance=("depth", "bankfull"))
    assert len(got) == 11 and list(got[10]) == list(KEYS)
    d = np.ascontiguousarray(got[1].reshape(lc.nseg, nts, 3)[:, :, 2])
    bfd = bankfull_of(lc.params9, np.float32)
    count = (d > bfd[:, None]).sum(1)
    assert np.count_nonzero(count) >= 20 and np.count_nonzero((count > 0) & (count < nts)) >= 10, (np.count_nonzero(count),)
    assert got[10]["steps_over"].shape == (lc.nseg, 1) and np.array_equal(got[10]["steps_over"][:, 0], count)
    assert_exceedance(got[10], d, bfd[:, None], "out of bank")


# ---- 7. through the drop-in -----------------------------------------------------------------------------------------------------
def test_the_drop_in_appends_the_exceedance_beside_a_decimated_block():
    from troute_amd.routing.compute import compute_nhd_routing_v02
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured, mc_only_args
    from test_gpu_window_summary import assert_summary
    lc = H.LowerColorado()
    nts = 48
    args = mc_only_args(nts, lc.dt, lc.qts, lc.reaches, lc.rconn, lc.ids, lc.data_cols, lc.data_values, lc.q0, lc.qlat, None, False)
    full = compute_network_structured(*args)
    assert len(full) == 10
    fvd = full[1].reshape(lc.nseg, nts, 3)
    rng = np.random.default_rng(8)
    th = edge_thresholds(column(fvd, "flow"), rng)
    got = compute_network_structured(*args, output_stride=12, exceedance=("flow", th))
    assert len(got) == 11 and isinstance(got[10], dict)
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[1].reshape(lc.nseg, nts // 12, 3), fvd[:, 11::12, :])
    want = assert_exceedance(got[10], column(fvd, "flow"), th, "drop-in")
    assert np.any(want["first_step"][:, :2] % 12 != 0)          # (what the decimated block cannot show)
    # members 0..9 do not change with the keyword
    same = compute_network_structured(*args, exceedance=("flow", th))
    for k in range(10):
        a, b = full[k], same[k]
        assert type(a) is type(b)
        for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True), k
    # one level as [rows]; another quantity on the kept plan; the summary in the same dict, behind the stats
    th1 = np.ascontiguousarray(edge_thresholds(column(fvd, "depth"), rng)[:, 1])
    both = compute_network_structured(*args, output_stride=12, summary=("peak", "mean"), exceedance=("depth", th1), return_stats=True)
    assert len(both) == 12 and "nseg" in both[10]
    assert list(both[11]) == ["peak_flow", "peak_step", "mean_flow"] + list(KEYS)
    assert_summary({k: both[11][k] for k in ("peak_flow", "peak_step", "mean_flow")}, fvd, "summary beside it", ("peak", "mean"))
    assert_exceedance({k: both[11][k] for k in KEYS}, column(fvd, "depth"), th1[:, None], "exceedance beside the summary")
    for bad in (("stage", th), ("flow", th[:-1]), ("flow", np.zeros((lc.nseg, 5), np.float32)), ("flow", "bankfull"), "flow"):
        with pytest.raises(ValueError):
            compute_network_structured(*args, exceedance=bad)
    # ... with upstream_results: the spliced-in row is left out, as it is of member [0]
    # (a headwater reach cut off and handed in as a hydrograph; the thresholds are in the order of the call's own data_idx)
    row = {int(s): i for i, s in enumerate(lc.ids)}
    cut_reach = next(r for r in lc.reaches if not lc.rconn.get(r[0]) and lc.to[row[r[-1]]] != 0)
    cut, upper = cut_reach[-1], set(cut_reach)
    ids_lo = np.array(sorted((set(lc.ids.tolist()) - upper) | {cut}), np.int64)
    sel = np.array([row[s] for s in ids_lo])
    ur = {cut: {"position_index": int(np.searchsorted(ids_lo, cut)), "results": fvd[row[cut]].reshape(-1)}}
    a = mc_only_args(nts, lc.dt, lc.qts, [r for r in lc.reaches if r[0] not in upper], lc.rconn, ids_lo, lc.data_cols, lc.data_values[sel],
                     lc.q0[sel], lc.qlat[sel], upstream_results=ur, assume_short_ts=False)
    spliced = compute_network_structured(*a, output_stride=12, exceedance=("flow", th[sel]))
    keep = np.array([row[int(s)] for s in spliced[0]])
    assert len(spliced) == 11 and spliced[0].shape[0] == len(ids_lo) - 1 and cut not in spliced[0]
    assert np.array_equal(spliced[1].reshape(-1, nts // 12, 3), fvd[keep][:, 11::12, :])
    assert_exceedance(spliced[10], column(fvd[keep], "flow"), th[keep], "upstream_results")
    # ... and through compute_nhd_routing_v02: a frame that lacks some ids (+inf there: zeros), one column per level
    conn = {int(s): ([int(t)] if t != 0 else []) for s, t in zip(lc.ids, lc.to)}
    ind, reaches_bytw, rconn = nn.organize_independent_networks(conn)
    cols = ["dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0"]
    param_df = pd.DataFrame(lc.params9[:, 1:], index=lc.ids, columns=cols)
    param_df["alt"] = 0.0
    q0_df, qlat_df = pd.DataFrame(lc.q0, index=lc.ids, columns=["qu0", "qd0", "h0"]), pd.DataFrame(lc.qlat, index=lc.ids)
    e = pd.DataFrame()

    def call(**kw):
        return compute_nhd_routing_v02(conn, rconn, {}, reaches_bytw, "V02-structured", "by-network", 10000, 4, None, 300.0, nts, lc.qts, ind,
                                       param_df, q0_df, qlat_df, e, e, e, e, e, e, e, e, e, e, e, {}, False, False, e, {}, e, False,
                                       [{}, {}], {}, **kw)[0]
    have = np.ones(lc.nseg, bool)
    have[rng.choice(lc.nseg, lc.nseg // 5, replace=False)] = False
    frame = pd.DataFrame(th[have][:, :2], index=lc.ids[have], columns=["action", "flood"]).sample(frac=1.0, random_state=1)
    th_v02 = np.where(have[:, None], th[:, :2], np.float32(np.inf)).astype(np.float32)
    plain = call()
    flagged = call(output_stride=12, exceedance=("flow", frame))
    summed = call(output_stride=12, summary=("peak",), exceedance=("flow", frame))
    assert all(len(r) == 10 for r in plain) and all(len(r) == 11 for r in flagged) and len(plain) == len(flagged) == len(summed)
    for a, b, c in zip(plain, flagged, summed):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
        rr = np.array([row[int(s)] for s in b[0]], dtype=np.int64)
        w = assert_exceedance(b[10], column(fvd[rr], "flow"), th_v02[rr], "v02")
        assert not any(w[k][~have[rr]].any() for k in KEYS)
        assert list(c[10]) == ["peak_flow", "peak_step"] + list(KEYS)
        assert_exceedance({k: c[10][k] for k in KEYS}, column(fvd[rr], "flow"), th_v02[rr], "v02 with the summary")
    assert sum(int(b[10]["steps_over"].sum()) for b in flagged) > 0
    bank = call(exceedance=("depth", "bankfull"))
    assert all(r[10]["steps_over"].shape == (r[0].shape[0], 1) for r in bank)
