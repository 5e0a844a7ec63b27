"""THE PER-ROW SUMMARY OF ONE ROUTING WINDOW (include/trmc.h trmc_window_summary; csrc/k_window_summary.inc;
RoutingPlan.window_summary; the ``summary`` keyword of the drop-in): peak flow / depth / velocity with the 1-based step each was
first reached at, and the mean flow, reduced on the device from the window's assembled result.

The definition is exact, so everything here compares bits.  Expected values are ALWAYS numpy over ``plan.download_fvd()`` of the
same window (``summary_of``): peak = x[1], step = 1, then in order ``if x[t] > peak: peak, step = x[t], t`` (the first of equal
peaks wins); mean = the left-to-right sum in the plan's precision over nsteps (np.cumsum).  The kernel stages tiles of R rows x C
steps (``RoutingPlan.window_summary_tile``): the shapes sit on the tile's edges.

The NaN rule (a NaN never replaces a number, a NaN at step 1 stays) and ties between positive peaks are not tested here -- no
flow of these windows is a NaN -- but in tests/test_gpu_products_nonfinite.py, on a network whose forcing carries NaN."""

import numpy as np
import pandas as pd
import pytest

import helpers as H
from troute_amd import _lib, nhd_network as nn
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

KEYS = ("peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step", "peak_velocity", "peak_velocity_step")
PARTS = {"peak": KEYS[0:2], "mean": KEYS[2:3], "peak_depth": KEYS[3:5], "peak_velocity": KEYS[5:7]}
ALL = tuple(PARTS)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def peak_of(x):
    x = np.ascontiguousarray(x)
    peak, step = x[:, 0].copy(), np.ones(x.shape[0], np.int32)
    for t in range(1, x.shape[1]):
        m = x[:, t] > peak
        peak[m] = x[m, t]
        step[m] = t + 1
    return peak, step


def summary_of(fvd):
    """the seven arrays of a full result fvd [rows, nsteps, 3] = (q, v, d) as include/trmc.h defines them"""
    q = np.ascontiguousarray(fvd[:, :, 0])
    want = dict(zip(("peak_flow", "peak_step"), peak_of(q)))
    want["mean_flow"] = np.cumsum(q, axis=1, dtype=q.dtype)[:, -1] / q.dtype.type(q.shape[1])
    want.update(zip(("peak_velocity", "peak_velocity_step"), peak_of(fvd[:, :, 1])))
    want.update(zip(("peak_depth", "peak_depth_step"), peak_of(fvd[:, :, 2])))
    return want


def assert_summary(got, fvd, what, parts=ALL):
    want = summary_of(fvd)
    assert list(got) == [k for k in KEYS if any(k in PARTS[p] for p in parts)], (what, list(got))
    for k, g in got.items():
        w = want[k]
        assert g.dtype == (np.int32 if k.endswith("_step") else fvd.dtype) and g.shape == w.shape, (what, k, g.dtype, g.shape)
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, (what, k, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    return want


def inputs(seed, nseg, nq):
    """a random forest of nseg rows with parameters, forcing [nseg, nq] and an initial state in the ranges the parity tests use"""
    rng = np.random.default_rng(seed)
    to = H.random_network(rng, nseg)
    _, _, ups = H.reaches_from_to(to)
    n = nseg
    p = np.stack([np.full(n, 300.0), rng.uniform(200, 4000, n), rng.uniform(0.5, 20, n), np.zeros(n), np.zeros(n),
                  rng.choice([0.04, 0.05, 0.06], n), np.zeros(n), rng.uniform(0.1, 2.0, n),
                  np.exp(rng.uniform(np.log(1e-4), np.log(0.1), n))], 1)
    p[:, 3] = p[:, 2] * 5 / 3
    p[:, 4] = p[:, 3] * 3
    p[:, 6] = 2 * p[:, 5]
    ql = (np.exp(rng.normal(np.log(5e-3), 2.0, (n, nq))) * (rng.random((n, nq)) > 0.1)).astype(np.float32)
    q0 = np.stack([rng.uniform(0, 2, n), rng.uniform(0, 2, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
    q0[rng.random(n) < 0.3] = 0
    return ups, p.astype(np.float32), ql, q0


def qts_for(nsteps, nq):
    return max(1, -(-nsteps // nq))


def tile(precision):
    R, C = RoutingPlan.window_summary_tile(precision)
    return R, C, 16 // (precision // 8)          # rows, steps, steps of one 16-byte group of the walk


# ---- 1. every way of routing a window ---------------------------------------------------------------------------------------
PATHS = {
    "levels-short": dict(engine="levels", short=True),
    "levels-general": dict(engine="levels", short=False),
    "flow-short": dict(engine="flow", short=True),
    "flow-general": dict(engine="flow", short=False),
    "fp64": dict(engine="auto", short=False, precision=64),
    "tolerance": dict(engine="levels", short=True, options={"arithmetic": "tolerance"}),
    "tiles": dict(engine="levels", short=True, options={"cluster_rows": 64, "wide_min_rows": 200, "wide_k": 4}),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_every_part_equals_numpy_on_the_full_block(path):
    """one plan per way of routing, two windows on it: nsteps = 3 C + one 16-byte group (wide loads, a short last chunk) and
    3 C + 1 (element-wise loads); more rows than four blocks"""
    cfg = dict(PATHS[path])
    short, precision = cfg.pop("short"), cfg.get("precision", 32)
    R, C, VE = tile(precision)
    nseg, nq = 4 * R + 37, 5
    if path == "tiles":
        nseg = 4000                                             # (the plan of test_gpu_stream_summary: slices and cluster tiles)
    ups, params, qlat, q0 = inputs(21, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=short, **cfg) as p:
        assert p.engine == ("flow" if cfg["engine"] == "flow" else "levels") and p.arithmetic == ("tolerance" if path == "tolerance" else "exact")
        for nsteps in (3 * C + VE, 3 * C + 1):
            p.route(nsteps, qts_for(nsteps, nq), short, qlat.astype(p.dtype), q0.astype(p.dtype))
            got = p.window_summary()
            fvd = p.download_fvd()
            assert fvd.dtype == p.dtype and fvd.shape == (nseg, nsteps, 3) and np.isfinite(fvd).all() and fvd[:, :, 0].max() > 0
            want = assert_summary(got, fvd, (path, nsteps))
            assert want["peak_step"].max() > 1 and want["peak_velocity"].max() > 0 and want["peak_depth"].max() > 0
            if path == "tiles":
                assert p.stats()["wide_segment_steps"] == p.stats()["nseg_routed"] * nsteps


# ---- 2. the tile's edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("rows", ["1", "R-1", "R", "R+1", "2R+3"])
def test_shapes_on_the_edges_of_the_tile(rows, precision):
    """nseg in {1, R - 1, R, R + 1, 2 R + 3} x nsteps in {1, 2, C - 1, C, C + 1, 3 C + 1} and, for the wide loads (every row's
    record 16-byte aligned), {VE, C + VE, 3 C + VE}"""
    R, C, VE = tile(precision)
    nseg = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}[rows]
    nq = 3
    ups, params, qlat, q0 = inputs(1000 + nseg, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    q0[:, :] = np.maximum(q0, 0.01)                             # (a single row, too, carries water)
    with RoutingPlan(up_ptr, up_idx, params, precision=precision) as p:
        for nsteps in (1, 2, C - 1, C, C + 1, 3 * C + 1, VE, C + VE, 3 * C + VE):
            p.route(nsteps, qts_for(nsteps, nq), False, qlat.astype(p.dtype), q0.astype(p.dtype))
            got = p.window_summary()
            fvd = p.download_fvd()
            assert fvd.shape == (nseg, nsteps, 3) and fvd[:, :, 0].max() > 0
            assert_summary(got, fvd, (rows, precision, nsteps))


# ---- 3. placed extremes -------------------------------------------------------------------------------------------------------
def extremes_case(precision=32):
    """Headwaters forced step by step (qts = 1) so that their flow, depth and velocity peak where the tile can go wrong: water in the channel at the start and none
    coming in (a recession from step 1 on); a ramp
    that still rises at the window's last step; a ramp that ends on the last step of the first chunk; one that ends on the first
    step of the second chunk; and headwaters with no water at all (a flat hydrograph: the first of equal values, step 1)."""
    R, C, _ = tile(precision)
    nsteps = 3 * C + 1
    nseg = 2 * R + 3
    ups, params, _, _ = inputs(5, nseg, 1)
    heads = [r for r in range(nseg) if not ups[r]]
    assert len(heads) >= 20
    rows = {k: np.array(heads[4 * i:4 * i + 4]) for i, k in enumerate(("first", "last", "chunk_end", "chunk_begin", "flat"))}
    qlat = np.full((nseg, nsteps), 0.01, np.float32)
    q0 = np.zeros((nseg, 3), np.float32)
    t = np.arange(1, nsteps + 1, dtype=np.float32)
    ramp = lambda end: np.where(t <= end, np.float32(0.02) * t, np.float32(0)).astype(np.float32)  # noqa: E731
    qlat[rows["first"]] = 0
    q0[rows["first"]] = (2.0, 2.0, 1.0)
    qlat[rows["last"]] = ramp(nsteps)
    qlat[rows["chunk_end"]] = ramp(C)
    qlat[rows["chunk_begin"]] = ramp(C + 1)
    qlat[rows["flat"]] = 0
    at = {"first": 1, "last": nsteps, "chunk_end": C, "chunk_begin": C + 1, "flat": 1}
    return ups, params, qlat, q0, nsteps, rows, at


def assert_extremes(want, rows, at):
    """the expected arrays really hold the five cases, for the flow, the depth and the velocity"""
    for k in ("peak_step", "peak_depth_step", "peak_velocity_step"):
        for case, rr in rows.items():
            assert np.all(want[k][rr] == at[case]), (k, case, want[k][rr].tolist(), at[case])
    for k in ("peak_flow", "peak_depth", "peak_velocity", "mean_flow"):
        assert not want[k][rows["flat"]].any() and np.all(want[k][rows["last"]] > 0), k


@pytest.mark.parametrize("precision", [32, 64])
def test_peaks_placed_on_the_edges_of_the_window_and_of_a_chunk(precision):
    ups, params, qlat, q0, nsteps, rows, at = extremes_case(precision)
    up_ptr, up_idx = csr_from_lists(ups)
    with RoutingPlan(up_ptr, up_idx, params, precision=precision) as p:
        p.route(nsteps, 1, False, qlat.astype(p.dtype), q0.astype(p.dtype))
        got = p.window_summary()
        fvd = p.download_fvd()
    want = assert_summary(got, fvd, ("extremes", precision))
    assert_extremes(want, rows, at)


# ---- 4. subsets of the parts, row sets ---------------------------------------------------------------------------------------
def test_parts_alone_and_in_pairs_and_row_sets():
    R, C, VE = tile(32)
    nseg, nq, nsteps = 3 * R + 5, 4, C + VE
    ups, params, qlat, q0 = inputs(8, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    rng = np.random.default_rng(2)
    scrambled = rng.permutation(nseg)
    subset = rng.choice(nseg, R + 9, replace=False)            # (unsorted, more than a block of rows)
    with RoutingPlan(up_ptr, up_idx, params) as p:
        p.route(nsteps, qts_for(nsteps, nq), False, qlat, q0)
        fvd = p.download_fvd()
        everything = p.window_summary()
        assert_summary(everything, fvd, "all")
        for parts in [(a,) for a in ALL] + [("peak", "mean"), ("mean", "peak_velocity"), ("peak_depth", "peak"), ("peak_velocity", "peak_depth")]:
            got = p.window_summary(parts)
            assert_summary(got, fvd, parts, parts)
            assert all(np.array_equal(bits(got[k]), bits(everything[k])) for k in got)
        assert list(p.window_summary("mean")) == ["mean_flow"]
        for name, rr in (("scrambled", scrambled), ("subset", subset)):
            rs = p.rowset(rr)
            assert_summary(p.window_summary(rowset=rs), fvd[rr], name)
            assert_summary(p.window_summary(("peak_velocity",), rowset=rs), fvd[rr], name, ("peak_velocity",))
        assert_summary(p.window_summary(), fvd, "all again")    # (a row set leaves nothing behind)


# ---- 5. a window against a one-day stream -------------------------------------------------------------------------------------
def test_a_window_and_a_one_day_stream_give_the_same_bits():
    """a plan in cluster order (slices + cluster tiles), one day routed as a window and as a one-day stream with the stream's
    summary: the five arrays the two have in common"""
    nseg, nsteps, qts = 4000, 24, 8
    ups, params, qlat, q0 = inputs(77, nseg, 3)
    up_ptr, up_idx = csr_from_lists(ups)
    shared = KEYS[:5]
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels",
                     options={"cluster_rows": 64, "wide_min_rows": 200, "wide_k": 4}) as p:
        p.route(nsteps, qts, True, qlat, q0)
        window = p.window_summary(("peak", "mean", "peak_depth"))
        assert_summary(window, p.download_fvd(), "window", ("peak", "mean", "peak_depth"))
        p.stream_set_summary(("peak", "mean", "peak_depth"))
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, qts)
        dest = tuple(_lib.result_empty((nseg,), np.int32 if k.endswith("_step") else np.float32, always_pinned=True) for k in shared)
        assert p.stream_push(pinned_like(qlat), summary=dest) == 0
        p.stream_flush()
        p.stream_wait(0)
        stream = {k: np.array(x, copy=True) for k, x in zip(shared, dest)}
        p.stream_end()
    assert list(window) == list(shared)
    for k in shared:
        assert window[k].dtype == stream[k].dtype and np.array_equal(bits(window[k]), bits(stream[k])), k
    assert window["peak_step"].max() > 1 and window["peak_depth"].max() > 0


# ---- 6. through the drop-in ---------------------------------------------------------------------------------------------------
def test_the_drop_in_appends_the_summary_beside_a_decimated_block():
    from troute_amd.routing.compute import compute_nhd_routing_v02
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured, mc_only_args
    lc = H.LowerColorado()
    nts, parts = 48, ("peak", "mean")
    args = mc_only_args(nts, lc.dt, lc.qts, lc.reaches, lc.rconn, lc.ids, lc.data_cols, lc.data_values, lc.q0, lc.qlat, None, False)
    full = compute_network_structured(*args)
    assert len(full) == 10
    fvd = full[1].reshape(lc.nseg, nts, 3)
    perm = np.random.default_rng(5).permutation(lc.nseg)
    for order in (None, perm):
        rows = np.arange(lc.nseg) if order is None else order
        got = compute_network_structured(*args, output_stride=4, summary=parts, result_order=order)
        assert len(got) == 11 and isinstance(got[10], dict)
        assert np.array_equal(got[0], full[0][rows])
        assert np.array_equal(bits(got[1].reshape(lc.nseg, nts // 4, 3)), bits(fvd[rows][:, 3::4, :]))
        want = assert_summary(got[10], fvd[rows], ("drop-in", order is None), parts)
        assert np.any(want["peak_step"] % 4 != 0)               # (peaks between the kept steps: what the decimated block misses)
        with_stats = compute_network_structured(*args, output_stride=4, summary=parts, result_order=order, return_stats=True)
        assert len(with_stats) == 12 and "nseg" in with_stats[10]
        assert_summary(with_stats[11], fvd[rows], "behind the stats", parts)
    with pytest.raises(ValueError):
        compute_network_structured(*args, summary=("peak", "flood"))
    # ... and forwarded by compute_nhd_routing_v02: an eleventh member of every tailwater's tuple, rows as its member [0]
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
    plain, summed = call(), call(output_stride=4, summary=parts)
    assert all(len(r) == 10 for r in plain) and all(len(r) == 11 for r in summed) and len(plain) == len(summed)
    row_of = {int(s): i for i, s in enumerate(lc.ids)}
    for a, b in zip(plain, summed):
        assert np.array_equal(a[0], b[0])
        rr = np.array([row_of[int(s)] for s in b[0]], dtype=np.int64)
        assert_summary(b[10], fvd[rr], "v02", parts)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    nseg, nq, nsteps = 50, 2, 8
    ups, params, qlat, q0 = inputs(4, nseg, nq)
    up_ptr, up_idx = csr_from_lists(ups)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={"cluster_rows": 8, "wide_min_rows": 3, "wide_k": 4}) as p:
        with pytest.raises(RuntimeError, match="nothing routed"):          # before any window: trmc_download_fvd's state error
            p.window_summary()
        p.route(nsteps, 4, True, qlat, q0)
        fvd = p.download_fvd()
        assert_summary(p.window_summary(), fvd, "after the window")
        for nothing in (None, (), []):
            with pytest.raises(ValueError):
                p.window_summary(nothing)
        with pytest.raises(ValueError, match="flood"):
            p.window_summary(("peak", "flood"))
        h = _lib.lib()
        pk, st = np.zeros(nseg, np.float32), np.zeros(nseg, np.int32)
        assert h.trmc_window_summary(p._h, -1, None, None, None, None, None, None, None) == _lib.TRMC_EINVAL
        assert h.trmc_window_summary(p._h, -1, None, _lib.ptr(st), None, None, None, None, None) == _lib.TRMC_EINVAL   # a step without its value
        assert h.trmc_window_summary(p._h, 7, _lib.ptr(pk), None, None, None, None, None, None) == _lib.TRMC_EINVAL    # no such row set
        assert h.trmc_window_summary(p._h, -1, _lib.ptr(pk), None, None, None, None, None, None) == 0                  # a value without its step
        assert np.array_equal(bits(pk), bits(summary_of(fvd)["peak_flow"]))
        p.route_begin(nsteps, 4, True)                                       # a window in progress: its result is not assembled yet
        with pytest.raises(RuntimeError, match="window is in progress"):
            p.window_summary()
        p.route_advance(nsteps)
        p.route_end()
        assert_summary(p.window_summary(), fvd, "the same forcing again")
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, 4)
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.window_summary()
        p.stream_push(pinned_like(qlat))
        p.stream_flush()
        p.stream_end()
        with pytest.raises(RuntimeError, match="nothing routed"):          # a stream leaves no window result behind
            p.window_summary()
