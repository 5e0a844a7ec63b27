"""THE COURANT METRICS OF ONE ROUTING WINDOW (include/trmc.h trmc_window_courant, trmc_window_courant_summary;
csrc/k_window_courant.inc; RoutingPlan.window_courant / window_courant_summary; ``return_courant`` of the drop-in): (cn, ck, X) of
every row-step, recomputed on the device from the window's result, initial state and forcing.

THE EXPECTED VALUES COME FROM THE REFERENCE.  ``expected`` rebuilds, from what the window returned (fvd), ``q0`` and ``qlat``, the
15-column input of the reference Fortran's single-segment step for every (row, step) asked for -- dt, qup, quc, qdp, ql, dx, bw, tw,
twcc, n, ncc, cs, s0, velp = 0, depthp; upstream flows summed one after the other in the plan's dtype -- and calls
``oracle.ref_segments`` (the reference Fortran built with Qj_0 = 0, fp32 and fp64; ``segments(det=True)`` where oracle/_ref is
absent).  (cn, ck, X) are the oracle's columns 4, 3, 5 and are compared with the block AS INTEGERS (a NaN equals itself).  Before it
is used the reconstruction is proven: on Muskingum-Cunge rows without a gage the oracle's (qdc, depthc) at those inputs are the
fvd's [t, 0] and [t, 2], bit for bit."""
import os

import numpy as np
import pandas as pd
import pytest

import helpers as H
from oracle import oracle as O
from troute_amd import _lib, nhd_network as nn, synthetic
from troute_amd.plan import RoutingPlan, csr_from_lists, segments as trmc_segments
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def oracle_segments(x):
    name = {4: "libmc_ref_qj0_f32.so", 8: "libmc_ref_qj0_f64.so"}[x.dtype.itemsize]
    return O.ref_segments(x, name) if O.have_ref(name) else O.segments(x, det=True)


def rebuilt_inputs(fvd, q0, qlat, params9, ups, qts, short, steps=None):
    """[rows, len(steps), 15]: the inputs of step t (1-based) of every row, from the flows and depths the window returned"""
    dt = fvd.dtype
    n, T = fvd.shape[:2]
    steps = np.arange(1, T + 1) if steps is None else np.asarray(steps)
    Q = np.concatenate([q0[:, :1].astype(dt), fvd[:, :, 0]], 1)            # flow at steps 0..T
    D = np.concatenate([q0[:, 2:3].astype(dt), fvd[:, :, 2]], 1)
    qup, quc = np.zeros((n, steps.size), dt), np.zeros((n, steps.size), dt)
    fan = max((len(u) for u in ups), default=0)
    for k in range(fan):                                                    # the k-th upstream row of every row that has one
        has = np.array([i for i, u in enumerate(ups) if len(u) > k], dtype=np.int64)
        uk = np.array([ups[i][k] for i in has], dtype=np.int64)
        qup[has] = qup[has] + Q[uk][:, steps - 1]
        quc[has] = quc[has] + Q[uk][:, steps]
    if short:
        quc = qup
    x = np.zeros((n, steps.size, 15), dt)
    p = params9.astype(dt)
    x[:, :, 0] = p[:, None, 0]
    x[:, :, 1], x[:, :, 2] = qup, quc
    x[:, :, 3] = Q[:, steps - 1]
    x[:, :, 4] = qlat.astype(dt)[:, (steps - 1) // qts]
    x[:, :, 5:13] = p[:, None, 1:9]
    x[:, :, 14] = D[:, steps - 1]
    return x


def expected(fvd, q0, qlat, params9, ups, qts, short, steps=None, mc_rows=None, ungaged=None):
    """(cn, ck, X) [rows, len(steps), 3] from the oracle, after proving the reconstruction on `ungaged` (default: all) MC rows"""
    n, T = fvd.shape[:2]
    steps = np.arange(1, T + 1) if steps is None else np.asarray(steps)
    x = rebuilt_inputs(fvd, q0, qlat, params9, ups, qts, short, steps)
    mc = np.arange(n) if mc_rows is None else np.asarray(mc_rows)
    o = oracle_segments(x[mc].reshape(-1, 15)).reshape(mc.size, steps.size, 6)
    prove = np.ones(mc.size, bool) if ungaged is None else np.isin(mc, ungaged)
    assert np.array_equal(bits(o[prove][:, :, 0]), bits(fvd[mc[prove]][:, steps - 1, 0])), "reconstruction: qdc"
    assert np.array_equal(bits(o[prove][:, :, 2]), bits(fvd[mc[prove]][:, steps - 1, 2])), "reconstruction: depthc"
    want = np.zeros((n, steps.size, 3), fvd.dtype)
    want[mc] = o[:, :, [4, 3, 5]]
    return want, o


def peak_of(x):
    """the summary's rule: pk = x[1], at = 1; t = 2..: if x[t] > pk -- numpy's first argmax + 1 wherever no value is a NaN"""
    x = np.ascontiguousarray(x)
    peak, step = x[:, 0].copy(), np.ones(x.shape[0], np.int32)
    for t in range(1, x.shape[1]):
        m = x[:, t] > peak
        peak[m] = x[m, t]
        step[m] = t + 1
    clean = ~np.isnan(x).any(1)
    assert np.array_equal(step[clean], x[clean].argmax(1) + 1) and np.array_equal(peak[clean], x[clean].max(1))
    return peak, step


def assert_block(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, len(bad), bad[:6].tolist(), [got[tuple(b)] for b in bad[:6]], [want[tuple(b)] for b in bad[:6]])


# ---- 1. the golden domain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [True, False])
def test_lowercolorado_every_row_against_the_reference(short):
    lc = H.LowerColorado()
    up_ptr, up_idx = lc.csr()
    ups = [up_idx[up_ptr[i]:up_ptr[i + 1]].tolist() for i in range(lc.nseg)]
    nsteps = 96
    with RoutingPlan(up_ptr, up_idx, lc.params9, assume_short_ts=short) as p:
        p.route(nsteps, lc.qts, short, lc.qlat, lc.q0)
        fvd = p.download_fvd()
        got = p.window_courant()
    want, o = expected(fvd, lc.q0, lc.qlat, lc.params9, ups, lc.qts, short)
    assert_block(got, want, ("lowercolorado", short))
    fan = np.array([len(u) for u in ups])
    dry = (fvd[:, :, 0] == 0).all(1) & (want[:, :, 2] == 0).all(1)         # the no-flow branch: X stays 0
    assert (fan == 0).sum() == 3871 and (fan == 3).sum() == 7 and dry.sum() > 0
    assert np.nanmax(want[:, :, 0]) > 0 and 0 < np.nanmax(want[:, :, 2]) <= 0.5


# ---- 2. a synthetic network under a flood: engines, modes, precisions, the tile's edges ---------------------------------------
def flood_case(nseg, nq, seed=3):
    d = synthetic.generate(nseg=nseg, nnet=3, seed=seed, nq=nq)
    up_ptr, up_idx = synthetic.upstream_csr(d["to"])
    ups = [up_idx[up_ptr[i]:up_ptr[i + 1]].tolist() for i in range(nseg)]
    rng = np.random.default_rng(seed)
    qlat = (d["qlat"] * 40 + rng.uniform(0.0, 6.0, (nseg, nq)) * (rng.random((nseg, 1)) < 0.6)).astype(np.float32)
    q0 = np.stack([rng.uniform(0, 30, nseg), rng.uniform(0, 30, nseg), rng.uniform(0, 3, nseg)], 1).astype(np.float32)
    q0[rng.random(nseg) < 0.2] = 0
    return up_ptr, up_idx, ups, d["params"], qlat, q0


PATHS = {
    "levels-short-32": dict(engine="levels", short=True, precision=32),
    "levels-general-32": dict(engine="levels", short=False, precision=32),
    "flow-short-32": dict(engine="flow", short=True, precision=32),
    "flow-general-32": dict(engine="flow", short=False, precision=32),
    "levels-short-64": dict(engine="levels", short=True, precision=64),
    "levels-general-64": dict(engine="levels", short=False, precision=64),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_a_flooded_synthetic_network_on_the_edges_of_the_tile(path):
    cfg = dict(PATHS[path])
    short, precision = cfg.pop("short"), cfg["precision"]
    R, C = RoutingPlan.window_courant_tile(precision)
    nseg, nq, qts = 75 * R + 1, 5, 7                                        # (no multiple of the tile's rows; qts does not divide C)
    assert nseg % R and C % qts
    up_ptr, up_idx, ups, params, qlat, q0 = flood_case(nseg, -(-(2 * C + 3) // qts))
    bfd = (params[:, 3] - params[:, 2]) / (2 / params[:, 7])
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=short, **cfg) as p:
        assert p.engine == cfg["engine"]
        for nsteps in (1, 2, C - 1, C, C + 1, 2 * C + 3):
            p.route(nsteps, qts, short, qlat.astype(p.dtype), q0.astype(p.dtype))
            fvd = p.download_fvd()
            got = p.window_courant()
            want, _ = expected(fvd, q0, qlat, params, ups, qts, short)
            assert_block(got, want, (path, nsteps))
            if nsteps >= C:
                assert (fvd[:, :, 2] > bfd[:, None]).any()                  # over bank: the compound-channel celerity is taken
                assert (want[:, :, 0] > 1).any() and (want[:, :, 0] <= 1).any()


# ---- 3. stride, row sets, the summary -------------------------------------------------------------------------------------------
def test_stride_row_sets_and_the_summary():
    R, C = RoutingPlan.window_courant_tile(32)
    nseg, qts, nsteps = 40 * R + 3, 7, C + 11
    up_ptr, up_idx, ups, params, qlat, q0 = flood_case(nseg, -(-nsteps // qts), seed=5)
    rng = np.random.default_rng(1)
    rows = np.concatenate([rng.permutation(nseg), rng.integers(0, nseg, 2 * R + 1)])      # a permutation with repeats
    with RoutingPlan(up_ptr, up_idx, params) as p:
        p.route(nsteps, qts, False, qlat, q0)
        full = p.window_courant()
        want, _ = expected(p.download_fvd(), q0, qlat, params, ups, qts, False)
        assert_block(full, want, "full")
        rs = p.rowset(rows)
        for stride in (1, 5, nsteps):
            assert_block(p.window_courant(stride), full[:, stride - 1::stride][:, :nsteps // stride], ("stride", stride))
            assert_block(p.window_courant(stride, rowset=rs), full[rows][:, stride - 1::stride][:, :nsteps // stride], ("rowset", stride))
        cn = full[:, :, 0]
        pk_all, at_all = peak_of(cn)
        assert not np.isnan(cn).all(1).any() and (~np.isnan(cn).any(1)).sum() > nseg // 2
        for limit in (1.0, 1e9):
            for rr, c in ((None, cn), (rs, cn[rows])):
                s = p.window_courant_summary(limit, rowset=rr)
                pk, at = peak_of(c)
                assert list(s) == ["peak_cn", "peak_cn_step", "steps_over"]
                assert s["peak_cn"].dtype == np.float32 and s["peak_cn_step"].dtype == np.int32 and s["steps_over"].dtype == np.int32
                assert np.array_equal(bits(s["peak_cn"]), bits(pk)), limit
                assert np.array_equal(s["peak_cn_step"], at), limit
                assert np.array_equal(s["steps_over"], (c > np.float32(limit)).sum(1)), limit
        assert (cn > 1).any() and not (cn > np.float32(1e9)).any() and (at_all > 1).any()
        # any subset of NULL destinations
        h, pk, st, ov = _lib.lib(), np.zeros(nseg, np.float32), np.zeros(nseg, np.int32), np.zeros(nseg, np.int32)
        for a, b, c in ((pk, None, None), (None, None, ov), (pk, st, None), (pk, None, ov)):
            for x in (pk, st, ov):
                x[:] = -1
            assert h.trmc_window_courant_summary(p._h, -1, 1.0, _lib.ptr(a), _lib.ptr(b), _lib.ptr(c)) == 0
            assert a is None or np.array_equal(bits(pk), bits(pk_all))
            assert b is None or np.array_equal(st, at_all)
            assert c is None or np.array_equal(ov, (cn > 1).sum(1))
        assert p.window_courant_kernel_ms() >= 0


# ---- 4. reservoirs and gages on the golden domain ----------------------------------------------------------------------------
@pytest.mark.parametrize("short", [True, False])
def test_reservoir_rows_are_zero_and_the_row_below_uses_the_outflow(short):
    from test_reservoirs import reservoir_case
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured, mc_only_args
    nts = 48
    lc, ids, dv, ql, q0, reaches, net, lakes, wbody_cols, lakeset, nts = reservoir_case(nts)
    args = mc_only_args(nts, lc.dt, lc.qts, reaches, net, ids, lc.data_cols, dv, q0, ql, assume_short_ts=short)
    args[3] = [(r, 1 if r[0] in lakeset else 0) for r in reaches]
    args[10], args[11], args[13], args[14] = lakes.tolist(), wbody_cols, np.ones((len(lakes), 1), np.int32), False
    assert compute_network_structured(*args)[2] == 0
    r = compute_network_structured(*args, return_courant=True)
    fvd, got = r[1].reshape(len(ids), nts, 3), r[2].reshape(len(ids), nts, 3)
    assert r[2].dtype == r[1].dtype and r[2].shape == r[1].shape
    row = {int(s): i for i, s in enumerate(ids)}
    ups = [[] for _ in ids]
    for rr in reaches:
        for k, s in enumerate(rr):
            ups[row[s]] = [row[u] for u in net.get(rr[0], [])] if k == 0 else [row[rr[k - 1]]]
    lake_rows = np.array([row[int(l)] for l in lakes])
    mc = np.setdiff1d(np.arange(len(ids)), lake_rows)
    params9 = dv[:, [H.DATA_COLS.index(c) for c in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")]]
    want, _ = expected(fvd, q0, ql, params9, ups, lc.qts, short, mc_rows=mc)
    assert_block(got, want, ("reservoirs", short))
    assert not got[lake_rows].any() and np.abs(fvd[lake_rows, :, 0]).max() > 0
    below = [i for i in mc if any(u in set(lake_rows.tolist()) for u in ups[i])]
    assert below and np.nanmax(got[below, :, 0]) > 0                              # (rows fed by a pool's outflow: compared above)


def test_reservoir_rows_peak_at_step_one():
    from test_reservoirs import reservoir_case
    lc, ids, dv, ql, q0, reaches, net, lakes, wbody_cols, lakeset, nts = reservoir_case(24)
    row = {int(s): i for i, s in enumerate(ids)}
    ups = [[] for _ in ids]
    for rr in reaches:
        for k, s in enumerate(rr):
            ups[row[s]] = [row[u] for u in net.get(rr[0], [])] if k == 0 else [row[rr[k - 1]]]
    lake_rows = np.array([row[int(l)] for l in lakes])
    params9 = np.nan_to_num(dv[:, [H.DATA_COLS.index(c) for c in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")]], nan=1.0)
    params9[:, 0] = lc.dt
    a = wbody_cols.astype(np.float32)
    par = np.concatenate([a[:, :8], np.full((len(lakes), 1), 10.0, np.float32)], 1)
    q0 = q0.copy()
    q0[lake_rows, 2] = (a[:, 4] + ((a[:, 1] - a[:, 4]).astype(np.float32) * a[:, 8]).astype(np.float32)).astype(np.float32)
    up_ptr, up_idx = csr_from_lists(ups)
    with RoutingPlan(up_ptr, up_idx, params9, assume_short_ts=True) as p:
        p.set_reservoirs(lake_rows, par, lc.dt)
        p.route(nts, lc.qts, True, ql, q0)
        s = p.window_courant_summary(1.0)
        assert not p.window_courant()[lake_rows].any()
    assert not s["peak_cn"][lake_rows].any() and (s["peak_cn_step"][lake_rows] == 1).all() and not s["steps_over"][lake_rows].any()


GAGES = np.load(os.path.join(H.GOLDEN, "lowercolorado_gages.npz"))


@pytest.mark.parametrize("short", [True, False])
def test_nudged_rows_and_the_rows_below_them(short):
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured, mc_only_args
    lc = H.LowerColorado()
    nts = 48
    conn = {int(s): ([int(t)] if t != 0 else []) for s, t in zip(lc.ids, lc.to)}
    present = np.isin(GAGES["gage_ids"], lc.ids)
    gage_ids = GAGES["gage_ids"][present].tolist()
    ind, reaches_bytw, rconn = nn.organize_independent_networks(conn, set(), set(gage_ids))
    reaches, net = reaches_bytw[lc.tailwaters[0]], ind[lc.tailwaters[0]]
    row = {int(s): i for i, s in enumerate(lc.ids)}
    reach_of = {r[-1]: i for i, r in enumerate(reaches)}
    gage_ids = [g for g in gage_ids if g in reach_of]
    sel = np.array([GAGES["gage_ids"].tolist().index(g) for g in gage_ids])
    upos = np.array([row[g] for g in gage_ids], np.int32)
    upr = np.array([reach_of[g] for g in gage_ids], np.int32)
    args = mc_only_args(nts, lc.dt, lc.qts, reaches, net, lc.ids, lc.data_cols, lc.data_values, lc.q0, lc.qlat, assume_short_ts=short)
    args[16], args[17], args[18], args[19] = GAGES["usgs"][sel], upos, upr, np.arange(len(gage_ids), dtype=np.int32)
    args[20], args[21], args[22] = GAGES["lastobs_discharge"][sel], GAGES["time_since_lastobs"][sel], 120.0
    r = compute_network_structured(*args, return_courant=True)
    fvd, got = r[1].reshape(lc.nseg, nts, 3), r[2].reshape(lc.nseg, nts, 3)
    assert np.abs(r[8]).max() > 0                                           # something was nudged
    ups = [[] for _ in lc.ids]
    for rr in reaches:
        for k, s in enumerate(rr):
            ups[row[s]] = [row[u] for u in net.get(rr[0], [])] if k == 0 else [row[rr[k - 1]]]
    ungaged = np.setdiff1d(np.arange(lc.nseg), upos)
    q0 = lc.q0.copy()                                                       # a gage's initial flow is its first observation (mc_reach.pyx:404-411)
    first = GAGES["usgs"][sel][:, 0]
    q0[upos[~np.isnan(first)], 0] = first[~np.isnan(first)]
    want, _ = expected(fvd, q0, lc.qlat, lc.params9, ups, lc.qts, short, ungaged=ungaged)
    assert_block(got, want, ("nudging", short))
    below = [i for i in range(lc.nseg) if any(u in set(upos.tolist()) for u in ups[i])]
    assert below and len(upos) > 0


# ---- 5. the drop-in -------------------------------------------------------------------------------------------------------------
def test_the_drop_in_returns_the_block_as_element_2():
    from troute_amd.routing.compute import compute_nhd_routing_v02
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured, mc_only_args
    lc = H.LowerColorado()
    nts = 48
    args = mc_only_args(nts, lc.dt, lc.qts, lc.reaches, lc.rconn, lc.ids, lc.data_cols, lc.data_values, lc.q0, lc.qlat, None, False)
    plain = compute_network_structured(*args)
    assert plain[2] == 0 and not isinstance(plain[2], np.ndarray)            # the default call: the reference's literal
    full = compute_network_structured(*args, return_courant=True)
    fvd = full[1].reshape(lc.nseg, nts, 3)
    assert np.array_equal(bits(full[1]), bits(plain[1])) and full[2].shape == full[1].shape and full[2].dtype == full[1].dtype
    up_ptr, up_idx = lc.csr()
    ups = [up_idx[up_ptr[i]:up_ptr[i + 1]].tolist() for i in range(lc.nseg)]
    want, _ = expected(fvd, lc.q0, lc.qlat, lc.params9, ups, lc.qts, False)
    cou = full[2].reshape(lc.nseg, nts, 3)
    assert_block(cou, want, "drop-in")
    with RoutingPlan(up_ptr, up_idx, lc.params9) as p:                       # ... and equals plan.window_courant
        p.route(nts, lc.qts, False, lc.qlat, lc.q0)
        assert_block(p.window_courant(), cou, "plan")
    perm = np.random.default_rng(5).permutation(lc.nseg)
    for order in (None, perm):
        rows = np.arange(lc.nseg) if order is None else order
        got = compute_network_structured(*args, return_courant=True, output_stride=4, result_order=order)
        assert np.array_equal(got[0], full[0][rows])
        assert np.array_equal(bits(got[1].reshape(lc.nseg, nts // 4, 3)), bits(fvd[rows][:, 3::4, :]))
        assert got[2].shape == got[1].shape and got[2].dtype == got[1].dtype
        assert np.array_equal(bits(got[2].reshape(lc.nseg, nts // 4, 3)), bits(cou[rows][:, 3::4, :]))
    # upstream_results: a headwater reach cut off and handed in as a hydrograph -- its last row is masked out of [2] as out of [0], [1]
    row = {int(s): i for i, s in enumerate(lc.ids)}
    cut_reach = next(r for r in lc.reaches if not lc.rconn.get(r[0]) and lc.to[row[r[-1]]] != 0)
    cut, upper = cut_reach[-1], set(cut_reach)
    ids_lo = np.array(sorted((set(lc.ids.tolist()) - upper) | {cut}), np.int64)
    sel = np.array([row[s] for s in ids_lo])
    ur = {cut: {"position_index": int(np.searchsorted(ids_lo, cut)), "results": fvd[row[cut]].reshape(-1)}}
    a = mc_only_args(nts, lc.dt, lc.qts, [r for r in lc.reaches if r[0] not in upper], lc.rconn, ids_lo, lc.data_cols, lc.data_values[sel],
                     lc.q0[sel], lc.qlat[sel], upstream_results=ur, assume_short_ts=False)
    got = compute_network_structured(*a, return_courant=True, output_stride=4)
    keep = np.array([row[int(s)] for s in got[0]])
    assert got[0].shape[0] == len(ids_lo) - 1 and cut not in got[0] and got[2].shape == got[1].shape
    assert np.array_equal(bits(got[1].reshape(-1, nts // 4, 3)), bits(fvd[keep][:, 3::4, :]))
    assert np.array_equal(bits(got[2].reshape(-1, nts // 4, 3)), bits(cou[keep][:, 3::4, :]))
    # through compute_nhd_routing_v02: every tuple carries it, rows as its member [0]
    conn = {int(s): ([int(t)] if t != 0 else []) for s, t in zip(lc.ids, lc.to)}
    ind, reaches_bytw, rconn = nn.organize_independent_networks(conn)
    cols = ["dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0"]
    param_df = pd.DataFrame(lc.params9[:, 1:], index=lc.ids, columns=cols)
    param_df["alt"] = 0.0
    q0_df, qlat_df = pd.DataFrame(lc.q0, index=lc.ids, columns=["qu0", "qd0", "h0"]), pd.DataFrame(lc.qlat, index=lc.ids)
    e = pd.DataFrame()

    def call(courant, **kw):
        return compute_nhd_routing_v02(conn, rconn, {}, reaches_bytw, "V02-structured", "by-network", 10000, 4, None, 300.0, nts, lc.qts, ind,
                                       param_df, q0_df, qlat_df, e, e, e, e, e, e, e, e, e, e, e, {}, False, courant, e, {}, e, False,
                                       [{}, {}], {}, **kw)[0]
    off, on, on4 = call(False), call(True), call(True, output_stride=4)
    row_of = row
    assert len(off) == len(on) == len(on4) and all(not isinstance(t[2], np.ndarray) and t[2] == 0 for t in off)
    for a, b, c in zip(off, on, on4):
        rr = np.array([row_of[int(s)] for s in b[0]], dtype=np.int64)
        assert np.array_equal(a[0], b[0]) and b[2].shape == b[1].shape and c[2].shape == c[1].shape
        assert np.array_equal(bits(b[2].reshape(len(rr), nts, 3)), bits(cou[rr]))
        assert np.array_equal(bits(c[2].reshape(len(rr), nts // 4, 3)), bits(cou[rr][:, 3::4, :]))


def test_a_tolerance_plan_equals_the_single_segment_entry_in_that_arithmetic():
    R, C = RoutingPlan.window_courant_tile(32)
    nseg, qts, nsteps = 20 * R + 1, 7, C + 1
    up_ptr, up_idx, ups, params, qlat, q0 = flood_case(nseg, -(-nsteps // qts), seed=9)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={"arithmetic": "tolerance"}) as p:
        assert p.arithmetic == "tolerance"
        p.route(nsteps, qts, True, qlat, q0)
        fvd, got = p.download_fvd(), p.window_courant()
    x = rebuilt_inputs(fvd, q0, qlat, params, ups, qts, True)
    o = trmc_segments(x.reshape(-1, 15), arithmetic="tolerance").reshape(nseg, nsteps, 6)
    assert_block(got, np.ascontiguousarray(o[:, :, [4, 3, 5]]), "tolerance")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    nseg, nsteps, qts = 50, 8, 4
    up_ptr, up_idx, ups, params, qlat, q0 = flood_case(nseg, 2, seed=4)
    h = _lib.lib()
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options={"cluster_rows": 8, "wide_min_rows": 3, "wide_k": 4}) as p:
        with pytest.raises(RuntimeError, match="nothing routed"):
            p.window_courant()
        with pytest.raises(RuntimeError, match="nothing routed"):
            p.window_courant_summary()
        p.route(nsteps, qts, True, qlat, q0)
        full = p.window_courant()
        want, _ = expected(p.download_fvd(), q0, qlat, params, ups, qts, True)
        assert_block(full, want, "cluster tiles")
        with pytest.raises(ValueError):
            p.window_courant(0)
        buf, st = np.zeros((nseg, nsteps, 3), np.float32), np.zeros(nseg, np.int32)
        assert h.trmc_window_courant(p._h, -1, 0, _lib.ptr(buf)) == _lib.TRMC_EINVAL            # stride = 0
        assert h.trmc_window_courant(p._h, 7, 1, _lib.ptr(buf)) == _lib.TRMC_EINVAL             # no such row set
        assert h.trmc_window_courant_summary(p._h, -1, 1.0, None, _lib.ptr(st), None) == _lib.TRMC_EINVAL   # a step without its peak
        assert h.trmc_window_courant_summary(p._h, -1, 1.0, None, None, None) == _lib.TRMC_EINVAL
        p.route_begin(nsteps, qts, True)
        with pytest.raises(RuntimeError, match="window is in progress"):
            p.window_courant()
        p.route_advance(nsteps)
        p.route_end()
        assert_block(p.window_courant(), full, "the same forcing again")
        p.upload_forcing(nsteps, qlat, q0)
        p.stream_begin(nsteps, qts)
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.window_courant()
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.window_courant_summary()
        p.stream_push(pinned_like(qlat))
        p.stream_flush()
        p.stream_end()
        with pytest.raises(RuntimeError, match="nothing routed"):
            p.window_courant()
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels") as p:        # a lagged plan
        lag = np.zeros(nseg, np.int32)
        fed = {u for us in ups for u in us}
        lag[[i for i in range(nseg) if ups[i] and i not in fed][:1]] = 1      # (an outlet: a lagged row may feed lagged rows only)
        p.set_lag(lag)
        p.route(nsteps, qts, True, qlat, q0)
        with pytest.raises(NotImplementedError, match="lagged rows"):
            p.window_courant()
        with pytest.raises(NotImplementedError, match="lagged rows"):
            p.window_courant_summary()
