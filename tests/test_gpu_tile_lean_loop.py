"""THE STEP LOOP OF THE PRODUCTS-ONLY TILE KERNELS after its registers were rearranged (det_pow.h: the power's constants formed in
scalar registers where they are used): k_mc_tile / k_mc_ctile <float, false, false, true> and their DEC variants, bit for bit.

One small network -- three wide levels of 300 rows (the slices: k_mc_tile) over a tail in clusters (k_mc_ctile), with junctions
of three and of four rows in the slices and in the tail (the CSR walk behind the table of the first two), rows without any flow
(the step's early exit), rows pushed over bank (the general body of the hydraulic point) -- routed as two days of 32 steps,
qts = 4, as a stream WITHOUT full_output: every row's hydrograph and the final states of both days against the oracle and
against the same days through the full_output instances; then with output_stride = 4 (kept steps carry velocities).

The level-pool row and the nudged gage -- the other two rare branches of the loop -- are routed here as one window at plan
level: the same network, full result against the oracle's level pool and simple_da.  (A stream of days carries reservoirs and
nudging too, its tables arriving with every day: test_gpu_stream_reservoirs_nudging, test_gpu_stream_reservoir_da.)

The hot-list boundaries: one wide level of 130 rows (a full block and a block of two rows) and one of 64 + 1."""
import functools

import numpy as np
import pytest

import test_gpu_ctile_block as CB
import test_gpu_ctile_tables as CT
from oracle import oracle as O
from troute_amd import _lib
from troute_amd.plan import RoutingPlan, topology_levels
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

NSTEPS, QTS, K = 32, 4, 8
bits = CB.bits
OPTS = {"cluster_rows": 64, "wide_min_rows": 200, "wide_k": K}


@functools.lru_cache(maxsize=None)
def network():
    """to[], the dry rows, the wet rows.  Levels 0..2 hold 300 rows each (level 0: 305 -- the extra headwaters make row 305 a
    junction of three and row 306 one of four); below them a tail that halves from 148 rows down to one outlet, whose first two
    rows are junctions of four and of three."""
    w = 300
    l0 = np.arange(0, w + 5)
    l1 = np.arange(w + 5, 2 * w + 5)
    l2 = np.arange(2 * w + 5, 3 * w + 5)
    to = []
    to += l1.tolist()                      # level 0 row i -> level 1 row i
    to += [l1[0], l1[0], l1[1], l1[1], l1[1]]   # fan-in 3 at l1[0], fan-in 4 at l1[1]
    to += l2.tolist()
    nxt = 3 * w + 5
    # level 2 -> tail: four rows into the first, three into the second, the other 293 in pairs (the last one alone)
    groups = [4, 3] + [2] * 146 + [1]
    assert sum(groups) == w
    t2 = []
    for g, n in enumerate(groups):
        t2 += [nxt + g] * n
    to += t2
    cur = list(range(nxt, nxt + len(groups)))
    nxt += len(groups)
    while len(cur) > 1:                    # the tail halves
        down = []
        for i in range(0, len(cur), 2):
            down.append(nxt)
            to += [nxt] * len(cur[i:i + 2])
            nxt += 1
        cur = down
    to.append(-1)
    to = np.array(to, np.int64)
    assert to.shape[0] == nxt
    rng = np.random.default_rng(77)
    n = to.shape[0]
    # dry: a headwater, its level-1 and level-2 rows (nothing flows in, nothing is in them); wet: a tenth of the rows
    dry = np.array([10, l1[10], l2[10], 11, l1[11]], np.int64)
    wet = rng.random(n) < 0.1
    wet[dry] = False
    return to, dry, wet


@functools.lru_cache(maxsize=None)
def inputs():
    to, dry, wet = network()
    rng = np.random.default_rng(78)
    n = to.shape[0]
    params, ql, q0 = CB.inputs(rng, n, nq=NSTEPS // QTS, wet=wet)
    ql[dry] = 0
    q0[dry] = 0
    days = [ql, (ql * np.float32(1.6)).astype(np.float32)]
    up_ptr, up_idx = CB.csr_of(to)
    level = topology_levels(up_ptr, up_idx)[0]
    for a in (params, q0, *days):
        a.setflags(write=False)
    return up_ptr, up_idx, level, params, days, q0


@functools.lru_cache(maxsize=None)
def oracle_days():
    """the two days by the CPU restatement of the reference loop, the state handed on as new_q0 does: [n, NSTEPS, 3] each"""
    up_ptr, up_idx, level, params, days, q0 = inputs()
    state, out = q0, []
    for q in days:
        w = O.network_by_segment(NSTEPS, QTS, up_ptr, up_idx, level, params, state, q, True, det=True)[:, 1:, :]
        w.setflags(write=False)
        out.append(w)
        state = np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], 1)
    return out


def open_plan():
    up_ptr, up_idx, level, params, days, q0 = inputs()
    return RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", options=OPTS)


def check_paths(plan):
    """every path the loop has is taken by this network on this plan: slices and clusters, fan-in three and four in both, rows
    without flow, rows over bank"""
    to, dry, wet = network()
    up_ptr, up_idx, level, params, days, q0 = inputs()
    lag, W, C = plan.lags()
    assert W == 3 and C >= 2, (W, C)
    fan = np.diff(up_ptr)
    assert np.count_nonzero((fan == 3) & (lag < W)) >= 1 and np.count_nonzero((fan == 4) & (lag < W)) >= 1
    assert np.count_nonzero((fan == 3) & (lag >= W)) >= 1 and np.count_nonzero((fan == 4) & (lag >= W)) >= 1
    assert np.count_nonzero(lag < W) == 905
    want = oracle_days()
    assert all(not w[dry].any() for w in want)                       # nothing is routed there: the step's early exit
    assert all(np.all(w[~np.isin(np.arange(to.shape[0]), dry), -1, 0] > 0) for w in want)


def stream(plan, full_output=False, output_stride=0):
    """both days as one stream; per day (hydrographs of every row [n, NSTEPS], final state [n, 3], the (q, v, d) block or None)"""
    up_ptr, up_idx, level, params, days, q0 = inputs()
    n = params.shape[0]
    rs = plan.rowset(np.arange(n))
    plan.upload_forcing(NSTEPS, days[0], q0)
    plan.stream_begin(NSTEPS, QTS, full_output=full_output, output_stride=output_stride)
    kept = NSTEPS // output_stride if output_stride else NSTEPS
    keep, out = [pinned_like(q) for q in days], []
    for q in keep:
        hyd = _lib.result_empty((n, NSTEPS), np.float32, always_pinned=True)
        st = _lib.result_empty((n, 3), np.float32, always_pinned=True)
        blk = _lib.result_empty((n, kept, 3), np.float32, always_pinned=True) if (full_output or output_stride) else None
        plan.stream_push(q, rowset=rs, hyd=hyd, q0=st, fvd=blk)
        out.append((hyd, st, blk))
    plan.stream_flush()
    for d in range(len(days)):
        plan.stream_wait(d)
    info = plan.stream_info()
    plan.stream_end()
    assert info["wide_levels"] == 3 and info["cluster_levels"] >= 2
    return out


def check_products(got, want, d):
    hyd, st, _ = got
    assert np.array_equal(bits(hyd), bits(want[:, :, 0])), d
    assert np.array_equal(bits(st), bits(np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1))), d


def test_products_only_stream_equals_the_oracle_and_the_full_output_instances():
    want = oracle_days()
    with open_plan() as plan:
        check_paths(plan)
        lean = stream(plan)
        full = stream(plan, full_output=True)
    for d in range(2):
        check_products(lean[d], want[d], d)
        assert np.array_equal(bits(full[d][2]), bits(want[d])), d
        assert np.array_equal(bits(lean[d][0]), bits(full[d][0])) and np.array_equal(bits(lean[d][1]), bits(full[d][1])), d


def test_decimated_stream_keeps_velocities_of_the_kept_steps():
    """output_stride = 4: the DEC instances; the kept steps' (q, v, d) -- velocities among them -- are the oracle's"""
    want = oracle_days()
    with open_plan() as plan:
        dec = stream(plan, output_stride=4)
    for d in range(2):
        check_products(dec[d], want[d], d)
        w = np.ascontiguousarray(want[d][:, 3::4])
        assert dec[d][2].shape == w.shape and np.any(w[:, :, 1] != 0)
        assert np.array_equal(bits(dec[d][2]), bits(w)), d


def test_rows_over_bank_are_routed_over_bank():
    """the plan's cost diagnostics: a step over bank counts four more than its iteration class (at most three) -- a row whose
    sum over the window exceeds 3 NSTEPS has taken the compound-channel body"""
    up_ptr, up_idx, level, params, days, q0 = inputs()
    to, dry, wet = network()
    with open_plan() as plan:
        lag, W, C = plan.lags()
        plan.collect_cost(True)
        plan.upload_forcing(NSTEPS, days[0], q0)
        plan.route_device(NSTEPS, QTS, True)
        cost, nts = plan.download_cost()
        assert nts == NSTEPS
        over = cost > 3 * NSTEPS
        assert np.count_nonzero(over & (lag < W)) >= 1 and np.count_nonzero(over & (lag >= W)) >= 1
        assert not cost[dry].any()
        assert np.array_equal(bits(plan.download_fvd()), bits(oracle_days()[0]))


def test_level_pool_and_nudged_gage_on_the_same_network():
    """a level-pool reservoir in the slices and a nudged gage in the tail (and the other way round): one window at plan level,
    the full result, the reservoirs' inflows and the nudges against the oracle"""
    to, dry, wet = network()
    up_ptr, up_idx, level, params, days, q0 = inputs()
    n = to.shape[0]
    lakes = {"lake_slice": 305 + 40, "lake_tail": n - 4}
    gages = {"gage_slice": 305 + 300 + 50, "gage_tail": n - 6}
    c = CT.make_case(to, lakes, gages, seed=9, nq=NSTEPS // QTS, extra_gages=0)
    order = np.argsort(c.level, kind="stable")
    res_of_row = np.full(n, -1, np.int64)
    res_of_row[c.lakes] = np.arange(c.lakes.shape[0])
    gage_of_row = np.full(n, -1, np.int64)
    gage_of_row[c.gages] = np.arange(c.gages.shape[0])
    res = dict(res_of_reach=res_of_row[order], par=c.par, water_elevation=c.h0, routing_period=CT.DT)
    da = dict(usgs_values=c.usgs, gage_row=c.gages, gage_of_reach=gage_of_row[order], decay_coeff=CT.DECAY, routing_period=CT.DT,
              lastobs_time=c.lt0, lastobs_val=c.lv0)
    want = O.network_by_segment(NSTEPS, QTS, c.up_ptr, c.up_idx, c.level, c.params, c.q0, c.ql, True, det=True, res=res, da=da)
    assert np.abs(da["nudge"][:, 1:]).max(axis=1).min() > 0 and np.all(want[c.lakes, 1:, 0].max(axis=1) > 0)
    with RoutingPlan(c.up_ptr, c.up_idx, c.params, assume_short_ts=True, engine="levels", options=OPTS) as plan:
        lag, W, C = plan.lags()
        c.lag = lag
        assert lag[lakes["lake_slice"]] < W <= lag[lakes["lake_tail"]] and lag[gages["gage_slice"]] < W <= lag[gages["gage_tail"]]
        CT.stage(plan, c, NSTEPS, QTS)
        stats = plan.route_device(NSTEPS, QTS, True)
        assert stats["wide_segment_steps"] == n * NSTEPS, stats
        CT.check_window(plan, c, want, res, da)


@pytest.mark.parametrize("rows", [130, 65])
def test_one_wide_level_that_ends_in_a_short_block(rows):
    """`rows` headwaters that are their own outlets: one slice of one full block (two for 130: 128 + 2; 64 + 1 for 65) whose last
    block holds one or two rows -- the class partition's `none` and the `s >= s_end` return, from the second tile on with the
    classes of the tile before; a tenth of the rows wet, so that the partition moves rows between threads"""
    rng = np.random.default_rng(rows)
    to = np.full(rows, -1, np.int64)
    up_ptr, up_idx = CB.csr_of(to)
    wet = rng.random(rows) < 0.1
    params, ql, q0 = CB.inputs(rng, rows, nq=NSTEPS // QTS, wet=wet)
    level = topology_levels(up_ptr, up_idx)[0]
    days = [ql, (ql * np.float32(0.5)).astype(np.float32)]
    rs_rows = np.arange(rows)
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels",
                     options={"cluster_rows": 64, "wide_min_rows": 1, "wide_k": K}) as plan:
        lag, W, C = plan.lags()
        assert W == 1 and np.all(lag == 0)
        rs = plan.rowset(rs_rows)
        plan.upload_forcing(NSTEPS, days[0], q0)
        plan.stream_begin(NSTEPS, QTS)
        keep, out = [pinned_like(q) for q in days], []
        for q in keep:
            hyd = _lib.result_empty((rows, NSTEPS), np.float32, always_pinned=True)
            st = _lib.result_empty((rows, 3), np.float32, always_pinned=True)
            plan.stream_push(q, rowset=rs, hyd=hyd, q0=st)
            out.append((hyd, st, None))
        plan.stream_flush()
        state = q0
        for d, q in enumerate(days):
            plan.stream_wait(d)
            want = O.network_by_segment(NSTEPS, QTS, up_ptr, up_idx, level, params, state, q, True, det=True)[:, 1:, :]
            check_products(out[d], want, d)
            state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
        plan.stream_end()
