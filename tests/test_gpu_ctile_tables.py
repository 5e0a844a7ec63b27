"""RESERVOIRS, RESERVOIR DATA ASSIMILATION AND NUDGING ON PLANS IN CLUSTER ORDER (csrc/k_mc_ctile.inc; k_mc_tile's table branches
under the cluster order's lags): single windows at plan level on small synthetic networks whose lakes and gages sit where the
cluster kernel can go wrong -- a lake whose inflows all come from the time-major plane, all through LDS, from both in one
junction sum (the CSR tail of a row with three upstream rows), below another lake, at a headwater, at an outlet; a gage whose
nudged flow must reach the plane (the next cluster level reads it), the LDS slot (a row of its own cluster reads it), a lake.

The reference is the oracle's restatement of the reference loop with its level pool and its simple_da, every row its own reach
(oracle.network_by_segment(..., res=, da=)): fp32, short timestep, bit for bit.  Which rows are read through LDS follows from
the lags alone: a cluster lies inside one block, every other edge comes from a row that runs at least a tile ahead
(test_gpu_ctile_block.shape_of) -- so the placements are found on the CPU (trmc_topology_clusters), a test without a GPU checks
them and what the oracle alone can say (the pools move, the nudges are not zero), and every GPU test asserts that the plan's
own lags and blocks are the ones the placements were found with."""
import functools

import numpy as np
import pytest

import helpers as H
import test_gpu_ctile_block as CB
import test_reservoirs as TR
from oracle import oracle as O
from troute_amd.plan import RoutingPlan, topology_clusters, topology_levels
from troute_amd.routing.fast_reach import simple_da as DA

K = 8            # steps per tile launch
NSTEPS = 44      # five tiles and a short one
DT = 300.0
DECAY = 120.0
GMAX = 2 * NSTEPS + 8
bits = CB.bits


# ---- networks --------------------------------------------------------------------------------------------------------------
def _ups_of(to):
    ups = [[] for _ in range(to.shape[0])]
    for i, d in enumerate(to.tolist()):
        if d >= 0:
            ups[d].append(i)
    return ups


def placement_network(seed=11, n_base=2600):
    """chain A (300 rows), helpers.random_network, chain B (200 rows), chain C (150 rows, an outlet of its own).  A and B end in
    rows of the random part that had two small tributaries: junctions of three rows, one of which -- the FIRST of the sum for A,
    the LAST (the CSR tail) for B -- has collected at least a cluster more than the others."""
    rng = np.random.default_rng(seed)
    base = H.random_network(rng, n_base)
    la, lb, lc_ = 300, 200, 150
    ups = _ups_of(base)
    size = np.ones(n_base, np.int64)                      # rows draining through every row
    order = np.argsort(topology_levels(*CB.csr_of(base))[0], kind="stable")
    for r in order:
        if base[r] >= 0:
            size[base[r]] += size[r]
    cand = [r for r in range(n_base) if len(ups[r]) == 2 and size[r] <= 12 and base[r] >= 0]
    assert len(cand) >= 2
    ja, jb = cand[0], cand[len(cand) // 2]
    to = np.full(la + n_base + lb + lc_, -1, np.int64)
    to[:la] = np.arange(1, la + 1)
    to[la - 1] = la + ja
    to[la:la + n_base] = np.where(base >= 0, base + la, -1)
    b0 = la + n_base
    to[b0:b0 + lb] = np.arange(b0 + 1, b0 + lb + 1)
    to[b0 + lb - 1] = la + jb
    c0 = b0 + lb
    to[c0:] = np.arange(c0 + 1, c0 + lc_ + 1)
    to[-1] = -1
    return to, la + ja, la + jb


def find_placements(to, up_ptr, up_idx, lag, W, ja, jb):
    """{name: row} of the lakes and gages of the placement cases.  Rows of lag >= W are cluster rows: an upstream row of the
    same lag hands its flow on through LDS, any other through the plane; rows of lag < W are rows of the slices."""
    n = to.shape[0]
    ups = [up_idx[up_ptr[r]:up_ptr[r + 1]] for r in range(n)]
    cl = lag >= W
    taken, out = set(), {}

    def free(r):
        return r not in taken and all(int(u) not in taken for u in ups[r]) and int(to[r]) not in taken

    def pick(name, cond, need_free=True):
        for r in range(n):
            if (not need_free or free(r)) and r not in taken and cond(r):
                out[name] = r
                taken.add(r)
                return r
        raise AssertionError(f"no row for {name}")

    # the two junctions of three first: rows given by the builder
    for name, j, chain_is in (("lake_junction_lds_first", ja, 0), ("lake_junction_lds_tail", jb, 2)):
        u = ups[j]
        assert cl[j] and u.shape[0] == 3
        same = lag[u] == lag[j]
        assert same[chain_is] and same.sum() == 1 and np.all(lag[u][~same] < lag[j]), (name, lag[u], lag[j])
        out[name] = j
        taken.add(j)
    pick("lake_cluster_head", lambda r: cl[r] and ups[r].shape[0] >= 1 and np.all(lag[ups[r]] < lag[r]) and to[r] >= 0
         and lag[to[r]] == lag[r])
    b = pick("lake_interior", lambda r: cl[r] and ups[r].shape[0] == 2 and np.all(lag[ups[r]] == lag[r]) and to[r] >= 0
             and lag[to[r]] == lag[r] and ups[to[r]].shape[0] == 1)
    out["lake_below_lake"] = int(to[b])                       # (its only inflow: the lake above, through LDS)
    taken.add(int(to[b]))
    if W == 0:                                                # (under slices every headwater is a row of the first slice)
        pick("lake_headwater", lambda r: ups[r].shape[0] == 0 and to[r] >= 0 and lag[to[r]] == lag[r])
    pick("lake_outlet", lambda r: cl[r] and to[r] < 0 and ups[r].shape[0] >= 1)
    # a lake right below a lake of the cluster level above: the inflow is a lake's outflow read from the plane
    a = pick("lake_feeds_next_level", lambda r: cl[r] and to[r] >= 0 and lag[to[r]] > lag[r] and ups[to[r]].shape[0] == 1
             and ups[r].shape[0] >= 1)
    out["lake_below_lake_plane"] = int(to[a])
    taken.add(int(to[a]))
    lakes = dict(out)
    # gages
    pick("gage_feeds_next_level", lambda r: cl[r] and to[r] >= 0 and lag[to[r]] > lag[r])
    pick("gage_interior", lambda r: cl[r] and to[r] >= 0 and lag[to[r]] == lag[r] and ups[r].shape[0] >= 1)
    for name, lake in (("gage_above_lake_plane", "lake_cluster_head"), ("gage_above_lake_lds", "lake_interior")):
        g = int(ups[out[lake]][0])
        assert g not in taken
        out[name] = g
        taken.add(g)
    pick("gage_modes_012", lambda r: cl[r] and to[r] >= 0 and lag[to[r]] == lag[r], need_free=False)
    pick("gage_no_obs_decays", lambda r: cl[r] and to[r] >= 0 and lag[to[r]] == lag[r], need_free=False)
    pick("gage_no_obs_no_lastobs", lambda r: cl[r] and to[r] >= 0 and lag[to[r]] > lag[r], need_free=False)
    if W > 0:
        pick("slice_lake_junction", lambda r: 0 < lag[r] < W and ups[r].shape[0] >= 2 and to[r] >= 0)
        pick("slice_lake_headwater", lambda r: lag[r] == 0 and to[r] >= 0 and lag[to[r]] < W)
        pick("slice_gage", lambda r: 0 < lag[r] < W and to[r] >= 0 and lag[to[r]] < W)
        pick("slice_gage_feeds_cluster", lambda r: 0 <= lag[r] < W and to[r] >= 0 and lag[to[r]] >= W)
        for k in ("slice_lake_junction", "slice_lake_headwater"):
            lakes[k] = out[k]
    gages = {k: v for k, v in out.items() if k not in lakes}
    return lakes, gages


# ---- a case: network, inputs, tables ----------------------------------------------------------------------------------------
class Case:
    pass


def lake_parameters(nlakes):
    """rows of test_reservoirs.lake_tables() in oracle.LP_PAR order, dam_length 10, reused cyclically; initial pool elevations
    between the orifice and a little above the dam's crest (the overtopping branch)"""
    _, cols = TR.lake_tables()
    a = cols.astype(np.float32)
    k = np.arange(nlakes) % a.shape[0]
    par = np.concatenate([a[k, :8], np.full((nlakes, 1), 10.0, np.float32)], 1)
    frac = np.array([0.9, 1.02, 0.5, 0.97], np.float32)[np.arange(nlakes) % 4]
    h0 = (par[:, 4] + ((par[:, 1] - par[:, 4]).astype(np.float32) * frac).astype(np.float32)).astype(np.float32)
    return par, h0


def make_case(to, lakes, gages, seed, nq=2 * NSTEPS // 4, extra_gages=24):
    """inputs and tables of a window of up to 2 NSTEPS steps: lakes / gages {name: row}"""
    rng = np.random.default_rng(seed)
    c = Case()
    n = to.shape[0]
    c.to, c.n = to, n
    c.up_ptr, c.up_idx = CB.csr_of(to)
    c.level = topology_levels(c.up_ptr, c.up_idx)[0]
    wet = rng.random(n) < 0.1
    c.params, ql, q0 = CB.inputs(rng, n, nq=nq, wet=wet)
    c.ql = (ql * np.float32(100.0)).astype(np.float32)               # wet enough for the pools to move
    c.lake_names, c.gage_names = list(lakes), list(gages)
    c.lakes = np.array([lakes[k] for k in c.lake_names], np.int64)
    g = [gages[k] for k in c.gage_names]
    used = set(c.lakes.tolist()) | set(g)
    more = [int(r) for r in rng.permutation(n) if int(r) not in used][:extra_gages]
    c.gage_names += [f"gage_random_{i}" for i in range(len(more))]
    c.gages = np.array(g + more, np.int64)
    assert len(set(c.gages.tolist())) == c.gages.shape[0] and not set(c.gages.tolist()) & set(c.lakes.tolist())
    c.par, c.h0 = lake_parameters(c.lakes.shape[0])
    ng = c.gages.shape[0]
    usgs = rng.lognormal(np.log(0.5), 1.0, (ng, GMAX)).astype(np.float32)
    usgs[rng.random((ng, GMAX)) < 0.3] = np.nan
    lv0 = rng.lognormal(np.log(0.5), 1.0, ng).astype(np.float32)
    lt0 = (-rng.integers(0, 7200, ng)).astype(np.float32)           # (whole seconds: a window that starts later shifts them exactly)
    for i, name in enumerate(c.gage_names):
        if name == "gage_modes_012":                                 # nothing known, then observations, then decay
            usgs[i, :] = np.nan
            usgs[i, 12:20] = rng.lognormal(0, 1, 8).astype(np.float32)
            lv0[i] = lt0[i] = np.nan
        elif name == "gage_no_obs_decays":
            usgs[i, :] = np.nan
        elif name == "gage_no_obs_no_lastobs":
            usgs[i, :] = np.nan
            lv0[i] = lt0[i] = np.nan
    c.usgs, c.lv0, c.lt0 = usgs, lv0, lt0
    q0 = q0.copy()
    q0[c.lakes, 2] = c.h0                                           # the pool's elevation lives in the depth slot
    q0[c.lakes, 1] = 0
    ok = ~np.isnan(usgs[:, 0])
    q0[c.gages[ok], 0] = usgs[ok, 0]                                # mc_reach.pyx:404-411
    c.q0 = q0
    return c


def nudging_tables(c, nsteps, start=0, lastobs=None):
    """(mode, a, w, lt_fin, lv_fin) of the window of `nsteps` steps that begins `start` steps after the case's t0, resolved as
    mc_reach.py does (simple_da.resolve_tables) from the observations indexed by the window's own timestep"""
    lv0, lt0 = (c.lv0, c.lt0) if lastobs is None else lastobs
    return DA.resolve_tables(nsteps, DT, DECAY, c.usgs[:, start:], lv0, lt0)


@functools.lru_cache(maxsize=None)
def reference(key, nsteps, qts):
    """the oracle's window of case `key` (OPTIONS): fvd [n, nsteps + 1, 3], res (inflow, final elevations), da (nudge, lastobs)"""
    c = case(key)
    order = np.argsort(c.level, kind="stable")
    res_of_row = np.full(c.n, -1, np.int64)
    res_of_row[c.lakes] = np.arange(c.lakes.shape[0])
    gage_of_row = np.full(c.n, -1, np.int64)
    gage_of_row[c.gages] = np.arange(c.gages.shape[0])
    res = dict(res_of_reach=res_of_row[order], par=c.par, water_elevation=c.h0, routing_period=DT)
    da = dict(usgs_values=c.usgs, gage_row=c.gages, gage_of_reach=gage_of_row[order], decay_coeff=DECAY, routing_period=DT,
              lastobs_time=c.lt0, lastobs_val=c.lv0)
    nq = -(-nsteps // qts)
    want = O.network_by_segment(nsteps, qts, c.up_ptr, c.up_idx, c.level, c.params, c.q0, c.ql[:, :nq], True, det=True, res=res, da=da)
    for a in (want, res["inflow"], res["water_elevation"], da["nudge"], da["lastobs_time"], da["lastobs_val"]):
        a.setflags(write=False)
    return want, res, da


OPTIONS = {
    "placement-24": {"cluster_rows": 24, "wide_min_rows": -1, "wide_k": K},
    "placement-128": {"cluster_rows": 128, "wide_min_rows": -1, "wide_k": K},
    "slices": {"cluster_rows": 64, "wide_min_rows": 200, "wide_k": K},
    "forest": {"cluster_rows": 128, "wide_min_rows": -1, "wide_k": K},
}
FOREST_WIDTH = 512          # (the forest is built for this block width; the GPU test asserts it is the library's)


def cpu_order(key, up_ptr, up_idx):
    o = OPTIONS[key]
    pos, lag, blk, W, C, nb = topology_clusters(up_ptr, up_idx, wide_min_rows=max(0, o["wide_min_rows"]), cluster_rows=o["cluster_rows"])
    return lag, W, C


@functools.lru_cache(maxsize=None)
def case(key):
    if key == "forest":
        # one cluster level of small trees, three blocks and a bit: a lake with a gage right above it and a gage below in
        # every third tree, so that some of them sit in clusters that are not their block's first
        rng = np.random.default_rng(5)
        sizes = CB.many_small_clusters(FOREST_WIDTH, rng)
        to = CB.forest(sizes, rng)
        up_ptr, up_idx = CB.csr_of(to)
        lag, W, C = cpu_order(key, up_ptr, up_idx)
        assert W == 0 and C == 1
        ups = _ups_of(to)
        root = np.arange(to.shape[0])
        for r in np.argsort(-topology_levels(up_ptr, up_idx)[0], kind="stable"):     # outlets first
            if to[r] >= 0:
                root[r] = root[to[r]]
        lakes, gages = {}, {}
        for t, o in enumerate(np.flatnonzero(to < 0).tolist()):
            if t % 3:
                continue
            tree = np.flatnonzero(root == o)
            junction = [int(r) for r in tree if len(ups[r]) >= 2 and to[r] >= 0]
            if not junction:
                continue
            lk = junction[0]
            lakes[f"lake_tree_{t}"] = lk
            gages[f"gage_above_lake_tree_{t}"] = ups[lk][0]
            gages[f"gage_below_lake_tree_{t}"] = int(to[lk])
        assert len(lakes) >= 12
        c = make_case(to, lakes, gages, seed=105, extra_gages=0)
        c.lag, c.W, c.C = lag, W, C
        return c
    to, ja, jb = placement_network()
    up_ptr, up_idx = CB.csr_of(to)
    lag, W, C = cpu_order(key, up_ptr, up_idx)
    assert (W > 0) == (key == "slices") and C >= 3
    lakes, gages = find_placements(to, up_ptr, up_idx, lag, W, ja, jb)
    c = make_case(to, lakes, gages, seed=100 + len(key))
    c.lag, c.W, c.C = lag, W, C
    return c


def check_oracle_conditions(key, nsteps, qts):
    """what the oracle alone can say about a case: every pool spills at some step and moves, the nudges are not zero, the
    gages meant to take every branch of simple_da do, the host's tables end on the oracle's lastobs"""
    c = case(key)
    want, res, da = reference(key, nsteps, qts)
    assert np.isfinite(want).all()
    q, h = want[c.lakes, 1:, 0], want[c.lakes, :, 2]
    assert np.all(q.max(axis=1) > 0), [c.lake_names[i] for i in np.flatnonzero(~(q.max(axis=1) > 0))]
    assert np.all((h[:, 1:] != h[:, :1]).any(axis=1)), [c.lake_names[i] for i in np.flatnonzero(~(h[:, 1:] != h[:, :1]).any(axis=1))]
    assert np.array_equal(h[:, 0], c.h0) and np.array_equal(h[:, -1], res["water_elevation"])
    fed = np.diff(c.up_ptr)[c.lakes] > 0                               # (a headwater lake only drains)
    assert np.all(res["inflow"][fed, 1:].max(axis=1) > 0) and not res["inflow"][~fed].any()
    mode, a, w, lt_fin, lv_fin = nudging_tables(c, nsteps)
    assert np.array_equal(bits(lt_fin), bits(da["lastobs_time"])) and np.array_equal(bits(lv_fin), bits(da["lastobs_val"]))
    nudge = da["nudge"][:, 1:]
    assert np.count_nonzero(np.abs(nudge).max(axis=1) > 0) >= c.gages.shape[0] - 2
    for i, name in enumerate(c.gage_names):
        if name == "gage_modes_012":
            assert set(mode[i].tolist()) == {0, 1, 2}
        elif name == "gage_no_obs_decays":
            assert set(mode[i].tolist()) == {2} and np.abs(nudge[i]).max() > 0
        elif name == "gage_no_obs_no_lastobs":
            assert set(mode[i].tolist()) == {0} and not nudge[i].any()
    return mode


def test_networks_placements_and_oracle_conditions():
    """no GPU: the builders, the placement search on the library's host-side cluster order, and the oracle-only conditions of
    every case the GPU tests route"""
    for key in OPTIONS:
        c = case(key)
        assert 1500 <= c.n <= 6000, c.n
        for qts in (4, 11):
            check_oracle_conditions(key, NSTEPS, qts)
    check_oracle_conditions("placement-24", 2 * NSTEPS, 4)
    for key in ("placement-24", "placement-128", "slices"):
        c = case(key)
        names = set(c.lake_names) | set(c.gage_names)
        assert {"lake_cluster_head", "lake_interior", "lake_junction_lds_first", "lake_junction_lds_tail", "lake_below_lake",
                "lake_below_lake_plane", "lake_outlet", "gage_feeds_next_level", "gage_interior",
                "gage_above_lake_plane", "gage_above_lake_lds", "gage_modes_012", "gage_no_obs_decays",
                "gage_no_obs_no_lastobs"} <= names
        assert key == "slices" or "lake_headwater" in names
        if key == "slices":
            assert {"slice_lake_junction", "slice_lake_headwater", "slice_gage", "slice_gage_feeds_cluster"} <= names
            assert np.all(c.lag[[c.lakes[c.lake_names.index(k)] for k in ("slice_lake_junction", "slice_lake_headwater")]] < c.W)


# ---- the GPU side -----------------------------------------------------------------------------------------------------------
def open_plan(key, cost_hint=None):
    c = case(key)
    return RoutingPlan(c.up_ptr, c.up_idx, c.params, assume_short_ts=True, engine="levels", cost_hint=cost_hint, options=OPTIONS[key])


def check_order(plan, key):
    """the plan's own order is the one the placements were found with (it does not depend on the tables): the lags, the slices,
    and -- the premise of the search -- an edge between rows of one cluster lag stays inside a block, any other crosses blocks"""
    c = case(key)
    lag, W, C = plan.lags()
    blk, width, nb = plan.cluster_blocks()
    assert np.array_equal(lag, c.lag) and (W, C) == (c.W, c.C)
    assert np.array_equal(blk < 0, lag < W)
    down = np.repeat(np.arange(c.n), np.diff(c.up_ptr))
    same = (lag[c.up_idx] == lag[down]) & (lag[down] >= W)
    assert np.all(blk[c.up_idx][same] == blk[down][same])
    assert np.all((blk[c.up_idx][~same] != blk[down][~same]) | (blk[down][~same] < 0))
    assert np.all(lag[c.up_idx][~same] < lag[down][~same])
    return blk, width


def stage(plan, c, nsteps, qts, q0="case", start=0, lastobs=None, reservoirs=True):
    """tables and forcing of a window in the order compute_network_structured sets them"""
    if reservoirs:
        plan.set_reservoirs(c.lakes, c.par, DT)
    nq = -(-nsteps // qts)
    c0 = start // qts
    plan.upload_forcing(nsteps, np.ascontiguousarray(c.ql[:, c0:c0 + nq]), c.q0 if isinstance(q0, str) else q0)
    mode, a, w, lt_fin, lv_fin = nudging_tables(c, nsteps, start, lastobs)
    plan.set_nudging(nsteps, c.gages, mode, a, w)
    return lt_fin, lv_fin


def check_window(plan, c, want, res, da, t0=0):
    """everything a window leaves against the oracle's steps (t0, t0 + nsteps]: the full result, the lakes' inflows, the nudges,
    the final state; the lakes' velocity slot and final pool elevations"""
    nsteps = plan._nsteps
    w = np.ascontiguousarray(want[:, t0 + 1:t0 + nsteps + 1])
    fvd = plan.download_fvd()
    bad = np.flatnonzero((bits(fvd) != bits(w)).any(axis=(1, 2)))
    names = {int(r): k for k, r in list(zip(c.lake_names, c.lakes)) + list(zip(c.gage_names, c.gages))}
    assert bad.size == 0, (bad.size, [(int(r), names.get(int(r)), int(c.lag[r])) for r in bad[:12]])
    assert np.array_equal(bits(plan.download_reservoir_inflow()), bits(res["inflow"][:, t0 + 1:t0 + nsteps + 1]))
    assert np.array_equal(bits(plan.download_nudge()), bits(da["nudge"][:, t0 + 1:t0 + nsteps + 1]))
    assert np.array_equal(bits(plan.download_final_state()), bits(np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], 1)))
    assert not fvd[c.lakes, :, 1].any()
    if t0 + nsteps + 1 == want.shape[1]:
        assert np.array_equal(bits(fvd[c.lakes, -1, 2]), bits(res["water_elevation"]))
    return fvd


def tiles_only(stats, c, nsteps):
    assert stats["wide_segment_steps"] == c.n * nsteps and stats["wide_levels"] == c.W and stats["wide_k"] == K, stats


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["placement-24", "placement-128", "slices"])
@pytest.mark.parametrize("qts", [4, 11])
def test_gpu_lakes_and_gages_where_cluster_rows_hand_flows_on(key, qts):
    """k_mc_ctile's reservoir branch and nudging epilogue (and, for "slices", k_mc_tile's under the cluster order's lags) at every
    placement of find_placements; the forcing column changes inside tiles"""
    c = case(key)
    want, res, da = reference(key, NSTEPS, qts)
    with open_plan(key) as plan:
        check_order(plan, key)
        lt_fin, lv_fin = stage(plan, c, NSTEPS, qts)
        tiles_only(plan.route_device(NSTEPS, qts, True), c, NSTEPS)
        check_window(plan, c, want, res, da)
    assert np.array_equal(bits(lt_fin), bits(da["lastobs_time"])) and np.array_equal(bits(lv_fin), bits(da["lastobs_val"]))


@pytest.mark.gpu
def test_gpu_lakes_and_gages_in_clusters_that_are_not_their_blocks_first():
    """the forest of test_gpu_ctile_block.test_many_clusters_per_block: lakes and gages whose LDS slot lies beyond the first 128
    of their block"""
    assert CB.block_width() == FOREST_WIDTH
    c = case("forest")
    want, res, da = reference("forest", NSTEPS, 4)
    with open_plan("forest") as plan:
        blk, width = check_order(plan, "forest")
        _, pos = plan.levels()
        first = np.full(blk.max() + 1, c.n, np.int64)
        np.minimum.at(first, blk, pos)
        slot = pos - first[blk]
        assert slot.max() < width and np.count_nonzero(slot[c.lakes] >= 128) >= 2 and np.count_nonzero(slot[c.gages] >= 128) >= 4
        assert np.count_nonzero(slot[c.lakes] < 128) >= 1
        stage(plan, c, NSTEPS, 4)
        tiles_only(plan.route_device(NSTEPS, 4, True), c, NSTEPS)
        check_window(plan, c, want, res, da)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["placement-24", "slices"])
def test_gpu_decimated_windows_with_tables(key):
    """set_output_stride: the DEC instances of the tile kernels with reservoir and gage rows.  The block written aside is the
    oracle's result sliced, the asynchronous fetch hands it over, and the full result, the tables and the state are those of a
    window that does not decimate"""
    c = case(key)
    rows = np.concatenate([c.lakes[:2], c.gages[:2]])
    with open_plan(key) as plan:
        check_order(plan, key)
        rs = plan.rowset(rows)
        for stride, qts in ((4, 4), (11, 11), (11, 4)):
            want, res, da = reference(key, NSTEPS, qts)
            plan.set_output_stride(stride)
            stage(plan, c, NSTEPS, qts)
            tiles_only(plan.route_device(NSTEPS, qts, True), c, NSTEPS)
            dec = np.ascontiguousarray(want[:, 1:][:, stride - 1::stride][:, :NSTEPS // stride])
            assert dec.shape[1] == NSTEPS // stride
            plan.fetch_begin(rs, True, stride)
            hyd, state, block = plan.fetch_wait()
            assert np.array_equal(bits(block), bits(dec)), stride
            assert np.array_equal(bits(hyd), bits(want[rows, 1:, 0]))
            assert np.array_equal(bits(state), bits(plan.download_final_state()))
            assert np.array_equal(bits(plan.download_fvd(stride)), bits(dec))
            check_window(plan, c, want, res, da)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["placement-24", "slices"])
def test_gpu_window_in_parts_and_a_second_window_from_the_resident_state(key):
    """route_begin / route_advance to steps that are no tile boundaries / route_end == one call; then a second window from the
    state the first left on the device, its nudging tables resolved from the first's final lastobs with the times counted
    from the new start: together the oracle's one window of twice the length"""
    c = case(key)
    qts = 4
    want, res, da = reference(key, 2 * NSTEPS, qts)
    with open_plan(key) as plan:
        check_order(plan, key)
        lt1, lv1 = stage(plan, c, NSTEPS, qts)
        plan.route_begin(NSTEPS, qts, True)
        for t_end in (13, 13, 30, NSTEPS - 1, NSTEPS):
            plan.route_advance(t_end)
        tiles_only(plan.route_end(), c, NSTEPS)
        check_window(plan, c, want, res, da, 0)
        w1 = reference(key, NSTEPS, qts)
        assert np.array_equal(bits(lt1), bits(w1[2]["lastobs_time"])) and np.array_equal(bits(lv1), bits(w1[2]["lastobs_val"]))
        shifted = (lt1 - np.float32(NSTEPS * DT)).astype(np.float32)
        lt2, lv2 = stage(plan, c, NSTEPS, qts, q0=None, start=NSTEPS, lastobs=(lv1, shifted), reservoirs=False)
        tiles_only(plan.route_device(NSTEPS, qts, True), c, NSTEPS)
        check_window(plan, c, want, res, da, NSTEPS)
    assert np.array_equal(lt2 + np.float32(NSTEPS * DT), da["lastobs_time"], equal_nan=True)
    assert np.array_equal(bits(lv2), bits(da["lastobs_val"]))


@pytest.mark.gpu
def test_gpu_cost_ordered_threads_with_tables():
    """a plan created with the cost hint of a routed window packs its clusters by cost, and from the second tile on the class
    partition deals a block's rows to other threads than their positions': the same bits, twice"""
    key, qts = "placement-128", 4
    c = case(key)
    want, res, da = reference(key, NSTEPS, qts)
    with open_plan(key) as plan:
        stage(plan, c, NSTEPS, qts)
        plan.route_device(NSTEPS, qts, True)
        hint = plan.download_iterations()
    assert np.unique(hint).shape[0] >= 3
    with open_plan(key, cost_hint=hint) as plan:
        lag, W, C = plan.lags()
        assert np.array_equal(lag, c.lag)                      # (the hint moves clusters between blocks, not rows between lags)
        for _ in range(2):
            stage(plan, c, NSTEPS, qts)
            tiles_only(plan.route_device(NSTEPS, qts, True), c, NSTEPS)
            check_window(plan, c, want, res, da)
            assert np.array_equal(plan.download_iterations(), hint)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["placement-24", "slices"])
def test_gpu_reservoir_da_tables_that_change_nothing(key):
    """k_mc_ctile_rda / k_mc_tile_rda on a cluster plan, DEC off and on.  There is no synthetic reference of the reservoir data
    assimilation (the recorded LowerColorado loop of test_reservoir_da_network is), so the tables here are ones that provably
    leave the level pool alone: kind 0, and RFC lakes of type 4 whose use_forecast is 0 (reservoir_RFC_da then returns the
    level pool's outflow and elevation).  With every kind 0 the library keeps the plain instances (trmc_set_reservoir_da: no
    table, nothing to download); with one RFC lake it launches the _rda instances for the whole window."""
    c = case(key)
    qts = 4
    want, res, da = reference(key, NSTEPS, qts)
    nres = c.lakes.shape[0]
    kind = np.zeros(nres, np.int32)
    with open_plan(key) as plan:
        rs = plan.rowset(c.lakes[:3])
        for stride in (0, 4):
            plan.set_output_stride(stride)
            plan.set_reservoirs(c.lakes, c.par, DT)
            plan.set_reservoir_da(kind, np.zeros(nres, np.int32))
            stage(plan, c, NSTEPS, qts, reservoirs=False)
            tiles_only(plan.route_device(NSTEPS, qts, True), c, NSTEPS)
            check_window(plan, c, want, res, da)
            with pytest.raises(RuntimeError, match="no reservoir data-assimilation tables"):
                plan.download_reservoir_da()
        rfc = np.arange(nres) % 2 == 0
        kind[rfc] = 4
        trow = np.where(rfc, np.cumsum(rfc) - 1, 0).astype(np.int32)
        n4 = int(rfc.sum())
        series = np.full((n4, 6), 1.0e3, np.float32)            # (never read: use_forecast = 0)
        update_time = np.arange(n4, dtype=np.float32) * np.float32(3600.0)
        ipar = np.tile(np.array([1, 6, 0, 3600, 10], np.int32), (n4, 1))       # timeseries_idx, total, use_forecast, da_dt, days
        for stride in (0, 4):
            plan.set_output_stride(stride)
            plan.set_reservoirs(c.lakes, c.par, DT)
            plan.set_reservoir_da(kind, trow, rfc=(series, update_time, ipar))
            stage(plan, c, NSTEPS, qts, reservoirs=False)
            tiles_only(plan.route_device(NSTEPS, qts, True), c, NSTEPS)
            fvd = check_window(plan, c, want, res, da)
            state, idx = plan.download_reservoir_da()           # (only a window routed by the _rda instances has one)
            assert np.array_equal(state[rfc, 0], update_time) and np.all(idx[rfc] == 1) and not state[~rfc].any()
            if stride:
                plan.fetch_begin(rs, True, stride)
                _, _, block = plan.fetch_wait()
                assert np.array_equal(bits(block), bits(fvd[:, stride - 1::stride][:, :NSTEPS // stride]))
