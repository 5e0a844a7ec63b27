"""Shared test helpers: golden fixture loading and reference-shaped inputs."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA_COLS = ["dt", "bw", "tw", "twcc", "dx", "n", "ncc", "cs", "s0", "alt"]  # compute.py:1447-1450


def load_kernel_vectors():
    return np.load(os.path.join(GOLDEN, "kernel_vectors.npz"))


def load_toy():
    return json.load(open(os.path.join(GOLDEN, "toy_network.json")))


class LowerColorado:
    """LowerColorado_TX MC-only inputs in the exact form compute_nhd_routing_v02 hands them to the
    kernel callable (compute.py:1447-1467, :1513-1576)."""

    def __init__(self):
        d = np.load(os.path.join(GOLDEN, "lowercolorado_domain.npz"))
        self.ids = d["ids"]
        self.to = d["to"]
        self.qlat = d["qlat"]
        par = dict(zip(d["param_cols"].tolist(), d["params"].T))
        self.nseg = self.ids.shape[0]
        self.dt = 300.0
        cols = {**par, "dt": np.full(self.nseg, self.dt, np.float32), "alt": np.zeros(self.nseg, np.float32)}
        self.data_cols = np.array(DATA_COLS, dtype=object)
        self.data_values = np.stack([cols[c] for c in DATA_COLS], 1).astype(np.float32)
        self.params9 = np.stack([cols[c] for c in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")], 1).astype(np.float32)
        rp, ri = d["ref_reach_ptr"], d["ref_reach_ids"]
        self.reaches = [ri[rp[i]:rp[i + 1]].tolist() for i in range(rp.shape[0] - 1)]
        up, ui = d["ref_rconn_ptr"], d["ref_rconn_ids"]
        self.rconn = {int(s): ui[up[i]:up[i + 1]].tolist() for i, s in enumerate(self.ids)}
        self.tailwaters = d["ref_tailwaters"].tolist()
        self.q0 = np.zeros((self.nseg, 3), np.float32)
        self.nts, self.qts = 288, 12

    def row_lists(self):
        row = {int(s): i for i, s in enumerate(self.ids)}
        reaches = [np.array([row[s] for s in r], dtype=np.int64) for r in self.reaches]
        ups = [np.array([row[s] for s in self.rconn.get(r[0], [])], dtype=np.int64) for r in self.reaches]
        return reaches, ups

    def csr(self):
        """upstream rows per row (reference summation order) as CSR arrays for RoutingPlan"""
        from troute_amd.plan import csr_from_lists
        row = {int(s): i for i, s in enumerate(self.ids)}
        return csr_from_lists([[row[u] for u in self.rconn.get(int(s), [])] for s in self.ids])

    def golden(self):
        return np.load(os.path.join(GOLDEN, "lowercolorado_golden.npz"))


def random_network(rng, nseg, max_chain=6, p_junction=0.45, p_triple=0.1):
    """Random dendritic forest as (to[nseg]) with ids 0..nseg-1 in random order: returns
    reaches (lists of rows, reference contract order), upstream lists per reach head, to-array."""
    to = np.full(nseg, -1, dtype=np.int64)
    # build by attaching each new node (in creation order) downstream-first: node i>0 flows into a
    # random earlier node with few upstreams, or starts a new network
    nup = np.zeros(nseg, dtype=np.int64)
    for i in range(1, nseg):
        if rng.random() < 0.02:
            continue                      # new independent network outlet
        for _ in range(8):
            j = int(rng.integers(max(0, i - 50), i))
            cap = 3 if rng.random() < p_triple else (2 if rng.random() < p_junction else 1)
            if nup[j] < cap:
                to[i] = j
                nup[j] += 1
                break
    perm = rng.permutation(nseg)          # shuffle labels so row order is unrelated to topology
    inv = np.empty(nseg, dtype=np.int64)
    inv[perm] = np.arange(nseg)
    to2 = np.full(nseg, -1, dtype=np.int64)
    for i in range(nseg):
        to2[perm[i]] = perm[to[i]] if to[i] >= 0 else -1
    return to2


def reaches_from_to(to):
    """Reference-contract decomposition of a forest given as to[row] (-1 = outlet): reaches are maximal
    chains broken where the downstream row has != 1 upstream; listed so upstream reaches come first."""
    nseg = to.shape[0]
    ups = [[] for _ in range(nseg)]
    for i in range(nseg):
        if to[i] >= 0:
            ups[to[i]].append(i)
    reaches, heads_up = [], []
    done = np.zeros(nseg, dtype=bool)
    # iterative post-order from each outlet
    for o in np.flatnonzero(to < 0).tolist():
        stack = [(o, False)]
        while stack:
            node, expanded = stack.pop()
            # node is the LAST (most downstream) segment of a reach; walk up while single upstream
            chain = [node]
            while len(ups[chain[-1]]) == 1:
                chain.append(ups[chain[-1]][0])
            head = chain[-1]
            if not expanded:
                stack.append((node, True))
                for u in ups[head]:
                    stack.append((u, False))
            else:
                reaches.append(chain[::-1])
                heads_up.append(list(ups[head]))
                done[chain] = True
    assert done.all()
    return reaches, heads_up, ups


# (short, engine) of the LowerColorado table tests: set_engine below
TABLE_ENGINES = [(True, None), (False, None), (True, "levels"), (True, "levels-wide"), (True, "levels-mid"), (True, "levels-clusters"),
                 (True, "levels-slices+clusters")]


def set_engine(engine, monkeypatch):
    """The engine parametrisation of the LowerColorado table tests (test_reservoirs, test_nudging, test_reservoir_da_network):
    None = the default (the dataflow kernels at this size); "levels" = k_mc_step; "levels-wide" = the level engine with its wide
    levels several steps per launch under a level skew (k_mc_tile); "levels-mid" = the same with a second tier below the wide
    levels, fewer steps per launch under its own skew (k_mc_tile twice, then k_mc_step); "levels-clusters" = a plan in cluster
    order without slices: every row a cluster row of k_mc_ctile, clusters of 24 rows, 7 steps per launch (288 = 41 x 7 + 1: the
    last tile is short); "levels-slices+clusters" = the same below leading levels of at least 32 rows, which k_mc_tile routes
    as slices with the cluster order's lags for levels.  Returns True for the engines in cluster order: their windows report
    every routed row as routed in tiles (cluster_stats)."""
    if not engine:
        return False
    monkeypatch.setenv("TRMC_ENGINE", "levels")
    monkeypatch.setenv("TRMC_PLAN_CACHE", "0")
    monkeypatch.setenv("TRMC_WIDE_K", "7")
    if engine in ("levels-clusters", "levels-slices+clusters"):
        monkeypatch.setenv("TRMC_CLUSTER_ROWS", "24")
        monkeypatch.setenv("TRMC_WIDE_MIN_ROWS", "0" if engine == "levels-clusters" else "32")
        return True
    assert engine in ("levels", "levels-wide", "levels-mid"), engine
    monkeypatch.setenv("TRMC_WIDE_MIN_ROWS", "0" if engine == "levels" else ("64" if engine.endswith("mid") else "32"))
    monkeypatch.setenv("TRMC_MID_MIN_ROWS", "8" if engine.endswith("mid") else "0")
    monkeypatch.setenv("TRMC_MID_K", "3")
    return False


def cluster_stats(stats, engine, nts):
    """A window on a plan in cluster order: no row took a one-step launch -- the window's stats count every routed row's
    every step as routed in tiles, which the library reports only when the cluster tiles ran (csrc/host_levels.inc,
    route_end_t) -- and the slices exist exactly where the engine asks for them."""
    assert stats["wide_segment_steps"] == stats["nseg_routed"] * nts, stats
    assert (stats["wide_levels"] > 0) == (engine == "levels-slices+clusters"), stats


def flow_engine(precision=32):
    """True when plans of this precision run on the dataflow engine (k_mc_flow), False on the level engine."""
    import os
    return precision == 32 and os.environ.get("TRMC_ENGINE", "flow") != "levels"


def reference_day_by_day(to, params, days, q0, nsteps, qts, checksums=False):
    """The reference's run-set loop on the CPU, one window per day (oracle.reference_windows, its decomposition into ordered
    sub-networks formed once): yields per day (q [nseg, nsteps + 1], the next day's q0 [nseg, 3], (chk_v, chk_d) or None) --
    q column 0 is the day's initial flow, the state is new_q0 (q_T, q_T, depth_T)."""
    from oracle import oracle as O
    from troute_amd.synthetic import upstream_csr
    ref_name = "libmc_ref_qj0_f32.so" if O.have_ref("libmc_ref_qj0_f32.so") else None
    order_ptr, job_ptr, rows = O.ordered_subnetworks(to, 10000)
    up_ptr, up_idx = upstream_csr(to)
    state = np.ascontiguousarray(q0, dtype=np.float32)
    for ql in days:
        q, d, _, _ = O.cpu_baseline_route(nsteps, qts, True, order_ptr, job_ptr, rows, up_ptr, up_idx, params, ql, state,
                                          ref_name=ref_name, checksums=checksums)
        state = np.ascontiguousarray(np.stack([q[:, -1], q[:, -1], d], axis=1))
        chk = (O.cpu_baseline_route.chk_v.copy(), O.cpu_baseline_route.chk_d.copy()) if checksums else None
        yield q, state, chk


def stream_days(r, make_day, nsteps, qts, q0, extra=2, pinned=True, ndays=None, min_days=0, **kw):
    """Route days make_day(0), make_day(1), ... through one RouteStream until the ring of day slots has wrapped (slots + extra
    days; or `ndays` days).  Returns (outlet rows, {day: (hyd, final[, fvd]) copies}, the days routed, stream_info at the start)."""
    from troute_amd.sequence import RouteStream, pinned_like
    got, days, start = {}, [], {}
    with RouteStream(r, nsteps, qts, **kw) as rs:
        def feed():
            k = 0
            while k == 0 or k < (ndays or max(min_days, rs.info["slots"] + extra)):
                if k == 1:
                    start.update(rs.info)
                d = make_day(k)
                days.append(d)
                yield pinned_like(d) if pinned else d
                k += 1
        for item in rs.route(feed(), q0):
            got[item[0]] = tuple(None if x is None else np.array(x, copy=True) for x in item[1:])
        rows = np.array(rs.outlet_rows, copy=True)
    assert sorted(got) == list(range(len(days))) and (ndays or len(days) >= start["slots"] + extra)
    return rows, got, days, start
