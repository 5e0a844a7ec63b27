"""THE LEVEL POOL IN EVERY REGIME (csrc/levelpool.hpp; oracle/mc_oracle_impl.inc lp_discharge): the cases, a classifying
restatement and the census that the level-pool tests share.  No GPU, no reference tree.

  sweep_cases()     a deterministic sweep of single pools: parameter row (oracle.LP_PAR order), routing period, starting
                    elevation, inflow series -- areas from 0 to 1 km2, elevation triples with we == oe, we == maxh, we < oe
                    and a pool 600 m up (one ulp there is 6e-5 m), coefficient sets with every coefficient distinct and with
                    weir_length, orifice_area or dam_length zero, starts on every edge and one ulp either side, in every
                    interior, overtopping, and cold starts formed as mc_reach.py forms them (ifd 0, 0.5, 0.9, 1)
  classify()        one routing period in numpy float32, elementwise over arrays of pools: which of the five outcomes each
                    of the four discharge evaluations took, with the new outflow and elevation.  It earns trust by
                    equality with oracle.levelpool on every step of the sweep (tests/test_levelpool_sweep.py)
  census()          counts per stage x branch, per start -> end crossing and per tag over a set of classified steps
  network_case()    68 independent basins  headwater(s) -> lake A -> channel -> lake B -> outlet channel  whose lakes take
                    their parameters and starts from the same classes; what tests/test_gpu_levelpool_sweep.py routes on
                    the device.  Every value the oracle computes for it is finite: the classes that produce NaN stay in
                    the sweep
"""
import ctypes as C
import functools
import hashlib

import numpy as np

from oracle import oracle as O

F = np.float32
BRANCHES = ("dead", "orifice", "weir", "overtop", "overtop_clipped")
DEAD, ORIFICE, WEIR, OVERTOP, OVERTOP_CLIPPED = range(5)
STAGES = ("stage1", "stage2", "stage3", "final")
# a step's start and end lie in one of four branches (an overtopping pool is one branch whether its weir depth is clipped or not)
CROSS = ("dead", "orifice", "weir", "overtop")
CROSSINGS = tuple((a, b) for a in CROSS for b in CROSS if a != b)
EDGES = ("orifice_elevation", "weir_elevation", "max_depth")
TAGS = (("area=0", "weir_length=0", "orifice_area=0", "dam_length=0")
        + tuple(f"H=={e}{s}" for e in EDGES for s in ("-1ulp", "", "+1ulp"))
        + ("overtop->below_crest", "stage2or3!=stage1", "sqrt(negative)_discarded", "pow(negative)_discarded"))
_P = {k: i for i, k in enumerate(O.LP_PAR)}


def f32(x):
    return np.asarray(x, dtype=np.float32)


def cold_start(par, ifd):
    """init_levelpool_reach as mc_reach.py:526-530 restates it: oe + (maxh - oe) * ifd, every operation in float32"""
    par = f32(par)
    oe, maxh = par[..., _P["orifice_elevation"]], par[..., _P["max_depth"]]
    return f32(oe + f32(f32(maxh - oe) * f32(ifd)))


# ---- the classifying restatement -------------------------------------------------------------------------------------------
def _pow15(x):
    return O.det_powf(np.ascontiguousarray(x, dtype=np.float32), F(3.) / F(2.)).reshape(np.shape(x))


def _discharge(h_eval, h_top, mwd, p):
    """lp_discharge: (discharge, branch, the orifice's sqrt took a negative, the weir's power took a negative)"""
    oe, we, maxh = p["orifice_elevation"], p["weir_elevation"], p["max_depth"]
    dh = h_eval - we
    clipped = dh > mwd
    dh = np.where(clipped, mwd, dh)
    head = h_eval - oe
    orifice = p["orifice_coefficient"] * p["orifice_area"] * np.sqrt(F(2.) * F(9.81) * head)
    weir = p["weir_coefficient"] * p["weir_length"] * _pow15(dh)
    over = orifice + weir + (p["weir_coefficient"] * (p["weir_length"] * p["dam_length"]) * _pow15(h_top - maxh))
    top = h_top > maxh
    q = np.where(top, over, np.where(dh > F(0), orifice + weir, np.where(h_eval > oe, orifice, F(0))))
    branch = np.where(top, np.where(clipped, OVERTOP_CLIPPED, OVERTOP),
                      np.where(dh > F(0), WEIR, np.where(h_eval > oe, ORIFICE, DEAD))).astype(np.int8)
    return f32(q), branch, (head < F(0)) & ~top, (dh < F(0)) & ~top


def classify(par, dt, H, inflow, lateral=0.0):
    """One routing period of the level pool, elementwise over pools: par [..., 9] (oracle.LP_PAR order), dt, H, inflow [...]
    (float32).  Returns a dict: branch [4, ...] int8 (index into BRANCHES, one per discharge evaluation in STAGES order),
    outflow and elevation [...] float32, and the two discarded-NaN masks [4, ...]."""
    par = f32(par)
    p = {k: par[..., i] for k, i in _P.items()}
    dt, h, qi0, lat = f32(dt), f32(H), f32(inflow), f32(lateral)
    with np.errstate(all="ignore"):
        qi1 = qi0
        it_0 = qi0
        it_1 = qi0 + ((qi1 + lat - qi0) * F(0.33))
        it_2 = qi0 + ((qi1 + lat - qi0) * F(0.67))
        mwd = p["max_depth"] - p["weir_elevation"]
        sap = p["area"] * F(1.0E6)
        wet = sap > F(0)
        br, neg_sqrt, neg_pow = [None] * 4, [None] * 4, [None] * 4
        q, br[0], neg_sqrt[0], neg_pow[0] = _discharge(h, h, mwd, p)
        dh1 = np.where(wet, ((it_0 - q) / sap) * dt, F(0))
        q, br[1], neg_sqrt[1], neg_pow[1] = _discharge(h + dh1 / F(3), h, mwd, p)
        dh2 = np.where(wet, ((it_1 - q) / sap) * dt, F(0))
        q, br[2], neg_sqrt[2], neg_pow[2] = _discharge(h + (F(0.667) * dh2), h, mwd, p)
        dh3 = np.where(wet, ((it_2 - q) / sap) * dt, F(0))
        h_new = f32(h + ((dh1 / F(4.)) + (F(0.75) * dh3)))
        q, br[3], neg_sqrt[3], neg_pow[3] = _discharge(h_new, h_new, mwd, p)
    return {"branch": np.stack(br), "outflow": f32(q), "elevation": h_new, "neg_sqrt": np.stack(neg_sqrt),
            "neg_pow": np.stack(neg_pow)}


def classify_series(par, dt, h0, inflows):
    """classify() over a series: par [n, 9], dt [n], h0 [n], inflows [n, T] -> dict of arrays with a step axis:
    start [n, T] (the elevation each step starts from), branch [n, T, 4], outflow / elevation [n, T], the masks [n, T, 4]"""
    par, dt, h, inflows = f32(par), f32(dt), f32(h0), f32(inflows)
    out = {k: [] for k in ("start", "branch", "outflow", "elevation", "neg_sqrt", "neg_pow")}
    for t in range(inflows.shape[1]):
        c = classify(par, dt, h, inflows[:, t])
        out["start"].append(h)
        for k in ("outflow", "elevation"):
            out[k].append(c[k])
        for k in ("branch", "neg_sqrt", "neg_pow"):
            out[k].append(np.moveaxis(c[k], 0, -1))
        h = c["elevation"]
    return {k: np.stack(v, axis=1) for k, v in out.items()}


def census(par, series):
    """Counts over the steps of classify_series() (par [n, 9]) that start from a finite elevation:
    {"cells": {(stage, branch): evaluations}, "crossings": {(from, to): steps}, "tags": {tag: steps}, "steps": n}.
    A crossing and the overtop->below_crest tag also need a finite end: a NaN elevation compares false with everything and
    would pass for a dead pool."""
    par = f32(par)
    start, end, br = series["start"], series["elevation"], series["branch"]
    ok = np.isfinite(start)
    both = ok & np.isfinite(end)
    cells = {(s, b): int(np.count_nonzero(ok & (br[..., i] == j))) for i, s in enumerate(STAGES) for j, b in enumerate(BRANCHES)}
    merged = np.minimum(br, OVERTOP)                                    # overtop_clipped -> overtop
    crossings = {(a, b): int(np.count_nonzero(both & (merged[..., 0] == CROSS.index(a)) & (merged[..., 3] == CROSS.index(b))))
                 for a, b in CROSSINGS}
    col = lambda k: par[:, _P[k]][:, None]                              # noqa: E731
    tags = {"area=0": ok & (col("area") == 0), "weir_length=0": ok & (col("weir_length") == 0),
            "orifice_area=0": ok & (col("orifice_area") == 0), "dam_length=0": ok & (col("dam_length") == 0)}
    for e in EDGES:
        edge = np.broadcast_to(col(e), start.shape)
        tags[f"H=={e}-1ulp"] = ok & (start == np.nextafter(edge, F(-np.inf)))
        tags[f"H=={e}"] = ok & (start == edge)
        tags[f"H=={e}+1ulp"] = ok & (start == np.nextafter(edge, F(np.inf)))
    tags["overtop->below_crest"] = both & (merged[..., 0] == OVERTOP) & (end <= col("max_depth"))
    tags["stage2or3!=stage1"] = ok & ((br[..., 1] != br[..., 0]) | (br[..., 2] != br[..., 0]))
    tags["sqrt(negative)_discarded"] = ok & series["neg_sqrt"].any(axis=-1)
    tags["pow(negative)_discarded"] = ok & series["neg_pow"].any(axis=-1)
    return {"cells": cells, "crossings": crossings, "tags": {k: int(np.count_nonzero(tags[k])) for k in TAGS},
            "steps": int(np.count_nonzero(ok))}


def census_table(c):
    """the census as text: the table the fixture maker prints"""
    lines = [f"{c['steps']} steps from a finite elevation", "evaluations   " + "".join(f"{b:>17s}" for b in BRANCHES)]
    lines += [f"  {s:12s}" + "".join(f"{c['cells'][s, b]:17d}" for b in BRANCHES) for s in STAGES]
    lines.append("start -> end  " + "".join(f"{b:>17s}" for b in CROSS))
    lines += [f"  {a:12s}" + "".join(f"{c['crossings'].get((a, b), 0) if a != b else '.':>17}" for b in CROSS) for a in CROSS]
    lines += [f"  {k:28s}{v:8d}" for k, v in c["tags"].items()]
    return "\n".join(lines)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
SWEEP_STEPS = 12
PERIODS = (300.0, 60.0, 3600.0)
AREAS = (0.0, 1.0e-3, 0.05, 1.0)                                        # km2
#          orifice_elevation, weir_elevation, max_depth
TRIPLES = {"plain": (1.0, 3.0, 4.0), "we==oe": (2.0, 2.0, 4.0), "we==maxh": (1.0, 4.0, 4.0), "we<oe": (3.0, 2.0, 4.0),
           "600m": (600.5, 603.25, 605.0)}
#          orifice_area, orifice_coefficient, weir_coefficient, weir_length, dam_length
COEFFICIENTS = {"lowercolorado": (1.0, 0.1, 0.4, 10.0, 10.0), "distinct": (2.5, 0.6, 1.7, 35.0, 120.0),
                "weir_length=0": (1.5, 0.3, 0.9, 0.0, 50.0), "orifice_area=0": (0.0, 0.3, 0.9, 20.0, 50.0),
                "dam_length=0": (1.5, 0.3, 0.9, 20.0, 0.0)}
IFD = (0.0, 0.5, 0.9, 1.0)
INFLOWS = ("zero", "small", "flood", "intermittent")


def par_row(area, triple, coefficients):
    oe, we, maxh = triple
    oa, oc, wc, wl, dl = coefficients
    return np.array([area, maxh, oa, oc, oe, wc, we, wl, dl], np.float32)


def starts_of(par):
    """[(name, elevation)]: every edge and its neighbours one ulp away, every interior, two overtopping, four cold starts"""
    oe, we, maxh = (F(par[_P[k]]) for k in EDGES)
    out = []
    for name, e in zip(EDGES, (oe, we, maxh)):
        out += [(f"{name}-1ulp", np.nextafter(e, F(-np.inf))), (name, e), (f"{name}+1ulp", np.nextafter(e, F(np.inf)))]
    out += [("below_orifice", F(oe - F(0.5))), ("orifice..weir", F((oe + we) * F(0.5))), ("weir..crest", F((we + maxh) * F(0.5))),
            ("overtop_5cm", F(maxh + F(0.05))), ("overtop_1m", F(maxh + F(1.0)))]
    out += [(f"ifd={ifd}", F(cold_start(par, ifd))) for ifd in IFD]
    return out


def inflow_series(kind, area, dt, rng):
    """SWEEP_STEPS inflows (m3/s).  The scale moves the pool by about a metre per step of a flood whatever its area and
    period (a pool of area 0 takes the smallest area's), so the steps cross the branches instead of staying in one."""
    scale = F(max(area, 1.0e-3) * 1.0e6 / dt)                           # m3/s that lift the pool 1 m in one period
    t = np.arange(SWEEP_STEPS)
    if kind == "zero":
        return np.zeros(SWEEP_STEPS, np.float32)
    if kind == "small":
        return f32(np.full(SWEEP_STEPS, 0.01) * scale)
    if kind == "flood":
        return f32(rng.uniform(0.5, 2.5, SWEEP_STEPS) * scale)
    return f32(np.where(t % 3 == 0, rng.uniform(1.0, 6.0, SWEEP_STEPS), 0.0) * scale)


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """[(name, par [9], dt, h0, inflows [SWEEP_STEPS])], float32.  The routing period and the inflow kind rotate over the
    other factors instead of multiplying them: every area, triple, coefficient set and start meets every period and every
    inflow kind, and the recording stays small."""
    cases = []
    for ia, area in enumerate(AREAS):
        for it, (tn, triple) in enumerate(TRIPLES.items()):
            for ic, (cn, coef) in enumerate(COEFFICIENTS.items()):
                par = par_row(area, triple, coef)
                for js, (sn, h0) in enumerate(starts_of(par)):
                    for k in range(2):
                        ii = (2 * (ia + it + ic + js) + k + (js // 2)) % 4
                        dt = PERIODS[(ia + 2 * it + ic + js + k) % 3]
                        rng = np.random.default_rng([11, ia, it, ic, js, k])
                        name = f"area={area:g}/{tn}/{cn}/{sn}/{INFLOWS[ii]}/dt={dt:g}"
                        cases.append((name, par, F(dt), F(h0), inflow_series(INFLOWS[ii], area, dt, rng)))
    return cases


def sweep_arrays():
    """the sweep as arrays: par [n, 9], dt [n], h0 [n], inflows [n, SWEEP_STEPS]"""
    cases = sweep_cases()
    return (np.stack([c[1] for c in cases]), f32([c[2] for c in cases]), f32([c[3] for c in cases]),
            np.stack([c[4] for c in cases]))


def input_hashes():
    """[n, 32] uint8: SHA-256 of each case's inputs (the bits of par, dt, h0, inflows)"""
    return np.array([np.frombuffer(hashlib.sha256(b"".join(f32(x).tobytes() for x in c[1:])).digest(), np.uint8)
                     for c in sweep_cases()])


def same(got, want):
    """the same bits where `want` is finite or infinite, a NaN where it holds a NaN (position for position)"""
    got, want = f32(got), f32(want)
    nan = np.isnan(want)
    return bool(np.array_equal(nan, np.isnan(got)) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


def oracle_sweep():
    """oracle.levelpool over the sweep: (outflow, elevation) [n, SWEEP_STEPS]"""
    cases = sweep_cases()
    q, h = np.empty((len(cases), SWEEP_STEPS), np.float32), np.empty((len(cases), SWEEP_STEPS), np.float32)
    for k, (_, par, dt, h0, inflows) in enumerate(cases):
        Hm = h0
        for i, inflow in enumerate(inflows):
            q[k, i], Hm = O.levelpool(inflow, dt, Hm, par)
            h[k, i] = Hm
    return q, h


def reference_sweep(lp):
    """the reference Fortran level pool (oracle/_ref/liblp_ref.so, opened by the caller as `lp`) over the sweep, every case
    on a fresh handle: (outflow, elevation) [n, SWEEP_STEPS]"""
    lp.get_lp_handle.restype = C.c_void_p
    f = C.c_float
    cases = sweep_cases()
    q, h = np.empty((len(cases), SWEEP_STEPS), np.float32), np.empty((len(cases), SWEEP_STEPS), np.float32)
    for k, (_, par, dt, h0, inflows) in enumerate(cases):
        hv = C.c_void_p(lp.get_lp_handle())
        p = {name: f(float(par[i])) for name, i in _P.items()}
        lp.init_lp(hv, C.byref(f(float(h0))), *[C.byref(p[name]) for name in (
            "area", "weir_elevation", "weir_coefficient", "weir_length", "dam_length", "orifice_elevation",
            "orifice_coefficient", "orifice_area", "max_depth")], C.byref(C.c_int(k + 1)), C.byref(C.c_int(1)))
        Hr = f(float(h0))
        for i, inflow in enumerate(inflows):
            out = f(0)
            lp.run_lp(hv, C.byref(f(float(inflow))), C.byref(f(0.0)), C.byref(Hr), C.byref(out), C.byref(f(float(dt))))
            q[k, i], h[k, i] = out.value, Hr.value
        lp.free_lp(hv)
    return q, h


# ---- the network case of the device tests --------------------------------------------------------------------------------------
NET_STEPS, NET_QTS, NET_DT = 48, 2, 300.0
NET_TRIPLES = ((1.0, 3.0, 4.0), (2.0, 2.0, 4.0), (2.75, 3.0, 4.0), (1.0, 4.0, 4.0), (600.5, 603.25, 605.0))
#               orifice_area, orifice_coefficient, weir_coefficient, weir_length; the drop-in fixes dam_length at 10 (mc_reach.py)
NET_COEFFICIENTS = ((1.0, 0.1, 0.4, 10.0), (2.5, 0.6, 1.7, 35.0), (1.5, 0.3, 0.9, 0.0), (0.0, 0.3, 0.9, 20.0), (0.3, 0.6, 0.4, 3.0))
NET_AREAS = (0.0, 2.0e-4, 5.0e-4, 1.0e-3, 2.0e-3, 5.0e-3)                # km2: pools that cross a branch in a step or two


def _candidate_lake(rng):
    area = NET_AREAS[int(rng.choice(len(NET_AREAS), p=(0.1, 0.2, 0.2, 0.2, 0.15, 0.15)))]
    par = par_row(area, NET_TRIPLES[int(rng.integers(len(NET_TRIPLES)))],
                  NET_COEFFICIENTS[int(rng.integers(len(NET_COEFFICIENTS)))] + (10.0,))
    starts = starts_of(par)[:14]                                        # warm starts: the cold ones go through the drop-in's own test
    return par, starts[int(rng.integers(len(starts)))][1]


def candidate_basin(k):
    """Basin number k of an endless deterministic family: rows  headwater [, second headwater] -> lake A -> 1-2 channel rows
    -> lake B -> 1-2 outlet rows.  Returns dict(to [m] (local rows, -1 = outlet), lake_a, lake_b (local rows), params [m, 9]
    (oracle.PARAM_COLS; NaN on the lakes, as the drop-in hands them on), qlat [m, NET_STEPS / NET_QTS], par [2, 9], h0 [2])."""
    rng = np.random.default_rng([29, k])
    n_hw, n_ch, n_out = (2 if k % 5 == 0 else 1), 1 + k % 2, 1 + (k // 2) % 2
    a = n_hw
    b = a + 1 + n_ch
    m = b + 1 + n_out
    to = np.arange(1, m + 1, dtype=np.int64)
    to[:n_hw] = a
    to[-1] = -1
    params = np.stack([np.full(m, NET_DT), rng.uniform(400, 1500, m), rng.uniform(3, 12, m), np.zeros(m), np.zeros(m),
                       np.full(m, 0.06), np.full(m, 0.12), rng.uniform(0.3, 1.0, m), rng.uniform(0.002, 0.02, m)], 1)
    params[:, 3] = params[:, 2] * 5 / 3
    params[:, 4] = params[:, 3] * 3
    params = params.astype(np.float32)
    params[[a, b]] = np.nan
    nq = NET_STEPS // NET_QTS
    kind = INFLOWS[int(rng.integers(4))]
    qlat = np.zeros((m, nq), np.float32)
    for r in range(n_hw):
        if kind == "small":
            qlat[r] = 0.05
        elif kind == "flood":
            qlat[r] = rng.uniform(5.0, 40.0, nq)
        elif kind == "intermittent":
            qlat[r] = np.where(rng.random(nq) < 0.35, rng.uniform(5.0, 60.0, nq), 0.0)
    la, lb = _candidate_lake(rng), _candidate_lake(rng)
    return dict(to=to, lake_a=a, lake_b=b, params=params, qlat=qlat, par=np.stack([la[0], lb[0]]), h0=f32([la[1], lb[1]]),
                inflow_kind=kind)


class Network:
    pass


def assemble(basins):
    """The basins side by side as one table: rows in basin order, ids = rows.  Lakes are listed in row order; c.is_b marks
    the lower lake of each basin."""
    c = Network()
    to, params, qlat, lakes, par, h0, is_b, basin_of = [], [], [], [], [], [], [], []
    base = 0
    for i, bs in enumerate(basins):
        m = bs["to"].shape[0]
        to.append(np.where(bs["to"] >= 0, bs["to"] + base, -1))
        params.append(bs["params"])
        qlat.append(bs["qlat"])
        lakes += [base + bs["lake_a"], base + bs["lake_b"]]
        par += [bs["par"][0], bs["par"][1]]
        h0 += [bs["h0"][0], bs["h0"][1]]
        is_b += [False, True]
        basin_of += [i] * m
        base += m
    c.n = base
    c.to, c.params, c.qlat = np.concatenate(to), np.concatenate(params), np.concatenate(qlat)
    c.lakes, c.par, c.h0, c.is_b = np.array(lakes, np.int64), np.stack(par), f32(h0), np.array(is_b)
    c.basin_of = np.array(basin_of)
    ups = [[] for _ in range(c.n)]
    for r, d in enumerate(c.to.tolist()):
        if d >= 0:
            ups[d].append(r)
    c.ups = ups
    c.up_ptr = np.zeros(c.n + 1, np.int64)
    c.up_ptr[1:] = np.cumsum([len(u) for u in ups])
    c.up_idx = np.array([x for u in ups for x in u], np.int64)
    level = np.zeros(c.n, np.int64)
    for r in range(c.n):                                                # (rows of a basin are listed upstream first)
        if c.to[r] >= 0:
            level[c.to[r]] = max(level[c.to[r]], level[r] + 1)
    c.level = level
    c.q0 = np.zeros((c.n, 3), np.float32)
    c.q0[c.lakes, 2] = c.h0                                             # the pool's elevation lives in the depth slot
    return c


def route_oracle(c, nsteps, qlat, q0, h0, short=True):
    """oracle.network_by_segment with the case's lakes: (fvd [n, nsteps, 3], inflow record [nres, nsteps], final elevations)"""
    order = np.argsort(c.level, kind="stable")
    res_of_row = np.full(c.n, -1, np.int64)
    res_of_row[c.lakes] = np.arange(c.lakes.shape[0])
    res = dict(res_of_reach=res_of_row[order], par=c.par, water_elevation=h0, routing_period=NET_DT)
    want = O.network_by_segment(nsteps, NET_QTS, c.up_ptr, c.up_idx, c.level, c.params, q0, qlat, short, det=True, res=res)
    return np.ascontiguousarray(want[:, 1:]), res["inflow"][:, 1:].copy(), res["water_elevation"].copy()


def lake_census(c, fvd, inflow, which):
    """census of the steps of lakes `which` (a mask over c.lakes), classified from the oracle's inflow record and starting
    elevations; classify must reproduce the oracle's outflow and elevation of every one of them"""
    s = classify_series(c.par[which], np.full(int(which.sum()), NET_DT, np.float32), c.h0[which], inflow[which])
    rows = c.lakes[which]
    assert same(s["outflow"], fvd[rows, :, 0]) and same(s["elevation"], fvd[rows, :, 2])
    return census(c.par[which], s)


NET_MIN_COUNT = 3
NET_TAGS = ("area=0", "weir_length=0", "orifice_area=0") + tuple(f"H=={e}" for e in EDGES)
NET_BRANCHES = ("dead", "orifice", "weir", "overtop_clipped")            # what stage 1 and the final evaluation can reach


def network_needs(cen):
    """{condition: count} of what the device case must reach on each of its two sets of lakes"""
    need = {("stage1", b): cen["cells"]["stage1", b] for b in NET_BRANCHES}
    need.update({("final", b): cen["cells"]["final", b] for b in NET_BRANCHES})
    need.update({("crossing",) + k: v for k, v in cen["crossings"].items()})
    need.update({("tag", t): cen["tags"][t] for t in NET_TAGS})
    return need


def search_basins(n_candidates=3000, n_basins=64):
    """How NET_BASINS was chosen (tests/golden/make_levelpool_fixtures.py --basins prints it): route the first n_candidates
    basins, drop every basin with a value that is not finite, then take greedily the basin that closes most of what is still
    missing from network_needs on lake A and on lake B, and fill up with the first unused ones."""
    c = assemble([candidate_basin(k) for k in range(n_candidates)])
    fvd, inflow, _ = route_oracle(c, NET_STEPS, c.qlat, c.q0, c.h0)
    finite = np.ones(n_candidates, bool)
    np.logical_and.at(finite, c.basin_of, np.isfinite(fvd).all(axis=(1, 2)))
    gains = {}
    for k in np.flatnonzero(finite):
        for j in (0, 1):
            one = np.zeros(c.lakes.shape[0], bool)
            one[2 * k + j] = True
            gains[k, j] = network_needs(lake_census(c, fvd, inflow, one))
    missing = {(j, key): NET_MIN_COUNT for j in (0, 1) for key in gains[next(iter(gains))[0], 0]}
    chosen = []
    while any(v > 0 for v in missing.values()):
        def gain(k):
            return sum(min(v, gains[k, j][key]) for (j, key), v in missing.items() if v > 0)
        best = max((k for k in np.flatnonzero(finite) if k not in chosen), key=gain)
        if gain(best) == 0:
            raise AssertionError(f"no candidate reaches {[k for k, v in missing.items() if v > 0]}")
        chosen.append(int(best))
        for (j, key) in missing:
            missing[j, key] -= gains[best, j][key]
    chosen += [int(k) for k in np.flatnonzero(finite) if k not in chosen][:max(0, n_basins - len(chosen))]
    return tuple(sorted(chosen))


# search_basins() on the first 3000 candidates
NET_BASINS = (1, 3, 4, 5, 6, 7, 9, 10, 11, 13, 14, 17, 20, 22, 24, 25, 28, 29, 30, 31, 33, 34, 35, 44, 45, 47, 48, 49, 52, 53, 54, 57,
              58, 60, 64, 66, 68, 69, 70, 72, 74, 76, 77, 78, 81, 82, 83, 84, 85, 86, 87, 89, 92, 94, 95, 96, 169, 261, 448, 902,
              1336, 1493, 2120, 2548)


# A weir below its orifice with the pool exactly on the weir's crest: the one place where `dh > 0` and `dh >= 0` part (on
# the crest the weir's term is zero, so wherever the orifice's term is finite both give the same bits; here the head on the
# orifice is negative, its sqrt is a NaN, and only the strict comparison discards it).  The pool must stay there -- between
# the weir and the orifice the reference itself returns NaN -- so it has no area, or no inflow; and it is the basin's outlet,
# so that an engine that got the comparison wrong would hand its NaN to no row below.
NET_DRY_WEIR_BASINS = (106, 101, 112, 103)
DRY_WEIR_TRIPLE = (3.0, 2.0, 4.0)


def dry_weir_basin(j):
    """candidate_basin(NET_DRY_WEIR_BASINS[j]) cut off below lake B, which becomes the pool described above"""
    bs = candidate_basin(NET_DRY_WEIR_BASINS[j])
    m = bs["lake_b"] + 1
    bs["to"], bs["params"], bs["qlat"] = bs["to"][:m].copy(), bs["params"][:m], bs["qlat"][:m].copy()
    bs["to"][-1] = -1
    area = 0.0 if j % 2 == 0 else 1.0e-3
    bs["par"][1] = par_row(area, DRY_WEIR_TRIPLE, NET_COEFFICIENTS[j % 2] + (10.0,))
    bs["h0"][1] = DRY_WEIR_TRIPLE[1]
    if area > 0:                                                        # nothing may reach the pool: lake A starts dead and stays so
        bs["qlat"][:] = 0
        bs["h0"][0] = bs["par"][0][_P["orifice_elevation"]] - F(0.5)
    return bs


def dry_weir_steps(c, fvd):
    """steps of the case's lakes that start exactly on a weir crest that lies below the orifice"""
    start = np.concatenate([c.h0[:, None], fvd[c.lakes, :-1, 2]], axis=1)
    we, oe = c.par[:, _P["weir_elevation"]], c.par[:, _P["orifice_elevation"]]
    return int(np.count_nonzero((start == we[:, None]) & (we < oe)[:, None]))


@functools.lru_cache(maxsize=None)
def network_case():
    """the device tests' case: assemble() of NET_BASINS and the dry-weir basins, with the oracle's window of NET_STEPS steps
    (c.fvd [n, NET_STEPS, 3], c.inflow [nres, NET_STEPS], c.h_final [nres]).  Shared and never written to."""
    c = assemble([candidate_basin(k) for k in NET_BASINS] + [dry_weir_basin(j) for j in range(len(NET_DRY_WEIR_BASINS))])
    c.fvd, c.inflow, c.h_final = route_oracle(c, NET_STEPS, c.qlat, c.q0, c.h0)
    for a in (c.to, c.params, c.qlat, c.par, c.h0, c.q0, c.fvd, c.inflow, c.h_final):
        a.setflags(write=False)
    return c


NET_DAYS, NET_DAY_STEPS = 3, 16


@functools.lru_cache(maxsize=None)
def network_days():
    """the case's window as a stream of NET_DAYS days of NET_DAY_STEPS steps, the oracle day by day with the state handed on
    as new_q0 does (q_T, q_T, depth_T) and the pools' elevations carried over: [(qlat, fvd, inflow, final state [n, 3])]"""
    c = network_case()
    nq = NET_DAY_STEPS // NET_QTS
    state, h, out = c.q0, c.h0, []
    for d in range(NET_DAYS):
        ql = np.ascontiguousarray(c.qlat[:, d * nq:(d + 1) * nq])
        fvd, inflow, h = route_oracle(c, NET_DAY_STEPS, ql, state, h)
        assert same(fvd[c.lakes, -1, 2], h)
        state = np.stack([fvd[:, -1, 0], fvd[:, -1, 0], fvd[:, -1, 2]], 1)
        out.append((ql, fvd, inflow, state))
    return out


@functools.lru_cache(maxsize=None)
def network_cold():
    """NET_BASINS with every pool cold-started, ifd 0.5, 1, 0 in turn: the network with c.ifd [nres], c.h0 = the starts as
    init_levelpool_reach forms them in float32, and the oracle's c.fvd, c.inflow, c.h_final.  The dry-weir basins are left
    out (a pool that drains into the gap between a weir and the orifice above it is a NaN in the reference), and the order
    of the three fractions is the one of the three rotations under which every value of the oracle is finite."""
    c = assemble([candidate_basin(k) for k in NET_BASINS])
    c.ifd = f32((0.5, 1.0, 0.0))[np.arange(c.lakes.shape[0]) % 3]
    c.h0 = cold_start(c.par, c.ifd)
    c.q0 = np.zeros((c.n, 3), np.float32)                              # (the drop-in is handed no elevation: it forms the start)
    c.fvd, c.inflow, c.h_final = route_oracle(c, NET_STEPS, c.qlat, c.q0, c.h0)
    return c
