"""HYBRID-PERSISTENCE AND RFC-FORECAST RESERVOIRS IN A STREAM OF DAYS (include/trmc.h trmc_stream_set_reservoir_da,
trmc_stream_reservoir_da; csrc/stream.inc, csrc/reservoir_da.hpp reservoir_da_row_day): set_reservoir_da is the declaration and
the state day 0 starts from, every day brings its own tables, the state lives on the device and is handed from day to day as
the reference's loop hands it from run set to run set (mc_reach.pyx:820-837).

The reference is the recorded long window of the reference loop (tests/golden/reservoir_da_network.npz, 72 steps on the
LowerColorado domain collapsed at its waterbodies, types {1..5}), routed here as 3 days of 24 steps: bit for bit."""
import functools

import numpy as np
import pytest

import helpers as H
import test_reservoir_da_network as DN
import test_reservoirs as TR
from troute_amd import _lib
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu

NET = DN.NET
NDAYS, NSTEPS = 3, 24
assert NDAYS * NSTEPS == DN.NTS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case():
    """the fixture's network as a plan takes it: CSR, parameters, the lakes' rows / parameters / kinds / table rows, the state"""
    lc, ids, dv, ql, q0, reaches, net, lakes, wbody_cols, lakeset, _ = TR.reservoir_case()
    c = Case()
    c.ids, c.n, c.dt, c.qts, c.lakes = ids, len(ids), float(lc.dt), int(lc.qts), lakes
    row = {int(s): i for i, s in enumerate(ids)}
    ups = [[] for _ in range(c.n)]
    for rr in reaches:
        r = [row[s] for s in rr]
        ups[r[0]] = [row[s] for s in net.get(rr[0], [])]
        for x, y in zip(r[1:], r[:-1]):
            ups[x] = [y]
    c.up_ptr, c.up_idx = csr_from_lists(ups)
    c.to = np.full(c.n, -1, np.int64)
    for r, u in enumerate(ups):
        c.to[u] = r
    c.params = np.ascontiguousarray(dv[:, [H.DATA_COLS.index(k) for k in ("dt", "dx", "bw", "tw", "twcc", "n", "ncc", "cs", "s0")]])
    a = wbody_cols.astype(np.float32)
    c.par = np.concatenate([a[:, :8], np.full((len(lakes), 1), 10.0, np.float32)], 1)
    h0 = a[:, 10].copy()
    cold = h0 < np.float32(-900000000)
    h0[cold] = (a[:, 4] + ((a[:, 1] - a[:, 4]).astype(np.float32) * a[:, 8]).astype(np.float32)).astype(np.float32)[cold]
    c.lake_rows = np.array([row[int(l)] for l in lakes])
    c.q0 = q0.copy()
    c.q0[c.lake_rows] = np.stack([a[:, 9], np.zeros(len(lakes), np.float32), h0], 1)
    c.kind = np.where(NET["types"] == 1, 0, NET["types"]).astype(np.int32)
    c.trow = np.zeros(len(lakes), np.int32)
    for i, (l, k) in enumerate(zip(lakes.tolist(), c.kind.tolist())):
        if k:
            c.trow[i] = int(np.flatnonzero(NET[{2: "usgs_idx", 3: "usace_idx", 4: "rfc_idx", 5: "rfc_idx"}[k]] == l)[0])
    assert ql.shape[1] * c.qts >= DN.NTS and NSTEPS % c.qts == 0
    nq = NSTEPS // c.qts
    c.days = [np.ascontiguousarray(ql[:, d * nq:(d + 1) * nq]) for d in range(NDAYS)]
    return c


def split(t):
    """the 23 arguments of DN.tables -> (usgs, usace, rfc) as set_reservoir_da takes them"""
    hyb = lambda o: (t[o], t[o + 2], np.stack([t[o + 3], t[o + 4], t[o + 6], t[o + 5]], 1).astype(np.float32))   # noqa: E731
    rfc = (t[14], np.asarray(t[20], np.float32), np.stack([t[19], t[16], t[18], t[21], t[22]], 1).astype(np.int32))
    return hyb(0), hyb(7), rfc


def day_tables(c, d, state=None):
    return split(DN.tables(t_shift=d * NSTEPS * c.dt, state=state))


def state_tuples(state, tsidx, c):
    """a day's state product -> the tuples [4], [5], [7] of compute_network_structured"""
    out = []
    for name, kind in (("usgs", 2), ("usace", 3)):
        idx = NET[f"{name}_idx"]
        cols = [np.zeros(len(idx), np.float32) for _ in range(4)]
        for i in np.flatnonzero(c.kind == kind):
            for j in range(4):
                cols[j][c.trow[i]] = state[i, j]
        out.append((idx, *cols))
    idx = NET["rfc_idx"]
    ut, ti = np.zeros(len(idx), np.float32), np.zeros(len(idx), np.int32)
    for i in np.flatnonzero(c.kind >= 4):
        ut[c.trow[i]], ti[c.trow[i]] = state[i, 0], tsidx[i]
    out.append((idx, ut, ti))
    return out


def open_plan(c, slices, K, precision=32, **opt):
    return RoutingPlan(c.up_ptr, c.up_idx, c.params, assume_short_ts=True, engine="levels", precision=precision,
                       options=dict({"cluster_rows": 24, "wide_min_rows": 32 if slices else 0, "wide_k": K}, **opt))


def declare(p, c):
    p.set_reservoirs(c.lake_rows, c.par, c.dt)
    p.set_reservoir_da(c.kind, c.trow, *day_tables(c, 0))


def stream_days(p, c, full_output=True, output_stride=0, slots=0, tables_of=None, caps=True):
    """[(fvd, inflow, state [nres, 4], tsidx [nres], final)] per day through a stream at plan level"""
    nres = len(c.lakes)
    declare(p, c)
    p.upload_forcing(NSTEPS, c.days[0], c.q0)
    p.stream_begin(NSTEPS, c.qts, slots=slots, full_output=full_output, output_stride=output_stride, reservoir_da=caps)
    info = p.stream_info()
    D = info["slots"]
    assert D >= NDAYS or slots == 0 or D >= slots
    keep = NSTEPS // output_stride if output_stride else NSTEPS
    ring = [(_lib.result_empty((c.n, keep, 3), np.float32, always_pinned=True),
             _lib.result_empty((nres, NSTEPS), np.float32, always_pinned=True),
             _lib.result_empty((nres, 4), np.float32, always_pinned=True),
             _lib.result_empty((nres,), np.int32, always_pinned=True),
             _lib.result_empty((c.n, 3), np.float32, always_pinned=True)) for _ in range(D)]
    got = []

    def take(d):
        p.stream_wait(d)
        got.append(tuple(np.array(x, copy=True) for x in ring[d % D]))
    for d in range(NDAYS):
        if d >= D:
            if p.stream_info()["days_complete"] <= d - D:
                p.stream_flush()
            take(d - D)
        fvd, rin, st, ti, fin = ring[d % D]
        tabs = day_tables(c, d) if tables_of is None else tables_of(d)
        p.stream_push(pinned_like(c.days[d]), fvd=fvd, q0=fin, reservoir_inflow=rin, reservoir_da=tabs, reservoir_da_state=(st, ti))
    p.stream_flush()
    for d in range(len(got), NDAYS):
        take(d)
    p.stream_end()
    return got, info


def window_days(p, c, stride=0):
    """the same days as single windows on the same plan, the state through the host, shifted as mc_reach.py shifts it"""
    out = []
    p.set_reservoirs(c.lake_rows, c.par, c.dt)
    state, da = c.q0, None
    t_end = np.float32(np.float32(NSTEPS) * np.float32(c.dt))
    for d in range(NDAYS):
        p.set_reservoir_da(c.kind, c.trow, *day_tables(c, d, da))
        p.upload_forcing(NSTEPS, c.days[d], state)
        p.route_device(NSTEPS, c.qts, True)
        fvd = p.download_fvd()
        state = p.download_final_state()
        st, ti = p.download_reservoir_da()
        hyb = np.isin(c.kind, (2, 3))
        st[c.kind != 0, 0] -= t_end
        st[hyb, 3] -= t_end
        da = state_tuples(st, ti, c)
        out.append((fvd[:, stride - 1::stride].copy() if stride else fvd, p.download_reservoir_inflow(), st, ti, state))
    return out


def assert_days_equal(got, want, what):
    assert len(got) == len(want)
    for d, (g, w) in enumerate(zip(got, want)):
        for k, name in enumerate(("fvd", "reservoir_inflow", "da_state", "da_tsidx", "final_state")):
            assert g[k].shape == w[k].shape and g[k].dtype == w[k].dtype, (what, d, name)
            assert np.array_equal(bits(g[k]), bits(w[k])), (what, d, name)


def as_result(c, day):
    upstream = np.zeros((c.n, NSTEPS), np.float32)
    upstream[c.lake_rows] = day[1]
    st = state_tuples(day[2], day[3], c)
    return (c.ids, day[0].reshape(c.n, -1), 0, None, st[0], st[1], upstream, st[2])


# ---- 1. against the reference's recorded long window -----------------------------------------------------------------------
@pytest.mark.parametrize("slices", [False, True])
@pytest.mark.parametrize("K", [4, 8])
def test_stream_days_equal_the_reference_long_window(slices, K):
    c = case()
    assert set(NET["types"].tolist()) == {1, 2, 3, 4, 5}
    assert {int(k) for k in c.kind} == {0, 2, 3, 4, 5}
    with open_plan(c, slices, K) as p:
        got, info = stream_days(p, c)
    assert (info["wide_levels"] > 0) == slices and info["cluster_levels"] > 0 and info["tiles_per_day"] == NSTEPS // K
    assert info["lag_max"] >= 1                                  # (rows that are still in the day before when a day is pushed)
    for d in range(NDAYS):
        DN.check_against_golden(as_result(c, got[d]), True, d * NSTEPS, (d + 1) * NSTEPS)
    DN.check_state(as_result(c, got[-1]), True)


# ---- 2. stream against its own windows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["full", "products-stride-12"])
@pytest.mark.parametrize("more_slots", [0, 1])
def test_stream_equals_its_own_windows(variant, more_slots):
    c = case()
    stride = 12 if variant != "full" else 0
    with open_plan(c, True, 4) as p:
        windows = window_days(p, c, stride)
        first, info = stream_days(p, c, full_output=not stride, output_stride=stride)
        got = first
        if more_slots:
            got, info2 = stream_days(p, c, full_output=not stride, output_stride=stride, slots=info["slots"] + 1)
            assert info2["slots"] == info["slots"] + 1
    assert_days_equal(got, windows, (variant, more_slots))
    moved = np.stack([g[2] for g in got])
    assert (moved[0] != moved[-1]).any()                         # (the state does move from day to day)


# ---- 3. a day's tables have their own shape --------------------------------------------------------------------------------
def test_per_day_table_shape_and_rfc_reset():
    c = case()
    with open_plan(c, True, 4) as p:
        plain, _ = stream_days(p, c)
        ncol = NET["usgs_obs"].shape[1]

        def tables_of(d):
            usgs, usace, rfc = day_tables(c, d)
            if d == 1:                                            # NaN columns appended, at times beyond every update_time
                pad = 3
                far = (usgs[1][-1] + np.float32(86400.0) * np.arange(1, pad + 1, dtype=np.float32)).astype(np.float32)
                usgs = (np.concatenate([usgs[0], np.full((usgs[0].shape[0], pad), np.nan, np.float32)], 1), np.concatenate([usgs[1], far]), None)
                far = (usace[1][-1] + np.float32(86400.0) * np.arange(1, pad + 1, dtype=np.float32)).astype(np.float32)
                usace = (np.concatenate([usace[0], np.full((usace[0].shape[0], pad), np.nan, np.float32)], 1), np.concatenate([usace[1], far]), None)
                return usgs, usace, rfc
            if d == 2:                                            # the index the device would have carried anyway
                ipar = rfc[2].copy()
                ipar[:, 0] = [plain[1][3][np.flatnonzero((c.kind >= 4) & (c.trow == j))[0]] for j in range(ipar.shape[0])]
                return usgs, usace, (rfc[0], None, ipar), True
            return usgs, usace, rfc
        got, _ = stream_days(p, c, tables_of=tables_of, caps=(ncol + 3, NET["usace_obs"].shape[1] + 3, 0))
    assert_days_equal(got, plain, "per-day shape")


# ---- 4. errors ------------------------------------------------------------------------------------------------------------
def test_stream_reservoir_da_errors():
    c = case()
    with open_plan(c, True, 4) as p:
        declare(p, c)
        p.upload_forcing(NSTEPS, c.days[0], c.q0)
        with pytest.raises(ValueError, match="types 2-5.*window by window"):          # (not asked for: as it always was)
            p.stream_begin(NSTEPS, c.qts)
        p.stream_begin(NSTEPS, c.qts, reservoir_da=True)
        ql = pinned_like(c.days[0])
        usgs, usace, rfc = day_tables(c, 0)
        with pytest.raises(ValueError, match="every day must bring its reservoir tables"):
            p.stream_push(ql)
        with pytest.raises(ValueError, match="usgs table of a day: 1 rows, the stream was declared with 2"):
            p.stream_push(ql, reservoir_da=((usgs[0][:1], usgs[1], None), usace, rfc))
        wide = (np.concatenate([usace[0], usace[0][:, :1]], 1), np.concatenate([usace[1], usace[1][:1]]), None)
        with pytest.raises(ValueError, match="usace table of a day: .* columns exceed the stream's capacity"):
            p.stream_push(ql, reservoir_da=(usgs, wide, rfc))
        bad = rfc[2].copy()
        bad[0, 0] = rfc[0].shape[1]
        with pytest.raises(ValueError, match="timeseries_idx outside the series"):
            p.stream_push(ql, reservoir_da=(usgs, usace, (rfc[0], None, bad), True))
        with pytest.raises(RuntimeError, match="stream of windows is in progress"):
            p.set_reservoir_da(c.kind, c.trow, usgs, usace, rfc)
        assert p.stream_info()["days_pushed"] == 0               # (a refused push leaves no day behind)
        p.stream_end()
        # tables on a stream without data assimilation
        p.set_reservoirs(c.lake_rows, c.par, c.dt)               # (drops the declaration)
        p.upload_forcing(NSTEPS, c.days[0], c.q0)
        p.stream_begin(NSTEPS, c.qts, reservoir_da=True)
        with pytest.raises(ValueError, match="tables for a stream without them"):
            p.stream_push(ql, reservoir_da=(usgs, usace, rfc))
        p.stream_end()
    for kw in (dict(precision=64), dict(arithmetic="tolerance")):
        with open_plan(c, True, 4, **kw) as p:
            p.set_reservoirs(c.lake_rows, c.par.astype(p.dtype), c.dt)
            with pytest.raises((ValueError, NotImplementedError), match="precision 32 plan in the exact arithmetic|precision 64 plan"):
                p.set_reservoir_da(c.kind, c.trow, *day_tables(c, 0))
            p.upload_forcing(NSTEPS, c.days[0].astype(p.dtype), c.q0.astype(p.dtype))
            with pytest.raises(ValueError, match="precision 32 plan in the exact arithmetic"):
                p.stream_begin(NSTEPS, c.qts, reservoir_da=True)
    with pytest.raises(NotImplementedError):
        ShardedRouter(c.to, c.params, rank=0, world=2, stream=True, reservoirs=(c.lake_rows, c.par, c.dt),
                      reservoir_da=(c.kind, c.trow, *day_tables(c, 0)))


# ---- 5. RouteStream end to end ---------------------------------------------------------------------------------------------
def test_routestream_with_reservoir_da_end_to_end():
    c = case()
    ids = (NET["usgs_idx"], NET["usace_idx"], NET["rfc_idx"])
    options = {"cluster_rows": 24, "wide_min_rows": 32, "wide_k": 4}
    r = ShardedRouter(c.to, c.params, stream=True, options=options, reservoirs=(c.lake_rows, c.par, c.dt),
                      reservoir_da=(c.kind, c.trow, *day_tables(c, 0), ids))
    got = {}
    with RouteStream(r, NSTEPS, c.qts) as rs:
        for item in rs.route(iter(c.days), c.q0, reservoir_da=(day_tables(c, d) for d in range(NDAYS))):
            assert len(item) == 4 and set(item[3]) == {"reservoir_inflow", "nudge", "lastobs", "reservoir_da"}
            got[item[0]] = (np.array(item[1]), item[3]["reservoir_da"])
        rows = rs.outlet_rows
        with pytest.raises(ValueError, match="must yield every day's tables"):
            next(rs.route(iter(c.days), c.q0))
        with pytest.raises(ValueError, match="reservoir_da ended before the forcings"):
            list(rs.route(iter(c.days), c.q0, reservoir_da=iter([day_tables(c, 0)])))
    r.close()
    assert sorted(got) == [0, 1, 2]
    last = got[2][1]
    DN.check_state((None,) * 4 + (last[0], last[1], None, last[2]), True)
    with open_plan(c, True, 4) as p:                              # (the outlet hydrographs of test 1's stream)
        days, _ = stream_days(p, c)
    for d in range(NDAYS):
        assert np.array_equal(bits(got[d][0]), bits(days[d][0][rows, :, 0])), d
    r = ShardedRouter(c.to, c.params, stream=True, options=options, reservoirs=(c.lake_rows, c.par, c.dt))
    with RouteStream(r, NSTEPS, c.qts) as rs:
        with pytest.raises(ValueError, match="needs a router with data-assimilation reservoirs"):
            next(rs.route(iter(c.days), c.q0, reservoir_da=iter([day_tables(c, 0)])))
    r.close()
