"""A stream day pushed as packed CHRTOUT columns (trmc_stream_set_packed_forcing, trmc_stream_push_day_packed): the device decodes
the raw int32 columns, joins them on the feature id and writes the forcing of the day's ring slot in one kernel.  Every comparison
is bit for bit, against the SAME plan fed the floats the host rule gives (``nhd_io.unpack_packed``, pinned to netCDF4's read by
test_file_formats.test_chrtout_packed_host_rule, then the join and the reference's cast to float32 -- the cast
``upload_forcing_packed`` makes in either precision: a precision-64 plan takes those float32 values widened).

The raw values that pass the mask stay below 2^24, the scale factor is a float32: raw * scale is exact in double, so the host's and
the device's double agree whatever the order of their roundings, and the non-zero add_offset adds one rounding on both sides."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import test_gpu_stream_reservoirs_nudging as RN
from troute_amd import _lib, nhd_io, synthetic
from troute_amd.plan import RoutingPlan
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

NSEG, NQ, NSTEPS, QTS, NDAYS, STRIDE = 3000, 4, 32, 8, 5, 8
OPTIONS = {"cluster_rows": 128, "wide_k": 8}
SCALE = float(np.float32(1e-5))
NAN = float("nan")
FILL, MISSING, VMAX = -999900000, -888800000, 2000000000
#          scale  add_offset  _FillValue  missing_value  valid_min  valid_max
PACK_A = [SCALE, 0.25, float(FILL), float(MISSING), 0.0, float(VMAX)]
PACK_B = [SCALE, -0.125, -9999.0, NAN, 20000.0, NAN]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def network():
    net = synthetic.generate(nseg=NSEG, nnet=9, seed=5, nq=NQ)
    up_ptr, up_idx = synthetic.upstream_csr(net["to"])
    rng = np.random.default_rng(55)
    q0 = np.stack([rng.uniform(0, 1, NSEG), np.zeros(NSEG), rng.uniform(0, 0.5, NSEG)], 1).astype(np.float32)
    rows = np.flatnonzero(np.asarray(net["to"]) < 0).astype(np.int64)       # the outlets: the day's hydrographs
    return up_ptr, up_idx, net["params"], q0, rows


@functools.lru_cache(maxsize=None)
def files(two):
    """the feature axis, the rows' ids and NDAYS days of raw columns: the row ids permuted, 37 ids that are no row of the network,
    about 1 % of the rows absent; every day has cells at _FillValue, at missing_value, below valid_min and above valid_max"""
    rng = np.random.default_rng(5 + two)
    ids = rng.permutation(np.arange(7_000_000, 7_000_000 + NSEG, dtype=np.int64))
    absent = np.sort(rng.choice(NSEG, NSEG // 100, replace=False))
    feature_id = rng.permutation(np.concatenate([np.delete(ids, absent), 9_000_000_000 + np.arange(37, dtype=np.int64)]))
    nfeat = feature_id.shape[0]
    assert nfeat == NSEG - NSEG // 100 + 37 and nfeat % 64 != 0
    days = []
    for d in range(NDAYS):
        a = rng.integers(0, 40000 + 20000 * d, (NQ, nfeat)).astype(np.int32)
        b = rng.integers(20000, 60000, (NQ, nfeat)).astype(np.int32)
        for j in range(NQ):
            for raw, planted in ((a, (FILL, MISSING, -7, VMAX + 1)), (b, (-9999, 19999, 3))):
                for v in planted:
                    raw[j, rng.choice(nfeat, 11, replace=False)] = v
        day = {"feature_id": feature_id, "raw_a": a, "raw_b": b if two else None,
               "pack_a": np.array(PACK_A), "pack_b": np.array(PACK_B) if two else None}
        for raw, planted in ((a, (FILL, MISSING, -7, VMAX + 1)),) + (((b, (-9999, 19999, 3)),) if two else ()):
            assert all((raw == v).any() for v in planted)
        days.append(day)
    return ids, absent, days


def host_floats(day, ids):
    """the host rule: unpack in double, the sum, the join on the feature id (a row the files do not hold: 0), the cast to float32"""
    host = nhd_io.unpack_packed(day)                                       # float64 [nq, nfeat]
    where = {int(f): i for i, f in enumerate(day["feature_id"])}
    qlat = np.zeros((ids.shape[0], host.shape[0]), np.float32)
    for r, f in enumerate(ids):
        if int(f) in where:
            qlat[r] = host[:, where[int(f)]].astype(np.float32)
    return qlat


def open_plan(precision):
    up_ptr, up_idx, params, _, _ = network()
    return RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels", precision=precision, options=OPTIONS)


def pinned_day(day):
    return dict(day, raw_a=pinned_like(day["raw_a"]), raw_b=None if day["raw_b"] is None else pinned_like(day["raw_b"]))


def stream(p, days, full_output, more_than_slots=True):
    """``days`` -- float arrays [nseg, nq] and packed dicts, in any mix -- as one stream: [(hyd, final, fvd)] per day"""
    _, _, _, q0, rows = network()
    dt, n = p.dtype, p.nseg
    rs = p.rowset(rows)
    nq = days[0]["raw_a"].shape[0] if isinstance(days[0], dict) else days[0].shape[1]
    p.upload_forcing(NSTEPS, np.zeros((n, nq), dt), q0.astype(dt))
    p.stream_begin(NSTEPS, QTS, full_output=full_output, output_stride=0 if full_output else STRIDE)
    D = p.stream_info()["slots"]
    if more_than_slots:
        assert len(days) > D                                               # (slots and the staging area are used again)
    keep = NSTEPS if full_output else NSTEPS // STRIDE
    out = [(_lib.result_empty((rows.shape[0], NSTEPS), dt, always_pinned=True), _lib.result_empty((n, 3), dt, always_pinned=True),
            _lib.result_empty((n, keep, 3), dt, always_pinned=True)) for _ in days]
    for d, day in enumerate(days):
        if d >= D:                                                         # (the slot's last day leaves before the slot is reused)
            if p.stream_info()["days_complete"] <= d - D:
                p.stream_flush()
            p.stream_wait(d - D)
        hyd, fin, fvd = out[d]
        if isinstance(day, dict):
            assert p.stream_push(packed=pinned_day(day), rowset=rs, hyd=hyd, q0=fin, fvd=fvd) == d
        else:
            assert p.stream_push(pinned_like(day.astype(dt)), rowset=rs, hyd=hyd, q0=fin, fvd=fvd) == d
    p.stream_flush()
    for d in range(max(0, len(days) - D), len(days)):
        p.stream_wait(d)
    got = [tuple(np.array(x, copy=True) for x in o) for o in out]
    p.stream_end()
    return got


def assert_streams_equal(got, want, what):
    assert len(got) == len(want)
    for d, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("hydrographs", "final state", "(q, v, d) block"), g, w):
            assert np.isfinite(b).all() and same(a, b), (what, d, name, int(np.count_nonzero(bits(a) != bits(b))))


@pytest.mark.parametrize("two", [True, False], ids=["two-variables", "q_lateral"])
@pytest.mark.parametrize("precision", [32, 64])
def test_packed_days_equal_the_days_unpacked_on_the_host(precision, two):
    ids, absent, days = files(two)
    floats = [host_floats(day, ids) for day in days]
    for q in floats:            # (the absent rows have no inflow, the others do)
        assert (q[absent] == 0).all() and np.delete(q, absent, 0).max() > 0.5
    mixed = [days[0], floats[1], floats[2], days[3], days[4]]
    with open_plan(precision) as p:
        feat_of_row = p.stream_set_packed_forcing(days[0], ids)
        assert (feat_of_row[absent] == -1).all() and (np.delete(feat_of_row, absent) >= 0).all()
        assert np.array_equal(days[0]["feature_id"][np.delete(feat_of_row, absent)], np.delete(ids, absent))
        for full in (True, False):      # the full (q, v, d) block; then the products-only stream with every 8th step
            want = stream(p, floats, full)
            assert not same(want[0][1], want[1][1])                        # (the days differ)
            assert_streams_equal(stream(p, days, full), want, ("packed", full))
            assert_streams_equal(stream(p, mixed, full), want, ("packed and float days in one stream", full))
        # the declaration withdrawn: the plan's streams are what they were
        p.stream_set_packed_forcing(None)
        assert_streams_equal(stream(p, floats, False), want, "after the declaration was withdrawn")


def test_packed_days_carry_nudging_tables_and_reservoirs_as_float_days_do():
    """a case of test_gpu_stream_reservoirs_nudging (its network, lakes, gages and observations): the days quantised to a packed
    variable, pushed with the day's nudging tables and level-pool reservoirs -- as packed days and as the floats they decode to"""
    c = copy.copy(RN.case())                                               # (the module's case is cached and shared: the days change on a copy)
    tabs, _ = RN.day_tables(c, len(c.days))
    rng = np.random.default_rng(3)
    ids = np.arange(100, 100 + c.n, dtype=np.int64)
    feature_id = rng.permutation(ids)
    col = np.argsort(feature_id, kind="stable")                            # (feature_id[col[r]] == ids[r])
    packed = []
    for q in c.days:
        raw = np.zeros((q.shape[1], c.n), np.int32)
        raw[:, col] = np.minimum(np.rint(q.T.astype(np.float64) / SCALE), 2.0 ** 23).astype(np.int32)
        packed.append({"feature_id": feature_id, "raw_a": raw, "raw_b": None, "pack_a": np.array([SCALE, 0.0, NAN, NAN, NAN, NAN]), "pack_b": None})
    c.days = [host_floats(day, ids) for day in packed]
    assert all(q.max() > 0 for q in c.days)
    with RN.open_plan(c) as p:
        want, info = RN.stream_days(p, c, tabs)
    with RN.open_plan(c) as p:
        dt = p.dtype
        p.set_reservoirs(c.lakes, c.par, RN.DT)
        p.stream_set_gages(c.gages)
        p.stream_set_packed_forcing(packed[0], ids)
        p.upload_forcing(RN.NSTEPS, c.days[0], c.q0)
        p.stream_begin(RN.NSTEPS, RN.QTS, full_output=True)
        D = p.stream_info()["slots"]
        assert D == info["slots"]
        ring = [(_lib.result_empty((c.n, RN.NSTEPS, 3), dt, always_pinned=True), _lib.result_empty((c.lakes.shape[0], RN.NSTEPS), dt, always_pinned=True),
                 _lib.result_empty((c.gages.shape[0], RN.NSTEPS), dt, always_pinned=True), _lib.result_empty((c.n, 3), dt, always_pinned=True))
                for _ in packed]
        for d, day in enumerate(packed):
            if d >= D:
                if p.stream_info()["days_complete"] <= d - D:
                    p.stream_flush()
                p.stream_wait(d - D)
            fvd, rin, nud, fin = ring[d]
            mode, a, w = tabs[d]
            p.stream_push(packed=pinned_day(day), fvd=fvd, q0=fin, nudging=(mode, a, w, c.usgs[d][:, 0]), nudge=nud, reservoir_inflow=rin)
        p.stream_flush()
        for d in range(max(0, len(packed) - D), len(packed)):
            p.stream_wait(d)
        got = [tuple(np.array(x, copy=True) for x in r) for r in ring]
        p.stream_end()
    assert np.abs(got[-1][2]).max() > 0 and np.abs(got[-1][1]).max() > 0       # (gages nudged, reservoirs filled)
    RN.assert_days_equal(got, want, "packed days with nudging tables and reservoirs")


def test_lowercolorado_files_as_a_one_day_stream_equal_the_packed_window():
    import test_file_formats as FF
    lc = H.LowerColorado()
    pk = nhd_io.chrtout_packed(FF.CHRT)                                    # one day of nq = 2
    assert pk["raw_a"].shape == (2, 11248) and pk["raw_b"] is not None
    up_ptr, up_idx = lc.csr()
    outlets = np.setdiff1d(np.arange(lc.nseg, dtype=np.int64), up_idx)        # (the rows that are nobody's upstream row)
    assert outlets.size > 0
    nsteps, qts = 24, 12
    with RoutingPlan(up_ptr, up_idx, lc.params9, assume_short_ts=True, engine="levels", options={"cluster_rows": 128, "wide_k": 8}) as p:
        feat_w = p.upload_forcing_packed(nsteps, pk, lc.ids, lc.q0)
        p.route_device(nsteps, qts, True)
        want_hyd, want_fin = p.download_fvd()[outlets, :, 0].copy(), p.download_final_state()
        assert np.isfinite(want_hyd).all() and want_hyd.max() > 0
        feat_s = p.stream_set_packed_forcing(pk, lc.ids)
        assert np.array_equal(feat_s, feat_w)
        rs = p.rowset(outlets)
        p.upload_forcing(nsteps, np.zeros((lc.nseg, 2), np.float32), lc.q0)
        p.stream_begin(nsteps, qts)
        hyd = _lib.result_empty((outlets.shape[0], nsteps), np.float32, always_pinned=True)
        fin = _lib.result_empty((lc.nseg, 3), np.float32, always_pinned=True)
        p.stream_push(packed=pinned_day(pk), rowset=rs, hyd=hyd, q0=fin)
        p.stream_flush()
        p.stream_wait(0)
        assert p.stream_packed_forcing_kernel_ms() >= 0.0
        p.stream_end()
        assert same(np.array(hyd), want_hyd) and same(np.array(fin), want_fin)


def test_the_library_refuses_what_it_must_with_its_reasons():
    lib = _lib.lib()
    up_ptr, up_idx, params, q0, rows = network()
    ids, _, days = files(True)
    one = files(False)[2][0]
    nfeat = days[0]["feature_id"].shape[0]
    err = lambda: lib.trmc_last_error().decode()
    pa, pb = np.array(PACK_A), np.array(PACK_B)
    day = pinned_day(days[0])
    with open_plan(32) as p:
        feat = p._feat_of_row(days[0], ids)
        args = lambda f=feat, n=nfeat, a=pa, b=pb: (p._h, n, _lib.ptr(f), _lib.ptr(a), _lib.ptr(b))
        # the declaration: the feature axis, its entries, the packing facts
        assert lib.trmc_stream_set_packed_forcing(*args(n=2 ** 31)) == _lib.TRMC_EINVAL and "feature axis too long" in err()
        assert lib.trmc_stream_set_packed_forcing(*args(n=-1)) == _lib.TRMC_EINVAL and "nfeat < 0" in err()
        bad = feat.copy()
        bad[17] = nfeat
        assert lib.trmc_stream_set_packed_forcing(*args(f=bad)) == _lib.TRMC_EINVAL and "feat_of_row entry outside the feature axis" in err()
        assert lib.trmc_stream_set_packed_forcing(*args(a=None)) == _lib.TRMC_EINVAL and "pack_a is NULL" in err()
        # a packed push without the declaration (none was accepted so far)
        p.upload_forcing(NSTEPS, np.zeros((NSEG, NQ), np.float32), q0)
        p.stream_begin(NSTEPS, QTS)
        sd = _lib.StreamDay()
        sd.nq, sd.rowset = NQ, -1
        push = lambda a, b: lib.trmc_stream_push_day_packed(p._h, C.byref(sd), _lib.ptr(a), _lib.ptr(b))
        assert push(day["raw_a"], day["raw_b"]) == _lib.TRMC_ESTATE and "without the declaration" in err()
        with pytest.raises(RuntimeError, match="stream_set_packed_forcing precedes stream_begin"):
            p.stream_push(packed=day)
        with pytest.raises(RuntimeError, match="no day of this stream has been pushed as packed columns"):
            p.stream_packed_forcing_kernel_ms()
        # ... and no declaration while a stream is in progress
        assert lib.trmc_stream_set_packed_forcing(*args()) == _lib.TRMC_ESTATE and "a stream of windows is in progress" in err()
        p.stream_end()
        # two variables declared
        assert lib.trmc_stream_set_packed_forcing(*args()) == _lib.TRMC_OK
        p.upload_forcing(NSTEPS, np.zeros((NSEG, NQ), np.float32), q0)
        p.stream_begin(NSTEPS, QTS)
        assert push(None, day["raw_b"]) == _lib.TRMC_EINVAL and "raw_a is NULL" in err()
        assert push(day["raw_a"], None) == _lib.TRMC_EINVAL and "declared with two variables" in err() and "raw_b is NULL" in err()
        sd.nq = NQ + 1
        assert push(day["raw_a"], day["raw_b"]) == _lib.TRMC_EINVAL and "every day of a stream has the forcing columns of the first (4)" in err()
        sd.nq = NQ
        sd.qlat = day["raw_a"].ctypes.data
        assert push(day["raw_a"], day["raw_b"]) == _lib.TRMC_EINVAL and "qlat must be NULL" in err()
        sd.qlat = None
        assert lib.trmc_stream_push_day_packed(p._h, None, _lib.ptr(day["raw_a"]), _lib.ptr(day["raw_b"])) == _lib.TRMC_EINVAL and "day is NULL" in err()
        assert p.stream_info()["days_pushed"] == 0                          # (a refused push leaves nothing behind)
        assert push(day["raw_a"], day["raw_b"]) == _lib.TRMC_OK
        p.stream_end()
        # one variable declared
        assert lib.trmc_stream_set_packed_forcing(*args(b=None)) == _lib.TRMC_OK
        p.upload_forcing(NSTEPS, np.zeros((NSEG, NQ), np.float32), q0)
        p.stream_begin(NSTEPS, QTS)
        assert push(day["raw_a"], day["raw_b"]) == _lib.TRMC_EINVAL and "declared with one variable" in err() and "raw_b must be NULL" in err()
        single = pinned_like(one["raw_a"])                                  # (alive until the stream has ended)
        assert push(single, None) == _lib.TRMC_OK
        p.stream_end()
        # withdrawn: by nfeat = 0 and by feat_of_row = NULL
        for withdrawn in (args(n=0), (p._h, nfeat, None, _lib.ptr(pa), None)):
            assert lib.trmc_stream_set_packed_forcing(*args(b=None)) == _lib.TRMC_OK
            assert lib.trmc_stream_set_packed_forcing(*withdrawn) == _lib.TRMC_OK
            p.upload_forcing(NSTEPS, np.zeros((NSEG, NQ), np.float32), q0)
            p.stream_begin(NSTEPS, QTS)
            assert push(day["raw_a"], None) == _lib.TRMC_ESTATE and "without the declaration" in err()
            p.stream_end()
    # the dataflow engine runs no stream
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="flow") as p:
        rc = lib.trmc_stream_set_packed_forcing(p._h, nfeat, _lib.ptr(feat), _lib.ptr(pa), _lib.ptr(pb))
        assert rc == _lib.TRMC_EINVAL and "a stream of windows runs on the level engine" in err()
        with pytest.raises(ValueError, match="level engine"):
            p.stream_set_packed_forcing(days[0], ids)
