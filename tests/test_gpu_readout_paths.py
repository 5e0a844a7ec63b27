"""The read-out and upload calls of a plan at BOTH precisions and on BOTH engines: the strided and row-set downloads, the
asynchronous fetch (after a window, queued with a window, from the block a window decimated as it went), the row gathers, the
NaN screen of an upload, the packed forcing and the hand-over of a sequence on a plan and its clone.  Every comparison is bit
for bit and between two paths of the library or against a numpy slice of ``download_fvd()`` -- the plain copy of the result.
A network of 300 rows with three boundary rows, 25 steps: with stride 4 the window is no multiple of the stride, with 8 steps
per tile launch none of the tile either."""
import functools

import numpy as np
import pytest

import helpers as H
from troute_amd import _lib
from troute_amd.plan import RoutingPlan, csr_from_lists

pytestmark = pytest.mark.gpu

NSEG, NSTEPS, QTS, STRIDE = 300, 25, 12, 4
# (precision, engine): the dataflow engine runs precision-32 plans only
CASES = [(32, "levels"), (64, "levels"), (32, "flow")]
LEVEL_OPTIONS = {"wide_min_rows": 8, "wide_k": 8}          # leading levels in tiles of 8 steps, the rest one step per launch


@functools.lru_cache(maxsize=None)
def network(with_boundary):
    rng = np.random.default_rng(11)
    to = H.random_network(rng, NSEG)
    _, _, ups = H.reaches_from_to(to)
    up_ptr, up_idx = csr_from_lists(ups)
    p = np.stack([np.full(NSEG, 300.0), rng.uniform(300, 3000, NSEG), rng.uniform(1, 9, NSEG), np.zeros(NSEG), np.zeros(NSEG),
                  np.full(NSEG, 0.06), np.full(NSEG, 0.12), rng.uniform(0.2, 1.5, NSEG), rng.uniform(1e-3, 2e-2, NSEG)], 1)
    p[:, 3] = p[:, 2] * 5 / 3
    p[:, 4] = 3 * p[:, 3]
    qlat = rng.uniform(0, 0.4, (NSEG, 3)).astype(np.float32)
    q0 = rng.uniform(0, 1, (NSEG, 3)).astype(np.float32)
    heads = np.array([r for r in range(NSEG) if not ups[r] and to[r] >= 0], np.int64)
    bnd = np.sort(rng.choice(heads, 3, replace=False)) if with_boundary else np.zeros(0, np.int64)
    mask = np.zeros(NSEG, np.uint8)
    mask[bnd] = 1
    bf = rng.uniform(0.1, 2.0, (bnd.shape[0], NSTEPS, 3)).astype(np.float32)
    # unsorted, one row twice, a boundary row (if any), the first and the last row of the table
    rows = np.array([217, 5, NSEG - 1, 5, 0, 130] + bnd[:1].tolist(), np.int64)
    return up_ptr, up_idx, p.astype(np.float32), mask, qlat, q0, bf, rows


class Case:
    def __init__(self, precision, engine, with_boundary=True, **options):
        self.precision, self.engine = precision, engine
        self.dtype = np.float32 if precision == 32 else np.float64
        self.up_ptr, self.up_idx, self.params, self.mask, qlat, q0, bf, self.rows = network(with_boundary)
        self.qlat, self.q0 = qlat.astype(self.dtype), q0.astype(self.dtype)
        self.bf = bf.astype(self.dtype) if with_boundary else None
        self.options = dict(LEVEL_OPTIONS, **options) if engine == "levels" else (options or None)

    def plan(self):
        return RoutingPlan(self.up_ptr, self.up_idx, self.params, self.mask if self.bf is not None else None, precision=self.precision,
                           assume_short_ts=True, engine=self.engine, options=self.options)

    def route(self, plan):
        plan.upload_forcing(NSTEPS, self.qlat, self.q0, self.bf)
        plan.route_device(NSTEPS, QTS, True)


@pytest.fixture(params=CASES, ids=lambda c: f"fp{c[0]}-{c[1]}")
def case(request):
    return Case(*request.param)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def kept(full):
    """the steps k_decimate keeps: stride, 2 stride, ... counted from 1"""
    return full[:, STRIDE - 1::STRIDE][:, :NSTEPS // STRIDE]


def test_strided_and_rowset_downloads_equal_slices_of_the_result(case):
    with case.plan() as plan:
        case.route(plan)
        full = plan.download_fvd()
        assert full.shape == (NSEG, NSTEPS, 3) and np.isfinite(full).all()
        assert same(plan.download_fvd(STRIDE), kept(full))
        rs = plan.rowset(case.rows)
        assert same(plan.download_fvd(STRIDE, rs), kept(full[case.rows]))
        assert same(plan.download_fvd(1, rs), full[case.rows])


def blocking(plan, rows):
    return plan.gather_flow_rows(rows), plan.download_final_state(), plan.download_fvd(STRIDE)


def assert_fetched(got, want):
    assert len(got) == 3
    for g, w in zip(got, want):
        assert same(g, w)


def test_fetch_hands_over_what_the_blocking_calls_return(case):
    with case.plan() as plan:
        rs = plan.rowset(case.rows)
        case.route(plan)
        want = blocking(plan, case.rows)
        plan.fetch_begin(rs, True, STRIDE)                       # after a finished window
        assert_fetched(plan.fetch_wait(), want)
        if case.engine != "levels":
            plan.upload_forcing(NSTEPS, case.qlat, None, case.bf)
            plan.route_begin(NSTEPS, QTS, True)
            plan.route_advance(NSTEPS)
            with pytest.raises(RuntimeError, match="needs the level engine"):
                plan.fetch_begin(rs, True, STRIDE)
            plan.route_end()
            return
        for told, scale in ((0, 1.3), (STRIDE, 1.7)):           # queued WITH a window advanced to its end: from `out`, then from `dec`
            plan.set_output_stride(told)
            plan.upload_forcing(NSTEPS, case.qlat * case.dtype(scale), None, case.bf)
            plan.route_begin(NSTEPS, QTS, True)
            plan.route_advance(NSTEPS)
            plan.fetch_begin(rs, True, STRIDE)
            assert plan.route_end()["wide_levels"] > 0           # (the tiles ran: they are what writes `dec`)
            got = plan.fetch_wait()
            now = blocking(plan, case.rows)
            assert not same(now[2], want[2])                     # (another result than the window before)
            assert_fetched(got, now)
            want = now
        plan.fetch_begin(rs, True, STRIDE)                       # ... and from the `dec` a finished window left
        assert_fetched(plan.fetch_wait(), want)


def test_row_gathers_agree_with_the_result(case):
    with case.plan() as plan:
        case.route(plan)
        want = plan.download_fvd()[case.rows, :, 0]
        assert same(plan.gather_flow_rows(case.rows), want)
        plan.gather_flow_rows_resident(case.rows)
        assert same(plan.download_gathered(), want)


def test_nan_in_an_upload_routes_as_zero(case):
    rng = np.random.default_rng(5)
    qlat, q0 = case.qlat.copy(), case.q0.copy()
    at_q, at_s = rng.choice(qlat.size, 9, replace=False), rng.choice(q0.size, 7, replace=False)
    with case.plan() as plan:
        plan.set_nan_is_zero(True)
        qlat.flat[at_q] = 0
        q0.flat[at_s] = 0
        want = plan.route(NSTEPS, QTS, True, qlat, q0, case.bf)
        qlat.flat[at_q] = np.nan
        q0.flat[at_s] = np.nan
        got = plan.route(NSTEPS, QTS, True, qlat, q0, case.bf)
        assert np.isfinite(got).all() and same(got, want)
        assert not same(want, plan.route(NSTEPS, QTS, True, case.qlat, case.q0, case.bf))   # (the entries matter)


def test_packed_forcing_equals_the_unpacked_upload(case):
    from troute_amd import nhd_io
    rng = np.random.default_rng(8)
    nfeat, nq = NSEG + 40, 3
    feature_id = rng.permutation(np.arange(1000, 1000 + nfeat, dtype=np.int64))
    ids = feature_id[rng.permutation(nfeat)[:NSEG]].copy()
    ids[[3, 77, 250]] = 9                                         # rows the files do not hold: no forcing
    raw_a = rng.integers(0, 40000, (nq, nfeat)).astype(np.int32)
    raw_b = rng.integers(0, 20000, (nq, nfeat)).astype(np.int32)
    raw_a[0, rng.choice(nfeat, 20, replace=False)] = -999900000   # fill value
    raw_a[1, rng.choice(nfeat, 10, replace=False)] = 2000000001   # above valid_max
    raw_b[2, rng.choice(nfeat, 10, replace=False)] = -7           # below valid_min
    nan = float("nan")
    pk = {"feature_id": feature_id, "raw_a": raw_a, "raw_b": raw_b,
          "pack_a": np.array([float(np.float32(1e-5)), 0.0, -999900000.0, -999900000.0, 0.0, 2000000000.0]),
          "pack_b": np.array([float(np.float32(1e-5)), 0.0, nan, nan, 0.0, nan])}
    host = nhd_io.unpack_packed(pk)                               # float64 [nq, nfeat]
    where = {int(f): i for i, f in enumerate(feature_id)}
    qlat = np.zeros((NSEG, nq), np.float32)
    for r, f in enumerate(ids):
        if int(f) in where:
            qlat[r] = host[:, where[int(f)]].astype(np.float32)   # (the ingest's cast)
    with case.plan() as plan:
        want = plan.route(NSTEPS, QTS, True, qlat.astype(case.dtype), case.q0, case.bf)
        feat_of_row = plan.upload_forcing_packed(NSTEPS, pk, ids, case.q0, case.bf)
        assert (feat_of_row[[3, 77, 250]] == -1).all() and np.count_nonzero(feat_of_row < 0) == 3
        plan.route_device(NSTEPS, QTS, True)
        assert same(plan.download_fvd(), want)


@pytest.mark.parametrize("precision", [32, 64])
def test_second_day_on_a_clone_in_sequence_mode_equals_two_windows_on_one_plan(precision):
    """trmc_stage_forcing (its transpose right behind the copy) + trmc_plan_chain_from + a window on the clone, queued while the
    plan's own window may still run -- the second day of a plain two-window run."""
    plain, seq = Case(precision, "levels", with_boundary=False), Case(precision, "levels", with_boundary=False, sequence_mode=1)
    day1 = _lib.result_empty(plain.qlat.shape, plain.dtype, always_pinned=True)
    day1[...] = plain.qlat * plain.dtype(0.6)
    with plain.plan() as ref:
        plain.route(ref)
        ref.upload_forcing(NSTEPS, day1, None)
        ref.route_device(NSTEPS, QTS, True)
        want, want_state = ref.download_fvd(), ref.download_final_state()
    with seq.plan() as a:
        b = a.clone()
        rs = b.rowset(seq.rows)
        a.upload_forcing(NSTEPS, seq.qlat, seq.q0)
        a.route_begin(NSTEPS, QTS, True)
        a.route_advance(NSTEPS)
        b.stage_forcing(NSTEPS, day1)
        b.chain_from(a)
        b.route_begin(NSTEPS, QTS, True)
        b.route_advance(NSTEPS)
        b.fetch_begin(rs, True, STRIDE)
        a.route_end()
        b.route_end()
        hyd, state, dec = b.fetch_wait()
        assert same(b.download_fvd(), want)
        assert same(hyd, want[seq.rows, :, 0]) and same(state, want_state) and same(dec, kept(want))
        # ... and the plan's own next day from a forcing staged on it, behind the clone's window
        a.stage_forcing(NSTEPS, day1)
        a.chain_from(b)
        a.route_device(NSTEPS, QTS, True)
        with plain.plan() as ref:
            ref.upload_forcing(NSTEPS, day1, want_state)
            ref.route_device(NSTEPS, QTS, True)
            assert same(a.download_fvd(), ref.download_fvd())
        b.close()
