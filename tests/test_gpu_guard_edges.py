"""The fp32 step's range-proved arithmetic AT the edges of its guards, through every kernel that carries the step -- needs an MI355X.

The shortened quotients, square root and power (csrc/dev_math.inc, DevMathF) stand on three guards: params_sane once per plan,
fast_ok per hydraulic point, coef_guard per forcing value; where one fails the kernels take the plain operations -- "slower,
never other bits".  tests/guard_edges.py builds inputs ON the bounds, one unit in the last place either side and far outside,
and tests/test_guard_edges_cpu.py shows (without a GPU) that they are where they are meant to be.  Here they are routed:

  single steps  k_segments, fp32 and fp64 -- coef_guard and div4 only: that entry point never sets `sane`
  networks      k_mc_flow, k_mc_step, k_mc_tile (one tier and two), k_mc_ctile without and below slices, both timestep modes
                where the engine has both; classes interleaved in row order (a wavefront holds several: the general body) and
                one class per plan (the uniform in-bank body); the forcing class of a row changes between consecutive columns
                through every ordered pair of classes; rows that enter the retry branch of the secant loop
  the stream    three days through RouteStream, products only (the lazy-velocity kernels) and with the full result
  one ulp out   one row of 65 one unit outside one bound of params_sane: the plan's fallback to the plain operations

Every comparison is bit for bit against the plain-division oracle (oracle.network_by_segment(det=True); the float64 oracle for
fp64), over every row the oracle leaves finite -- all of them, for these inputs; the cap of 1 % is the CPU test's."""
import numpy as np
import pytest

import guard_edges as G
import helpers as H
from oracle import oracle as O
from test_gpu_parity import ENGINES, assert_bit_identical
from test_gpu_parity import set_engine as set_parity_engine
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, segments
from troute_amd.sequence import RouteStream

pytestmark = pytest.mark.gpu

CLUSTER_ENGINES = ["levels-clusters", "levels-slices+clusters"]
# (engine, short): both timestep modes for the four engines of test_gpu_parity.py, short timesteps for the plans in cluster order
CASES = [(e, s) for e in ENGINES for s in (True, False)] + [(e, True) for e in CLUSTER_ENGINES]


def choose_engine(engine, monkeypatch):
    if engine in CLUSTER_ENGINES:
        H.set_engine(engine, monkeypatch)
    else:
        set_parity_engine(monkeypatch, engine)


def compare(got, want, what):
    """bit for bit on every row the oracle leaves finite; at most 1 % of the rows may be excluded, and there the device must be
    non-finite too"""
    fin = np.isfinite(want).all(axis=(1, 2))
    assert fin.mean() >= 0.99, what
    assert_bit_identical(np.ascontiguousarray(got[fin]), np.ascontiguousarray(want[fin]), what)
    assert (np.isfinite(got).all(axis=(1, 2)) == fin).all(), what


def route(fx, short, precision=32, check=None, known_mode=False):
    """known_mode: the plan is told its timestep mode when it is created -- what puts it in cluster order (helpers.set_engine)"""
    with RoutingPlan(fx.up_ptr, fx.up_idx, fx.params, precision=precision, assume_short_ts=short if known_mode else None) as plan:
        got = plan.route(fx.nsteps, fx.qts, short, fx.qlat, fx.q0)
        if check:
            check(plan)
    return got


def path_check(engine, short, nsteps):
    """the rows really went through the kernels the case is about"""
    def check(plan):
        stats = plan.stats()
        if engine in CLUSTER_ENGINES:
            H.cluster_stats(stats, engine, nsteps)
        elif engine in ("levels-wide", "levels-mid") and short:
            assert plan.engine == "levels" and stats["wide_levels"] > 0 and stats["wide_segment_steps"] > 0, stats
        else:
            assert plan.engine == engine.split("-")[0]
    return check


# ---- single steps ---------------------------------------------------------------------------------------------------------
def compare_steps(got, want, what):
    """every element the oracle leaves finite bit for bit, the same elements non-finite (the unguarded Courant outputs of a dry
    result or of ncc == 0); the step's own four outputs are finite on every row (the CPU test)"""
    fin = np.isfinite(want)
    assert fin[:, [0, 1, 2, 5]].all()
    assert np.array_equal(np.isfinite(got), fin), what
    assert_bit_identical(np.where(fin, got, 0).astype(got.dtype), np.where(fin, want, 0).astype(want.dtype), what)


def test_directed_single_steps_fp32():
    x, _ = G.single_steps()
    got, iters = segments(x, with_iterations=True)
    want, want_iters = O.segments(x, return_iters=True, det=True)
    print(f"{x.shape[0]} steps, {int((want_iters > 100).sum())} in the retry branch")
    compare_steps(got, want, "directed single steps vs the oracle")
    assert np.array_equal(iters, want_iters) and (iters > 100).any()
    if O.have_ref("libmc_ref_qj0_f32.so"):
        compare_steps(got, O.ref_segments(x), "directed single steps vs the reference Fortran")


def test_directed_single_steps_fp64():
    x = G.single_steps()[0].astype(np.float64)
    got = segments(x)
    compare_steps(got, O.segments(x), "fp64 directed single steps vs the oracle")
    if O.have_ref("libmc_ref_qj0_f64.so"):
        compare_steps(got, O.ref_segments(x), "fp64 directed single steps vs the reference Fortran (-fdefault-real-8)")


# ---- networks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine,short", CASES)
def test_interleaved_classes_on_every_engine(engine, short, monkeypatch):
    """every forcing class and every ordered change of class between columns, the depths on fast_ok's bounds and at the bank's
    edge, the parameters on the bounds of params_sane and the rows of the retry branch, interleaved in row order"""
    choose_engine(engine, monkeypatch)
    fx = G.interleaved(0)
    got = route(fx, short, check=path_check(engine, short, fx.nsteps), known_mode=engine in CLUSTER_ENGINES)
    compare(got, fx.oracle(short)[:, 1:, :], f"interleaved engine={engine} short={short}")


@pytest.mark.parametrize("name", G.UNIFORM_CLASSES)
@pytest.mark.parametrize("engine,short", CASES)
def test_one_class_per_plan_on_every_engine(engine, short, name, monkeypatch):
    """every row in bank, inside fast_ok's range and of one forcing class: the uniform in-bank body, under one verdict of
    coef_guard for the whole plan (on the bound: pass; one unit below it, negative: fail; the clamped negative loss: pass)"""
    choose_engine(engine, monkeypatch)
    fx = G.uniform(name)
    got = route(fx, short, check=path_check(engine, short, fx.nsteps), known_mode=engine in CLUSTER_ENGINES)
    compare(got, fx.oracle(short)[:, 1:, :], f"uniform {name} engine={engine} short={short}")


def test_interleaved_classes_fp64():
    fx = G.interleaved(0)
    got = route(fx, True, precision=64)
    compare(got, np.ascontiguousarray(fx.oracle(True, 64)[:, 1:, :]), "interleaved fp64")


def test_cost_collection_marks_the_over_bank_rows(monkeypatch):
    """cost = the sum over the steps of min(iterations, 3) + 4 per step that evaluated the compound channel: a row whose census
    says over bank at the start of k solved steps carries at least 4 k; a row whose bank is never reached carries no such 4"""
    choose_engine("levels", monkeypatch)
    fx = G.interleaved(0)
    res = fx.oracle(True)
    flags = G.census_flags(fx.params, fx.qlat, fx.q0, res, fx.qts)
    k = (flags["over-bank"] & flags["flow"]).sum(axis=1)
    with RoutingPlan(fx.up_ptr, fx.up_idx, fx.params) as plan:
        plan.collect_cost(True)
        got = plan.route(fx.nsteps, fx.qts, True, fx.qlat, fx.q0)
        cost, n = plan.download_cost()
    compare(got, res[:, 1:, :], "cost collection on")
    assert n == fx.nsteps and (k > 0).sum() >= 8
    assert (cost.astype(np.int64) >= 4 * k).all()
    never = G.bankfull(fx.params) > np.float32(1e5)               # (bw > tw, and the rows whose bank is at 5e5)
    assert never.sum() >= 8 and (k[never] == 0).all() and (cost[never] <= 3 * fx.nsteps).all()


# ---- the stream of days ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_three_days_as_a_stream(full):
    """the interleaved fixture as three days through one RouteStream -- products only (velocities formed lazily) and with the
    full result -- against the reference's day-by-day loop; a row's forcing class changes from day to day as well"""
    fxs = [G.interleaved(d) for d in range(3)]
    fx = fxs[0]
    days = [f.qlat for f in fxs]
    r = ShardedRouter(fx.to, fx.params, stream=True, options={"wide_min_rows": 64, "wide_k": 8})
    _, W, C = r.plan0.lags()
    assert C + W > 0                     # (a plan in cluster order: the days run as tile launches)
    got = {}
    with RouteStream(r, fx.nsteps, fx.qts, full_output=full) as rs:
        for item in rs.route(iter(days), fx.q0):
            got[item[0]] = tuple(None if x is None else np.array(x, copy=True) for x in item[1:])
        rows = np.array(rs.outlet_rows, copy=True)
    r.close()
    assert sorted(got) == [0, 1, 2]
    for d, (q, state, _) in enumerate(H.reference_day_by_day(fx.to, fx.params, days, fx.q0, fx.nsteps, fx.qts)):
        assert np.isfinite(q).all() and np.isfinite(state).all()
        assert_bit_identical(got[d][0], np.ascontiguousarray(q[rows, 1:]), f"day {d}: outlet hydrographs")
        assert_bit_identical(got[d][1], state, f"day {d}: final state of every row")
        if full:
            assert_bit_identical(np.ascontiguousarray(got[d][2][:, :, 0]), np.ascontiguousarray(q[:, 1:]), f"day {d}: every flow")
            assert_bit_identical(np.ascontiguousarray(got[d][2][:, -1, 2]), np.ascontiguousarray(state[:, 2]), f"day {d}: last depth")
            if d == 0:
                compare(got[d][2], fx.oracle(True)[:, 1:, :], "day 0: every (q, v, d)")


# ---- one unit in the last place outside params_sane --------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["flow", "levels"])
@pytest.mark.parametrize("name,side", G.OUTSIDE_CASES)
def test_one_row_one_ulp_outside_one_bound(name, side, engine, monkeypatch):
    """65 rows, row 32 one unit in the last place outside one bound: the plan takes the plain operations, with the oracle's bits;
    and every row that is not the row itself or downstream of it has the bits of the twin plan whose row 32 sits ON the bound
    (the short forms)"""
    set_parity_engine(monkeypatch, engine)
    out, twin = G.outside(name, side), G.outside(name, side, inside=True)
    same = np.ones(G.OUTSIDE_NSEG, dtype=bool)
    same[G.OUTSIDE_ROW] = False
    same[out.downstream_of(G.OUTSIDE_ROW)] = False
    for short in (True, False):
        got_out, got_twin = route(out, short), route(twin, short)
        compare(got_out, out.oracle(short)[:, 1:, :], f"{name} {side} outside, short={short}")
        compare(got_twin, twin.oracle(short)[:, 1:, :], f"{name} {side} on the bound, short={short}")
        assert_bit_identical(np.ascontiguousarray(got_out[same]), np.ascontiguousarray(got_twin[same]), "rows not downstream of it")
