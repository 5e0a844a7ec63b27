"""THE LIFETIME OF A PLAN'S DEVICE RESOURCES (csrc/dev_owner.hpp; trmc_plan, PlanShared, StreamRun): a plan, its clones and the
clones of its clones closed in every order; trmc_plan_set_lag's refusals around clones; row sets past a reallocation of their
vector; a plan that has made every lazily made stream, event and buffer, and one closed in the middle of a stream of days.

Every comparison is bit for bit against a FRESHLY CREATED plan routing the same inputs (`fresh`, computed once per timestep
mode), never against the plan under test.  Nothing here reads the device's free memory: that number is device-wide;
tests/test_dev_owner_host.py is the leak check."""
import functools

import numpy as np
import pytest

import test_gpu_stream_reservoir_da as SR
import test_gpu_window_api as WA
from troute_amd import _lib
from troute_amd.plan import RoutingPlan
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

NSEG, NSTEPS, QTS = 300, 24, 12
TILES = {"wide_min_rows": 16, "wide_k": 8}            # a level-engine plan whose leading levels run as tiles on their own stream
CLUSTERS = {"cluster_rows": 8, "wide_min_rows": 3, "wide_k": 4}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def net():
    return WA.small_forest(seed=5, nseg=NSEG)


@functools.lru_cache(maxsize=None)
def fresh(short, days=1):
    """(fvd of the last day, final state) of `days` consecutive windows with the same forcing on a freshly created plan"""
    _, _, up_ptr, up_idx, p, qlat, q0 = net()
    with RoutingPlan(up_ptr, up_idx, p) as ref:
        for d in range(days):
            fvd = ref.route(NSTEPS, QTS, short, qlat, q0 if d == 0 else None)
        out = fvd.copy(), ref.download_final_state().copy()
    for a in out:
        a.setflags(write=False)
    return out


def routes_like_fresh(plan, short):
    _, _, _, _, _, qlat, q0 = net()
    got = plan.route(NSTEPS, QTS, short, qlat, q0)
    return np.array_equal(bits(got), bits(fresh(short)[0]))


def new_plan(engine="auto", short=None, options=None):
    _, _, up_ptr, up_idx, p, _, _ = net()
    return RoutingPlan(up_ptr, up_idx, p, assume_short_ts=short, engine=engine, options=options)


@pytest.mark.parametrize("engine", ["flow", "levels"])
@pytest.mark.parametrize("short", [True, False])
@pytest.mark.parametrize("order", ["abc", "cba", "bac"])
def test_a_plan_its_clone_and_the_clone_of_the_clone_closed_in_any_order(order, short, engine):
    """after every close, each plan that is left routes a window: the shared static data lives as long as any of them"""
    a = new_plan(engine)
    b = a.clone()
    c = b.clone()                                            # a clone of a clone
    left = {"a": a, "b": b, "c": c}
    for name in order:
        left.pop(name).close()
        for other, pl in left.items():
            assert routes_like_fresh(pl, short), (order, name, other)
    assert not left


def test_set_lag_is_refused_around_clones_as_it_always_was():
    refusal = r"set the lag before cloning the plan \(a clone shares the lag table\)"
    none = np.zeros(NSEG, np.int32)
    a = new_plan()
    a.set_lag(none)
    b = a.clone()
    c = a.clone()
    for lag in (none, None):
        for pl in (a, b, c):
            with pytest.raises(RuntimeError, match=refusal):  # an original with a live clone; a clone
                pl.set_lag(lag)
    c.close()
    with pytest.raises(RuntimeError, match=refusal):          # (one clone is still alive)
        a.set_lag(none)
    assert routes_like_fresh(a, True) and routes_like_fresh(a, False)
    d = b.clone()
    b.close()
    d.close()
    a.set_lag(none)                                           # accepted again: no clone is left
    a.set_lag(None)
    assert routes_like_fresh(a, True) and routes_like_fresh(a, False)
    b = a.clone()
    c = a.clone()
    a.close()
    c.close()
    with pytest.raises(RuntimeError, match=refusal):          # a clone, even when the original and its siblings are gone
        b.set_lag(none)
    assert routes_like_fresh(b, True) and routes_like_fresh(b, False)
    b.close()


@pytest.mark.parametrize("short", [True, False])
def test_five_row_sets_on_one_plan(short):
    """(their vector of device buffers grows by moving them)"""
    rng = np.random.default_rng(9)
    sets = [rng.choice(NSEG, size=n, replace=False) for n in (7, 1, 64, 33, 120)]
    want = fresh(short)[0]
    with new_plan() as p:
        ids = [p.rowset(rows) for rows in sets]
        assert ids == list(range(5))
        assert routes_like_fresh(p, short)
        for k in (0, 4):
            assert np.array_equal(bits(p.download_fvd(rowset=ids[k])), bits(want[sets[k]])), k
            assert np.array_equal(bits(p.gather_flow_rows(sets[k])), bits(want[sets[k], :, 0])), k


def test_a_plan_that_has_made_every_lazily_made_resource_closes_cleanly():
    _, _, _, _, _, qlat, q0 = net()
    # one plan: tiles on their own stream, an asynchronous fetch with an output stride, the window's summary and Courant summary,
    # a clone, and the state handed over in both directions
    a = new_plan("levels", True, TILES)
    rs = a.rowset(np.arange(0, NSEG, 7))
    a.set_output_stride(4)
    a.upload_forcing(NSTEPS, qlat, q0)
    a.route_device(NSTEPS, QTS, True)
    a.fetch_begin(rs, True, output_stride=4)
    hyd, state, dec = a.fetch_wait()
    want, want_state = fresh(True)
    assert np.array_equal(bits(hyd), bits(want[::7, :, 0])) and np.array_equal(bits(state), bits(want_state))
    assert np.array_equal(bits(dec), bits(want[:, 3::4]))
    a.set_output_stride(0)
    assert np.array_equal(a.window_summary(("peak",))["peak_flow"], want[:, :, 0].max(axis=1))
    assert a.window_courant_summary()["peak_cn"].shape == (NSEG,)
    b = a.clone()
    day = pinned_like(qlat)
    a.upload_forcing(NSTEPS, qlat, q0)
    a.route_begin(NSTEPS, QTS, True)
    a.route_advance(NSTEPS)
    b.stage_forcing(NSTEPS, day)
    b.chain_from(a)
    b.route_begin(NSTEPS, QTS, True)
    b.route_advance(NSTEPS)
    a.route_end()
    a.stage_forcing(NSTEPS, day)
    a.chain_from(b)                                          # ... and back
    a.route_begin(NSTEPS, QTS, True)
    a.route_advance(NSTEPS)
    b.route_end()
    a.route_end()
    want3, want_state3 = fresh(True, days=3)
    assert np.array_equal(bits(a.download_fvd()), bits(want3)) and np.array_equal(bits(a.download_final_state()), bits(want_state3))
    a.close()
    b.close()
    # a plan in cluster order: a stream of two days with a summary, its totals and reservoir data assimilation, to stream_end
    c = SR.case()
    nres = len(c.lakes)
    with SR.open_plan(c, True, 4) as p:
        SR.declare(p, c)
        p.stream_set_summary(("peak", "mean", "total"))
        p.upload_forcing(SR.NSTEPS, c.days[0], c.q0)
        p.stream_begin(SR.NSTEPS, c.qts, reservoir_da=True)
        keep = []
        for d in range(2):
            dest = (_lib.result_empty((c.n,), np.float32, always_pinned=True), _lib.result_empty((c.n,), np.int32, always_pinned=True),
                    _lib.result_empty((c.n,), np.float32, always_pinned=True))
            st = (_lib.result_empty((nres, 4), np.float32, always_pinned=True), _lib.result_empty((nres,), np.int32, always_pinned=True))
            keep.append((dest, st))
            assert p.stream_push(pinned_like(c.days[d]), reservoir_da=SR.day_tables(c, d), reservoir_da_state=st, summary=dest) == d
        p.stream_flush()
        for d in range(2):
            p.stream_wait(d)
        assert np.isfinite(keep[1][0][0]).all() and keep[1][0][1].min() >= 1
        p.stream_end()
    with new_plan() as after:
        assert routes_like_fresh(after, True) and routes_like_fresh(after, False)


def test_a_plan_closed_in_the_middle_of_a_stream_of_days():
    _, _, _, _, _, qlat, q0 = net()
    p = new_plan("levels", True, CLUSTERS)
    p.upload_forcing(NSTEPS, qlat, q0)
    p.stream_begin(NSTEPS, QTS, full_output=True)
    outs = [_lib.result_empty((NSEG, NSTEPS, 3), np.float32, always_pinned=True) for _ in range(2)]
    days = [pinned_like(qlat), pinned_like(qlat)]
    for d in range(2):
        assert p.stream_push(days[d], fvd=outs[d]) == d
    p.stream_flush()
    for d in range(2):
        p.stream_wait(d)
    assert np.array_equal(bits(outs[0]), bits(fresh(True)[0])) and np.array_equal(bits(outs[1]), bits(fresh(True, days=2)[0]))
    p.close()                                                # (no stream_end: the plan takes the stream's state with it)
    with new_plan() as after:
        assert routes_like_fresh(after, True) and routes_like_fresh(after, False)
