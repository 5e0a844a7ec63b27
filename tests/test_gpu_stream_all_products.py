"""EVERY PRODUCT OF A STREAM DAY AT ONCE (csrc/stream.inc: the table of a day's products, stream_complete_day's one loop of copies).

Each product has a file of its own in which it is the only one asked for; the table that all of them share is exercised only when
several are live in one stream.  The network is the one of test_gpu_stream_summary's reservoir-and-gage test (RN.case(3000, 78):
level-pool reservoirs and gages in the slices and in the clusters), nsteps = 24 on a plan with wide_k = 4, slots + 2 days so that
every slot of the ring is used twice, in both precisions.

No oracle and no tolerance: both sides of every comparison are streams of the same kernels over the same inputs -- what is asked
for must not change a bit of what is handed over."""
import functools

import numpy as np
import pytest

import test_gpu_stream_reservoirs_nudging as RN
from troute_amd import _lib
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

NSTEPS, QTS, STRIDE = RN.NSTEPS, RN.QTS, 6
NDAYS_MAX = 12
SUMMARY = ("peak", "mean", "peak_depth", "total")
SUM_KEYS = ("peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step")
BASE = ("hyd", "final")
ALL = BASE + ("fvd", "nudge", "reservoir_inflow") + SUM_KEYS


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = (got, want) if got.dtype.kind == "i" else (RN.bits(got), RN.bits(want))
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


@functools.lru_cache(maxsize=None)
def inputs():
    c = RN.case(3000, 78, NDAYS_MAX)
    tabs, _ = RN.day_tables(c, NDAYS_MAX)
    # the hydrographs' row set: the tailwaters, the gages and the lakes -- rows of the slices and of the clusters, an odd number
    rows = np.unique(np.concatenate([np.flatnonzero(c.to < 0), c.gages, c.lakes]))
    rows = rows[:rows.shape[0] - 1 + rows.shape[0] % 2]
    assert rows.shape[0] % 2 == 1 and np.any(c.lag[rows] < c.W) and np.any(c.lag[rows] >= c.W)
    return c, tabs, rows


def open_plan(precision):
    c, _, rows = inputs()
    p = RN.open_plan(c, precision)
    p.set_reservoirs(c.lakes, c.par, RN.DT)
    p.stream_set_gages(c.gages)
    return p, p.rowset(rows)


def stream(p, rowset, ask, summary=None, output_stride=0, no_products_on=None, ndays=None, probe=None):
    """one stream on `p` that hands over the products named in `ask` (of ALL): ([{name: copy} per day], totals or None, days).
    ndays: default slots + 2.  no_products_on: a day pushed with no host destination at all.  probe: called right after
    stream_begin."""
    c, tabs, rows = inputs()
    dt = p.dtype
    p.stream_set_summary(summary)
    p.upload_forcing(NSTEPS, c.days[0].astype(dt), c.q0.astype(dt))
    p.stream_begin(NSTEPS, QTS, output_stride=output_stride)
    if probe is not None:
        probe(p)
    D = p.stream_info()["slots"]
    ndays = D + 2 if ndays is None else ndays
    assert D + 2 <= ndays <= NDAYS_MAX
    shapes = {"hyd": ((rows.shape[0], NSTEPS), dt), "final": ((c.n, 3), dt), "fvd": ((c.n, NSTEPS // STRIDE, 3), dt),
              "nudge": ((c.gages.shape[0], NSTEPS), dt), "reservoir_inflow": ((c.lakes.shape[0], NSTEPS), dt),
              "peak_flow": ((c.n,), dt), "peak_step": ((c.n,), np.int32), "mean_flow": ((c.n,), dt),
              "peak_depth": ((c.n,), dt), "peak_depth_step": ((c.n,), np.int32)}
    ring = [{k: _lib.result_empty(*shapes[k], always_pinned=True) for k in ask} for _ in range(D)]
    for r in ring:
        for a in r.values():
            a.view(np.uint8)[...] = 0xAB                      # (what a day leaves untouched would show)
    got = []

    def take(d):
        p.stream_wait(d)
        got.append(None if d == no_products_on else {k: np.array(v, copy=True) for k, v in ring[d % D].items()})
    for d in range(ndays):
        if d >= D:                                            # (the slot's last day leaves before its arrays are reused)
            if p.stream_info()["days_complete"] <= d - D:
                p.stream_flush()
            take(d - D)
        r = {} if d == no_products_on else ring[d % D]
        mode, a, w = tabs[d]
        sm = tuple(r.get(k) for k in SUM_KEYS[:5 if "peak_depth" in ask else 3])
        assert p.stream_push(pinned_like(c.days[d].astype(dt)), rowset=rowset if "hyd" in r else None, hyd=r.get("hyd"), q0=r.get("final"),
                             fvd=r.get("fvd"), nudging=(mode, a.astype(dt), w.astype(dt), c.usgs[d][:, 0]), nudge=r.get("nudge"),
                             reservoir_inflow=r.get("reservoir_inflow"), summary=sm if any(x is not None for x in sm) else None) == d
    p.stream_flush()
    total = p.stream_summary_total() if "total" in (summary or ()) else None
    for d in range(len(got), ndays):
        take(d)
    p.stream_end()
    return got, total, ndays


SMALL = ("final", "mean_flow")


@functools.lru_cache(maxsize=None)
def everything(precision):
    """the stream that asks for everything at once -> (days, totals, ndays) -- and, on the same plan right after it, a second
    stream with the summary ("mean",), no output_stride and no row set -> (days, what trmc_stream_summary_depth_dest answered)"""
    refused = []

    def probe(q):
        n = inputs()[0].n
        pd, ps = np.zeros(n, q.dtype), np.zeros(n, np.int32)
        refused.append(_lib.lib().trmc_stream_summary_depth_dest(q._h, _lib.ptr(pd), _lib.ptr(ps)))
    p, rs = open_plan(precision)
    with p:
        got, total, ndays = stream(p, rs, ALL, summary=SUMMARY, output_stride=STRIDE)
        second, _, _ = stream(p, rs, SMALL, summary=("mean",), ndays=ndays, probe=probe)
    return got, total, ndays, second, refused


@pytest.mark.parametrize("precision", [32, 64])
def test_all_products_together_equal_each_product_alone(precision):
    both, total, ndays = everything(precision)[:3]
    assert total["days"] == ndays and set(total) == set(SUM_KEYS) | {"days"}
    alone = [(BASE, None, 0), (BASE + ("fvd",), None, STRIDE), (BASE + ("nudge",), None, 0), (BASE + ("reservoir_inflow",), None, 0),
             (BASE + SUM_KEYS, SUMMARY, 0)]
    for ask, summary, stride in alone:
        p, rs = open_plan(precision)
        with p:
            one, one_total, n = stream(p, rs, ask, summary=summary, output_stride=stride, ndays=ndays)
        assert n == ndays
        for d in range(ndays):
            assert set(one[d]) == set(ask)
            for k in ask:                                     # (hydrographs and state: the common base of every stream)
                assert_same(both[d][k], one[d][k], (precision, ask[-1], d, k))
        if summary:
            assert set(one_total) == set(total)
            for k in SUM_KEYS:
                assert_same(total[k], one_total[k], (precision, "total", k))
    for d in range(ndays):                                    # (the products are there at all: nothing compared 0xAB with 0xAB)
        assert np.isfinite(both[d]["fvd"]).all() and both[d]["hyd"].max() > 0 and np.abs(both[d]["nudge"]).max() > 0
        assert both[d]["reservoir_inflow"].max() > 0 and both[d]["peak_depth"].max() > 0 and both[d]["peak_step"].min() >= 1


@pytest.mark.parametrize("precision", [32, 64])
def test_second_stream_with_a_smaller_mask_on_the_same_plan(precision):
    """after the stream with every summary part: summary=("mean",), no output_stride, no row set -- the buffers of the other parts
    are released, the stream has no peak depth to hand over, and its days are a fresh plan's"""
    both, _, ndays, second, refused = everything(precision)
    ask = SMALL
    assert refused == [_lib.TRMC_ESTATE]
    fresh_plan, fresh_rs = open_plan(precision)
    with fresh_plan:
        fresh, _, _ = stream(fresh_plan, fresh_rs, ask, summary=("mean",), ndays=ndays)
    for d in range(ndays):
        for k in ask:
            assert_same(second[d][k], fresh[d][k], (precision, d, k))
    # (and the mask alone moves no bit of the mean and of the state)
    for d in range(ndays):
        for k in ask:
            assert_same(second[d][k], both[d][k], (precision, "against the full mask", d, k))


@pytest.mark.parametrize("precision", [32, 64])
def test_a_day_without_any_host_destination(precision):
    """a day in the middle of the stream pushed with None everywhere: nothing goes to the copy stream for it, stream_wait on it
    returns, the days after it and the totals (which fold every day) are those of the stream that handed every day over"""
    both, total, ndays = everything(precision)[:3]
    quiet = ndays // 2
    p, rs = open_plan(precision)
    with p:
        got, got_total, _ = stream(p, rs, ALL, summary=SUMMARY, output_stride=STRIDE, no_products_on=quiet, ndays=ndays)
    assert got[quiet] is None and 0 < quiet < ndays - 1
    for d in range(ndays):
        if d != quiet:
            for k in ALL:
                assert_same(got[d][k], both[d][k], (precision, d, k))
    assert got_total["days"] == ndays
    for k in SUM_KEYS:
        assert_same(got_total[k], total[k], (precision, "total", k))
