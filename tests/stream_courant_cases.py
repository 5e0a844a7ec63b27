"""TEST INFRASTRUCTURE of tests/test_gpu_stream_courant.py (no GPU here): a small forest under five days of forcing, the Courant
number the ORACLE gives for it, and the census of what that expectation holds.

The forest: ``helpers.random_network`` with 301 rows -- no multiple of 64 or of the block of 256, rows of fan-in 3.  The forcing:
``QTS`` = 12 steps to a column, every day a scale of one base pattern (a flood on day 2 that goes over bank, a smaller one on day 4,
recessions between them), the last column of days 0 and 1 raised so that rows below the headwaters peak on the first step of the
day after.  ``DRY`` headwaters start cold with no forcing: the step takes its no-flow branch and cn comes from the bracket of the
depth before; on day 1 half of them get water and go from dry to wet, the others on day 3 -- at the first step of days 1 to 3 these
take the no-flow branch from the flow and depth the day before left in time row 0, while the days whose slots follow in the ring end
with water in them.

``oracle_cn`` routes the days as ONE window with the oracle (oracle.network_by_segment), rebuilds every row-step's inputs from
its result as tests/test_gpu_window_courant.py does (``expected``: the reconstruction is proven there) and takes cn from the
reference Fortran's single-segment step.  ``census`` names the conditions; ``summary_of`` is the window's rule over cn."""
import functools

import numpy as np

import helpers as H
from oracle import oracle as O
from troute_amd.plan import csr_from_lists, topology_levels

NSEG, SEED = 301, 9
QTS, NDAYS = 12, 5
SCALE = (1.0, 0.25, 6.0, 0.1, 2.5)            # the days' forcing against the base pattern
LIMIT = 1.0                                   # cn > LIMIT at some rows and not at others (asserted by ``census``)
NDRY = 6


class Net:
    pass


@functools.lru_cache(maxsize=None)
def network():
    from test_gpu_parity import synth_inputs
    rng = np.random.default_rng(SEED)
    net = Net()
    net.to = H.random_network(rng, NSEG, p_junction=0.9, p_triple=0.3)   # (bushy: 15 levels, which a plan can route as slices alone)
    _, _, net.ups = H.reaches_from_to(net.to)
    net.up_ptr, net.up_idx = csr_from_lists(net.ups)
    net.params, qlat, q0 = synth_inputs(rng, NSEG, 4)
    net.level, _, _ = topology_levels(net.up_ptr, net.up_idx)
    net.fan = np.array([len(u) for u in net.ups])
    net.dry = np.flatnonzero(net.fan == 0)[:NDRY]
    net.base = qlat.astype(np.float32)
    net.q0 = q0.astype(np.float32)
    net.q0[net.dry] = 0
    net.bfd = (net.params[:, 3] - net.params[:, 2]) / (2 / net.params[:, 7])      # (tw - bw) / (2 z), z = 1 / cs
    return net


def day_of(d, nsteps):
    """the forcing of day d [NSEG, nq] for days of nsteps steps (fp32)"""
    net = network()
    nq = -(-nsteps // QTS)
    q = (net.base[:, :nq] * np.float32(SCALE[d % len(SCALE)])).astype(np.float32)
    if d < 2:
        q[:, -1] = q[:, -1] * np.float32(8)        # a pulse that ends with the day: the rows below crest on the next day's first step
    q[net.dry[::2]] = np.float32(0.4) if d >= 1 else 0   # the cold headwaters: dry through day 0, wet from day 1 on ...
    q[net.dry[1::2]] = np.float32(0.4) if d >= 3 else 0  # ... or dry through day 2: no flow at the first step of days 1, 2 and 3
    return np.ascontiguousarray(q)


def days_of(nsteps, ndays=NDAYS, dtype=np.float32):
    return [day_of(d, nsteps).astype(dtype) for d in range(ndays)]


def as_one_window(days):
    """the days' forcing side by side: the forcing of ONE window of len(days) * nsteps steps (nsteps a multiple of QTS, or a
    single day)"""
    return np.ascontiguousarray(np.concatenate(days, axis=1))


def summary_of(cn, limit):
    """the window's rule over cn [rows, steps]: (peak, 1-based step int64, steps over int64); a NaN never replaces a number, a
    NaN at step 1 stays, a NaN is not counted"""
    cn = np.ascontiguousarray(cn)
    pk, at = cn[:, 0].copy(), np.ones(cn.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, cn.shape[1]):
            m = cn[:, t] > pk
            pk[m] = cn[m, t]
            at[m] = t + 1
        over = (cn > cn.dtype.type(limit)).sum(axis=1).astype(np.int64)
    return pk, at, over


@functools.lru_cache(maxsize=None)
def oracle_cn(nsteps, ndays=NDAYS):
    """(cn [rows, ndays * nsteps] fp32, fvd [rows, ndays * nsteps, 3]) of the days routed by the oracle, cn from the reference
    Fortran's step at the rebuilt inputs of every row-step"""
    from test_gpu_window_courant import expected
    net = network()
    assert nsteps % QTS == 0
    qlat = as_one_window(days_of(nsteps, ndays))
    T = nsteps * ndays
    fvd = np.ascontiguousarray(O.network_by_segment(T, QTS, net.up_ptr, net.up_idx, net.level, net.params, net.q0, qlat, True, det=True)[:, 1:, :])
    want, _ = expected(fvd, net.q0, qlat, net.params, net.ups, QTS, True)
    cn = np.ascontiguousarray(want[:, :, 0])
    cn.setflags(write=False)
    fvd.setflags(write=False)
    return cn, fvd


def census(cn, fvd, q0, nsteps, limit, routed=None):
    """the conditions the expectation (cn, and the flows and depths fvd it was formed from) must hold, asserted; returns the counts"""
    net = network()
    n, T = cn.shape
    routed = np.ones(n, bool) if routed is None else routed
    q = np.concatenate([q0[:, :1].astype(fvd.dtype), fvd[:, :, 0]], axis=1)        # flows of steps 0..T
    d = fvd[:, :, 2]
    # a step that routed nothing leaves (0, 0, 0); a step with flow leaves a positive depth
    no_flow = (q[:, 1:] == 0) & (d == 0) & routed[:, None]
    dry_to_wet = no_flow[:, :-1] & ~no_flow[:, 1:] & (d[:, 1:] > 0)
    over_bank = (d > net.bfd[:, None].astype(d.dtype)) & routed[:, None]
    pk, at, over = summary_of(cn, limit)
    first_of_a_later_day = routed & (at > 1) & ((at - 1) % nsteps == 0)
    # a day's first step without flow while a later day ends with flow in the row: a stale time row 0 would change the branch
    starts = np.arange(nsteps, T, nsteps)
    carried_dry = no_flow[:, starts] & (q[:, -1] > 0)[:, None]
    # the first local maximum of a row: the first t with cn[t] > cn[t + 1] after a rise; the peak on a later DAY than that
    rise = cn[:, 1:] > cn[:, :-1]
    fall = cn[:, 1:] < cn[:, :-1]
    later = np.zeros(n, bool)
    for r in np.flatnonzero(routed):
        up = np.flatnonzero(rise[r])
        if up.size == 0:
            continue
        dn = np.flatnonzero(fall[r][up[0]:])
        if dn.size == 0:
            continue
        first_max = up[0] + dn[0] + 1                                              # 1-based step of the first local maximum
        later[r] = (at[r] - 1) // nsteps > (first_max - 1) // nsteps
    c = {"no_flow": int(no_flow.sum()), "dry_to_wet": int(dry_to_wet.sum()), "over_bank": int(over_bank.sum()),
         "rows_over": int((over[routed] > 0).sum()), "rows_never_over": int((over[routed] == 0).sum()),
         "peak_on_a_days_first_step": int(first_of_a_later_day.sum()), "peak_on_a_later_day": int(later.sum()),
         "no_flow_at_a_later_days_first_step": int(carried_dry.sum()), "fan3": int((net.fan == 3).sum())}
    assert all(v > 0 for v in c.values()), c
    return c
