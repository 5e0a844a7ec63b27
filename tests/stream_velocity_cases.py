"""TEST INFRASTRUCTURE of tests/test_gpu_stream_velocity.py (no GPU here): the forest and the five days of
tests/stream_courant_cases.py (``network()``, ``days_of()``: 301 rows, ten of fan-in 3, scales 1, 0.25, 6, 0.1, 2.5, six dry rows), a
per-row threshold table built from EXPECTED velocities, the numpy statement of the six figures and the census of what an
expectation holds.

``thresholds_of(v, K)``: K levels a row, each an ATTAINED value of the row's own series (``np.quantile(..., method="lower")``), so
that "equality is not over" is exercised at every row and level; at every fifth row one level -- the levels in turn -- is the row's
maximum itself, which no step is over.  ``rule_of(v, th)``: the window's rules over v [rows, steps] -- the peak and its step as
``window_summary``, the four figures as ``window_exceedance``.  ``census`` names the conditions."""
import numpy as np

from stream_courant_cases import NDAYS, QTS, as_one_window, days_of, network, oracle_cn   # noqa: F401  (the shared case)

QUANTILES = (0.5, 0.8, 0.95, 0.3)          # (not sorted: the levels of a row are independent of each other)
PARTS = ("steps_over", "first_step", "last_step", "longest_run")
KEYS = ("days", "peak_velocity", "peak_velocity_step") + PARTS


def thresholds_of(v, K):
    """[rows, K] in v's dtype, every entry a value the row attains; rows 0, 5, 10, ...: one level, the levels in turn, is the row's
    maximum"""
    v = np.ascontiguousarray(v)
    with np.errstate(invalid="ignore"):
        th = np.stack([np.nanquantile(v, q, axis=1, method="lower") for q in QUANTILES[:K]], axis=1).astype(v.dtype)
        top = np.arange(0, v.shape[0], 5)
        th[top, (top // 5) % K] = np.nanmax(v[top], axis=1)
    assert all(np.any(v[r] == th[r, k]) for r in range(0, v.shape[0], 7) for k in range(K))
    return np.ascontiguousarray(th)


def peak_of(v):
    """(peak, 1-based step int64): pk = v[1]; t = 2..: if (v[t] > pk) -- a NaN never replaces a number, a NaN at step 1 stays"""
    v = np.ascontiguousarray(v)
    pk, at = v[:, 0].copy(), np.ones(v.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, v.shape[1]):
            m = v[:, t] > pk
            pk[m] = v[m, t]
            at[m] = t + 1
    return pk, at


def rule_of(v, th=None):
    """the six figures over v [rows, steps] as a dict in ``KEYS``' order without "days" (th None: the peak and its step only)"""
    pk, at = peak_of(v)
    out = {"peak_velocity": pk, "peak_velocity_step": at}
    if th is None:
        return out
    n, T = v.shape
    K = th.shape[1]
    with np.errstate(invalid="ignore"):
        over = v[:, :, None] > th[:, None, :].astype(v.dtype)                   # [rows, steps, K]: false when either side is a NaN
    steps = np.arange(1, T + 1, dtype=np.int64)[None, :, None]
    cnt = over.sum(axis=1).astype(np.int64)
    first = np.where(over.any(axis=1), np.where(over, steps, T + 1).min(axis=1), 0).astype(np.int64)
    last = np.where(over, steps, 0).max(axis=1).astype(np.int64)
    run, best = np.zeros((n, K), np.int64), np.zeros((n, K), np.int64)
    for t in range(T):
        run = np.where(over[:, t, :], run + 1, 0)
        best = np.maximum(best, run)
    out.update(steps_over=cnt, first_step=first, last_step=last, longest_run=best)
    return out


def census(v, th, nsteps, routed=None):
    """the conditions the expectation v [rows, days * nsteps] and its table th must hold, asserted; returns the counts.  "A peak of
    0 at step 1" is a row that has had no flow yet: the dry headwaters all get water by day 3, so that condition is asserted over the
    first two days -- what a fetch in mid-stream reports."""
    n, T = v.shape
    routed = np.ones(n, bool) if routed is None else routed
    f = rule_of(v, th)
    pk, at = f["peak_velocity"], f["peak_velocity_step"]
    no_flow = (v == 0) & routed[:, None]
    dry_to_wet = no_flow[:, :-1] & (v[:, 1:] > 0)
    with np.errstate(invalid="ignore"):
        over = v[:, :, None] > th[:, None, :]
    edges = np.arange(nsteps, T, nsteps)                                            # (0-based index of a day's first step)
    across = (over[:, edges - 1, :] & over[:, edges, :]).any(axis=(1, 2))
    equal = (v[:, :, None] == th[:, None, :]).any(axis=1)                           # a level equal to an attained value
    rise, fall = v[:, 1:] > v[:, :-1], v[:, 1:] < v[:, :-1]
    later = np.zeros(n, bool)
    for r in np.flatnonzero(routed):
        up = np.flatnonzero(rise[r])
        if up.size == 0:
            continue
        dn = np.flatnonzero(fall[r][up[0]:])
        if dn.size == 0:
            continue
        first_max = up[0] + dn[0] + 1                                               # 1-based step of the first local maximum
        later[r] = (at[r] - 1) // nsteps > (first_max - 1) // nsteps
    pk2, at2 = peak_of(v[:, :2 * nsteps])
    c = {"no_flow": int(no_flow.sum()), "dry_to_wet": int(dry_to_wet.sum()),
         "run_across_a_days_end": int(across.sum()), "level_equals_an_attained_value": int(equal.sum()),
         "peak_on_a_days_first_step": int((routed & (at > 1) & ((at - 1) % nsteps == 0)).sum()),
         "peak_on_a_later_day": int(later.sum()),
         "peak_zero_at_step_one_after_two_days": int((routed & (pk2 == 0) & (at2 == 1)).sum())}
    for k in range(th.shape[1]):
        c[f"rows_over_level_{k}"] = int((f["steps_over"][routed, k] > 0).sum())
        c[f"rows_never_over_level_{k}"] = int((f["steps_over"][routed, k] == 0).sum())
    assert all(x > 0 for x in c.values()), c
    return c
