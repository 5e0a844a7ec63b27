"""The NaN case of tests/nonfinite_cases.py is what it is meant to be -- shown on the CPU oracle, without a GPU.

tests/test_gpu_products_nonfinite.py routes this case on the device and compares every product with the oracle's; here the oracle
alone shows that the case holds the classes it names, where they are wanted: every class at least three times among the wide
slices and three times among the cluster tiles of the plan of ``OPTIONS``, at most a quarter of the rows ever NaN, the rest of the
network with ordinary peaks inside the window, at least half of the planted rows with a number at the last step, and the planted
NaN on every edge the reducers have.  ``classify``'s consequences of the header's promises (``promised_peak``) are checked against
the transcription of its three-line rule (``rule_peak``).  Run with -s to see the census."""
import numpy as np
import pytest

import nonfinite_cases as N

# (nsteps, the summary's chunk): 24 and 3 C + 1 steps of the routing tests, 3 C + VE of the wide loads; C = 32 in fp32, 16 in fp64
WINDOWS = {32: [(24, 32), (97, 32), (100, 32)], 64: [(24, 16), (49, 16), (52, 16)]}
CASES = [(p, n, c, s) for p in (32, 64) for n, c in WINDOWS[p] for s in (True, False)]


def check(case, x, what, day=None):
    """x [rows, n, 3] = the oracle's (q, v, d)"""
    n, T = x.shape[:2]
    labels = {k: N.classify(np.ascontiguousarray(x[:, :, col]), day) for k, col in (("q", 0), ("d", 2), ("v", 1))}
    classes = N.STREAM_CLASSES if day else N.WINDOW_CLASSES
    for k, lab in labels.items():
        cen = N.census(lab, case.in_slices)
        print(what, k, " ".join(f"{c}:{a}+{b}" for c, (a, b) in cen.items()))
        for c in classes:
            assert c in cen and min(cen[c]) >= 3, (what, k, c, cen.get(c))                 # three in the slices, three in the tiles
        wrong = [(r, case.intended[r], lab[r]) for r in case.planted if lab[r] != case.intended[r]]
        assert not wrong, (what, k, wrong)
    ever = np.isnan(x).any(axis=(1, 2))
    assert 0 < ever.mean() <= 0.25, (what, ever.mean())
    assert np.all(ever[case.planted] == np.array([case.intended[r] != "I" for r in case.planted]))
    assert not x[case.dried].any()                                                         # the headwaters kept dry are dry
    assert 2 * np.sum(~np.isnan(x[case.planted, -1, 0])) >= case.planted.size, what        # a number at the last step
    for col in range(3):
        xc = np.ascontiguousarray(x[:, :, col])
        pk, at = N.rule_peak(xc)
        ppk, pat, nan_mean = N.promised_peak(xc)
        assert np.array_equal(at, pat), (what, col)
        assert np.array_equal(np.isnan(pk), np.isnan(ppk)) and np.array_equal(N.bits(pk)[~np.isnan(pk)], N.bits(ppk)[~np.isnan(pk)]), (what, col)
        assert np.array_equal(np.isnan(N.rule_mean(xc)), nan_mean), (what, col)
        clean = ~ever
        assert np.mean((at[clean] > 1) & (at[clean] < T)) >= 0.25, (what, col)            # ordinary peaks inside the window: a quarter
        for r in case.planted:                                                             # what each class is planted for
            c, v = case.intended[r], xc[r]
            if c in ("A", "G"):
                assert np.isnan(pk[r]) and at[r] == 1 and np.isfinite(v).any()
            elif c in ("B", "C", "D", "H"):
                f = int(np.argmax(np.isnan(v)))
                if f == 0:                                                                 # (H at step 1: the NaN stays, zeros behind it)
                    assert c == "H" and np.isnan(pk[r]) and at[r] == 1
                    continue
                assert np.isfinite(pk[r]) and pk[r] > 0 and ((at[r] - 1 > f) if c == "B" else (at[r] - 1 < f)), (what, col, r, c)
                if c == "D":
                    assert np.sum(N.bits(v) == N.bits(pk[r:r + 1])[0]) >= 2 and at[r] - 1 == int(np.argmax(v == pk[r]))
            elif c == "I":
                assert pk[r] == 0 and at[r] == 1
    steps = case.nan_steps | {1}
    edges = {1, N.K, N.K + 1, 8, 9, 10, case.chunk, case.chunk + 1, N.DAY, N.DAY + 1, T}
    assert {t for t in edges if t <= T} <= steps, (what, sorted(steps))
    q = np.ascontiguousarray(x[:, :, 0])
    assert np.array_equal(np.isnan(q[case.planted, [case.nan_step[r] - 1 for r in case.planted]]),
                          np.array([case.intended[r] != "I" for r in case.planted]))       # the NaN is where it was put
    return labels


@pytest.mark.parametrize("precision,nsteps,chunk,short", CASES)
def test_a_window_holds_every_class_where_it_is_wanted(precision, nsteps, chunk, short):
    case = N.case(nsteps, chunk)
    x = case.oracle(short, precision)
    assert x.dtype == {32: np.float32, 64: np.float64}[precision] and x.shape == (N.NSEG, nsteps, 3)
    check(case, x, f"fp{precision} {nsteps} steps short={short}")
    for col in range(3):                                                                   # the thresholds put a NaN in and between runs
        xc = np.ascontiguousarray(x[:, :, col])
        inside, between, _ = N.nan_in_runs(xc, N.thresholds(xc))
        assert inside >= 3 and between >= 3, (col, inside, between)


def test_a_shorter_window_is_the_head_of_a_longer_one():
    """the device tests route the first 24 steps of a longer case's forcing as well: the oracle's are the longer window's head"""
    case = N.case(97, 32)
    assert np.array_equal(N.bits(case.oracle(True, 32, 24)), N.bits(np.ascontiguousarray(case.oracle(True, 32)[:, :24])))


@pytest.mark.parametrize("precision", [32, 64])
def test_the_days_of_a_stream_hold_every_class_and_the_totals_tell_them_apart(precision):
    case = N.case(N.DAY * N.NDAYS, 32, stream=True)
    days = case.oracle_days(precision)
    x = np.concatenate([f for f, _ in days], axis=1)
    check(case, x, f"fp{precision} stream", day=N.DAY)
    q = np.ascontiguousarray(x[:, :, 0])
    pk = np.stack([N.rule_peak(np.ascontiguousarray(f[:, :, 0]))[0] for f, _ in days])
    F = np.array([r for r in case.planted if case.intended[r] == "F"])
    G = np.array([r for r in case.planted if case.intended[r] == "G"])
    assert np.isnan(pk[1, F]).all() and np.isfinite(pk[0, F]).all() and np.all(pk[2, F] < pk[0, F])    # the totals keep day 0
    assert np.isnan(pk[0, G]).all() and np.isfinite(pk[1:, G]).any(axis=0).all()                      # the totals stay NaN beside later numbers
    assert np.isnan(days[1][1][F]).all() and np.isnan(days[1][1][F][:, 2]).all()                       # a NaN state is handed on
    inside, between, (last, first) = N.nan_in_runs(q, N.thresholds(q), N.DAY)
    assert inside >= 3 and between >= 3 and last >= 2 and first >= 2, (inside, between, last, first)
    # np.maximum over the days' peaks is NOT the fold: it differs wherever a day's peak is NaN and the fold keeps a number
    fold = pk[0].copy()
    for d in (1, 2):
        m = pk[d] > fold
        fold[m] = pk[d][m]
    differs = N.bits(np.maximum.reduce(pk)) != N.bits(fold)
    assert differs[F].all() and not differs[~np.isnan(pk).any(axis=0)].any()
