"""TEST INFRASTRUCTURE: one small network whose forcing carries NaN, and the census of what the oracle makes of it (no GPU).

Every per-row product of the device is one ordered comparison (include/trmc.h):

    peaks        pk = x[1]; at = 1; for t = 2..n: if (x[t] > pk) { pk = x[t]; at = t; }
    exceedance   over(t) := x[t] > th

so the first of equal peaks wins, a NaN never replaces a number and a NaN at step 1 stays.  This module plants rows whose flow,
depth and velocity hold NaN and bit-equal maxima where the reducers can go wrong, and names what came out (``classify``).  All
values come from the oracle (oracle.network_by_segment), never from the code under test.

WHAT A NaN DOES IN THE ROUTING (the reference's semantics, which the oracle restates): a row with some input > 0 and a NaN among
its inputs gives NaN flow, depth and velocity; a row whose inputs are only NaN or 0 takes the no-flow branch (`x > 0` is false for a
NaN) and comes back as exactly (0, 0, 0).  A row without upstream flow therefore recovers from a NaN through one step of zero
forcing, and the next pulse from the dry state repeats an earlier pulse from the dry state bit for bit.

THE PLANTED ROWS are rows without upstream flow, forced column by column (qts = 1: a column is a step): headwaters -- level 0, which
the plan of ``OPTIONS`` routes as wide slices -- and rows of level 1 whose upstream rows (headwaters all) are kept dry, which makes
them headwaters in effect among the cluster tiles.  They are chosen so that their paths to the outlets share rows: at most a
quarter of the network ever holds a NaN.  The NaN of a planted row sits on a step of ``positions``: step 1, a tile's first and last
step (K = 4), the stream summary's groups of eight (8, 9, 10) and its scalar tail, a window chunk's last step and the next one,
the last step of a day and the first of the next, the window's last steps.

CLASSES (``classify``; a row has one for each of q, d, v -- the three agree on every planted row):
    A  NaN at step 1, numbers later: the peak is the NaN at step 1, the mean is NaN
    B  number, NaN, then a strictly greater number: the peak is the later one
    C  number, NaN, then only smaller numbers: the peak and its step stay before the NaN
    D  two bit-equal positive maxima separated by a NaN and a zero: the first wins
    E  NaN from some step to the end of the window
    H  a lone NaN followed by exact zeros
    I  zeros only: ties at zero
    F  (a stream of days) a whole day NaN while an earlier day has numbers: the totals keep the earlier day
    G  (a stream of days) NaN at step 1 of day 0: the totals stay NaN, step 1
    -  no NaN, not all zero;  ?  a NaN pattern none of the above names (rows below the planted ones)
"""
import functools

import numpy as np

import helpers as H
from oracle import oracle as O
from troute_amd.plan import csr_from_lists, topology_clusters, topology_levels

NSEG, SEED = 800, 5                                                  # (the smallest forest of these whose level 0 is a wide slice)
OPTIONS = {"cluster_rows": 64, "wide_min_rows": 200, "wide_k": 4}       # (the option set of the other product tests)
K = OPTIONS["wide_k"]
DAY, NDAYS = 24, 3                                                     # the stream: three days of 24 steps
PER_CLASS = 4                                                          # planted rows per class and layout (slices, cluster tiles)
WINDOW_CLASSES = ("A", "B", "C", "D", "E", "H", "I")
STREAM_CLASSES = ("G", "B", "C", "D", "E", "H", "I", "F")
NAN = np.float32(np.nan)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the rule and what the spec's text says follows from it ------------------------------------------------------------------
def rule_peak(x):
    """the three lines of include/trmc.h, transcribed: (peak, 1-based step) of x [rows, n]"""
    x = np.ascontiguousarray(x)
    pk, at = x[:, 0].copy(), np.ones(x.shape[0], np.int32)
    with np.errstate(invalid="ignore"):
        for t in range(1, x.shape[1]):
            m = x[:, t] > pk
            pk[m] = x[m, t]
            at[m] = t + 1
    return pk, at


def rule_mean(x):
    x = np.ascontiguousarray(x)
    return np.cumsum(x, axis=1, dtype=x.dtype)[:, -1] / x.dtype.type(x.shape[1])


def promised_peak(x):
    """(peak, step, mean-is-NaN) from the PROMISES the header draws from the rule, without its loop: a NaN at step 1 stays; else
    a NaN never replaces a number, so the peak is the largest number, and the first of equal ones wins; a mean over a NaN is NaN"""
    x = np.ascontiguousarray(x)
    n = x.shape[0]
    first_nan = np.isnan(x[:, 0])
    y = np.where(np.isnan(x), -np.inf, x)
    at = y.argmax(axis=1)                                               # (numpy: the first of equal maxima)
    pk = x[np.arange(n), at]
    at = np.where(first_nan, 0, at).astype(np.int32) + 1
    pk = np.where(first_nan, x.dtype.type(np.nan), pk).astype(x.dtype)
    return pk, at, np.isnan(x).any(axis=1)


def classify(x, day=None):
    """the class of every row of x [rows, n] (an array of one-letter strings); day: the steps of a stream day -- F and G are
    then looked for first"""
    x = np.ascontiguousarray(x)
    n, T = x.shape
    out = np.empty(n, dtype="<U1")
    nan = np.isnan(x)
    for r in range(n):
        v, m = x[r], nan[r]
        if not m.any():
            out[r] = "I" if not v.any() else "-"
            continue
        if day:
            days = m.reshape(-1, day)
            whole = days.all(axis=1)
            if m[0] and not m.all():
                out[r] = "G"
                continue
            if any(whole[d] and not days[:d].all() for d in range(1, len(whole))) and not whole[-1]:
                out[r] = "F"
                continue
        f = int(np.argmax(m))
        if m[f:].all():
            out[r] = "E"
        elif m.sum() == 1 and not v[f + 1:].any():
            out[r] = "H"
        elif f == 0:
            out[r] = "A"
        else:
            before, after = v[:f].max(), v[f + 1:][~m[f + 1:]].max()
            if after > before:
                out[r] = "B"
            elif after < before:
                out[r] = "C"
            else:
                a, b = int(np.argmax(v[:f] == before)), f + 1 + int(np.argmax(v[f + 1:] == before))
                between = v[a + 1:b]
                tie = before > 0 and bits(v[a:a + 1])[0] == bits(v[b:b + 1])[0] and np.isnan(between).any() and (between == 0).any()
                out[r] = "D" if tie else "?"
    return out


# ---- the network, its layout on the plan of OPTIONS, the planted rows ------------------------------------------------------------
class Net:
    pass


@functools.lru_cache(maxsize=None)
def network():
    from test_gpu_parity import synth_inputs
    rng = np.random.default_rng(SEED)
    net = Net()
    net.to = H.random_network(rng, NSEG)
    _, _, net.ups = H.reaches_from_to(net.to)
    net.up_ptr, net.up_idx = csr_from_lists(net.ups)
    net.params, _, q0 = synth_inputs(rng, NSEG, 1)
    net.q0 = np.maximum(q0, np.float32(0.01))                           # (every ordinary row carries water from the start)
    net.amp = rng.uniform(0.5, 2.0, NSEG).astype(np.float32)
    net.seed_ql = int(rng.integers(1 << 30))
    net.level, _, _ = topology_levels(net.up_ptr, net.up_idx)
    _, net.lag, blk, net.wide_levels, net.cluster_levels, _ = topology_clusters(
        net.up_ptr, net.up_idx, wide_min_rows=OPTIONS["wide_min_rows"], cluster_rows=OPTIONS["cluster_rows"])
    net.in_slices = blk < 0
    assert net.wide_levels > 0 and net.cluster_levels > 0, (net.wide_levels, net.cluster_levels)
    heads = np.array([len(u) == 0 for u in net.ups])
    assert np.all(net.in_slices[heads])
    # rows of the cluster tiles whose upstream rows are headwaters all: with those kept dry, headwaters in effect
    second = np.array([len(u) > 0 and all(heads[v] for v in u) and not net.in_slices[r] for r, u in enumerate(net.ups)])
    below = []
    for r in range(NSEG):
        path, d = [], net.to[r]
        while d >= 0:
            path.append(int(d))
            d = net.to[d]
        below.append(path)
    net.below = below
    return net, heads, second


def plant(nclasses):
    """rows for nclasses x PER_CLASS planted rows in the slices and as many in the cluster tiles, chosen one by one so that each
    adds the fewest rows to those below a planted row; returns (slice rows, tile rows, the headwaters kept dry above the latter)"""
    net, heads, second = network()
    want = nclasses * PER_CLASS
    dried = set()
    tainted = set()
    chosen = {True: [], False: []}
    for in_slices in (False, True):                                     # (the tile rows first: they dry headwaters up)
        while len(chosen[in_slices]) < want:
            best, cost = None, None
            for r in range(NSEG):
                if r in dried or r in tainted or r in chosen[True] or r in chosen[False]:
                    continue
                if in_slices and not heads[r] or not in_slices and not second[r]:
                    continue
                if not in_slices and any(u in chosen[True] or u in chosen[False] for u in net.ups[r]):
                    continue
                if any(b in chosen[False] for b in net.below[r]):     # (a planted row has no planted row above it)
                    continue
                c = len(set(net.below[r]) - tainted)
                if cost is None or c < cost:
                    best, cost = r, c
            assert best is not None, "no row left to plant"
            chosen[in_slices].append(best)
            tainted.update(net.below[best])
            if not in_slices:
                dried.update(net.ups[best])
    return chosen[True], chosen[False], sorted(dried)


def positions(n, chunk):
    """the steps (1-based) a planted NaN is put on in a window of n steps summarised in chunks of `chunk` steps"""
    p = {1, K, K + 1, 8, 9, 10, 17, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, DAY, DAY + 1, 2 * DAY, 2 * DAY + 1, 3 * chunk, 3 * chunk + 1,
         n - K, n - K + 1, n - 2, n - 1, n}
    return sorted(t for t in p if 1 <= t <= n)


RANGE = {"A": lambda n: (5, n), "B": lambda n: (2, n - 6), "C": lambda n: (3, n - 2), "D": lambda n: (2, n - 2), "E": lambda n: (1, n),
         "H": lambda n: (1, n - 1), "G": lambda n: (5, n)}


def pattern(cls, p, n, a):
    """(ql [n], wet) of a planted row of class cls whose NaN sits at step p (1-based); wet: the row starts with water (q0 > 0)"""
    ql = np.zeros(n, np.float32)
    i = p - 1
    wet = False
    if cls in ("A", "G"):                # NaN at step 1 with water in the channel, a zero, then numbers -- and a second NaN at p
        wet = True
        ql[0], ql[2:] = NAN, a
        ql[i] = NAN
        if i + 1 < n:
            ql[i + 1] = 0
    elif cls == "B":
        ql[:i], ql[i], ql[i + 2:] = 0.02 * a, NAN, 5 * a
    elif cls == "C":
        ql[:i], ql[i], ql[i + 2:] = 5 * a, NAN, 0.002 * a
    elif cls == "D":                     # a pulse from the dry state, the NaN, a zero, the same pulse, a NaN and zeros
        ql[i - 1], ql[i], ql[i + 2] = a, NAN, a
        if i + 3 < n:
            ql[i + 3] = NAN              # (no recession behind the second pulse: its depth and velocity would rise above the pulse's)
    elif cls == "E":
        wet = p == 1
        ql[:] = a
        ql[i] = NAN
    elif cls == "H":
        wet = p == 1
        ql[:i], ql[i] = a, NAN
    elif cls == "F":                     # day 0 numbers, day 1 NaN throughout, day 2 a zero and smaller numbers
        ql[:DAY], ql[DAY], ql[DAY + 1:2 * DAY], ql[2 * DAY + 1:] = a, NAN, a, 0.02 * a
    else:
        assert cls == "I", cls
        if p:
            ql[i] = NAN                  # (a dry row forced with a NaN takes the no-flow branch: zeros)
    return ql, wet


class Case:
    """inputs of one window (or of the days of a stream, concatenated in time) and what was planted where"""

    def oracle(self, short, precision=32, nsteps=None):
        """the oracle's (q, v, d) [rows, nsteps, 3] of the window's first nsteps steps (default: all), computed once"""
        return _oracle(self, bool(short), precision, nsteps or self.nsteps)

    def oracle_days(self, precision=32):
        """a stream's days routed one after the other, each from the state the one before left: [(fvd, state)]"""
        return _oracle_days(self, precision)

    def day(self, d):
        return np.ascontiguousarray(self.qlat[:, d * DAY:(d + 1) * DAY])


@functools.lru_cache(maxsize=None)
def _oracle(case, short, precision, nsteps):
    net = network()[0]
    dt = {32: np.float32, 64: np.float64}[precision]
    out = O.network_by_segment(nsteps, 1, net.up_ptr, net.up_idx, net.level, net.params.astype(dt), case.q0.astype(dt),
                               np.ascontiguousarray(case.qlat[:, :nsteps]).astype(dt), short, det=precision == 32)
    out = np.ascontiguousarray(out[:, 1:, :])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_days(case, precision):
    net = network()[0]
    dt = {32: np.float32, 64: np.float64}[precision]
    state, out = case.q0.astype(dt), []
    for d in range(case.nsteps // DAY):
        fvd = O.network_by_segment(DAY, 1, net.up_ptr, net.up_idx, net.level, net.params.astype(dt), state, case.day(d).astype(dt), True,
                                   det=precision == 32)
        fvd = np.ascontiguousarray(fvd[:, 1:, :])
        state = np.ascontiguousarray(np.stack([fvd[:, -1, 0], fvd[:, -1, 0], fvd[:, -1, 2]], 1))
        fvd.setflags(write=False)
        out.append((fvd, state))
    return out


@functools.lru_cache(maxsize=None)
def case(nsteps, chunk, stream=False):
    """the case of a window of nsteps steps summarised in chunks of `chunk` steps (32 in fp32, 16 in fp64:
    RoutingPlan.window_summary_tile); stream: the NDAYS days of a stream in a row, with F and G"""
    net = network()[0]
    classes = STREAM_CLASSES if stream else WINDOW_CLASSES
    assert not stream or nsteps == DAY * NDAYS
    sl, ti, dried = plant(len(classes))
    c = Case()
    c.nsteps, c.chunk, c.stream = nsteps, chunk, stream
    rng = np.random.default_rng(net.seed_ql)
    c.qlat = np.exp(rng.normal(np.log(5e-3), 1.5, (NSEG, nsteps))).astype(np.float32)       # ordinary rows: positive forcing
    c.q0 = net.q0.copy()
    c.qlat[dried] = 0
    c.q0[dried] = 0
    c.dried = np.array(dried)
    c.intended, c.nan_step = {}, {}
    pos = positions(nsteps, chunk)

    def span(cls):
        lo, hi = RANGE[cls](nsteps) if cls in RANGE else (1, nsteps)
        return (2 if stream and cls in ("E", "H") else lo), hi              # (step 1 of a stream is G's)
    takers = {t: sum(span(cls)[0] <= t <= span(cls)[1] for cls in classes) for t in pos}
    used = dict.fromkeys(pos, 0)
    c.nan_steps = set()
    for rows in (sl, ti):
        for k, r in enumerate(rows):
            cls = classes[k % len(classes)]
            p = 0
            if cls == "I" and k // len(classes) % 2:                        # (every other dry row is forced with a NaN: it stays dry)
                p = pos[k % len(pos)]
            elif cls in RANGE:
                lo, hi = span(cls)
                p = min((t for t in pos if lo <= t <= hi), key=lambda t: (used[t], takers[t], t))     # the step least used so far
                used[p] += 1
                c.nan_steps.add(p)
            ql, wet = pattern(cls, p, nsteps, net.amp[r])
            c.qlat[r] = ql
            c.q0[r] = (1.0, 1.0, 0.5) if wet else 0
            c.intended[r] = cls
            c.nan_step[r] = 1 if cls in ("A", "G") else (DAY + 1 if cls == "F" else p)
    c.planted = np.array(sorted(c.intended))
    c.in_slices = net.in_slices
    c.qlat.setflags(write=False)
    c.q0.setflags(write=False)
    return c


def census(labels, in_slices):
    """{class: (rows in the slices, rows in the cluster tiles)} of the labels of every row"""
    return {k: (int(np.sum((labels == k) & in_slices)), int(np.sum((labels == k) & ~in_slices))) for k in sorted(set(labels.tolist()))}


# ---- thresholds that put the NaN where the exceedance can go wrong --------------------------------------------------------------
def thresholds(x, seed=3):
    """[rows, 4] in x's dtype from the row's own values: level 0 half its smallest positive number (numbers over, zeros and NaN
    not: a NaN between two runs); level 1 a negative number (every number over: a NaN breaks a run); level 2 its value at a random
    step (equality occurs; a NaN threshold where that value is one); level 3 its median (NaN where the row holds one)"""
    n, T = x.shape
    rng = np.random.default_rng(seed)
    th = np.empty((n, 4), x.dtype)
    pos = np.where(x > 0, x, np.inf).min(axis=1)
    th[:, 0] = np.where(np.isfinite(pos), pos / 2, 0)
    th[:, 1] = -1
    th[:, 2] = x[np.arange(n), rng.integers(0, T, n)]
    with np.errstate(invalid="ignore"):
        th[:, 3] = np.median(x, axis=1).astype(x.dtype)
    return np.ascontiguousarray(th)


def nan_in_runs(x, th, day=None):
    """how many (row, level) pairs have a NaN step strictly inside a run over the threshold (over, NaN, over), how many between two
    runs (over ... NaN ... over with a step not over beside the NaN), how many on both sides of a day's end inside a run"""
    with np.errstate(invalid="ignore"):
        over = x[:, :, None] > th[:, None, :]
    nan = np.isnan(x)[:, :, None]
    inside = (over[:, :-2] & nan[:, 1:-1] & over[:, 2:]).any(axis=1)
    seen_before = np.maximum.accumulate(over, axis=1)
    seen_after = np.maximum.accumulate(over[:, ::-1], axis=1)[:, ::-1]
    between = (seen_before[:, :-2] & nan[:, 1:-1] & ~over[:, 2:] & seen_after[:, 2:]).any(axis=1)
    edge = 0
    if day:
        T = x.shape[1]
        last, first = np.arange(day - 1, T - 1, day), np.arange(day, T, day)
        a = (over[:, last - 1] & nan[:, last] & over[:, first]).any(axis=1)              # the day's last step
        b = (over[:, last] & nan[:, first] & over[:, first + 1]).any(axis=1)             # the next day's first
        edge = (int(a.sum()), int(b.sum()))
    return int(inside.sum()), int(between.sum()), edge
