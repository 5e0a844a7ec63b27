"""Inputs at the edges of the three guards behind the fp32 step's range-proved arithmetic, and host mirrors of the guards.

The shortened quotients, square root and power of the segment step (csrc/dev_math.inc, DevMathF) have the bits of the IEEE
operations only while their operands stay inside ranges that three guards enforce; outside, the kernels take the plain
operations: "slower, never other bits".  This module states the guards once more, in numpy fp32 and from their text alone
(params_sane: csrc/host_levels.inc, upload_params; fast_ok and coef_guard: csrc/dev_math.inc; the two points a step starts from:
csrc/mc_segment.hpp, step_bracket / section_at / make_const), and builds inputs that sit ON the bounds, one unit in the last
place either side of them, and far outside.  Every builder records the class a row is MEANT to land in; `census` finds the
class each (row, step) really lands in by applying the mirrors to the inputs and to the oracle's depth of the step before.
tests/test_guard_edges_cpu.py compares the two without a GPU; tests/test_gpu_guard_edges.py routes the same inputs through
every kernel that carries the step and asks for the oracle's bits.  The mirrors are never compared with the device.

Parameter columns: dt, dx, bw, tw, twcc, n, ncc, cs, s0 (oracle.PARAM_COLS); single steps: the 15 columns of oracle.segments."""
import functools
import itertools

import numpy as np

import helpers as H

F = np.float32
P_DT, P_DX, P_BW, P_TW, P_TWCC, P_N, P_NCC, P_CS, P_S0 = range(9)
INF = F(np.inf)


def up(x, k=1):
    x = F(x)
    for _ in range(k):
        x = np.nextafter(x, INF)
    return x


def down(x, k=1):
    x = F(x)
    for _ in range(k):
        x = np.nextafter(x, -INF)
    return x


def u32(a):
    return np.asarray(a, dtype=F).view(np.uint32)


# ---- the guards, restated -----------------------------------------------------------------------------------------------
# name -> (column, low, high, zero admitted)
BOUNDS = {
    "bw": (P_BW, F(2.0 ** -14), F(2.0 ** 17), False),
    "n": (P_N, F(2.0 ** -14), F(2.0 ** 17), False),
    "cs": (P_CS, F(2.0 ** -14), F(2.0 ** 17), True),
    "twcc": (P_TWCC, F(2.0 ** -14), F(2.0 ** 17), True),
    "ncc": (P_NCC, F(2.0 ** -14), F(2.0 ** 17), True),
    "dt": (P_DT, F(2.0 ** -20), F(2.0 ** 40), False),
    "dx": (P_DX, F(2.0 ** -10), F(2.0 ** 19), False),
    "s0": (P_S0, F(2.0 ** -30), F(2.0 ** 10), False),
}
H_LO, H_HI = F(2.0 ** -30), F(2.0 ** 17)          # fast_ok: in-bank and over-bank depth at least H_LO, depth at most H_HI
N4_LO, N4_HI = F(2.0 ** -60), F(2.0 ** 60)        # coef_guard: |ql*dt| within [N4_LO, N4_HI], or ql*dt bitwise +0
DT_LO, DT_HI = F(2.0 ** -20), F(2.0 ** 40)


def params_sane(params):
    """bool per row; a plan takes the short forms only when EVERY row of it holds"""
    p = np.asarray(params, dtype=F)
    ok = np.ones(p.shape[0], dtype=bool)
    for col, lo, hi, zero in BOUNDS.values():
        v = p[:, col]
        inside = (v >= lo) & (v <= hi)
        ok &= (inside | (v == 0)) if zero else inside
    return ok


def coef_guard(dt, ql):
    """bool, elementwise: the once-per-forcing-value part of div4's condition (the device also wants its reciprocal proved)"""
    dt, ql = np.asarray(dt, dtype=F), np.asarray(ql, dtype=F)
    with np.errstate(all="ignore"):
        n4 = ql * dt
    a = np.abs(n4)
    return (dt >= DT_LO) & (dt <= DT_HI) & ((u32(n4) == 0) | ((a >= N4_LO) & (a <= N4_HI)))


def bankfull(params):
    """the bankfull depth as make_const forms it, fp32"""
    p = np.asarray(params, dtype=F)
    bw, tw, cs = p[:, P_BW], p[:, P_TW], p[:, P_CS]
    with np.errstate(all="ignore"):
        z = np.where(cs == 0, F(1), F(1) / cs).astype(F)
        two_z = F(2) * z
        bfd = np.where(bw > tw, bw / F(0.00001), np.where(bw == tw, bw / two_z, (tw - bw) / two_z))
    return bfd.astype(F)


def start_points(depthp):
    """(h, h_0): the bracket a step starts from (step_bracket)"""
    d0 = np.maximum(np.asarray(depthp, dtype=F), F(0))
    with np.errstate(all="ignore"):
        return (d0 * F(1.33)) + F(0.01), d0 * F(0.67)


def section(x, bfd, twcc):
    """(h_in, h_over, raw over-bank depth) at depth x (section_at)"""
    with np.errstate(all="ignore"):
        raw = np.maximum(x - bfd, F(0))
    h_in = np.minimum(bfd, x)
    extend = (raw > 0) & (twcc <= 0)                      # NWM 3.0: no flood plain -> the trapezoid goes on
    return np.where(extend, x, h_in).astype(F), np.where(extend, F(0), raw).astype(F), raw.astype(F)


def fast_ok(x, h_in, h_over):
    return (h_in >= H_LO) & (x <= H_HI) & ((h_over == 0) | (h_over >= H_LO))


def fast_ok_start(depthp, bfd, twcc):
    """the verdict of fast_ok at the two points a step starts from: dict of arrays -- ok0 / ok1 (at h_0 / at h), the points,
    their in-bank and over-bank depths, and `raw0`, h_0 - bfd before the NWM-3.0 extension"""
    bfd, twcc = np.asarray(bfd, dtype=F), np.asarray(twcc, dtype=F)
    h, h0 = start_points(depthp)
    in0, over0, raw0 = section(h0, bfd, twcc)
    in1, over1, _ = section(h, bfd, twcc)
    return {"h": h, "h0": h0, "in0": in0, "over0": over0, "raw0": raw0, "in1": in1, "over1": over1,
            "ok0": fast_ok(h0, in0, over0), "ok1": fast_ok(h, in1, over1)}


# ---- classes --------------------------------------------------------------------------------------------------------------
# forcing classes (by n4 = ql*dt) and the verdict coef_guard must give them
FORCING = ["+0", "-0", "+edge", "+below", "+far", "+ord", "-small", "-big", "-edge", "-below"]
FORCING_PASSES = {"+0": True, "-0": False, "+edge": True, "+below": False, "+far": False, "+ord": True, "-small": True,
                  "-big": True, "-edge": True, "-below": False}


def forcing_class(dt, ql):
    """int index into FORCING per element, -1 for anything else (NaN, beyond 2**60)"""
    dt, ql = np.atleast_1d(np.asarray(dt, dtype=F)), np.atleast_1d(np.asarray(ql, dtype=F))
    with np.errstate(all="ignore"):
        n4 = ql * dt
    a, neg = np.abs(n4), np.signbit(n4)
    out = np.full(n4.shape, -1, dtype=np.int64)
    out[u32(n4) == 0] = 0
    out[u32(n4) == 0x80000000] = 1
    band = a == down(N4_LO)                                # one unit in the last place below the bound
    far = (a > 0) & (a < N4_LO * F(0.5))
    out[~neg & (a == N4_LO)] = 2
    out[~neg & band] = 3
    out[~neg & far] = 4
    out[~neg & (a > N4_LO) & (a <= N4_HI)] = 5
    out[neg & (a > N4_LO) & (a <= N4_HI) & (ql > F(-1))] = 6
    out[neg & (a > N4_LO) & (a <= N4_HI) & (ql <= F(-1))] = 7
    out[neg & (a == N4_LO)] = 8
    out[neg & band] = 9
    return out


def _search(x0, f, want, span=4096):
    """the float nearest x0 (within `span` neighbours either way) with want(f(x))"""
    lo = hi = F(x0)
    for _ in range(span):
        if want(f(lo)):
            return lo
        if want(f(hi)):
            return hi
        lo, hi = down(lo), up(hi)
    raise AssertionError("no float near %r does it" % (x0,))


@functools.lru_cache(None)
def forcing_values(dt=300.0):
    """class -> the fp32 forcing value that puts n4 = fl(ql*dt) there (a product by dt > 1 skips floats; for dt = 300 both 2**-60
    and the float right below it are products, which the CPU test asserts)"""
    dt = F(dt)
    n4 = lambda q: F(q) * dt  # noqa: E731
    edge = _search(float(N4_LO) / float(dt), n4, lambda v: v == N4_LO)
    below = edge
    while n4(below) >= N4_LO:
        below = down(below)
    return {"+0": F(0.0), "-0": F(-0.0), "+edge": edge, "+below": below, "+far": F(1e-30), "+ord": F(2e-3),
            "-small": F(-1e-4), "-big": F(-5.0), "-edge": F(-edge), "-below": F(-below)}


@functools.lru_cache(None)
def pair_sequence():
    """a cyclic sequence over the forcing classes in which every ORDERED pair (a, b), a == b included, is adjacent exactly
    once: an Euler circuit of the complete digraph with loops (Hierholzer), 100 long"""
    k = len(FORCING)
    nxt = {a: list(range(k)) for a in range(k)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            circuit.append(stack.pop())
    seq = circuit[::-1][:-1]
    assert len(seq) == k * k and {(seq[i], seq[(i + 1) % len(seq)]) for i in range(len(seq))} == set(itertools.product(range(k), range(k)))
    return np.array(seq)


def schedules(nseg, ncol, day=0):
    """class index [nseg, ncol].  Four rows in five walk the pair sequence (row r starts at 7 r, so over 100 such rows every
    ordered pair of classes meets between every two consecutive columns); every fifth row keeps one class for the whole
    window.  Later days go on along the sequence, so a row's class also changes from day to day."""
    seq = pair_sequence()
    r = np.arange(nseg)[:, None]
    c = np.arange(ncol)[None, :]
    walk = seq[(7 * r + c + ncol * day) % seq.shape[0]]
    const = np.broadcast_to(((r // 5) + 3 * day) % len(FORCING), walk.shape)
    return np.where(r % 5 == 0, const, walk)


def forcing_from_classes(cls, dt=300.0):
    v = forcing_values(dt)
    return np.array([v[name] for name in FORCING], dtype=F)[cls]


# starting depths on the bounds of fast_ok, for a row whose bankfull depth is far away: name -> (depth, fast_ok at both points?)
@functools.lru_cache(None)
def start_depths():
    h0_of = lambda d: F(d) * F(0.67)                      # noqa: E731
    h_of = lambda d: (F(d) * F(1.33)) + F(0.01)           # noqa: E731
    out = {}
    for name, target, ok in (("h0=lo", H_LO, True), ("h0=lo+1ulp", up(H_LO), True)):
        out[name] = (_search(float(target) / 0.67, h0_of, lambda v, t=target: v == t), ok)
    # (below 2**-30 the floats are twice as dense as the products 0.67 d: the float right below the bound is no h_0 of any
    # depth; the nearest one that is lies two units below it, and the CPU test asserts that it is the nearest)
    d = out["h0=lo"][0]
    while h0_of(d) >= H_LO:
        d = down(d)
    out["h0=lo-2ulp"] = (d, False)
    for name, target, ok in (("h=hi", H_HI, True), ("h=hi-1ulp", down(H_HI), True), ("h=hi+1ulp", up(H_HI), False)):
        out[name] = (_search((float(target) - 0.01) / 1.33, h_of, lambda v, t=target: v == t), ok)
    out["dry"] = (F(0.0), False)
    out["h0<<lo"] = (F(1e-12), False)
    out["ordinary"] = (F(0.3), True)
    return out


# a channel whose bankfull depth is the exact power of two 2**-9 (cs = 1 so z = 1; tw - bw = 2**-8): one unit in the last place
# of it is 2**-32, so h_0 - bfd can be 0, one unit, a value inside (0, 2**-30), and 2**-30 itself
BFD_EXACT = F(2.0 ** -9)
BANK_EDGES = {"over0=0": 0, "over0=1ulp": 1, "over0=2ulp": 2, "over0=lo": 4}     # h_0 = bfd + k * 2**-32


@functools.lru_cache(None)
def bank_depths():
    """name -> starting depth with h_0 = fl(0.67 d) = 2**-9 + k * 2**-32"""
    h0_of = lambda d: F(d) * F(0.67)                      # noqa: E731
    out = {}
    for name, k in BANK_EDGES.items():
        target = up(BFD_EXACT, k)
        assert target - BFD_EXACT == F(k * 2.0 ** -32)
        out[name] = _search(float(target) / 0.67, h0_of, lambda v, t=target: v == t)
    return out


def bank_channel(flood_plain):
    """the parameter row of such a channel (dt = 300), with a flood plain or with twcc = 0 (the NWM-3.0 extension)"""
    p = middle_row()
    p[P_BW], p[P_TW], p[P_CS] = F(2.0), F(2.0) + F(2.0 ** -8), F(1.0)
    p[P_TWCC] = F(6.0) if flood_plain else F(0.0)
    return p


def middle_row():
    p = np.zeros(9, dtype=F)
    p[P_DT], p[P_DX], p[P_BW], p[P_TW], p[P_TWCC] = 300.0, 1000.0, 4.0, 6.0, 18.0
    p[P_N], p[P_NCC], p[P_CS], p[P_S0] = 0.05, 0.1, 1.0, 1e-3
    return p


SWEPT = ["bw", "n", "cs", "twcc", "ncc", "dx", "s0"]


def _set(p, name, v):
    p[BOUNDS[name][0]] = v
    if name == "bw":
        p[P_TW] = F(v) * F(1.5)


@functools.lru_cache(None)
def bound_variants():
    """list of (name, parameter row): every swept parameter at the low and at the high end of its range on its own, the
    all-low, all-high and the two alternating corners, and cs == 0, twcc == 0, ncc == 0, bw > tw, bw == tw.  All of them inside
    params_sane."""
    out = []
    for name in SWEPT:
        for side in (1, 2):
            p = middle_row()
            _set(p, name, BOUNDS[name][side])
            out.append((f"{name}={'lo' if side == 1 else 'hi'}", p))
    for label, pick in (("all-lo", lambda i: 1), ("all-hi", lambda i: 2), ("alt-lo-hi", lambda i: 1 + i % 2), ("alt-hi-lo", lambda i: 2 - i % 2)):
        p = middle_row()
        for i, name in enumerate(SWEPT):
            _set(p, name, BOUNDS[name][pick(i)])
        out.append((label, p))
    for label, col in (("cs=0", P_CS), ("twcc=0", P_TWCC), ("ncc=0", P_NCC)):
        p = middle_row()
        p[col] = 0
        out.append((label, p))
    p = middle_row()
    p[P_TW] = p[P_BW] * F(0.5)
    out.append(("bw>tw", p))
    p = middle_row()
    p[P_TW] = p[P_BW]
    out.append(("bw==tw", p))
    assert all(params_sane(p[None, :])[0] for _, p in out)
    return out


def outside_value(name, side):
    """(the value one unit in the last place OUTSIDE the bound, the bound itself); side "lo" | "hi" """
    _, lo, hi, _ = BOUNDS[name]
    return (down(lo), lo) if side == "lo" else (up(hi), hi)


OUTSIDE_CASES = [(name, side) for name in BOUNDS for side in ("lo", "hi")]


# ---- the census -----------------------------------------------------------------------------------------------------------
def census_flags(params, qlat, q0, oracle_result, qts):
    """dict name -> bool [nseg, nsteps]: the classes every (row, step) is in.  `oracle_result` [nseg, nsteps + 1, 3], column 0 the
    initial state.  The forcing class is that of the step's column; the depth classes come from the depth of the step before
    (the oracle's), through fast_ok_start.  "flow": the row's own flow of the step before is positive, so the step is solved."""
    params = np.asarray(params, dtype=F)
    res = np.asarray(oracle_result)
    nseg, nsteps = res.shape[0], res.shape[1] - 1
    col = (np.arange(nsteps) // qts)
    ql = np.asarray(qlat, dtype=F)[:, col]
    dt = params[:, P_DT][:, None]
    fc = forcing_class(np.broadcast_to(dt, ql.shape), ql)
    flags = {f"ql:{name}": fc == i for i, name in enumerate(FORCING)}
    flags["guard:pass"] = coef_guard(np.broadcast_to(dt, ql.shape), ql)
    flags["guard:fail"] = ~flags["guard:pass"]
    depth = np.concatenate([np.asarray(q0, dtype=F)[:, 2:3], res[:, 1:nsteps, 2].astype(F)], axis=1)
    qdp = np.concatenate([np.asarray(q0, dtype=F)[:, 1:2], res[:, 1:nsteps, 0].astype(F)], axis=1)
    bfd = bankfull(params)[:, None]
    twcc = params[:, P_TWCC][:, None]
    fp_ok = ((params[:, P_TWCC] > 0) & (params[:, P_NCC] > 0))[:, None]
    with np.errstate(all="ignore"):
        s = fast_ok_start(depth, np.broadcast_to(bfd, depth.shape), np.broadcast_to(twcc, depth.shape))
        fin = np.isfinite(depth)
        flags["flow"] = qdp > 0
        flags["fast:both"] = s["ok0"] & s["ok1"] & fin
        flags["fast:neither-or-one"] = ~(s["ok0"] & s["ok1"]) & fin
        flags["inbank-fast"] = flags["fast:both"] & (s["h"] <= bfd)
        flags["over-bank"] = (s["h"] > bfd) & fp_ok & fin
        flags["h0<lo"] = (s["in0"] < H_LO) & fin
        flags["h0=lo"] = s["in0"] == H_LO
        flags["h0=lo-2ulp"] = s["in0"] == down(H_LO, 2)
        flags["h0=lo+1ulp"] = s["in0"] == up(H_LO)
        flags["h>hi"] = (s["h"] > H_HI) & fin
        flags["h=hi"] = s["h"] == H_HI
        flags["h=hi-1ulp"] = s["h"] == down(H_HI)
        flags["h=hi+1ulp"] = s["h"] == up(H_HI)
        ext = twcc <= 0
        flags["over0=0@bank"] = (s["h0"] == bfd) & fin
        flags["over0=1ulp"] = (s["raw0"] > 0) & (s["h0"] == np.nextafter(np.broadcast_to(bfd, depth.shape), INF))
        flags["over0-tiny:flood-plain"] = (s["raw0"] > 0) & (s["raw0"] < H_LO) & ~ext
        flags["over0-tiny:extended"] = (s["raw0"] > 0) & (s["raw0"] < H_LO) & ext
        flags["over0=lo:flood-plain"] = (s["raw0"] == H_LO) & ~ext
        flags["over0=lo:extended"] = (s["raw0"] == H_LO) & ext
    return flags


def census(params, qlat, q0, oracle_result, qts):
    """dict class -> number of (row, step) pairs in it"""
    return {k: int(v.sum()) for k, v in census_flags(params, qlat, q0, oracle_result, qts).items()}


def pair_census(params, qlat):
    """[10, 10] counts of (row, column) pairs whose forcing class goes from a (column c) to b (column c + 1)"""
    params = np.asarray(params, dtype=F)
    fc = forcing_class(np.broadcast_to(params[:, P_DT][:, None], np.shape(qlat)), qlat)
    out = np.zeros((len(FORCING), len(FORCING)), dtype=np.int64)
    a, b = fc[:, :-1].ravel(), fc[:, 1:].ravel()
    keep = (a >= 0) & (b >= 0)
    np.add.at(out, (a[keep], b[keep]), 1)
    return out


# ---- fixtures -------------------------------------------------------------------------------------------------------------
NSEG, NSTEPS, QTS = 3000, 24, 3
NCOL = NSTEPS // QTS
RETRY_ROWS = 16


def benign_params(rng, n):
    """ordinary channels, deep enough that a depth under 0.3 m stays in bank (bankfull depth = bw cs / 3 >= 0.5)"""
    bw = rng.uniform(3, 20, n)
    nn = rng.choice([0.04, 0.05, 0.06], n)
    p = np.stack([np.full(n, 300.0), rng.uniform(200, 4000, n), bw, bw * 5 / 3, bw * 5, nn, 2 * nn, rng.uniform(0.5, 2.0, n),
                  np.exp(rng.uniform(np.log(1e-4), np.log(0.1), n))], 1)
    return p.astype(F)


def _topology(to):
    from troute_amd.synthetic import upstream_csr
    up_ptr, up_idx = upstream_csr(to)
    level = np.zeros(to.shape[0], dtype=np.int64)
    order = []
    indeg = np.diff(up_ptr).copy()
    ready = list(np.flatnonzero(indeg == 0))
    while ready:
        i = ready.pop()
        order.append(i)
        j = to[i]
        if j >= 0:
            level[j] = max(level[j], level[i] + 1)
            indeg[j] -= 1
            if indeg[j] == 0:
                ready.append(j)
    assert len(order) == to.shape[0]
    return up_ptr, up_idx, level


class Fixture:
    """one network and its inputs; `intent`: dict name -> rows meant to be in that class at step 1 (depth and parameter classes)
    or [nseg, ncol] class indices (`cls`, the forcing)"""

    def __init__(self, name, to, params, qlat, q0, cls, intent, nsteps=NSTEPS, qts=QTS):
        self.name, self.to, self.params, self.qlat, self.q0 = name, to, params, qlat, q0
        self.cls, self.intent, self.nsteps, self.qts = cls, intent, nsteps, qts
        self.up_ptr, self.up_idx, self.level = _topology(to)
        self._oracle = {}

    def oracle(self, short=True, precision=32, qlat=None, q0=None):
        """[nseg, nsteps + 1, 3] from the plain-division oracle (computed once per mode and left unchanged)"""
        from oracle import oracle as O
        key = (short, precision)
        if qlat is not None or key not in self._oracle:
            p = self.params if precision == 32 else self.params.astype(np.float64)
            r = O.network_by_segment(self.nsteps, self.qts, self.up_ptr, self.up_idx, self.level, p, self.q0 if q0 is None else q0,
                                     self.qlat if qlat is None else qlat, short, det=(precision == 32))
            if qlat is not None:
                return r
            r.setflags(write=False)
            self._oracle[key] = r
        return self._oracle[key]

    def downstream_of(self, row):
        out, j = [], self.to[row]
        while j >= 0:
            out.append(int(j))
            j = self.to[j]
        return np.array(out, dtype=np.int64)


def _base(seed, nseg):
    rng = np.random.default_rng(seed)
    to = H.random_network(rng, nseg)
    params = benign_params(rng, nseg)
    q0 = np.stack([rng.uniform(0.2, 2, nseg), rng.uniform(0.2, 2, nseg), rng.uniform(0.05, 0.3, nseg)], 1).astype(F)
    return rng, to, params, q0


@functools.lru_cache(None)
def interleaved(day=0):
    """3 000 rows, the classes interleaved in row order (a wavefront holds several of each kind): every row walks the forcing
    classes (schedules); rows 7k + 2 carry the parameter variants on the bounds; of the others, rows 3k + 1 start from the
    depths on fast_ok's bounds and at the bank's edge."""
    rng, to, params, q0 = _base(5, NSEG)
    cls = schedules(NSEG, NCOL, day)
    intent = {}
    rows = np.arange(NSEG)
    par_rows = rows[rows % 7 == 2]
    variants = bound_variants()
    for i, r in enumerate(par_rows):
        label, p = variants[i % len(variants)]
        params[r] = p
        intent.setdefault("par:" + label, []).append(int(r))
    dep_rows = rows[(rows % 3 == 1) & (rows % 7 != 2)]
    generic = [(k, v[0], v[1], None) for k, v in start_depths().items()]
    bank = [(f"{k}:{'flood-plain' if fp else 'extended'}", d, None, fp) for fp in (True, False) for k, d in bank_depths().items()]
    kinds = generic + bank
    for i, r in enumerate(dep_rows):
        label, d, _, fp = kinds[i % len(kinds)]
        if fp is None:
            params[r] = middle_row()
            params[r, P_TW] = F(1e6)                                  # (the bank, at 5e5, far above any depth here)
        else:
            params[r] = bank_channel(fp)
        q0[r, 2] = d
        intent.setdefault("depth:" + label, []).append(int(r))
    # the retry branch of the secant loop (more than 100 iterations, csrc/mc_segment.hpp step_solve): the all-low channel starting
    # from 0.3 m with its own 0.2 m3/s and no inflow spends 755 iterations when n4 sits at 2**-60 or right below it (found by
    # oracle.segments(return_iters=True) over single_steps()).  Headwater rows, so the first step's inputs are exactly these.
    has_up = np.zeros(NSEG, dtype=bool)
    has_up[to[to >= 0]] = True
    retry = rows[~has_up & (rows % 7 != 2) & (rows % 3 != 1)][:RETRY_ROWS]
    assert retry.size == RETRY_ROWS
    all_lo = dict(variants)["all-lo"]
    for i, r in enumerate(retry):
        params[r] = all_lo
        q0[r] = (0.0, 0.2, 0.3)
        if day == 0:
            cls[r, 0] = FORCING.index("+edge" if i % 2 == 0 else "+below")
    intent["retry"] = [int(r) for r in retry]
    qlat = forcing_from_classes(cls)
    return Fixture(f"interleaved-day{day}", to, params, qlat, q0, cls, {k: np.array(v) for k, v in intent.items()})


def step_inputs(fx, res, t, rows):
    """the single-step inputs [len(rows), 15] of step t (1-based) of `rows`, rebuilt from a short-timestep oracle result"""
    q = res[:, :, 0].astype(F)
    x = np.zeros((len(rows), 15), dtype=F)
    for i, r in enumerate(rows):
        ups = fx.up_idx[fx.up_ptr[r]:fx.up_ptr[r + 1]]
        qup = F(0)
        for u in ups:
            qup = F(qup + q[u, t - 1])
        p = fx.params[r]
        x[i] = [p[P_DT], qup, qup, q[r, t - 1] if t > 1 else fx.q0[r, 1], fx.qlat[r, (t - 1) // fx.qts], p[P_DX], p[P_BW], p[P_TW],
                p[P_TWCC], p[P_N], p[P_NCC], p[P_CS], p[P_S0], 0.0, res[r, t - 1, 2] if t > 1 else fx.q0[r, 2]]
    return x


UNIFORM_CLASSES = ["+edge", "-below", "-big"]


@functools.lru_cache(None)
def uniform(name):
    """3 000 ordinary in-bank rows, every row and column of ONE forcing class: every wavefront takes the uniform in-bank branch
    at the first step, and coef_guard gives one verdict for the whole plan"""
    rng, to, params, q0 = _base(6, NSEG)
    cls = np.full((NSEG, NCOL), FORCING.index(name))
    return Fixture("uniform" + name, to, params, forcing_from_classes(cls), q0, cls, {})


OUTSIDE_ROW, OUTSIDE_NSEG = 32, 65


@functools.lru_cache(None)
def outside(name, side, inside=False):
    """65 ordinary rows, row 32 one unit in the last place outside one bound of params_sane (inside=True: ON the bound, the twin
    the fallback plan is compared with); ordinary positive forcing with dry columns"""
    rng, to, params, q0 = _base(7, OUTSIDE_NSEG)
    v_out, v_in = outside_value(name, side)
    params[OUTSIDE_ROW] = middle_row()
    _set(params[OUTSIDE_ROW], name, v_in)          # (bw: the top width follows the bound, the same in both twins)
    params[OUTSIDE_ROW, BOUNDS[name][0]] = v_in if inside else v_out
    cls = np.where(rng.random((OUTSIDE_NSEG, NCOL)) < 0.2, 0, FORCING.index("+ord"))
    qlat = (forcing_from_classes(cls) * rng.uniform(0.5, 2.0, cls.shape)).astype(F)
    return Fixture(f"outside-{name}-{side}-{'in' if inside else 'out'}", to, params, qlat, q0, cls, {})


@functools.lru_cache(None)
def single_steps():
    """(inputs [n, 15] fp32, labels): the directed single steps -- every parameter variant (and the middle row) x every forcing class
    x every starting depth on fast_ok's bounds x two inflow sets, and the bank-edge channels x forcing x bank-edge depths"""
    fv = forcing_values()
    rows, labels = [], []
    inflows = [(0.5, 0.6, 0.7), (0.0, 0.0, 0.2)]
    depths = [(k, v[0]) for k, v in start_depths().items()] + [("deep", F(5.0))]
    for (pl, p), fc, (dl, d), (qup, quc, qdp) in itertools.product([("middle", middle_row())] + bound_variants(), FORCING, depths, inflows):
        rows.append([p[P_DT], qup, quc, qdp, fv[fc], p[P_DX], p[P_BW], p[P_TW], p[P_TWCC], p[P_N], p[P_NCC], p[P_CS], p[P_S0], 0.0, d])
        labels.append((pl, fc, dl))
    for fp, fc, (dl, d), (qup, quc, qdp) in itertools.product((True, False), FORCING, bank_depths().items(), inflows):
        p = bank_channel(fp)
        rows.append([p[P_DT], qup, quc, qdp, fv[fc], p[P_DX], p[P_BW], p[P_TW], p[P_TWCC], p[P_N], p[P_NCC], p[P_CS], p[P_S0], 0.0, d])
        labels.append(("bank:" + ("flood-plain" if fp else "extended"), fc, dl))
    return np.array(rows, dtype=F), labels
