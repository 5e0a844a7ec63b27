"""THE HAND-OVER of the reservoir data-assimilation state between two windows -- or two days of a stream (csrc/stream.inc) --
checked on the CPU: csrc/reservoir_da.hpp's ``reservoir_da_handover`` is ``__host__ __device__``, built here into a small shared
object with g++ (tests/reservoir_da_host.cpp; -ffp-contract=off, as the library is built), beside the hybrid step of the same
header.

What the loop does at a window's end (mc_reach.pyx:820-837; the drop-in's mc_reach.py): update_time and
persistence_update_time (RFC: update_time) less t_end = float(nsteps) * float(dt), in fp32; everything else unchanged.

A value where ``update_time - t_end`` differs in the last bit between that fp32 form and a double or fused form: none exists in
the fixtures themselves -- their dt is 300 s and nsteps * 300 is exact in fp32 for every window they use (24, 36, 72 steps), so
the product rounds nowhere and all three forms agree (searched over every update_time / persistence_update_time /
rfc update_time of reservoir_da_vectors.npz and reservoir_da_network.npz: 2716 distinct values, no difference).  With a
routing period that is not a whole number the forms part: LAST_BIT below is the fixture's update_time 3120.0 at nsteps = 24,
dt = float32(300.1): fp32 form -4082.4004, double form -4082.4001."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = np.load(os.path.join(H.GOLDEN, "reservoir_da_network.npz"))
VEC = np.load(os.path.join(H.GOLDEN, "reservoir_da_vectors.npz"))
NTS, DT = int(NET["nts"]), 300.0
LAST_BIT = dict(update_time=np.float32(3120.0), nsteps=24, dt=np.float32(300.1))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("da_host") / "libda_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "t-route_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "reservoir_da_host.cpp")])
    lib = C.CDLL(so)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.da_handover.argtypes = [C.c_int, fp, ip, C.c_float]
    lib.da_handover.restype = None
    lib.da_hybrid_step.argtypes = [fp, fp, C.c_int, fp, fp]
    lib.da_hybrid_step.restype = None
    return lib


def t_end_of(nsteps, dt):
    return np.float32(np.float32(nsteps) * np.float32(dt))           # (rounded once, by the caller)


def handover(lib, kind, state, idx, t_end):
    st = np.array(state, dtype=np.float32)
    i = C.c_int(int(idx))
    lib.da_handover(int(kind), st.ctypes.data_as(C.POINTER(C.c_float)), C.byref(i), C.c_float(float(t_end)))
    return st, i.value


def hybrid_step(lib, obs, time, fin):
    obs, time, fin = (np.ascontiguousarray(a, dtype=np.float32) for a in (obs, time, fin))
    out = np.zeros(6, np.float32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))        # noqa: E731
    lib.da_hybrid_step(p(obs), p(time), obs.shape[0], p(fin), p(out))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_handover_touches_the_times_only(host):
    s = [7200.0, 3.25, 4.0, 90000.0]
    t = t_end_of(24, DT)
    for kind, want in ((0, [7200.0, 3.25, 4.0, 90000.0]), (2, [0.0, 3.25, 4.0, 82800.0]), (3, [0.0, 3.25, 4.0, 82800.0]),
                       (4, [0.0, 3.25, 4.0, 90000.0]), (5, [0.0, 3.25, 4.0, 90000.0])):
        st, idx = handover(host, kind, s, 17, t)
        assert np.array_equal(bits(st), bits(want)) and idx == 17, kind
    st, _ = handover(host, 2, [np.nan, np.nan, 0.0, np.inf], 0, t)
    assert np.isnan(st[0]) and np.isnan(st[1]) and st[3] == np.inf


def test_handover_is_the_fp32_form_to_the_last_bit(host):
    """see the module's docstring: the named value, and the three forms on it"""
    u, n, dt = LAST_BIT["update_time"], LAST_BIT["nsteps"], LAST_BIT["dt"]
    t = t_end_of(n, dt)
    fp32_form = np.float32(u - t)
    double_form = np.float32(np.float64(u) - np.float64(np.float32(n)) * np.float64(dt))    # (= the fused form: one rounding)
    assert bits(fp32_form) != bits(double_form) and abs(int(bits(fp32_form)[0]) - int(bits(double_form)[0])) == 1
    for kind in (2, 3, 4, 5):
        st, _ = handover(host, kind, [u, 0.0, 0.0, u], 0, t)
        assert bits(st[0]) == bits(fp32_form), kind
        assert bits(st[3]) == bits(fp32_form if kind <= 3 else u), kind
    # ... and none in the fixtures (dt = 300: every window's length is exact)
    vals = np.concatenate([VEC["hybrid_out"][:, 3], VEC["hybrid_out"][:, 5], VEC["rfc_out"][:, 2], VEC["hybrid_in"][:, 11],
                           NET["usgs_update_time"], NET["usgs_put"], NET["usace_update_time"], NET["usace_put"], NET["rfc_update_time"]])
    vals = np.unique(vals[np.isfinite(vals)].astype(np.float32))
    assert vals.size > 2000
    for n in (24, 36, 72):
        t = t_end_of(n, DT)
        assert float(t) == n * DT
        assert np.array_equal(bits(vals - t), bits((vals.astype(np.float64) - n * DT).astype(np.float32)))


def test_recorded_steps_chained_through_two_windows(host):
    """The recorded hybrid steps (the reference function's own returns): the host build reproduces every one bit for bit; then
    each is taken as the LAST step of a window that ends at its `now` -- its state handed over, the next step made in the new
    window's time (now = dt, the observation times less the window's length) -- and lands on the step made without the cut, the
    times less the window's length: two windows equal one long one, at the level of the function."""
    fin, fout, obs, time = VEC["hybrid_in"], VEC["hybrid_out"], VEC["hybrid_obs"], VEC["hybrid_time"]
    checked = 0
    for k in range(0, fin.shape[0], 7):
        f = fin[k]
        o = hybrid_step(host, obs[k], time[k], f)
        assert np.array_equal(bits(o), bits(fout[k])), k
        now, dt = f[0], f[6]
        # (a window's end is a whole number of steps, and its length must leave the times exact for the comparison to be one of bits)
        if not (now > 0 and float(now) % float(dt) == 0 and np.isfinite(o[[1, 3, 5]]).all()):
            continue
        t = np.float32(now)
        nxt = f.copy()
        nxt[[0, 1, 2, 3, 11]] = now + dt, o[1], o[5], o[4], o[3]          # the step after, without a cut
        nxt[10] = o[2]
        long = hybrid_step(host, obs[k], time[k], nxt)
        st, _ = handover(host, 2, [o[3], o[1], o[4], o[5]], 0, t)
        cut = nxt.copy()
        cut[[0, 11, 1, 3, 2]] = dt, st[0], st[1], st[2], st[3]
        short = hybrid_step(host, obs[k], (time[k] - t).astype(np.float32), cut)
        exact = all(float(np.float32(x) - t) == float(x) - float(t) for x in (o[3], o[5], long[3], long[5]))
        if not exact or not np.array_equal(bits(time[k] - t), bits((time[k].astype(np.float64) - float(t)).astype(np.float32))):
            continue
        want, _ = handover(host, 2, [long[3], long[1], long[4], long[5]], 0, t)
        assert np.array_equal(bits(short[[0, 1, 2]]), bits(long[[0, 1, 2]])), k
        assert np.array_equal(bits([short[3], short[1], short[4], short[5]]), bits(want)), k
        checked += 1
    assert checked >= 100


def test_golden_states_are_handed_over_once_or_twice(host):
    """The network fixture's recorded final state (golden state_*: what the reference loop returned after the long window of 72
    steps) is its initial state moved on by whole update intervals, handed over -- and the same through two windows of 36 steps
    each, the first window's tuple going in as the second's state (test_gpu_two_windows_equal_one_long_window's arithmetic)."""
    half, full = t_end_of(NTS // 2, DT), t_end_of(NTS, DT)

    def reach(kind, init, inc, want, col):
        for k in range(0, 40):
            for k1 in range(0, k + 1):
                s = [0.0] * 4
                s[col] = np.float32(init) + np.float32(k * inc)
                once, _ = handover(host, kind, s, 0, full)
                s[col] = np.float32(init) + np.float32(k1 * inc)
                first, _ = handover(host, kind, s, 0, half)
                first[col] = first[col] + np.float32((k - k1) * inc)
                twice, _ = handover(host, kind, first, 0, half)
                assert bits(once[col]) == bits(twice[col])
            if bits(once[col]) == bits(want):
                return True
        return False
    for name, kind in (("usgs", 2), ("usace", 3)):
        for j in range(len(NET[f"{name}_idx"])):
            assert reach(kind, NET[f"{name}_update_time"][j], 3600.0, NET[f"short_long_state_{name}_1"][j], 0), (name, j)
            assert reach(kind, NET[f"{name}_put"][j], 86400.0, NET[f"short_long_state_{name}_4"][j], 3), (name, j)
    use = NET["rfc_use"].astype(bool)
    for j in range(len(NET["rfc_idx"])):
        want = NET["short_long_state_rfc_1"][j]
        if use[j]:
            assert reach(4, NET["rfc_update_time"][j], float(NET["rfc_da_dt"][j]), want, 0), j
        else:
            once, _ = handover(host, 4, [NET["rfc_update_time"][j], 0, 0, 0], 0, full)
            assert bits(once[0]) == bits(want), j
