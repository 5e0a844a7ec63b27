"""The C ABI and the Python surface of the peak velocity and the velocity exceedance over a whole stream of days (include/trmc.h
trmc_stream_set_velocity, trmc_stream_velocity, trmc_stream_velocity_kernel_ms; RoutingPlan.stream_set_velocity / stream_velocity /
stream_velocity_kernel_ms; ``velocity`` of RouteStream): additions WITHIN ABI 19 -- three new functions, no existing prototype
changed, no new product of the day, no new member of trmc_stream_day.  No GPU here: the header, the library's exports, the ctypes
table, the signatures and the errors Python raises before the library is called."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from troute_amd import _lib, stream_products
from troute_amd.plan import RoutingPlan
from troute_amd.sequence import RouteStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trmc_stream_set_velocity", "trmc_stream_velocity", "trmc_stream_velocity_kernel_ms")
KEYS = ["days", "peak_velocity", "peak_velocity_step", "steps_over", "first_step", "last_step", "longest_run"]


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes_behind_the_depth_exceedance():
    w, lp = r"\s*\w+\s*", r"\s*int64_t\s*\*"
    plan = r"\(\s*trmc_plan\s*\*" + w
    c = code()
    assert re.search(r"\bint\s+trmc_stream_set_velocity\s*" + plan + r",\s*int\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*const\s+void\s*\*" + w + r"\)\s*;", c)
    assert re.search(r"\bint\s+trmc_stream_velocity\s*" + plan + r",\s*void\s*\*" + w + ("," + lp + w) * 6 + r"\)\s*;", c)
    assert re.search(r"\bint\s+trmc_stream_velocity_kernel_ms\s*" + plan + r",\s*double\s*\*" + w + r"\)\s*;", c)
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", c)
    at = [c.index(name + "(") for name in ("trmc_stream_depth_exceedance_kernel_ms",) + NAMES]
    assert at == sorted(at)
    # what was there stays as it was: the flow exceedance goes on with its one argument
    assert re.search(r"\bint\s+trmc_stream_set_exceedance\s*" + plan + r",\s*int\s+\w+\s*\)\s*;", c)


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_stream_set_velocity"] == (C.c_int, [vp, C.c_int, C.c_int32, vp])
    assert _lib.SIGNATURES["trmc_stream_velocity"] == (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int64)])
    assert _lib.SIGNATURES["trmc_stream_velocity_kernel_ms"] == (C.c_int, [vp, C.POINTER(C.c_double)])
    # (a NULL plan is refused before anything touches a device)
    th = np.zeros(4, np.float32)
    for on, nlevels, ptr in ((0, 0, None), (1, 0, None), (1, 1, th.ctypes.data_as(vp)), (1, 1, None), (1, 5, th.ctypes.data_as(vp))):
        assert raw.trmc_stream_set_velocity(None, C.c_int(on), C.c_int32(nlevels), ptr) == _lib.TRMC_EINVAL
    days = C.c_int64(-5)
    assert raw.trmc_stream_velocity(None, None, None, None, None, None, None, C.byref(days)) == _lib.TRMC_EINVAL and days.value == -5
    ms = C.c_double(-1.0)
    assert raw.trmc_stream_velocity_kernel_ms(None, C.byref(ms)) == _lib.TRMC_EINVAL and ms.value == -1.0
    assert lib.trmc_abi_version() == 19


def test_the_python_surface_and_its_defaults():
    sig = inspect.signature(RoutingPlan.stream_set_velocity)
    assert list(sig.parameters) == ["self", "thresholds"] and sig.parameters["thresholds"].default is True
    assert list(inspect.signature(RoutingPlan.stream_velocity).parameters) == ["self"]
    assert list(inspect.signature(RoutingPlan.stream_velocity_kernel_ms).parameters) == ["self"]
    p = inspect.signature(RouteStream.__init__).parameters
    assert p["velocity"].default is None
    assert isinstance(RouteStream.velocity, property)
    # (what was there keeps its place and its default)
    assert list(p)[:4] == ["self", "router", "nsteps", "qts_subdivisions"] and list(p)[-2:] == ["stage", "exceedance"]
    assert p["exceedance"].default is None and p["courant"].default is None and p["depth_exceedance"].default is None
    assert "velocity=" in RouteStream.__doc__


def handle_free_plan(nseg=6, dtype=np.float32):
    """a RoutingPlan object without a library handle: whatever reaches the library from it fails loudly"""
    p = object.__new__(RoutingPlan)
    p.nseg, p.dtype, p.precision, p.engine = nseg, np.dtype(dtype).type, 32, "levels"

    class NoHandle:
        def __getattr__(self, name):
            raise AssertionError("the library was called")
    p._h = NoHandle()
    return p


class NoRouter:
    nseg, world, rank = 6, 1, 0


class TwoRanks(NoRouter):
    world = 2


class WithReservoirDa(NoRouter):
    _reservoir_da = object()


def library_must_not_be_called(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "lib", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("the library was called")))
    return called


def test_bad_arguments_are_refused_before_the_library_is_called(monkeypatch):
    p = handle_free_plan()
    called = library_must_not_be_called(monkeypatch)
    for bad in (np.zeros(5), np.zeros((5, 2)), np.zeros((6, 0)), np.zeros((6, 2, 1)), np.zeros(()), np.zeros((2, 6))):    # a wrong shape
        with pytest.raises(ValueError, match="thresholds"):
            RouteStream(NoRouter(), 24, 8, velocity=bad)
        with pytest.raises(ValueError, match="thresholds"):
            p.stream_set_velocity(bad)
    with pytest.raises(ValueError, match=r"K <= 4.*\(6, 5\)"):                                                            # more than four levels
        RouteStream(NoRouter(), 24, 8, velocity=np.zeros((6, 5)))
    with pytest.raises(ValueError, match=r"K <= 4.*\(6, 5\)"):
        p.stream_set_velocity(np.zeros((6, 5)))
    for bad in ("peak", "bankfull", ""):                                                                                  # a string
        with pytest.raises(ValueError, match="thresholds"):
            RouteStream(NoRouter(), 24, 8, velocity=bad)
        with pytest.raises(ValueError, match="thresholds"):
            p.stream_set_velocity(bad)
    for v in (True, np.zeros(6, np.float32), np.zeros((6, 4))):
        with pytest.raises(NotImplementedError, match="several ranks"):                                                   # several ranks
            RouteStream(TwoRanks(), 24, 8, comm=object(), velocity=v)
        with pytest.raises(NotImplementedError, match="reservoir data assimilation"):                                     # reservoir_da
            RouteStream(WithReservoirDa(), 24, 8, velocity=v)
    p.engine = "flow"                                                                                                     # the dataflow engine
    for v in (True, np.zeros(6)):
        with pytest.raises(ValueError, match="level engine"):
            p.stream_set_velocity(v)
    p.stream_set_velocity(None)                                                 # (withdrawing nothing is no error, on either engine ...
    p.engine = "levels"
    p.stream_set_velocity(None)                                                 # ... and does not reach the library)
    p.engine = "flow"
    assert not called
    # accepted: nothing is set before route(); beside the other accumulators
    for good in (True, np.zeros(6), np.zeros((6, 1)), np.zeros((6, 3)), np.zeros((6, 4), np.float64), [1.0] * 6):
        rs = RouteStream(NoRouter(), 24, 8, velocity=good)
        assert rs.velocity is None and rs.depth_exceedance is None and rs.exceedance is None and rs.total is None and rs.courant is None
    rs = RouteStream(NoRouter(), 24, 8, velocity=np.zeros(6), depth_exceedance="bankfull", courant=1.0, exceedance=("flow", np.zeros((6, 2))))
    assert rs.velocity is None
    assert RouteStream(NoRouter(), 24, 8).velocity is None and RouteStream(TwoRanks(), 24, 8, comm=object()).velocity is None
    # exceedance= and stream_set_exceedance go on refusing velocity, pointing to the window
    with pytest.raises(NotImplementedError, match=r"(?s)window"):
        RouteStream(NoRouter(), 24, 8, exceedance=("velocity", np.zeros(6)))
    p.engine = "levels"
    with pytest.raises(NotImplementedError, match=r"(?s)window"):
        p.stream_set_exceedance("velocity")
    assert not called
    p._h = None                                                 # (nothing for __del__ to release)


def test_the_order_of_the_fetchs_keys(monkeypatch):
    """``stream_velocity()``: "days", the peak, its step and, with thresholds, the four figures [rows, K] -- in that order"""
    seen = {}

    class Lib:
        def trmc_stream_velocity(self, h, peak, step, over, first, last, run, days):
            seen["levels"] = [a is not None for a in (over, first, last, run)]
            days._obj.value = 3
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    p = handle_free_plan()
    p._h = None
    p._stream_velocity = 2
    got = p.stream_velocity()
    assert list(got) == KEYS and got["days"] == 3 and seen["levels"] == [True] * 4
    assert got["peak_velocity"].shape == (6,) and got["peak_velocity"].dtype == np.float32 and got["peak_velocity_step"].dtype == np.int64
    assert all(got[k].shape == (6, 2) and got[k].dtype == np.int64 for k in KEYS[3:])
    p._stream_velocity = 0
    got = p.stream_velocity()
    assert list(got) == KEYS[:3] and seen["levels"] == [False] * 4


def test_the_symbols_came_without_a_new_product_a_new_day_member_or_a_new_abi():
    """the three functions are there, and what the issue says must stay beside them has stayed"""
    assert all(name in _lib.SIGNATURES and hasattr(_lib.lib(), name) for name in NAMES)
    assert _lib.lib().trmc_abi_version() == 19
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    assert len(stream_products.PRODUCTS) == 12
    assert not any("velocity" in q.name for q in stream_products.ALL)
    assert C.sizeof(_lib.StreamDay) == 152
