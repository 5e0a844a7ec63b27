"""The C ABI and the Python surface of the DEPTH exceedance over a whole stream of days (include/trmc.h
trmc_stream_set_depth_exceedance, trmc_stream_depth_exceedance, trmc_stream_depth_exceedance_kernel_ms;
RoutingPlan.stream_set_depth_exceedance / stream_depth_exceedance / stream_depth_exceedance_kernel_ms; ``depth_exceedance`` of
RouteStream): additions WITHIN ABI 19 -- three new functions, no existing prototype changed, no new product of the day, no new
member of trmc_stream_day.  No GPU here: the header, the library's exports, the ctypes table, the signatures and the errors Python
raises before the library is called."""
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
NAMES = ("trmc_stream_set_depth_exceedance", "trmc_stream_depth_exceedance", "trmc_stream_depth_exceedance_kernel_ms")
PARTS = ("steps_over", "first_step", "last_step", "longest_run")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes_behind_the_flow_exceedance():
    w, lp = r"\s*\w+\s*", r"\s*int64_t\s*\*"
    plan = r"\(\s*trmc_plan\s*\*" + w
    c = code()
    assert re.search(r"\bint\s+trmc_stream_set_depth_exceedance\s*" + plan + r",\s*int32_t\s+\w+\s*,\s*const\s+void\s*\*" + w + r"\)\s*;", c)
    assert re.search(r"\bint\s+trmc_stream_depth_exceedance\s*" + plan + "," + lp + w + "," + lp + w + "," + lp + w + "," + lp + w + "," + lp + w
                     + r"\)\s*;", c)
    assert re.search(r"\bint\s+trmc_stream_depth_exceedance_kernel_ms\s*" + plan + r",\s*double\s*\*" + w + r"\)\s*;", c)
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", c)
    at = [c.index(name + "(") for name in ("trmc_stream_exceedance",) + NAMES]
    assert at == sorted(at)
    # what was there stays as it was: the flow exceedance's prototypes
    assert re.search(r"\bint\s+trmc_stream_set_exceedance\s*" + plan + r",\s*int\s+\w+\s*\)\s*;", c)
    assert re.search(r"\bint\s+trmc_stream_exceedance\s*" + plan + "," + lp + w + "," + lp + w + "," + lp + w + "," + lp + w + "," + lp + w + r"\)\s*;", c)


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_stream_set_depth_exceedance"] == (C.c_int, [vp, C.c_int32, vp])
    assert _lib.SIGNATURES["trmc_stream_depth_exceedance"] == (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_int64)])
    assert _lib.SIGNATURES["trmc_stream_depth_exceedance_kernel_ms"] == (C.c_int, [vp, C.POINTER(C.c_double)])
    # (a NULL plan is refused before anything touches a device)
    th = np.zeros(4, np.float32)
    for nlevels, ptr in ((0, None), (1, th.ctypes.data_as(vp)), (1, None), (5, th.ctypes.data_as(vp)), (-1, None)):
        assert raw.trmc_stream_set_depth_exceedance(None, C.c_int32(nlevels), ptr) == _lib.TRMC_EINVAL
    days = C.c_int64(-5)
    assert raw.trmc_stream_depth_exceedance(None, None, None, None, None, C.byref(days)) == _lib.TRMC_EINVAL and days.value == -5
    ms = C.c_double(-1.0)
    assert raw.trmc_stream_depth_exceedance_kernel_ms(None, C.byref(ms)) == _lib.TRMC_EINVAL and ms.value == -1.0
    assert lib.trmc_abi_version() == 19


def test_the_python_surface_and_its_defaults():
    sig = inspect.signature(RoutingPlan.stream_set_depth_exceedance)
    assert list(sig.parameters) == ["self", "th"] and sig.parameters["th"].default == "bankfull"
    sig = inspect.signature(RoutingPlan.stream_depth_exceedance)
    assert list(sig.parameters) == ["self", "parts"] and tuple(sig.parameters["parts"].default) == PARTS
    assert list(inspect.signature(RoutingPlan.stream_depth_exceedance_kernel_ms).parameters) == ["self"]
    p = inspect.signature(RouteStream.__init__).parameters
    assert p["depth_exceedance"].default is None
    # (what was there keeps its place and its default)
    assert list(p)[:4] == ["self", "router", "nsteps", "qts_subdivisions"] and list(p)[-2:] == ["stage", "exceedance"]
    assert p["exceedance"].default is None and p["courant"].default is None and p["stage"].default is False and p["summary"].default is None


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
            RouteStream(NoRouter(), 24, 8, depth_exceedance=bad)
        with pytest.raises(ValueError, match="thresholds"):
            p.stream_set_depth_exceedance(bad)
    with pytest.raises(ValueError, match=r"K <= 4.*\(6, 5\)"):                                                            # K = 5
        RouteStream(NoRouter(), 24, 8, depth_exceedance=np.zeros((6, 5)))
    with pytest.raises(ValueError, match=r"K <= 4.*\(6, 5\)"):
        p.stream_set_depth_exceedance(np.zeros((6, 5)))
    for bad in ("flood", "depth", "Bankfull", ""):                                                                        # a string other than "bankfull"
        with pytest.raises(ValueError, match="bankfull"):
            RouteStream(NoRouter(), 24, 8, depth_exceedance=bad)
        with pytest.raises(ValueError, match="bankfull"):
            p.stream_set_depth_exceedance(bad)
    for th in ("bankfull", np.zeros(6, np.float32), np.zeros((6, 4))):                                                    # reservoir_da
        with pytest.raises(NotImplementedError, match="reservoir data assimilation"):
            RouteStream(WithReservoirDa(), 24, 8, depth_exceedance=th)
    with pytest.raises(ValueError, match="peak"):
        p.stream_depth_exceedance(("steps_over", "peak"))
    for nothing in ((), [], None):
        with pytest.raises(ValueError):
            p.stream_depth_exceedance(nothing)
    p.engine = "flow"
    with pytest.raises(ValueError, match="level engine"):
        p.stream_set_depth_exceedance(np.zeros(6))
    assert not called
    # accepted: nothing is set before route(); several ranks too; beside exceedance=
    for good in ("bankfull", np.zeros(6), np.zeros((6, 1)), np.zeros((6, 3)), np.zeros((6, 4), np.float64), [1.0] * 6):
        rs = RouteStream(NoRouter(), 24, 8, depth_exceedance=good)
        assert rs.depth_exceedance is None and rs.exceedance is None and rs.total is None and rs.courant is None
    rs = RouteStream(NoRouter(), 24, 8, depth_exceedance="bankfull", exceedance=("flow", np.zeros((6, 2))))
    assert rs.depth_exceedance is None and rs.exceedance is None
    assert RouteStream(TwoRanks(), 24, 8, comm=object(), depth_exceedance=np.zeros(6)).depth_exceedance is None
    assert RouteStream(NoRouter(), 24, 8).depth_exceedance is None
    # exceedance= goes on refusing depth, with its message
    with pytest.raises(NotImplementedError, match=r"(?s)flow planes.*window"):
        RouteStream(NoRouter(), 24, 8, exceedance=("depth", "bankfull"))
    assert not called
    p._h = None                                                 # (nothing for __del__ to release)


def test_the_stream_product_table_the_day_struct_and_the_abi_are_untouched():
    assert _lib.lib().trmc_abi_version() == 19
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    assert len(stream_products.PRODUCTS) == 12
    assert stream_products.ALL == stream_products.PRODUCTS + (stream_products.STAGE,)
    assert not any("over" in q.name or "exceed" in q.name or "run" in q.name for q in stream_products.ALL)
    assert C.sizeof(_lib.StreamDay) == 152
    body = re.search(r"typedef\s+struct\s+trmc_stream_day\s*\{(.*?)\}\s*trmc_stream_day\s*;", code(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?(\w+)$", r"\1", part.strip()) for part in decl.split(",")]
    assert names == [n for n, _ in _lib.StreamDay._fields_]
    assert not any("over" in n or "exceed" in n or "run" in n for n in names)
