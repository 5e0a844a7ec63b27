"""The C ABI and the Python surface of the threshold exceedance over a whole stream of days (include/trmc.h
trmc_stream_set_exceedance, trmc_stream_exceedance; RoutingPlan.stream_set_exceedance / stream_exceedance; ``exceedance`` of
RouteStream): additions WITHIN ABI 19 -- two new functions, no existing prototype changed, no new product of the day, no new member
of trmc_stream_day.  No GPU here: the header, the library's exports, the ctypes table, the signatures and the errors Python raises
before the library is called."""
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
NAMES = ("trmc_stream_set_exceedance", "trmc_stream_exceedance")
PARTS = ("steps_over", "first_step", "last_step", "longest_run")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes_behind_the_windows_block():
    w, lp = r"\s*\w+\s*", r"\s*int64_t\s*\*"
    plan = r"\(\s*trmc_plan\s*\*" + w
    assert re.search(r"\bint\s+trmc_stream_set_exceedance\s*" + plan + r",\s*int\s+\w+\s*\)\s*;", code())
    assert re.search(r"\bint\s+trmc_stream_exceedance\s*" + plan + "," + lp + w + "," + lp + w + "," + lp + w + "," + lp + w + "," + lp + w + r"\)\s*;",
                     code())
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", code())
    assert code().index("trmc_plan_bankfull_depth") < code().index("trmc_stream_set_exceedance") < code().index("trmc_stream_exceedance")
    # what was there stays as it was: the window's prototypes and the quantities
    assert re.search(r"enum\s*\{\s*TRMC_X_FLOW\s*=\s*0\s*,\s*TRMC_X_VELOCITY\s*=\s*1\s*,\s*TRMC_X_DEPTH\s*=\s*2\s*\}\s*;", code())
    assert re.search(r"\bint\s+trmc_stream_summary_total\s*" + plan + r",\s*void\s*\*" + w + "," + lp + w + r",\s*void\s*\*" + w + r",\s*void\s*\*" + w
                     + "," + lp + w + "," + lp + w + r"\)\s*;", code())


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_stream_set_exceedance"] == (C.c_int, [vp, C.c_int])
    assert _lib.SIGNATURES["trmc_stream_exceedance"] == (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_int64)])
    # (a NULL plan is refused before anything touches a device)
    for quantity in (_lib.TRMC_X_FLOW, _lib.TRMC_X_DEPTH, -1, 9):
        assert raw.trmc_stream_set_exceedance(None, quantity) == _lib.TRMC_EINVAL
    days = C.c_int64(-5)
    assert raw.trmc_stream_exceedance(None, None, None, None, None, C.byref(days)) == _lib.TRMC_EINVAL and days.value == -5
    assert lib.trmc_abi_version() == 19


def test_the_python_surface_and_its_defaults():
    sig = inspect.signature(RoutingPlan.stream_set_exceedance)
    assert list(sig.parameters) == ["self", "quantity"] and sig.parameters["quantity"].default == "flow"
    sig = inspect.signature(RoutingPlan.stream_exceedance)
    assert list(sig.parameters) == ["self", "parts"] and tuple(sig.parameters["parts"].default) == PARTS
    p = inspect.signature(RouteStream.__init__).parameters
    assert p["exceedance"].default is None and list(p)[-1] == "exceedance"
    # (what was there keeps its place and its default)
    assert list(p)[:4] == ["self", "router", "nsteps", "qts_subdivisions"] and p["summary"].default is None and p["daily_summary"].default is True


def handle_free_plan(nseg=6, dtype=np.float32):
    """a RoutingPlan object without a library handle: whatever reaches the library from it fails loudly"""
    p = object.__new__(RoutingPlan)
    p.nseg, p.dtype, p.precision, p._th_levels = nseg, np.dtype(dtype).type, 32, 2

    class NoHandle:
        def __getattr__(self, name):
            raise AssertionError("the library was called")
    p._h = NoHandle()
    return p


class NoRouter:
    nseg, world, rank = 6, 1, 0


def library_must_not_be_called(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "lib", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("the library was called")))
    return called


def test_depth_velocity_and_bankfull_are_refused_before_the_library_is_called(monkeypatch):
    p = handle_free_plan()
    called = library_must_not_be_called(monkeypatch)
    for quantity in ("depth", "velocity", "bankfull"):
        # the message says why and points to the window call
        with pytest.raises(NotImplementedError, match=r"(?s)flow planes.*" + quantity + r".*window"):
            p.stream_set_exceedance(quantity)
        with pytest.raises(NotImplementedError, match=r"(?s)flow planes.*window"):
            RouteStream(NoRouter(), 24, 8, exceedance=(quantity, np.zeros(6, np.float32)))
    with pytest.raises(NotImplementedError, match="bankfull"):          # (the drop-in's named thresholds: a depth)
        RouteStream(NoRouter(), 24, 8, exceedance=("depth", "bankfull"))
    with pytest.raises(ValueError, match="stage"):
        p.stream_set_exceedance("stage")
    with pytest.raises(ValueError, match="stage"):
        RouteStream(NoRouter(), 24, 8, exceedance=("stage", np.zeros(6, np.float32)))
    assert not called
    p._h = None                                                 # (nothing for __del__ to release)


def test_wrong_shapes_and_parts_are_refused_before_the_library_is_called(monkeypatch):
    p = handle_free_plan()
    called = library_must_not_be_called(monkeypatch)
    for bad in (np.zeros(5), np.zeros((5, 2)), np.zeros((6, 5)), np.zeros((6, 0)), np.zeros((6, 2, 1)), np.zeros(()), np.zeros((2, 6))):
        with pytest.raises(ValueError, match="thresholds"):
            RouteStream(NoRouter(), 24, 8, exceedance=("flow", bad))
    for bad in ("flow", ("flow",), ("flow", np.zeros(6), 1), 7):
        with pytest.raises(ValueError, match="exceedance"):
            RouteStream(NoRouter(), 24, 8, exceedance=bad)
    with pytest.raises(ValueError, match="peak"):
        p.stream_exceedance(("steps_over", "peak"))
    for nothing in ((), [], None):
        with pytest.raises(ValueError):
            p.stream_exceedance(nothing)
    assert not called
    rs = RouteStream(NoRouter(), 24, 8, exceedance=("flow", np.zeros((6, 3))))      # (accepted: nothing is set before route())
    assert rs.exceedance is None and rs.total is None
    assert RouteStream(NoRouter(), 24, 8).exceedance is None
    p._h = None


def test_the_stream_product_table_the_day_struct_and_the_abi_are_untouched():
    assert _lib.lib().trmc_abi_version() == 19
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    assert len(stream_products.PRODUCTS) == 12
    assert not any("over" in q.name or "exceed" in q.name or "run" in q.name for q in stream_products.PRODUCTS)
    assert C.sizeof(_lib.StreamDay) == 152
    body = re.search(r"typedef\s+struct\s+trmc_stream_day\s*\{(.*?)\}\s*trmc_stream_day\s*;", code(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?(\w+)$", r"\1", part.strip()) for part in decl.split(",")]
    assert names == [n for n, _ in _lib.StreamDay._fields_]
    assert not any("over" in n or "exceed" in n or "run" in n for n in names)
