"""The C ABI and the Python surface of a window's threshold exceedance (include/trmc.h trmc_plan_set_thresholds,
trmc_window_exceedance, trmc_window_exceedance_tile, trmc_window_exceedance_kernel_ms, trmc_plan_bankfull_depth;
RoutingPlan.set_thresholds / window_exceedance / bankfull_depth; ``exceedance`` of the drop-in): additions WITHIN ABI 19 -- five new
functions and one enum, no existing prototype and nothing of the stream's product table touched.  No GPU here: the header, the
library's exports, the ctypes table, the signatures and the errors Python raises before the library is called."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from troute_amd import _lib, stream_products
from troute_amd.plan import RoutingPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trmc_plan_set_thresholds", "trmc_window_exceedance", "trmc_window_exceedance_tile", "trmc_window_exceedance_kernel_ms",
         "trmc_plan_bankfull_depth")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes_and_the_enum():
    w, vp, ip = r"\s*\w+\s*", r"\s*void\s*\*", r"\s*int32_t\s*\*"
    plan = r"\(\s*trmc_plan\s*\*" + w
    assert re.search(r"\bint\s+trmc_plan_set_thresholds\s*" + plan + r",\s*int32_t\s+\w+\s*,\s*const" + vp + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_exceedance\s*" + plan + r",\s*int32_t\s+\w+\s*,\s*int\s+\w+\s*," + ip + w + "," + ip + w + "," + ip + w + ","
                     + ip + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_exceedance_tile\s*\(\s*int\s+\w+\s*," + ip + w + "," + ip + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_exceedance_kernel_ms\s*\(\s*const\s+trmc_plan\s*\*" + w + r",\s*double\s*\*" + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_plan_bankfull_depth\s*" + plan + "," + vp + w + r"\)\s*;", code())
    assert re.search(r"enum\s*\{\s*TRMC_X_FLOW\s*=\s*0\s*,\s*TRMC_X_VELOCITY\s*=\s*1\s*,\s*TRMC_X_DEPTH\s*=\s*2\s*\}\s*;", code())
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", code())
    # behind the Courant block
    assert code().index("trmc_window_courant_kernel_ms") < code().index("trmc_plan_set_thresholds")


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_plan_set_thresholds"] == (C.c_int, [vp, C.c_int32, vp])
    assert _lib.SIGNATURES["trmc_window_exceedance"] == (C.c_int, [vp, C.c_int32, C.c_int, vp, vp, vp, vp])
    assert _lib.SIGNATURES["trmc_plan_bankfull_depth"] == (C.c_int, [vp, vp])
    assert (_lib.TRMC_X_FLOW, _lib.TRMC_X_VELOCITY, _lib.TRMC_X_DEPTH) == (0, 1, 2)
    assert _lib.X_NAMES == {"flow": 0, "velocity": 1, "depth": 2}
    # (a NULL plan is refused before anything touches a device)
    assert raw.trmc_plan_set_thresholds(None, 1, None) == _lib.TRMC_EINVAL
    assert raw.trmc_window_exceedance(None, -1, 0, None, None, None, None) == _lib.TRMC_EINVAL
    assert raw.trmc_window_exceedance_kernel_ms(None, None) == _lib.TRMC_EINVAL
    assert raw.trmc_plan_bankfull_depth(None, None) == _lib.TRMC_EINVAL
    assert lib.trmc_abi_version() == 19


def test_the_tile_is_exposed_without_a_device():
    """rows per block and steps per chunk of a row: what the GPU tests place their shapes around; the summary kernel's tiling"""
    assert RoutingPlan.window_exceedance_tile(32) == RoutingPlan.window_summary_tile(32)
    assert RoutingPlan.window_exceedance_tile(64) == RoutingPlan.window_summary_tile(64)
    assert _lib.lib().trmc_window_exceedance_tile(16, None, None) == _lib.TRMC_EINVAL


def test_the_python_surface_and_its_defaults():
    from troute_amd.routing.compute import compute_nhd_routing_v02
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    sig = inspect.signature(RoutingPlan.window_exceedance)
    assert list(sig.parameters) == ["self", "quantity", "parts", "rowset"]
    assert sig.parameters["quantity"].default == "flow" and sig.parameters["rowset"].default is None
    assert tuple(sig.parameters["parts"].default) == ("steps_over", "first_step", "last_step", "longest_run")
    assert list(inspect.signature(RoutingPlan.set_thresholds).parameters) == ["self", "th"]
    assert list(inspect.signature(RoutingPlan.bankfull_depth).parameters) == ["self"]
    assert hasattr(RoutingPlan, "window_exceedance_kernel_ms")
    for fn in (compute_network_structured, compute_nhd_routing_v02):
        p = inspect.signature(fn).parameters
        assert p["exceedance"].kind is inspect.Parameter.KEYWORD_ONLY and p["exceedance"].default is None
        assert list(p)[-2:] == ["exceedance", "summary"]        # beside `summary`, which stays the last one


def handle_free_plan(nseg=6, dtype=np.float32):
    """a RoutingPlan object without a library handle: whatever reaches the library from it fails loudly"""
    p = object.__new__(RoutingPlan)
    p.nseg, p.dtype, p.precision, p._th_levels = nseg, np.dtype(dtype).type, 32, 0

    class NoHandle:
        def __getattr__(self, name):
            raise AssertionError("the library was called")
    p._h = NoHandle()
    return p


def test_wrong_thresholds_are_refused_before_the_library_is_called(monkeypatch):
    p = handle_free_plan()
    called = []
    monkeypatch.setattr(_lib, "lib", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("the library was called")))
    for bad in (np.zeros(5), np.zeros((5, 2)), np.zeros((6, 5)), np.zeros((6, 0)), np.zeros((6, 2, 1)), np.zeros(()), np.zeros((2, 6))):
        with pytest.raises(ValueError):
            p.set_thresholds(bad)
    with pytest.raises(ValueError, match="stage"):
        p.window_exceedance("stage")
    with pytest.raises(ValueError, match="peak"):
        p.window_exceedance("flow", ("steps_over", "peak"))
    for nothing in ((), [], None):
        with pytest.raises(ValueError):
            p.window_exceedance("flow", nothing)
    assert not called
    p._h = None                                                 # (nothing for __del__ to release)


def test_the_stream_product_table_is_untouched():
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    assert len(stream_products.PRODUCTS) == 12
    assert not any("over" in p.name or "exceed" in p.name or "run" in p.name for p in stream_products.PRODUCTS)
