"""The C ABI and the Python surface of a window's Courant metrics (include/trmc.h trmc_window_courant, trmc_window_courant_summary,
trmc_window_courant_tile, trmc_window_courant_kernel_ms; RoutingPlan.window_courant / window_courant_summary; ``return_courant`` of
the drop-in): additions WITHIN ABI 19 -- four new functions, no existing prototype and nothing of the stream's product table
touched.  No GPU here: the header, the library's exports, the ctypes table and the signatures."""
import ctypes as C
import inspect
import os
import re

from troute_amd import _lib, stream_products
from troute_amd.plan import RoutingPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trmc_window_courant", "trmc_window_courant_summary", "trmc_window_courant_tile", "trmc_window_courant_kernel_ms")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes():
    w, vp, ip = r"\s*\w+\s*", r"\s*void\s*\*", r"\s*int32_t\s*\*"
    plan = r"\(\s*trmc_plan\s*\*" + w + r",\s*int32_t\s+\w+\s*,"
    assert re.search(r"\bint\s+trmc_window_courant\s*" + plan + r"\s*int\s+\w+\s*," + vp + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_courant_summary\s*" + plan + r"\s*double\s+\w+\s*," + vp + w + "," + ip + w + "," + ip + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_courant_tile\s*\(\s*int\s+\w+\s*," + ip + w + "," + ip + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_courant_kernel_ms\s*\(\s*const\s+trmc_plan\s*\*" + w + r",\s*double\s*\*" + w + r"\)\s*;", code())
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", code())


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_window_courant"] == (C.c_int, [vp, C.c_int32, C.c_int, vp])
    assert _lib.SIGNATURES["trmc_window_courant_summary"] == (C.c_int, [vp, C.c_int32, C.c_double, vp, vp, vp])
    # (a NULL plan is refused before anything touches a device)
    raw.trmc_window_courant_summary.argtypes = [vp, C.c_int32, C.c_double, vp, vp, vp]
    assert raw.trmc_window_courant(None, -1, 1, None) == _lib.TRMC_EINVAL
    assert raw.trmc_window_courant_summary(None, -1, 1.0, None, None, None) == _lib.TRMC_EINVAL
    assert raw.trmc_window_courant_kernel_ms(None, None) == _lib.TRMC_EINVAL
    assert lib.trmc_abi_version() == 19


def test_the_tile_is_exposed_without_a_device():
    """rows per block and steps per chunk of a row: what the GPU tests place their shapes around"""
    r32, c32 = RoutingPlan.window_courant_tile(32)
    r64, c64 = RoutingPlan.window_courant_tile(64)
    assert r32 >= 1 and r64 >= 1 and c32 >= 2 and c64 >= 2
    assert _lib.lib().trmc_window_courant_tile(16, None, None) == _lib.TRMC_EINVAL


def test_the_python_surface_and_its_defaults():
    from troute_amd.routing.compute import compute_nhd_routing_v02
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    sig = inspect.signature(RoutingPlan.window_courant)
    assert list(sig.parameters) == ["self", "stride", "rowset"]
    assert sig.parameters["stride"].default == 1 and sig.parameters["rowset"].default is None
    sig = inspect.signature(RoutingPlan.window_courant_summary)
    assert list(sig.parameters) == ["self", "limit", "rowset"]
    assert sig.parameters["limit"].default == 1.0 and sig.parameters["rowset"].default is None
    # no new keyword: return_courant is the reference's positional parameter, and `summary` stays the last one
    for fn in (compute_network_structured, compute_nhd_routing_v02):
        p = inspect.signature(fn).parameters
        assert p["return_courant"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert list(p)[-1] == "summary"
    assert inspect.signature(compute_network_structured).parameters["return_courant"].default is False
    # window_summary keeps its seven names and its signature
    assert list(inspect.signature(RoutingPlan.window_summary).parameters) == ["self", "parts", "rowset"]
    assert sum(len(v) for v in RoutingPlan.WINDOW_SUMMARY_PARTS.values()) == 7


def test_the_stream_product_table_is_untouched():
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    assert len(stream_products.PRODUCTS) == 12
    assert not any("courant" in p.name or "cn" == p.name for p in stream_products.PRODUCTS)
