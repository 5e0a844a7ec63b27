"""The C ABI and the Python surface of a window's per-row summary (include/trmc.h trmc_window_summary, trmc_window_summary_tile;
trmc_window_summary_kernel_ms; RoutingPlan.window_summary; the ``summary`` keyword of the drop-in): additions WITHIN ABI 19 -- three
new functions, nothing of the stream's product table touched.  No GPU here: the header, the library's exports, the ctypes table and the signatures."""
import ctypes as C
import inspect
import os
import re

from troute_amd import _lib, stream_products
from troute_amd.plan import RoutingPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ("peak", "mean", "peak_depth", "peak_velocity")
KEYS = ("peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step", "peak_velocity", "peak_velocity_step")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototype():
    w, vp, ip = r"\s*\w+\s*", r"\s*void\s*\*", r"\s*int32_t\s*\*"
    assert re.search(r"\bint\s+trmc_window_summary\s*\(\s*trmc_plan\s*\*" + w + r",\s*int32_t\s+\w+\s*," + vp + w + "," + ip + w + "," + vp + w + ","
                     + vp + w + "," + ip + w + "," + vp + w + "," + ip + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_summary_tile\s*\(\s*int\s+\w+\s*," + ip + w + "," + ip + w + r"\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_summary_kernel_ms\s*\(\s*const\s+trmc_plan\s*\*" + w + r",\s*double\s*\*" + w + r"\)\s*;", code())


def test_the_library_exports_it_and_ctypes_knows_the_signature():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in ("trmc_window_summary", "trmc_window_summary_tile", "trmc_window_summary_kernel_ms"):
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_window_summary"] == (C.c_int, [vp, C.c_int32] + [vp] * 7)
    # (a NULL plan is refused before anything touches a device)
    assert raw.trmc_window_summary(None, -1, None, None, None, None, None, None, None) == _lib.TRMC_EINVAL
    assert raw.trmc_window_summary_kernel_ms(None, None) == _lib.TRMC_EINVAL
    assert lib.trmc_abi_version() == 19


def test_the_tile_is_exposed_without_a_device():
    """rows per block and steps per chunk of a row's record, per precision: what the GPU tests place their shapes around; a row's
    chunk is the same number of bytes in both precisions"""
    r32, c32 = RoutingPlan.window_summary_tile(32)
    r64, c64 = RoutingPlan.window_summary_tile(64)
    assert r32 == r64 and r32 >= 1 and c32 >= 2 and c64 >= 2
    assert c32 * 4 == c64 * 8
    assert _lib.lib().trmc_window_summary_tile(16, None, None) == _lib.TRMC_EINVAL


def test_the_python_surface_and_its_defaults():
    from troute_amd.routing.compute import compute_nhd_routing_v02
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    sig = inspect.signature(RoutingPlan.window_summary)
    assert list(sig.parameters) == ["self", "parts", "rowset"]
    assert sig.parameters["parts"].default == PARTS and sig.parameters["rowset"].default is None
    names = [n for part in PARTS for n in RoutingPlan.WINDOW_SUMMARY_PARTS[part]]
    assert sorted(names) == sorted(KEYS)
    # the first five are the stream summary's names, on purpose
    assert [p.name for p in stream_products.SUMMARY] == list(KEYS[:5])
    for fn, first in ((compute_network_structured, 59), (compute_nhd_routing_v02, 37)):
        p = inspect.signature(fn).parameters
        assert p["summary"].default is None and p["summary"].kind is inspect.Parameter.KEYWORD_ONLY
        assert list(p)[-1] == "summary"
        assert all(v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for v in list(p.values())[:first])
        assert list(p.values())[first].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_stream_product_table_is_untouched():
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    assert len(stream_products.PRODUCTS) == 12
    assert "peak_velocity" not in _lib.SUMMARY_NAMES and not any("velocity" in p.name for p in stream_products.PRODUCTS)
