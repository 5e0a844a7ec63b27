"""The C ABI and the Python surface of the Courant number over a whole stream of days (include/trmc.h trmc_stream_set_courant,
trmc_stream_courant, trmc_stream_courant_kernel_ms; RoutingPlan.stream_set_courant / stream_courant; ``courant`` of RouteStream): additions WITHIN ABI 19 -- three
new functions, no existing prototype changed, no new product of the day, no new member of trmc_stream_day.  No GPU here: the header,
the library's exports, the ctypes table, the signatures and the errors Python raises before the library is called."""
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
NAMES = ("trmc_stream_set_courant", "trmc_stream_courant", "trmc_stream_courant_kernel_ms")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes_behind_the_exceedances():
    w, lp = r"\s*\w+\s*", r"\s*int64_t\s*\*"
    plan = r"\(\s*trmc_plan\s*\*" + w
    assert re.search(r"\bint\s+trmc_stream_set_courant\s*" + plan + r",\s*int\s+\w+\s*,\s*double\s+\w+\s*\)\s*;", code())
    assert re.search(r"\bint\s+trmc_stream_courant\s*" + plan + r",\s*void\s*\*" + w + "," + lp + w + "," + lp + w + "," + lp + w + r"\)\s*;", code())
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", code())
    assert code().index("trmc_stream_exceedance") < code().index("trmc_stream_set_courant") < code().index("trmc_stream_courant")
    # what was there stays as it was: the exceedance's and the window's prototypes
    assert re.search(r"\bint\s+trmc_stream_set_exceedance\s*" + plan + r",\s*int\s+\w+\s*\)\s*;", code())
    assert re.search(r"\bint\s+trmc_window_courant_summary\s*" + plan + r",\s*int32_t\s+\w+\s*,\s*double\s+\w+\s*,\s*void\s*\*" + w
                     + r",\s*int32_t\s*\*" + w + r",\s*int32_t\s*\*" + w + r"\)\s*;", code())


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_stream_set_courant"] == (C.c_int, [vp, C.c_int, C.c_double])
    assert _lib.SIGNATURES["trmc_stream_courant"] == (C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_int64)])
    assert _lib.SIGNATURES["trmc_stream_courant_kernel_ms"] == (C.c_int, [vp, C.POINTER(C.c_double)])
    assert raw.trmc_stream_courant_kernel_ms(None, None) == _lib.TRMC_EINVAL
    # (a NULL plan is refused before anything touches a device)
    raw.trmc_stream_set_courant.argtypes = [vp, C.c_int, C.c_double]
    for on in (0, 1):
        assert raw.trmc_stream_set_courant(None, on, 1.0) == _lib.TRMC_EINVAL
    days = C.c_int64(-5)
    assert raw.trmc_stream_courant(None, None, None, None, C.byref(days)) == _lib.TRMC_EINVAL and days.value == -5
    assert lib.trmc_abi_version() == 19


def test_the_python_surface_and_its_defaults():
    sig = inspect.signature(RoutingPlan.stream_set_courant)
    assert list(sig.parameters) == ["self", "limit"] and sig.parameters["limit"].default == 1.0
    assert list(inspect.signature(RoutingPlan.stream_courant).parameters) == ["self"]
    p = inspect.signature(RouteStream.__init__).parameters
    assert p["courant"].default is None
    # (what was there keeps its place and its default)
    assert list(p)[:4] == ["self", "router", "nsteps", "qts_subdivisions"] and list(p)[-2:] == ["stage", "exceedance"]
    assert p["stage"].default is False and p["exceedance"].default is None and p["summary"].default is None
    assert isinstance(inspect.getattr_static(RouteStream, "courant"), property)


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
    for bad in ("1.0", b"1", [1.0], (1.0,), np.ones(2), {}, True, 1j, object()):
        with pytest.raises(ValueError, match="real number"):
            p.stream_set_courant(bad)
        with pytest.raises(ValueError, match="real number"):
            RouteStream(NoRouter(), 24, 8, courant=bad)
    with pytest.raises(NotImplementedError, match="several ranks"):
        RouteStream(TwoRanks(), 24, 8, courant=1.0)
    with pytest.raises(NotImplementedError, match="reservoir data assimilation"):
        RouteStream(WithReservoirDa(), 24, 8, courant=1.0)
    p.engine = "flow"
    with pytest.raises(ValueError, match="level engine"):
        p.stream_set_courant(1.0)
    assert not called
    for good in (1, 1.0, 0.5, np.float32(2), np.int64(3), -1.0):                # (accepted: nothing is set before route())
        rs = RouteStream(NoRouter(), 24, 8, courant=good)
        assert rs.courant is None and rs.exceedance is None and rs.total is None
    assert RouteStream(NoRouter(), 24, 8).courant is None
    assert RouteStream(TwoRanks(), 24, 8, comm=object()).courant is None         # (several ranks without it: as before)
    assert not called
    p._h = None                                                                  # (nothing for __del__ to release)


def test_the_stream_product_table_the_day_struct_and_the_abi_are_untouched():
    assert _lib.lib().trmc_abi_version() == 19
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    assert len(stream_products.PRODUCTS) == 12
    assert stream_products.ALL == stream_products.PRODUCTS + (stream_products.STAGE,)
    assert not any("courant" in q.name or "cn" in q.name.split("_") for q in stream_products.ALL)
    assert C.sizeof(_lib.StreamDay) == 152
    body = re.search(r"typedef\s+struct\s+trmc_stream_day\s*\{(.*?)\}\s*trmc_stream_day\s*;", code(), flags=re.S).group(1)
    assert "courant" not in body
