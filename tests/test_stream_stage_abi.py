"""The C ABI and the Python surface of the stage hydrographs of a stream day (include/trmc.h trmc_stream_set_stage,
trmc_stream_stage_dest; RoutingPlan.stream_set_stage, ``stage=`` of RoutingPlan.stream_push and of RouteStream): additions WITHIN
ABI 19 -- two new functions, no existing prototype changed, no new member of trmc_stream_day.  No GPU here: the header, the
library's exports, the ctypes table, the signatures and the errors Python raises before the library is called."""
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
NAMES = ("trmc_stream_set_stage", "trmc_stream_stage_dest")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes_next_to_the_exceedance_block():
    plan = r"\(\s*trmc_plan\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+trmc_stream_set_stage\s*" + plan + r",\s*int\s+\w+\s*\)\s*;", code())
    assert re.search(r"\bint\s+trmc_stream_stage_dest\s*" + plan + r",\s*void\s*\*\s*\w+\s*\)\s*;", code())
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", code())
    assert code().index("trmc_stream_exceedance") < code().index("trmc_stream_set_stage") < code().index("trmc_stream_stage_dest")
    text = open(os.path.join(ROOT, "include", "trmc.h")).read()
    doc = text[text.index("STAGE HYDROGRAPHS"):text.index("int trmc_stream_set_stage")]
    for word in ("TRMC_ESTATE", "TRMC_EINVAL", "TRMC_EUNSUPPORTED", "row set", "reservoir"):
        assert word in doc, word


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_stream_set_stage"] == (C.c_int, [vp, C.c_int])
    assert _lib.SIGNATURES["trmc_stream_stage_dest"] == (C.c_int, [vp, vp])
    # (a NULL plan is refused before anything touches a device)
    for on in (0, 1):
        assert raw.trmc_stream_set_stage(None, on) == _lib.TRMC_EINVAL
    assert raw.trmc_stream_stage_dest(None, None) == _lib.TRMC_EINVAL
    assert lib.trmc_abi_version() == 19


def test_the_abi_version_the_day_struct_and_the_mirrored_table_are_untouched():
    assert _lib.lib().trmc_abi_version() == 19
    assert C.sizeof(_lib.StreamDay) == 152
    body = re.search(r"typedef\s+struct\s+trmc_stream_day\s*\{(.*?)\}\s*trmc_stream_day\s*;", code(), flags=re.S).group(1)
    assert "stage" not in body
    assert not any("stage" in n for n, _ in _lib.StreamDay._fields_)
    # the rows that mirror the device table's first enumeration stay twelve; stage stands behind them, as P_STAGE does behind P_N
    assert len(stream_products.PRODUCTS) == 12 and stream_products.STAGE not in stream_products.PRODUCTS
    assert stream_products.ALL == stream_products.PRODUCTS + (stream_products.STAGE,)
    s = stream_products.STAGE
    assert (s.name, s.push, s.pos, s.dtype, s.shape, s.on) == ("stage", "stage", None, stream_products.PLAN, ("outlets", "nsteps"), "stage")
    src = open(os.path.join(ROOT, "t-route_amd", "csrc", "stream.inc")).read()
    assert re.search(r"P_STAGE\s*=\s*P_N\s*,", src) and src.index("P_N\n") < src.index("P_STAGE = P_N")
    a = np.zeros((2, 3), np.float32)
    assert stream_products.push_keywords({"hyd": a, "stage": a}) == {"hyd": a, "stage": a}


def test_the_python_surface_and_its_defaults():
    sig = inspect.signature(RoutingPlan.stream_set_stage)
    assert list(sig.parameters) == ["self", "on"] and sig.parameters["on"].default is True
    p = inspect.signature(RoutingPlan.stream_push).parameters
    assert p["stage"].default is None and list(p)[-1] == "stage" and list(p)[-2] == "summary"
    p = inspect.signature(RouteStream.__init__).parameters
    assert p["stage"].default is False and list(p)[-2:] == ["stage", "exceedance"]
    # (what was there keeps its place and its default)
    assert list(p)[:4] == ["self", "router", "nsteps", "qts_subdivisions"] and p["exceedance"].default is None and p["summary"].default is None


def handle_free_plan(nseg=6, dtype=np.float32, engine="levels"):
    """a RoutingPlan object without a library handle: whatever reaches the library from it fails loudly"""
    p = object.__new__(RoutingPlan)
    p.nseg, p.dtype, p.precision, p.engine, p._nsteps = nseg, np.dtype(dtype).type, 32, engine, 24

    class NoHandle:
        def __getattr__(self, name):
            raise AssertionError("the library was called")
    p._h = NoHandle()
    return p


class NoRouter:
    nseg, world, rank = 6, 1, 0


class TwoRanks:
    nseg, world, rank = 6, 2, 0


class RouterWithReservoirDa:
    nseg, world, rank = 6, 1, 0
    _reservoir_da = (None,)


def library_must_not_be_called(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "lib", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("the library was called")))
    return called


def test_python_refuses_what_it_can_before_the_library_is_called(monkeypatch):
    called = library_must_not_be_called(monkeypatch)
    qlat = np.zeros((6, 2), np.float32)
    good = np.zeros((3, 24), np.float32)
    # the dataflow engine runs no stream
    p = handle_free_plan(engine="flow")
    with pytest.raises(ValueError, match="level engine"):
        p.stream_set_stage(True)
    p._h = None
    p = handle_free_plan()
    # a stream begun without stage takes no such array
    with pytest.raises(RuntimeError, match="begun without stage"):
        p.stream_push(qlat, rowset=0, stage=good)
    p._stream_stage = True
    p._rowset_n = {0: 3}
    # a day with no row set has no stage
    with pytest.raises(ValueError, match="rowset is required"):
        p.stream_push(qlat, stage=good)
    # the array: the plan's type, C-contiguous, two-dimensional, the set's rows by the day's steps
    for bad in (np.zeros((3, 24), np.float64), np.zeros((24, 3), np.float32).T, np.zeros(72, np.float32), [[0.0] * 24] * 3):
        with pytest.raises(ValueError, match="stage must be a C-contiguous float32 array"):
            p.stream_push(qlat, rowset=0, stage=bad)
    for bad in (np.zeros((2, 24), np.float32), np.zeros((3, 23), np.float32)):
        with pytest.raises(ValueError, match=r"stage must hold \[3, 24\]"):
            p.stream_push(qlat, rowset=0, stage=bad)
    # several ranks, and reservoir data assimilation: refused with the reason
    with pytest.raises(NotImplementedError, match="(?s)several ranks.*gathered over the ranks"):
        RouteStream(TwoRanks(), 24, 8, stage=True)
    with pytest.raises(NotImplementedError, match="reservoir data assimilation"):
        RouteStream(RouterWithReservoirDa(), 24, 8, stage=True)
    assert not called
    assert RouteStream(NoRouter(), 24, 8, stage=True).stage is True and RouteStream(NoRouter(), 24, 8).stage is False
    assert RouteStream(TwoRanks(), 24, 8, comm=object()).stage is False         # (off: several ranks as before)
    p._h = None                                                                 # (nothing for __del__ to release)
