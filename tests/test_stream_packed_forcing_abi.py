"""The C ABI and the Python surface of a stream day pushed as packed CHRTOUT columns (include/trmc.h trmc_stream_set_packed_forcing,
trmc_stream_push_day_packed, trmc_stream_packed_forcing_kernel_ms; RoutingPlan.stream_set_packed_forcing, ``packed=`` of
RoutingPlan.stream_push, ``packed_forcing=`` of RouteStream): additions WITHIN ABI 19 -- new functions only, no existing prototype
changed, no new member of trmc_stream_day.  No GPU here: the header, the library's exports, the ctypes table, the signatures and
the errors Python raises before the library is called."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from troute_amd import _lib
from troute_amd.plan import RoutingPlan
from troute_amd.sequence import RouteStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trmc_stream_set_packed_forcing", "trmc_stream_push_day_packed", "trmc_stream_packed_forcing_kernel_ms")
NFEAT = 9


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_prototypes_behind_the_day_push():
    plan = r"\(\s*trmc_plan\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+trmc_stream_set_packed_forcing\s*" + plan + r",\s*int64_t\s+\w+\s*,\s*const\s+int64_t\s*\*\s*\w+\s*,\s*const\s+double\s*\*"
                     r"\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)\s*;", code())
    assert re.search(r"\bint\s+trmc_stream_push_day_packed\s*" + plan + r",\s*const\s+trmc_stream_day\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*\)\s*;", code())
    assert re.search(r"\bint\s+trmc_stream_packed_forcing_kernel_ms\s*" + plan + r",\s*double\s*\*\s*\w+\s*\)\s*;", code())
    assert re.search(r"#define\s+TRMC_ABI_VERSION\s+19\b", code())
    assert code().index("trmc_stream_push_day(") < code().index("trmc_stream_set_packed_forcing") < code().index("trmc_stream_push_day_packed")
    text = open(os.path.join(ROOT, "include", "trmc.h")).read()
    doc = text[text.index("A STREAM DAY AS PACKED CHRTOUT COLUMNS"):text.index("int trmc_stream_set_packed_forcing")]
    for word in ("TRMC_ESTATE", "TRMC_EINVAL", "feat_of_row", "pack_b", "page-locked", "trmc_upload_forcing_packed", "alternate"):
        assert word in doc, word


def test_the_library_exports_them_and_ctypes_knows_the_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp = C.c_void_p
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["trmc_stream_set_packed_forcing"] == (C.c_int, [vp, C.c_int64, vp, vp, vp])
    assert _lib.SIGNATURES["trmc_stream_push_day_packed"] == (C.c_int, [vp, vp, vp, vp])
    assert _lib.SIGNATURES["trmc_stream_packed_forcing_kernel_ms"] == (C.c_int, [vp, C.POINTER(C.c_double)])
    # (a NULL plan is refused before anything touches a device)
    raw.trmc_stream_set_packed_forcing.argtypes = [vp, C.c_int64, vp, vp, vp]
    assert raw.trmc_stream_set_packed_forcing(None, 0, None, None, None) == _lib.TRMC_EINVAL
    assert raw.trmc_stream_push_day_packed(None, None, None, None) == _lib.TRMC_EINVAL
    assert raw.trmc_stream_packed_forcing_kernel_ms(None, None) == _lib.TRMC_EINVAL
    assert lib.trmc_abi_version() == 19


def test_the_abi_version_and_the_day_struct_are_untouched():
    assert _lib.lib().trmc_abi_version() == 19
    assert C.sizeof(_lib.StreamDay) == 152
    body = re.search(r"typedef\s+struct\s+trmc_stream_day\s*\{(.*?)\}\s*trmc_stream_day\s*;", code(), flags=re.S).group(1)
    assert "raw" not in body and "pack" not in body
    assert not any("raw" in n or "pack" in n for n, _ in _lib.StreamDay._fields_)
    # ONE rule: the window's kernel and the stream's call the same device function
    src = open(os.path.join(ROOT, "t-route_amd", "csrc", "kernels_levels.inc")).read()
    assert src.count("ingest_packed_at<T>(") == 2 and src.count("unpack_cf(") == 3


def test_the_python_surface_and_its_defaults():
    sig = inspect.signature(RoutingPlan.stream_set_packed_forcing)
    assert list(sig.parameters) == ["self", "packed", "row_ids"]
    p = inspect.signature(RoutingPlan.stream_push).parameters
    assert p["packed"].default is None and p["qlat"].default is None
    assert list(p)[:2] == ["self", "qlat"] and list(p)[-2:] == ["summary", "stage"]     # (what was there keeps its place)
    p = inspect.signature(RouteStream.__init__).parameters
    assert p["packed_forcing"].default is None
    assert list(p)[:4] == ["self", "router", "nsteps", "qts_subdivisions"] and list(p)[-2:] == ["stage", "exceedance"]


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


def library_must_not_be_called(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "lib", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("the library was called")))
    return called


def day(two=True, nq=2, nfeat=NFEAT, dtype=np.int32):
    return {"raw_a": np.zeros((nq, nfeat), dtype), "raw_b": np.zeros((nq, nfeat), dtype) if two else None}


def test_python_refuses_what_it_can_before_the_library_is_called(monkeypatch):
    called = library_must_not_be_called(monkeypatch)
    qlat = np.zeros((6, 2), np.float32)
    files = {"feature_id": np.arange(100, 100 + NFEAT), "pack_a": np.zeros(6), "pack_b": np.zeros(6)}
    # the dataflow engine runs no stream
    p = handle_free_plan(engine="flow")
    with pytest.raises(ValueError, match="level engine"):
        p.stream_set_packed_forcing(files, np.arange(6))
    p._h = None
    p = handle_free_plan()
    # the ids of the rows: one per row
    for bad in (np.arange(5), np.arange(7), np.zeros((6, 1), np.int64)):
        with pytest.raises(ValueError, match=r"row_ids must be \[nseg\]"):
            p.stream_set_packed_forcing(files, bad)
    # a packed day before the declaration
    with pytest.raises(RuntimeError, match="stream_set_packed_forcing precedes stream_begin"):
        p.stream_push(packed=day())
    # a day is the float array or the packed columns
    with pytest.raises(ValueError, match="either qlat or packed"):
        p.stream_push(qlat, packed=day())
    with pytest.raises(ValueError, match="qlat, or packed="):
        p.stream_push()
    p._stream_packed = (NFEAT, True)
    # the raw blocks: int32, C-contiguous, [nq, nfeat] of the declared axis, both of one shape, raw_b exactly when pack_b was declared
    wrong = (day(dtype=np.int64), day(dtype=np.float32), day(nfeat=NFEAT + 1), day(nfeat=NFEAT - 1),
             {"raw_a": np.zeros(2 * NFEAT, np.int32), "raw_b": np.zeros(2 * NFEAT, np.int32)},
             {"raw_a": np.zeros((NFEAT, 2), np.int32).T, "raw_b": np.zeros((2, NFEAT), np.int32)},
             {"raw_a": [[0] * NFEAT] * 2, "raw_b": np.zeros((2, NFEAT), np.int32)})
    for bad in wrong:
        with pytest.raises(ValueError, match=rf"raw_a must be a C-contiguous int32 array of shape \(nq, {NFEAT}\)"):
            p.stream_push(packed=bad)
    with pytest.raises(ValueError, match=r"raw_b must be a C-contiguous int32 array"):
        p.stream_push(packed={"raw_a": np.zeros((2, NFEAT), np.int32), "raw_b": np.zeros((2, NFEAT), np.int64)})
    with pytest.raises(ValueError, match="raw_a and raw_b must have one shape"):
        p.stream_push(packed={"raw_a": np.zeros((2, NFEAT), np.int32), "raw_b": np.zeros((3, NFEAT), np.int32)})
    with pytest.raises(ValueError, match="raw_b is required"):
        p.stream_push(packed=day(two=False))
    p._stream_packed = (NFEAT, False)
    with pytest.raises(ValueError, match="raw_b must be None"):
        p.stream_push(packed=day(two=True))
    # several ranks: refused with the reason
    with pytest.raises(NotImplementedError, match="(?s)several ranks.*join of their own"):
        RouteStream(TwoRanks(), 24, 8, packed_forcing=np.arange(6))
    with pytest.raises(ValueError, match=r"packed_forcing: the ids of the router's rows, \[6\]"):
        RouteStream(NoRouter(), 24, 8, packed_forcing=np.arange(5))
    assert not called
    assert RouteStream(NoRouter(), 24, 8, packed_forcing=np.arange(6))._pk_ids.dtype == np.int64
    assert RouteStream(NoRouter(), 24, 8, packed_forcing=(np.arange(6), files))._pk_like is files
    assert RouteStream(TwoRanks(), 24, 8, comm=object())._pk_ids is None        # (off: several ranks as before)
    p._h = None                                                                 # (nothing for __del__ to release)
