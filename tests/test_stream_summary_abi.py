"""The C ABI of the per-row day summary of a stream (include/trmc.h trmc_stream_set_summary, trmc_stream_summary_dest): additions
WITHIN ABI 19 -- new functions, no new member of trmc_stream_day (which has no reserved member left), the version unchanged.  No
GPU here: the header, the library's exports and the ctypes table."""
import ctypes as C
import os
import re

from troute_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trmc_stream_set_summary", "trmc_stream_summary_dest")


def header():
    return open(os.path.join(ROOT, "include", "trmc.h")).read()


def test_the_header_declares_the_summary_functions_and_the_mask():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+trmc_stream_set_summary\s*\(\s*trmc_plan\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+trmc_stream_summary_dest\s*\(\s*trmc_plan\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"\bTRMC_SUMMARY_PEAK\s*=\s*1\b", code) and re.search(r"\bTRMC_SUMMARY_MEAN\s*=\s*2\b", code)
    assert (_lib.SUMMARY_PEAK, _lib.SUMMARY_MEAN) == (1, 2)


def test_the_library_exports_them_and_ctypes_knows_their_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    vp = C.c_void_p
    assert _lib.SIGNATURES["trmc_stream_set_summary"] == (C.c_int, [vp, C.c_int])
    assert _lib.SIGNATURES["trmc_stream_summary_dest"] == (C.c_int, [vp, vp, vp, vp])
    # (a NULL plan is refused before anything touches a device)
    assert raw.trmc_stream_set_summary(None, 3) != 0
    assert raw.trmc_stream_summary_dest(None, None, None, None) != 0


def test_abi_19_and_the_day_struct_keep_their_shape():
    assert _lib.lib().trmc_abi_version() == 19
    # (17 pointers and 64-bit counts and two pairs of int32: 152 bytes, what a C compiler gives the header's struct before and
    # after the summary was added)
    assert C.sizeof(_lib.StreamDay) == 19 * 8 == 152
    # the header's struct, member by member, against the Python mirror: nothing was added to it for the summary
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+trmc_stream_day\s*\{(.*?)\}\s*trmc_stream_day\s*;", code, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?(\w+)$", r"\1", part.strip()) for part in decl.split(",")]
    assert names == [n for n, _ in _lib.StreamDay._fields_]
    assert not any("peak" in n or "mean" in n or "summary" in n for n in names)
