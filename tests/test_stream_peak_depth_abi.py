"""The C ABI of the peak depth of a day and of the totals over the days of a stream (include/trmc.h TRMC_SUMMARY_PEAK_DEPTH,
TRMC_SUMMARY_TOTAL, trmc_stream_summary_depth_dest, trmc_stream_summary_total): additions WITHIN ABI 19 -- two new functions, two
new mask bits, no new member of trmc_stream_day, the functions of the summary with the signatures they had.  No GPU here: the
header, the library's exports and the ctypes table."""
import ctypes as C
import os
import re

from troute_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trmc_stream_summary_depth_dest", "trmc_stream_summary_total")


def code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trmc.h")).read(), flags=re.S)


def test_the_header_declares_the_two_functions_and_the_two_mask_bits():
    c = code()
    w, vp = r"\s*\w+\s*", r"\s*void\s*\*"
    assert re.search(r"\bint\s+trmc_stream_summary_depth_dest\s*\(\s*trmc_plan\s*\*" + w + "," + vp + w + r",\s*int32_t\s*\*" + w + r"\)\s*;", c)
    assert re.search(r"\bint\s+trmc_stream_summary_total\s*\(\s*trmc_plan\s*\*" + w + "," + vp + w + r",\s*int64_t\s*\*" + w + "," + vp + w + ","
                     + vp + w + r",\s*int64_t\s*\*" + w + r",\s*int64_t\s*\*" + w + r"\)\s*;", c)
    assert re.search(r"\bTRMC_SUMMARY_PEAK_DEPTH\s*=\s*4\b", c) and re.search(r"\bTRMC_SUMMARY_TOTAL\s*=\s*8\b", c)
    assert re.search(r"\bTRMC_SUMMARY_PEAK\s*=\s*1\b", c) and re.search(r"\bTRMC_SUMMARY_MEAN\s*=\s*2\b", c)
    assert (_lib.SUMMARY_PEAK, _lib.SUMMARY_MEAN, _lib.SUMMARY_PEAK_DEPTH, _lib.SUMMARY_TOTAL) == (1, 2, 4, 8)
    assert _lib.SUMMARY_NAMES == {"peak": 1, "mean": 2, "peak_depth": 4, "total": 8}
    # the summary's own two functions keep their signatures
    assert re.search(r"\bint\s+trmc_stream_set_summary\s*\(\s*trmc_plan\s*\*" + w + r",\s*int" + r"\s+\w+\s*\)\s*;", c)
    assert re.search(r"\bint\s+trmc_stream_summary_dest\s*\(\s*trmc_plan\s*\*" + w + "," + vp + w + r",\s*int32_t\s*\*" + w + "," + vp + w + r"\)\s*;", c)
    assert re.search(r"\bTRMC_EUNSUPPORTED\s*=\s*-7\b", c) and _lib.TRMC_EUNSUPPORTED == -7


def test_the_library_exports_them_and_ctypes_knows_their_signatures():
    lib = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), f"{name} is not exported by libtrmc.so"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    vp = C.c_void_p
    assert _lib.SIGNATURES["trmc_stream_summary_depth_dest"] == (C.c_int, [vp, vp, vp])
    assert _lib.SIGNATURES["trmc_stream_summary_total"] == (C.c_int, [vp] * 7)
    assert _lib.SIGNATURES["trmc_stream_set_summary"] == (C.c_int, [vp, C.c_int])
    assert _lib.SIGNATURES["trmc_stream_summary_dest"] == (C.c_int, [vp, vp, vp, vp])
    # (a NULL plan is refused before anything touches a device)
    assert raw.trmc_stream_summary_depth_dest(None, None, None) != 0
    assert raw.trmc_stream_summary_total(None, None, None, None, None, None, None) != 0
    assert raw.trmc_stream_set_summary(None, 15) != 0


def test_abi_19_and_the_day_struct_keep_their_shape():
    assert _lib.lib().trmc_abi_version() == 19
    assert C.sizeof(_lib.StreamDay) == 152
    body = re.search(r"typedef\s+struct\s+trmc_stream_day\s*\{(.*?)\}\s*trmc_stream_day\s*;", code(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?(\w+)$", r"\1", part.strip()) for part in decl.split(",")]
    assert names == [n for n, _ in _lib.StreamDay._fields_]
    assert not any("depth" in n or "total" in n or "summary" in n for n in names)
