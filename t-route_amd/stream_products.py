"""THE PRODUCTS A DAY OF A STREAM CAN HAND TO THE HOST -- the host half of the table in csrc/stream.inc (P_*, StreamRun::tab): one
row per product, in that order, and nothing else in the package lists them.  ``RoutingPlan.stream_push`` checks a day's
destinations against it and ``RoutingPlan.stream_summary_total`` takes the totals' parts from it; ``RouteStream`` allocates its
ring of page-locked destinations from it and builds the dict it yields from it.

A row says

  name    what the product is called: in a wrong destination's message, among a slot's arrays -- and, where ``keyed``, in the dict
          that ends ``RouteStream``'s tuples
  push    the keyword of ``stream_push`` it goes under, and ``pos``: its place in that keyword's tuple (None: the array itself)
  dtype   PLAN (the plan's precision) or a numpy type
  shape   extents by name -- rows, nsteps, keep (the steps an output stride keeps), outlets, nres, ngage -- or as numbers
  on      when a stream carries it: None (always) or what the stream must have -- "fvd" (full_output / output_stride), "ngage",
          "nres", "rda" (reservoir data assimilation), "stage" (stage hydrographs), or the word of ``SUMMARY_NAMES`` that asks for the part
  total   (summary parts) the type of the part's total over the days
  wrong   what ``stream_push`` says of a destination that does not fit (None: the library checks it)

A new product: its enumerator and row in stream.inc, and its row here.
"""
from collections import namedtuple

import numpy as np

PLAN = "plan"
Product = namedtuple("Product", "name push pos dtype shape on keyed total wrong")

_RECORD = "{name} must be a C-contiguous {plan} array [rows, nsteps]"
_RDA = "reservoir_da_state must be (float32 [{nres}, 4], int32 [{nres}]), C-contiguous"
_STAGE = "stage must be a C-contiguous {plan} array [rows of the day's row set, nsteps]"
_PART = "summary: {name} must be a C-contiguous {dtype} array of shape ({rows},)"

PRODUCTS = (
    Product("hyd", "hyd", None, PLAN, ("outlets", "nsteps"), None, False, None, None),
    Product("q0", "q0", None, PLAN, ("rows", 3), None, False, None, None),
    Product("fvd", "fvd", None, PLAN, ("rows", "keep", 3), "fvd", False, None, None),
    Product("nudge", "nudge", None, PLAN, ("ngage", "nsteps"), "ngage", True, None, _RECORD),
    Product("reservoir_inflow", "reservoir_inflow", None, PLAN, ("nres", "nsteps"), "nres", True, None, _RECORD),
    Product("reservoir_da_state", "reservoir_da_state", 0, np.float32, ("nres", 4), "rda", False, None, _RDA),
    Product("reservoir_da_tsidx", "reservoir_da_state", 1, np.int32, ("nres",), "rda", False, None, _RDA),
    Product("peak_flow", "summary", 0, PLAN, ("rows",), "peak", True, PLAN, _PART),
    Product("peak_step", "summary", 1, np.int32, ("rows",), "peak", True, np.int64, _PART),
    Product("mean_flow", "summary", 2, PLAN, ("rows",), "mean", True, PLAN, _PART),
    Product("peak_depth", "summary", 3, PLAN, ("rows",), "peak_depth", True, PLAN, _PART),
    Product("peak_depth_step", "summary", 4, np.int32, ("rows",), "peak_depth", True, np.int64, _PART),
)
# ... and, behind the rows that mirror the device table's first enumeration one for one, the products whose destination a call of
# its own names (stream.inc, P_STAGE on): checked, allocated and pushed as the rows above are
STAGE = Product("stage", "stage", None, PLAN, ("outlets", "nsteps"), "stage", False, None, _STAGE)
ALL = PRODUCTS + (STAGE,)
SUMMARY = tuple(p for p in PRODUCTS if p.push == "summary")
# the records of reservoirs and gages, in the order RouteStream's dict has always had them (the inflows first)
RECORDS = tuple(sorted((p for p in PRODUCTS if p.keyed and p not in SUMMARY), key=lambda p: p.name != "reservoir_inflow"))
# a summary tuple holds what ONE call of the library names: trmc_stream_summary_dest's three, or those and _depth_dest's two
SUMMARY_LENGTHS = (3, len(SUMMARY))
SUMMARY_WRONG = "summary must be ({}[, {}]); any may be None".format(*(", ".join(p.name for p in part) for part in (SUMMARY[:3], SUMMARY[3:])))


def dtype_of(p, plan_dtype, total=False):
    t = p.total if total else p.dtype
    return np.dtype(plan_dtype if t == PLAN else t)


def shape_of(p, dims):
    """the row's extents with ``dims`` for the names (a name that ``dims`` lacks: None, any extent)"""
    return tuple(dims.get(n) if isinstance(n, str) else n for n in p.shape)


def given(p, keywords):
    """the product's destination among ``stream_push``'s keywords (None: not asked for)"""
    v = keywords.get(p.push)
    if v is None or p.pos is None:
        return v
    return v[p.pos] if p.pos < len(v) else None


def fits(p, array, plan_dtype, dims):
    """``stream_push``'s check of a destination: type, layout, and the extents of a tuple's member -- a record's own extents
    are the library's to check, against the day's tables"""
    shape = shape_of(p, dims if p.pos is not None else {})
    return (isinstance(array, np.ndarray) and array.dtype == dtype_of(p, plan_dtype) and array.flags.c_contiguous
            and array.ndim == len(shape) and all(n in (None, m) for n, m in zip(shape, array.shape)))


def wrong(p, plan_dtype, dims):
    return p.wrong.format(name=p.name, plan=np.dtype(plan_dtype).name, dtype=dtype_of(p, plan_dtype).name, **dims)


def push_keywords(arrays):
    """``stream_push``'s keywords for a slot's arrays {name: array}: a product the slot lacks is left out (in a tuple: None)"""
    kw = {}
    for p in ALL:
        if arrays.get(p.name) is None:
            continue
        if p.pos is None:
            kw[p.push] = arrays[p.name]
        else:
            members = kw.setdefault(p.push, [])
            members += [None] * (p.pos - len(members)) + [arrays[p.name]]
    if "summary" in kw:
        n = len(kw["summary"])
        kw["summary"] += [None] * (min(g for g in SUMMARY_LENGTHS if g >= n) - n)
    return {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}
