"""RoutingPlan -- Python handle of a trmc_plan (include/trmc.h).

A plan owns the flattened topology and the channel parameters in HBM; one plan
serves any number of routing windows (the reference rebuilds its MC_Segment /
MC_Reach objects on every compute_network_structured call,
mc_reach.pyx:283-378).
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import stream_products as SP


def csr_from_lists(lists):
    """[[rows...], ...] -> (ptr int64[n+1], idx int64[nnz])"""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.fromiter((v for x in lists for v in x), dtype=np.int64, count=int(ptr[-1]))
    return ptr, idx


def topology_levels(up_ptr, up_idx, boundary=None, cost_hint=None):
    """Host-only level flattening (no GPU).  Returns (level_of_row, plan_pos_of_row, nlevels)."""
    up_ptr = np.ascontiguousarray(up_ptr, dtype=np.int64)
    up_idx = np.ascontiguousarray(up_idx, dtype=np.int64)
    nseg = up_ptr.shape[0] - 1
    b = None if boundary is None else np.ascontiguousarray(boundary, dtype=np.uint8)
    lvl = np.empty(nseg, dtype=np.int32)
    pos = np.empty(nseg, dtype=np.int64)
    nl = C.c_int32(0)
    h = None if cost_hint is None else np.ascontiguousarray(cost_hint, dtype=np.uint8)
    _lib.check(_lib.lib().trmc_topology_levels_hinted(nseg, _lib.ptr(up_ptr), _lib.ptr(up_idx), _lib.ptr(b), _lib.ptr(h),
                                                      _lib.ptr(lvl), _lib.ptr(pos), C.byref(nl)))
    return lvl, pos, nl.value


def topology_blocks(up_ptr, up_idx, boundary=None, cost_hint=None, cost_tiers=True):
    """Host-only block order of the dataflow engine (no GPU).  Returns (plan_pos_of_row, rank_of_row, block_rows, nblocks)."""
    up_ptr = np.ascontiguousarray(up_ptr, dtype=np.int64)
    up_idx = np.ascontiguousarray(up_idx, dtype=np.int64)
    nseg = up_ptr.shape[0] - 1
    b = None if boundary is None else np.ascontiguousarray(boundary, dtype=np.uint8)
    h = None if cost_hint is None else np.ascontiguousarray(cost_hint, dtype=np.uint8)
    pos = np.empty(nseg, dtype=np.int64)
    rank = np.empty(nseg, dtype=np.int32)
    br, nb = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().trmc_topology_blocks(nseg, _lib.ptr(up_ptr), _lib.ptr(up_idx), _lib.ptr(b), _lib.ptr(h),
                                               int(bool(cost_tiers)), _lib.ptr(pos), _lib.ptr(rank), C.byref(br),
                                               C.byref(nb)))
    return pos, rank, br.value, nb.value


def topology_clusters(up_ptr, up_idx, boundary=None, cost_hint=None, wide_min_rows=0, wide_max_levels=16, cluster_rows=128):
    """Host-only cluster order of a short-timestep plan of the level engine (no GPU; csrc/topology.hpp).  Returns
    (plan_pos_of_row, lag_of_row, block_of_row, wide_levels, cluster_levels, cluster_blocks)."""
    up_ptr = np.ascontiguousarray(up_ptr, dtype=np.int64)
    up_idx = np.ascontiguousarray(up_idx, dtype=np.int64)
    nseg = up_ptr.shape[0] - 1
    b = None if boundary is None else np.ascontiguousarray(boundary, dtype=np.uint8)
    h = None if cost_hint is None else np.ascontiguousarray(cost_hint, dtype=np.uint8)
    pos = np.empty(nseg, dtype=np.int64)
    lag = np.empty(nseg, dtype=np.int32)
    blk = np.empty(nseg, dtype=np.int32)
    w, c, nb = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().trmc_topology_clusters(nseg, _lib.ptr(up_ptr), _lib.ptr(up_idx), _lib.ptr(b), _lib.ptr(h),
                                                 int(wide_min_rows), int(wide_max_levels), int(cluster_rows), _lib.ptr(pos),
                                                 _lib.ptr(lag), _lib.ptr(blk), C.byref(w), C.byref(c), C.byref(nb)))
    return pos, lag, blk, w.value, c.value, nb.value


def topology_blocks_general(up_ptr, up_idx, boundary=None, stem_min_rows=1024):
    """Host-only block order of a dataflow plan built for the general mode (no GPU): long stems last in their basin, their
    side tributaries from the top down.  Returns (plan_pos_of_row, rank_of_row, block_rows, nblocks, early_blocks)."""
    up_ptr = np.ascontiguousarray(up_ptr, dtype=np.int64)
    up_idx = np.ascontiguousarray(up_idx, dtype=np.int64)
    nseg = up_ptr.shape[0] - 1
    b = None if boundary is None else np.ascontiguousarray(boundary, dtype=np.uint8)
    pos = np.empty(nseg, dtype=np.int64)
    rank = np.empty(nseg, dtype=np.int32)
    early = np.empty(256, dtype=np.int32)
    br, nb, ne = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().trmc_topology_blocks_general(nseg, _lib.ptr(up_ptr), _lib.ptr(up_idx), _lib.ptr(b), int(stem_min_rows),
                                                       _lib.ptr(pos), _lib.ptr(rank), C.byref(br), C.byref(nb),
                                                       _lib.ptr(early), early.shape[0], C.byref(ne)))
    return pos, rank, br.value, nb.value, early[:min(ne.value, early.shape[0])].copy()


class RoutingPlan:
    def __init__(self, up_ptr, up_idx, params, boundary=None, precision=32, device=0, cost_hint=None,
                 assume_short_ts=None, engine="auto", options=None):
        """
        options       : dict of trmc_plan_options fields (include/trmc.h), e.g. {"arithmetic": "tolerance"} or
                        {"wide_min_rows": 32, "wide_k": 8}; the TRMC_* variables of ``_lib.OPTION_ENV`` (tests, A/B runs)
                        fill what the dict leaves out.  ``engine="auto"`` also honours TRMC_ENGINE=levels|flow.
        assume_short_ts : the timestep mode the plan will be routed with, if known (None: unknown) -- it routes
                        correctly either way, the value picks the row order that is fast for the mode
        engine        : "auto" | "levels" | "flow"  (include/trmc.h, trmc_plan_create_ex)
        up_ptr/up_idx : CSR of upstream rows per row, reference summation order
        params        : float32 [nseg, 9] in _lib.PARAM_COLS order
        boundary      : optional bool/uint8 [nseg], rows with prescribed hydrographs
        cost_hint     : optional uint8 [nseg], e.g. ``download_iterations()`` of a plan of the same network after
                        a window: rows of equal cost are placed together inside their level (results unchanged)
        """
        self._h = C.c_void_p(0)
        up_ptr = np.ascontiguousarray(up_ptr, dtype=np.int64)
        up_idx = np.ascontiguousarray(up_idx, dtype=np.int64)
        params = np.ascontiguousarray(params, dtype=np.float32)
        nseg = up_ptr.shape[0] - 1
        if params.shape != (nseg, _lib.NPARAM):
            raise ValueError("data_values shape mismatch")
        b = None if boundary is None else np.ascontiguousarray(boundary, dtype=np.uint8)
        if b is not None and b.shape != (nseg,):
            raise ValueError("boundary mask shape mismatch")
        self.nseg = nseg
        self.precision = precision
        self.dtype = _lib.np_dtype(precision)
        self.nboundary = 0 if b is None else int(np.count_nonzero(b == 1))   # (2 = a routed row kept out of the leading levels)
        hint = None if cost_hint is None else np.ascontiguousarray(cost_hint, dtype=np.uint8)
        if hint is not None and hint.shape != (nseg,):
            raise ValueError("cost_hint shape mismatch")
        h = C.c_void_p(0)
        if engine == "auto" and precision == 32 and os.environ.get("TRMC_ENGINE"):       # (A/B runs; fp64 plans: level engine)
            engine = os.environ["TRMC_ENGINE"]
            if engine not in ("levels", "flow"):
                raise ValueError("TRMC_ENGINE must be 'flow' or 'levels'")
        flags = {"auto": _lib.ENGINE_AUTO, "levels": _lib.ENGINE_LEVELS, "flow": _lib.ENGINE_FLOW}[engine]
        if assume_short_ts is not None:
            flags |= _lib.PLAN_SHORT_TS if assume_short_ts else _lib.PLAN_FULL_TS
        opt = _lib.plan_options(options)
        _lib.mark_hip_started()
        _lib.check(_lib.lib().trmc_plan_create_opt(nseg, _lib.ptr(up_ptr), _lib.ptr(up_idx), _lib.ptr(params),
                                                   _lib.ptr(b), _lib.ptr(hint), precision, device, flags, C.byref(opt),
                                                   C.byref(h)))
        self._h = h
        self.arithmetic = "tolerance" if opt.arithmetic == _lib.ARITH_TOLERANCE else "exact"
        self.tile_steps = int(opt.wide_k) if opt.wide_k > 0 else 16          # steps per tile launch (trmc_plan_options.wide_k)
        f = C.c_int32(0)
        _lib.check(_lib.lib().trmc_plan_engine(self._h, C.byref(f)))
        self.engine = "flow" if f.value else "levels"
        self._nsteps = None
        self._stream_keep = {}
        self._th_levels = 0                                                 # levels of set_thresholds (0: none set)
        self.maxlag = 0

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().trmc_plan_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- facts ------------------------------------------------------------------------
    def info(self):
        nseg, nr = C.c_int64(0), C.c_int64(0)
        nl, pr, dev = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib().trmc_plan_info(self._h, C.byref(nseg), C.byref(nr), C.byref(nl), C.byref(pr),
                                             C.byref(dev)))
        return {"nseg": nseg.value, "nseg_routed": nr.value, "nlevels": nl.value, "precision": pr.value,
                "device": dev.value}

    def levels(self):
        lvl = np.empty(self.nseg, dtype=np.int32)
        pos = np.empty(self.nseg, dtype=np.int64)
        _lib.check(_lib.lib().trmc_plan_levels(self._h, _lib.ptr(lvl), _lib.ptr(pos)))
        return lvl, pos

    def lags(self):
        """A plan in cluster order: (tiles every row runs behind the headwaters [-1: boundary row], levels kept as slices,
        cluster levels) -- include/trmc.h, trmc_plan_lags."""
        lag = np.empty(self.nseg, dtype=np.int32)
        w, c = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib().trmc_plan_lags(self._h, _lib.ptr(lag), C.byref(w), C.byref(c)))
        return lag, w.value, c.value

    def cluster_blocks(self):
        """A plan in cluster order: (the cluster block that routes every row [-1: a row of the slices, a boundary row], the most
        rows a block holds, the number of blocks) -- include/trmc.h, trmc_plan_cluster_blocks."""
        blk = np.empty(self.nseg, dtype=np.int32)
        w, nb = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib().trmc_plan_cluster_blocks(self._h, _lib.ptr(blk), C.byref(w), C.byref(nb)))
        return blk, w.value, nb.value

    def stats(self):
        s = _lib.Stats()
        _lib.check(_lib.lib().trmc_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- one routing window -------------------------------------------------------------
    def upload_forcing(self, nsteps, qlat, q0, boundary_fvd=None):
        qlat = np.ascontiguousarray(qlat, dtype=self.dtype)
        if qlat.ndim != 2 or qlat.shape[0] != self.nseg:
            raise ValueError(f"Number of rows in Qlat is incorrect: expected ({self.nseg}), got ({qlat.shape[0]})")
        if q0 is not None:                       # None: continue from the state resident in HBM
            q0 = np.ascontiguousarray(q0, dtype=self.dtype)
            if q0.shape != (self.nseg, 3):
                raise ValueError("initial_conditions shape mismatch")
        bf = None
        if self.nboundary and boundary_fvd is not None:   # None: set_boundary_flow_device() follows
            bf = np.ascontiguousarray(boundary_fvd, dtype=self.dtype)
            if bf.shape != (self.nboundary, nsteps, 3):
                raise ValueError("boundary hydrograph shape mismatch")
        _lib.check(_lib.lib().trmc_upload_forcing(self._h, nsteps, _lib.ptr(qlat), qlat.shape[1], _lib.ptr(q0),
                                                  _lib.ptr(bf)))
        self._nsteps = nsteps

    def _feat_of_row(self, packed, row_ids):
        """the join of packed CHRTOUT columns on the feature id: the index of every row on the files' feature axis, -1 where the
        files do not hold the row (int64 [nseg])"""
        feat = np.asarray(packed["feature_id"], dtype=np.int64)
        row_ids = np.asarray(row_ids, dtype=np.int64)
        if row_ids.shape != (self.nseg,):
            raise ValueError("row_ids must be [nseg]")
        order = np.argsort(feat, kind="stable")
        where = np.searchsorted(feat[order], row_ids)
        where = np.clip(where, 0, max(0, feat.shape[0] - 1))
        hit = feat[order][where] == row_ids if feat.size else np.zeros(self.nseg, dtype=bool)
        return np.where(hit, order[where], -1).astype(np.int64)

    def upload_forcing_packed(self, nsteps, packed, row_ids, q0, boundary_fvd=None):
        """Forcing straight from packed CHRTOUT columns (``nhd_io.chrtout_packed``): the device decodes, joins
        on feature id and lays the forcing out.  row_ids: int64 [nseg] id of every row of the table."""
        feat_of_row = self._feat_of_row(packed, row_ids)
        raw_a = np.ascontiguousarray(packed["raw_a"], dtype=np.int32)
        raw_b = None if packed["raw_b"] is None else np.ascontiguousarray(packed["raw_b"], dtype=np.int32)
        pa = np.ascontiguousarray(packed["pack_a"], dtype=np.float64)
        pb = None if packed["pack_b"] is None else np.ascontiguousarray(packed["pack_b"], dtype=np.float64)
        if q0 is not None:
            q0 = np.ascontiguousarray(q0, dtype=self.dtype)
            if q0.shape != (self.nseg, 3):
                raise ValueError("initial_conditions shape mismatch")
        bf = None
        if self.nboundary and boundary_fvd is not None:
            bf = np.ascontiguousarray(boundary_fvd, dtype=self.dtype)
        _lib.check(_lib.lib().trmc_upload_forcing_packed(
            self._h, nsteps, raw_a.shape[0], raw_a.shape[1], _lib.ptr(raw_a), _lib.ptr(raw_b), _lib.ptr(pa),
            _lib.ptr(pb), _lib.ptr(feat_of_row), _lib.ptr(q0), _lib.ptr(bf)))
        self._nsteps = nsteps
        return feat_of_row

    def set_boundary_flow_device(self, nsteps, device_ptr):
        """Boundary rows' flow hydrographs from a device buffer [nboundary][nsteps] (plan precision)."""
        _lib.check(_lib.lib().trmc_set_boundary_flow_device(self._h, nsteps, C.c_void_p(device_ptr)))

    def set_reservoirs(self, res_rows, par, routing_period):
        """Level-pool reservoirs: rows [nres], parameters [nres, 9] (include/trmc.h trmc_set_reservoirs)."""
        res_rows = np.ascontiguousarray(res_rows, dtype=np.int64)
        par = np.ascontiguousarray(par, dtype=self.dtype)
        if par.shape != (res_rows.shape[0], 9):
            raise ValueError("reservoir parameters must be [nres, 9]")
        self._nres = res_rows.shape[0]
        _lib.check(_lib.lib().trmc_set_reservoirs(self._h, self._nres, _lib.ptr(res_rows), _lib.ptr(par),
                                                  float(routing_period)))

    def set_reservoir_da(self, kind, table_row, usgs=None, usace=None, rfc=None):
        """Data-assimilation tables of the plan's reservoirs for the staged window (include/trmc.h trmc_set_reservoir_da;
        after set_reservoirs).  kind / table_row [nres]; usgs, usace: None or (obs [n, ncol], time [ncol], state [n, 4]);
        rfc: None or (series [n, ncol], update_time [n], ipar [n, 5])."""
        if self.precision != 32:
            raise NotImplementedError("reservoir data assimilation (reservoir types 2..5) on a precision 64 plan: the reference "
                                      "has no double-precision form of this branch")
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        table_row = np.ascontiguousarray(table_row, dtype=np.int32)
        if kind.shape != (getattr(self, "_nres", 0),) or table_row.shape != kind.shape:
            raise ValueError("kind and table_row must be [nres] of set_reservoirs")
        tabs, _keep = self._reservoir_da_tables(usgs, usace, rfc)
        _lib.check(_lib.lib().trmc_set_reservoir_da(self._h, kind.shape[0], _lib.ptr(kind), _lib.ptr(table_row),
                                                    C.byref(tabs[0]), C.byref(tabs[1]), C.byref(tabs[2])))

    @staticmethod
    def _reservoir_da_tables(usgs, usace, rfc, with_state=True):
        """the three trmc_reservoir_da_table of ``set_reservoir_da`` 's tuples and the arrays they point into; with_state=False
        (a day of a stream, whose state the device carries): the hybrid tables' state may be missing or None, and is not passed"""
        keep, tabs = [], []
        for t, hybrid in ((usgs, True), (usace, True), (rfc, False)):
            s = _lib.ReservoirDaTable()
            if t is not None and len(t[0]):
                obs = np.ascontiguousarray(t[0], dtype=np.float32)
                if obs.ndim != 2:
                    raise ValueError("a reservoir data-assimilation table's observations must be [n, ncol]")
                n, ncol = obs.shape
                if hybrid:
                    time, ipar = np.ascontiguousarray(t[1], dtype=np.float32), None
                    state = np.ascontiguousarray(t[2], dtype=np.float32) if with_state else None
                    if time.shape != (ncol,) or (with_state and state.shape != (n, 4)):
                        raise ValueError("hybrid table: time must be [ncol], state [n, 4]")
                else:
                    time, ipar = None, np.ascontiguousarray(t[2], dtype=np.int32)
                    state = np.ascontiguousarray(t[1], dtype=np.float32) if with_state else None
                    if (with_state and state.shape != (n,)) or ipar.shape != (n, 5):
                        raise ValueError("rfc table: update_time must be [n], ipar [n, 5]")
                keep += [obs, time, state, ipar]
                s.n, s.ncol = n, ncol
                s.obs, s.time, s.state, s.ipar = (None if a is None else a.ctypes.data for a in (obs, time, state, ipar))
            tabs.append(s)
        return tabs, keep

    def download_reservoir_da(self):
        """(state [nres, 4] float32, timeseries_idx [nres] int32) the routed window left: include/trmc.h
        trmc_download_reservoir_da -- times in seconds from the start of the window."""
        state = np.zeros((getattr(self, "_nres", 0), 4), dtype=np.float32)
        idx = np.zeros(state.shape[0], dtype=np.int32)
        _lib.check(_lib.lib().trmc_download_reservoir_da(self._h, _lib.ptr(state), _lib.ptr(idx)))
        return state, idx

    def download_reservoir_inflow(self):
        out = np.zeros((getattr(self, "_nres", 0), self._nsteps), dtype=self.dtype)
        _lib.check(_lib.lib().trmc_download_reservoir_inflow(self._h, _lib.ptr(out)))
        return out

    def set_nudging(self, nsteps, gage_rows, mode, a, w):
        """Nudging tables [ngage, nsteps] for the staged window (see include/trmc.h trmc_set_nudging)."""
        gage_rows = np.ascontiguousarray(gage_rows, dtype=np.int64)
        mode = np.ascontiguousarray(mode, dtype=np.uint8)
        a = np.ascontiguousarray(a, dtype=self.dtype)
        w = np.ascontiguousarray(w, dtype=self.dtype)
        ng = gage_rows.shape[0]
        if mode.shape != (ng, nsteps) or a.shape != (ng, nsteps) or w.shape != (ng, nsteps):
            raise ValueError("nudging tables must be [ngage, nsteps]")
        self._ngage = ng
        _lib.check(_lib.lib().trmc_set_nudging(self._h, nsteps, ng, _lib.ptr(gage_rows), _lib.ptr(mode),
                                               _lib.ptr(a), _lib.ptr(w)))

    def set_nudging_successors(self, successor_rows):
        """Rows directly below gages that sit INSIDE their reach (-1: the gage ends its reach), for a window routed without
        assume_short_ts on a level-engine plan (include/trmc.h trmc_set_nudging_successors)."""
        succ = np.ascontiguousarray(successor_rows, dtype=np.int64)
        _lib.check(_lib.lib().trmc_set_nudging_successors(self._h, succ.shape[0], _lib.ptr(succ)))

    def download_nudge(self):
        out = np.zeros((getattr(self, "_ngage", 0), self._nsteps), dtype=self.dtype)
        _lib.check(_lib.lib().trmc_download_nudge(self._h, _lib.ptr(out)))
        return out

    def route_device(self, nsteps, qts_subdivisions, assume_short_ts):
        _lib.check(_lib.lib().trmc_route_device(self._h, nsteps, qts_subdivisions, int(bool(assume_short_ts))))
        self._nsteps = nsteps
        return self.stats()

    # -- the same window in parts (asynchronous; see include/trmc.h) ------------------------------
    def clone(self):
        """A second set of window buffers on this plan's static data (trmc_plan_clone): same topology, parameters and
        order in HBM, its own forcing / state / result / streams -- for a sequence of windows that takes turns on the two
        (``chain_from``, ``stage_forcing``)."""
        other = object.__new__(RoutingPlan)
        for k in ("nseg", "precision", "dtype", "nboundary", "engine", "maxlag", "arithmetic", "tile_steps"):
            setattr(other, k, getattr(self, k))
        h = C.c_void_p(0)
        other._h = C.c_void_p(0)
        _lib.check(_lib.lib().trmc_plan_clone(self._h, C.byref(h)))
        other._h = h
        other._nsteps = None
        other._stream_keep = {}
        other._th_levels = 0
        return other

    def set_sequence_mode(self, on=True):
        """The plan is one of several that take turns on the device (``clone``, ``chain_from``): a window's set-up goes to
        the tile stream and its end is queued with its last launch (include/trmc.h, trmc_plan_options.sequence_mode)."""
        _lib.check(_lib.lib().trmc_plan_set_sequence_mode(self._h, int(bool(on))))

    def stage_forcing(self, nsteps, qlat):
        """The next window's forcing on its way to the device without waiting for anything (trmc_stage_forcing): `qlat`
        [nseg, nq] should live in page-locked memory (``_lib.result_empty(..., always_pinned=True)``) for the copy to run
        beside the window another plan is routing.  The array must stay alive and unchanged until that window has begun."""
        if qlat.dtype != self.dtype or not qlat.flags.c_contiguous or qlat.ndim != 2 or qlat.shape[0] != self.nseg:
            raise ValueError(f"qlat must be a C-contiguous {np.dtype(self.dtype).name} array of shape ({self.nseg}, nq)")
        self._staged_qlat = qlat                      # (kept alive while the copy may be in flight)
        _lib.check(_lib.lib().trmc_stage_forcing(self._h, int(nsteps), _lib.ptr(qlat), qlat.shape[1]))
        # (the STAGED window's length: the window in progress, whose products a fetch queued right after this call sizes its
        # arrays for, keeps its own until route_begin starts the staged one)
        self._staged_nsteps = nsteps
        if getattr(self, "_nsteps", None) is None:
            self._nsteps = nsteps

    def chain_from(self, source):
        """This plan's NEXT window starts from the state `source`'s window (queued to its end) leaves, handed over on the
        device in two parts so that this plan's wide levels can start before the source's tail has finished (trmc.h)."""
        _lib.check(_lib.lib().trmc_plan_chain_from(self._h, source._h))

    def route_begin(self, nsteps, qts_subdivisions, assume_short_ts):
        _lib.check(_lib.lib().trmc_route_begin(self._h, nsteps, qts_subdivisions, int(bool(assume_short_ts))))
        self._nsteps = nsteps
        self._staged_nsteps = None

    def route_advance(self, t_end):
        _lib.check(_lib.lib().trmc_route_advance(self._h, int(t_end)))

    def route_end(self):
        _lib.check(_lib.lib().trmc_route_end(self._h))
        return self.stats()

    # -- a stream of windows (include/trmc.h, trmc_stream_*) ------------------------------------------------
    def stream_begin(self, nsteps, qts_subdivisions, slots=0, full_output=False, output_stride=0, reservoir_da=None):
        """After ``upload_forcing`` (the state, the shape of the forcing): days are then ``stream_push``-ed one after the other.
        ``reservoir_da``: True, or the most columns ``(usgs, usace, rfc)`` a day's tables may have (True: as many as the declared
        ones) -- the stream carries the data assimilation of the reservoirs that ``set_reservoir_da`` declared (kind, table_row,
        the tables' rows, the state day 0 starts from), and every ``stream_push`` brings the day's tables; None (default): a plan
        with such tables is refused, as it always was (include/trmc.h trmc_stream_set_reservoir_da)."""
        caps = (0, 0, 0) if reservoir_da in (None, False, True) else tuple(int(x) for x in reservoir_da)
        if len(caps) != 3:
            raise ValueError("reservoir_da: True or the three column capacities (usgs, usace, rfc)")
        _lib.check(_lib.lib().trmc_stream_set_reservoir_da(self._h, int(reservoir_da not in (None, False)), *caps))
        _lib.check(_lib.lib().trmc_stream_begin(self._h, int(nsteps), int(qts_subdivisions), int(slots), int(bool(full_output)),
                                                int(output_stride or 0)))
        self._nsteps = nsteps
        self._stream_keep = {}

    def stream_set_gages(self, rows):
        """The rows whose flow the streams on this plan nudge (trmc_stream_set_gages): declared once, before ``stream_begin``;
        every ``stream_push`` then carries the day's tables.  ``None`` or an empty list: none."""
        rows = np.ascontiguousarray([] if rows is None else rows, dtype=np.int64)
        _lib.check(_lib.lib().trmc_stream_set_gages(self._h, rows.shape[0], _lib.ptr(rows)))
        self._stream_ngage = int(rows.shape[0])

    def stream_set_summary(self, what):
        """The per-row summary the streams on this plan form of every day (trmc_stream_set_summary): an iterable of ``"peak"`` (peak
        flow and the 1-based step of the peak), ``"mean"`` (mean flow), ``"peak_depth"`` (peak depth and its step; carried by the
        tile kernels, refused by ``stream_begin`` with NotImplementedError in a stream with reservoir data assimilation) and
        ``"total"`` (running totals of the other parts over the days of the stream: ``stream_summary_total``), or ``None`` for
        none.  Declared before ``stream_begin``; it stays until the next call.  Every ``stream_push`` then says where the day's
        arrays go (``summary=``)."""
        names = _lib.SUMMARY_NAMES
        if isinstance(what, str):
            what = (what,)
        mask = 0
        for w in (what or ()):
            if w not in names:
                raise ValueError(f"summary: 'peak' and / or 'mean', 'peak_depth', 'total', got {w!r}")
            mask |= names[w]
        _lib.check(_lib.lib().trmc_stream_set_summary(self._h, mask))
        self._stream_summary = mask

    def stream_set_stage(self, on=True):
        """The streams on this plan hand over STAGE HYDROGRAPHS (trmc_stream_set_stage): the depth of every step at the rows of a
        day's row set -- a reservoir row: its pool's elevation -- which ``stream_push(..., rowset=, stage=)`` names a page-locked
        array for.  Declared before ``stream_begin``; it stays until the next call.  ``stream_begin`` then raises
        NotImplementedError in a stream with reservoir data assimilation, as it does for ``"peak_depth"``."""
        if self.engine != "levels":
            raise ValueError("a stream of days runs on the level engine: stage hydrographs need engine='levels'")
        _lib.check(_lib.lib().trmc_stream_set_stage(self._h, int(bool(on))))
        self._stream_stage = bool(on)

    def stream_set_packed_forcing(self, packed, row_ids=None):
        """The streams on this plan take days as packed CHRTOUT columns (trmc_stream_set_packed_forcing): ``packed`` is a dict of
        ``nhd_io.chrtout_packed`` -- its feature axis and packing facts are declared, its raw values are not read -- and
        ``row_ids`` int64 [nseg] the id of every row of the table.  Declared once, before ``stream_begin``; it stays until the next
        call.  ``stream_push(packed=day)`` then hands over a day's raw columns, which the device decodes, joins and lays out in
        one kernel; float days may still be pushed in between.  Returns ``feat_of_row`` as ``upload_forcing_packed`` does;
        ``None`` for ``packed`` withdraws the declaration."""
        if self.engine != "levels":
            raise ValueError("a stream of days runs on the level engine: packed days need engine='levels'")
        if packed is None:
            _lib.check(_lib.lib().trmc_stream_set_packed_forcing(self._h, 0, None, None, None))
            self._stream_packed = None
            return None
        feat_of_row = self._feat_of_row(packed, row_ids)
        nfeat = int(np.asarray(packed["feature_id"]).shape[0])
        if nfeat < 1:
            raise ValueError("packed: the files' feature axis is empty")
        pa = np.ascontiguousarray(packed["pack_a"], dtype=np.float64)
        pb = None if packed.get("pack_b") is None else np.ascontiguousarray(packed["pack_b"], dtype=np.float64)
        if pa.shape != (6,) or (pb is not None and pb.shape != (6,)):
            raise ValueError("pack_a / pack_b: (scale_factor, add_offset, _FillValue, missing_value, valid_min, valid_max)")
        _lib.check(_lib.lib().trmc_stream_set_packed_forcing(self._h, nfeat, _lib.ptr(feat_of_row), _lib.ptr(pa), _lib.ptr(pb)))
        self._stream_packed = (nfeat, pb is not None)
        return feat_of_row

    def stream_packed_forcing_kernel_ms(self):
        """device time (ms) of the decode kernel of the last packed day pushed (trmc_stream_packed_forcing_kernel_ms)"""
        ms = C.c_double(0.0)
        _lib.check(_lib.lib().trmc_stream_packed_forcing_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def _packed_day(self, packed):
        """the raw blocks of a packed day as ``trmc_stream_push_day_packed`` takes them, checked against the declaration"""
        decl = getattr(self, "_stream_packed", None)
        if decl is None:
            raise RuntimeError("packed: the plan's streams were not told to take packed days (stream_set_packed_forcing precedes stream_begin)")
        nfeat, two = decl
        raw_a, raw_b = packed["raw_a"], packed.get("raw_b")
        if (raw_b is not None) != two:
            raise ValueError("packed: the declaration has two variables (pack_b): raw_b is required" if two else
                             "packed: the declaration has one variable (pack_b = None): raw_b must be None")
        for name, raw in (("raw_a", raw_a), ("raw_b", raw_b)):
            if raw is None:
                continue
            if not isinstance(raw, np.ndarray) or raw.dtype != np.int32 or not raw.flags.c_contiguous or raw.ndim != 2 or raw.shape[1] != nfeat:
                raise ValueError(f"packed: {name} must be a C-contiguous int32 array of shape (nq, {nfeat})")
        if raw_b is not None and raw_b.shape != raw_a.shape:
            raise ValueError("packed: raw_a and raw_b must have one shape")
        return raw_a, raw_b

    def stream_push(self, qlat=None, boundary_q_ptr=None, rowset=None, hyd=None, q0=None, fvd=None, nudging=None, nudge=None,
                    reservoir_inflow=None, reservoir_da=None, reservoir_da_state=None, packed=None, summary=None, stage=None):
        """The next day: ``qlat`` [nseg, nq] (page-locked: ``_lib.result_empty(..., always_pinned=True)``), where its products go
        (page-locked arrays or None), the device pointer of its boundary rows' flows.  A plan with gage rows
        (``stream_set_gages``): ``nudging=(mode, a, w)``, the day's tables [ngage, nsteps] as ``set_nudging`` takes them for a
        window -- or ``(mode, a, w, first)`` with the day's first observations ``usgs_values[:, 0]`` [ngage]: where one is not NaN
        the gage row starts the day from it (mc_reach.pyx:404-411; the drop-in writes it into a window's initial state); ``nudge`` [ngage, nsteps] and ``reservoir_inflow`` [nres, nsteps]: page-locked arrays for the day's nudge record
        and the inflows of the plan's reservoirs.  A stream begun with ``reservoir_da``: ``reservoir_da=(usgs, usace, rfc[,
        rfc_reset_idx])``, the day's tables as ``set_reservoir_da`` takes them -- times from the day's start; the state members are
        ignored and may be None, the device carries them; the RFC timeseries_idx counts only with ``rfc_reset_idx`` -- and
        ``reservoir_da_state=(state [nres, 4] float32, timeseries_idx [nres] int32)``: page-locked arrays for the state the day
        leaves, times already counted from the next day's start.  A plan whose streams form a summary (``stream_set_summary``):
        ``summary=`` a tuple of page-locked [nseg] arrays (any may be None) for the day's peak flow, the 1-based step of the peak
        and the mean flow -- with ``"peak_depth"`` two more, the peak depth and its step: the rows of ``stream_products.SUMMARY``
        with their types.  A plan whose streams carry stage (``stream_set_stage``): ``stage=`` a page-locked array
        [rows of ``rowset``, nsteps] for the depth of every step at the set's rows (``rowset`` is then required).  Returns the
        day's number in the stream.  A plan whose streams take packed days (``stream_set_packed_forcing``): ``packed=`` a day's dict of
        ``nhd_io.chrtout_packed`` in place of ``qlat`` -- ``raw_a`` / ``raw_b`` C-contiguous int32 [nq, nfeat], page-locked for a
        copy that runs beside the launches; they are kept alive with the day's other host arrays."""
        raw = None
        if packed is not None:
            if qlat is not None:
                raise ValueError("a day's forcing is either qlat or packed, not both")
            raw = self._packed_day(packed)
        elif qlat is None:
            raise ValueError("a day needs its forcing: qlat, or packed=")
        elif qlat.dtype != self.dtype or not qlat.flags.c_contiguous or qlat.ndim != 2 or qlat.shape[0] != self.nseg:
            raise ValueError(f"qlat must be a C-contiguous {np.dtype(self.dtype).name} array of shape ({self.nseg}, nq)")
        if stage is not None:  # (what the library would refuse, before it is called)
            if not getattr(self, "_stream_stage", False):
                raise RuntimeError("stage: the stream was begun without stage hydrographs (stream_set_stage precedes stream_begin)")
            if rowset is None:
                raise ValueError("stage: a day's stage covers the rows of its row set -- rowset is required")
            n = getattr(self, "_rowset_n", {}).get(rowset)
            if n is not None and isinstance(stage, np.ndarray) and stage.ndim == 2 and (stage.shape[0] < n or stage.shape[1] != self._nsteps):
                raise ValueError(f"stage must hold [{n}, {self._nsteps}] (the rows of the day's row set, nsteps), got {stage.shape}")
        day_s = _lib.StreamDay()
        tables = ()
        if nudging is not None:
            mode = np.ascontiguousarray(nudging[0], dtype=np.uint8)
            a = np.ascontiguousarray(nudging[1], dtype=self.dtype)
            w = np.ascontiguousarray(nudging[2], dtype=self.dtype)
            if mode.ndim != 2 or a.shape != mode.shape or w.shape != mode.shape:
                raise ValueError("nudging tables must be [ngage, nsteps]")
            tables = (mode, a, w)
            if len(nudging) > 3 and nudging[3] is not None:
                first = np.ascontiguousarray(nudging[3], dtype=self.dtype)
                if first.shape != (mode.shape[0],):
                    raise ValueError("the day's first observations must be [ngage]")
                tables += (first,)
                day_s.da_q0 = first.ctypes.data
            day_s.da_ngage, day_s.da_nsteps = mode.shape
            day_s.da_mode, day_s.da_a, day_s.da_w = mode.ctypes.data, a.ctypes.data, w.ctypes.data
        # the day's destinations, each checked against its row of the table (None = not asked for)
        if summary is not None and len(summary) not in SP.SUMMARY_LENGTHS:
            raise ValueError(SP.SUMMARY_WRONG)
        dims = {"rows": self.nseg, "nres": getattr(self, "_nres", 0)}
        dest = {p.name: SP.given(p, {"hyd": hyd, "q0": q0, "fvd": fvd, "nudge": nudge, "reservoir_inflow": reservoir_inflow,
                                     "reservoir_da_state": reservoir_da_state, "summary": summary, "stage": stage}) for p in SP.ALL}
        for p in SP.ALL:
            if p.wrong and dest[p.name] is not None and not SP.fits(p, dest[p.name], self.dtype, dims):
                raise ValueError(SP.wrong(p, self.dtype, dims))
        if nudge is not None and nudge.shape != (tables[0].shape if tables else ()):
            raise ValueError("nudge must have the shape of the day's nudging tables")
        if reservoir_inflow is not None:
            day_s.res_nres, day_s.res_nsteps = reservoir_inflow.shape
        day_s.nudge_host, day_s.res_inflow_host, day_s.res_da_state_host, day_s.res_da_tsidx_host = (
            None if x is None else x.ctypes.data for x in (nudge, reservoir_inflow, dest["reservoir_da_state"], dest["reservoir_da_tsidx"]))
        rda_s = None
        if reservoir_da is not None:
            if len(reservoir_da) not in (3, 4):
                raise ValueError("reservoir_da must be (usgs, usace, rfc[, rfc_reset_idx])")
            rtabs, rkeep = self._reservoir_da_tables(*reservoir_da[:3], with_state=False)
            rda_s = _lib.StreamReservoirDa()
            rda_s.usgs, rda_s.usace, rda_s.rfc = rtabs
            rda_s.rfc_reset_idx = int(bool(reservoir_da[3])) if len(reservoir_da) == 4 else 0
            tables += tuple(rkeep)
            day_s.reservoir_da = C.addressof(rda_s)
        info = self.stream_info()
        day = info["days_pushed"]
        # (alive while the copies may be in flight: a day's products are queued up to `slots` days on)
        self._stream_keep[day] = {"qlat": qlat if raw is None else raw, "tables": tables, "dests": list(dest.values())}
        for old in [k for k in self._stream_keep if isinstance(k, int) and k < day - max(8, info["slots"])]:
            del self._stream_keep[old]
        parts = [dest[p.name] for p in SP.SUMMARY]
        depth = any(x is not None for x in parts[3:])
        if summary is not None:  # (where the NEXT day's summary goes: the push below consumes it)
            _lib.check(_lib.lib().trmc_stream_summary_dest(self._h, *(_lib.ptr(x) for x in parts[:3])))
        try:
            if stage is not None:    # (likewise)
                _lib.check(_lib.lib().trmc_stream_stage_dest(self._h, _lib.ptr(stage)))
            if depth:
                _lib.check(_lib.lib().trmc_stream_summary_depth_dest(self._h, *(_lib.ptr(x) for x in parts[3:])))
            if raw is None and nudging is None and reservoir_inflow is None and reservoir_da is None and reservoir_da_state is None:  # (the entry point every stream without tables has always used)
                _lib.check(_lib.lib().trmc_stream_push(self._h, _lib.ptr(qlat), qlat.shape[1], C.c_void_p(boundary_q_ptr or 0),
                                                       -1 if rowset is None else int(rowset), _lib.ptr(hyd), _lib.ptr(q0), _lib.ptr(fvd)))
                return day
            day_s.boundary_q_dev = boundary_q_ptr or None
            day_s.rowset = -1 if rowset is None else int(rowset)
            day_s.hyd_host, day_s.q0_host, day_s.fvd_host = (None if x is None else x.ctypes.data for x in (hyd, q0, fvd))
            if raw is not None:      # (the day's raw columns in place of qlat; every other member as in a float day)
                day_s.nq = raw[0].shape[0]
                _lib.check(_lib.lib().trmc_stream_push_day_packed(self._h, C.byref(day_s), _lib.ptr(raw[0]), _lib.ptr(raw[1])))
                return day
            day_s.qlat, day_s.nq = qlat.ctypes.data, qlat.shape[1]
            _lib.check(_lib.lib().trmc_stream_push_day(self._h, C.byref(day_s)))
            return day
        except Exception:
            if summary is not None:  # (a refused push has not consumed the arrays: they must not wait for another day)
                _lib.lib().trmc_stream_summary_dest(self._h, None, None, None)
            if depth:
                _lib.lib().trmc_stream_summary_depth_dest(self._h, None, None)
            if stage is not None:
                _lib.lib().trmc_stream_stage_dest(self._h, None)
            raise

    def stream_summary_total(self):
        """The totals over all days of the stream in progress that have been handed over so far (a stream whose summary has
        ``"total"``; trmc_stream_summary_total, synchronous): a dict with ``"days"`` and, for the parts of the summary, their
        totals under the parts' names (``stream_products.SUMMARY``; the steps int64, 1-based from the stream's first step) --
        [nseg] arrays in row order, the folds of the days' arrays that include/trmc.h defines."""
        mask = getattr(self, "_stream_summary", 0)
        out = {p.name: np.empty(self.nseg, SP.dtype_of(p, self.dtype, total=True)) for p in SP.SUMMARY if mask & _lib.SUMMARY_NAMES[p.on]}
        days = C.c_int64(0)
        _lib.check(_lib.lib().trmc_stream_summary_total(self._h, *(_lib.ptr(out.get(p.name)) for p in SP.SUMMARY), C.byref(days)))
        out["days"] = int(days.value)
        return out

    # what a stream cannot form an exceedance of, and why (include/trmc.h trmc_stream_set_exceedance says the same)
    STREAM_EXCEEDANCE_FLOW_ONLY = ("the exceedance of a stream of days is formed from the flow planes of its ring, which hold every step's flow of "
                                   "every row: they hold the depth of a tile's last step only and a stream without full_output forms no velocity, "
                                   "so {what!r} is not available -- route the day in question as a window (RoutingPlan.window_exceedance, "
                                   "the drop-in's exceedance=)")

    @classmethod
    def stream_exceedance_quantity(cls, quantity):
        """``quantity`` of a stream's exceedance, checked: "flow" (returned as trmc's number) or None; NotImplementedError for
        "depth", "velocity" and "bankfull", ValueError for anything else."""
        if quantity is None:
            return -1
        if quantity in ("depth", "velocity", "bankfull"):
            raise NotImplementedError(cls.STREAM_EXCEEDANCE_FLOW_ONLY.format(what=quantity))
        if quantity != "flow":
            raise ValueError(f"exceedance of a stream: quantity 'flow' or None, got {quantity!r}")
        return _lib.TRMC_X_FLOW

    def stream_set_exceedance(self, quantity="flow"):
        """The streams on this plan keep, on the device and over ALL their days, the threshold exceedance of every row's flow
        against ``set_thresholds`` (which must precede this call): steps over, first and last step, longest run, the steps counted
        on over the days and a run carried over a day's end (trmc_stream_set_exceedance; ``stream_exceedance`` fetches).  Declared
        before ``stream_begin``; it stays until the next call; ``None`` withdraws it.  Flow only: "depth", "velocity" and
        "bankfull" raise NotImplementedError -- route the day in question as a window."""
        q = self.stream_exceedance_quantity(quantity)
        _lib.check(_lib.lib().trmc_stream_set_exceedance(self._h, q))
        self._stream_exceedance = q

    def stream_exceedance(self, parts=("steps_over", "first_step", "last_step", "longest_run")):
        """The exceedance over all days of the stream in progress that have been handed over so far (trmc_stream_exceedance,
        synchronous): a dict with ``"days"`` and, of ``steps_over``, ``first_step``, ``last_step`` and ``longest_run``, the parts
        asked for -- int64 [nseg, K] arrays in row order, the steps 1-based from the stream's first step, as ``window_exceedance``
        defines them over the days' flows one after the other."""
        parts = (parts,) if isinstance(parts, str) else tuple(parts or ())
        unknown = [p for p in parts if p not in self.WINDOW_EXCEEDANCE_PARTS]
        if unknown:
            raise ValueError(f"unknown part(s) of a stream's exceedance {unknown}: one of {list(self.WINDOW_EXCEEDANCE_PARTS)}")
        if not parts:
            raise ValueError("stream_exceedance: no part asked for")
        k = getattr(self, "_th_levels", 0)
        out = {name: (np.empty((self.nseg, k), np.int64) if name in parts else None) for name in self.WINDOW_EXCEEDANCE_PARTS}
        days = C.c_int64(0)
        _lib.check(_lib.lib().trmc_stream_exceedance(self._h, *(_lib.ptr(out[name]) for name in self.WINDOW_EXCEEDANCE_PARTS), C.byref(days)))
        res = {"days": int(days.value)}
        res.update((name, a) for name, a in out.items() if a is not None)
        return res

    def stream_depth_thresholds(self, th):
        """``th`` of a stream's depth exceedance, checked: [nseg] or [nseg, K] with K <= 4 (returned [nseg, K], contiguous, in the
        plan's dtype), the string "bankfull" (``bankfull_depth()`` of this plan: +inf, never over, on rows that route no
        Muskingum-Cunge step) or None; ValueError otherwise."""
        if th is None:
            return None
        if isinstance(th, str):
            if th != "bankfull":
                raise ValueError(f"depth exceedance of a stream: thresholds [nseg] or [nseg, K], 'bankfull' or None, got {th!r}")
            th = self.bankfull_depth()
        th = np.asarray(th)
        th = th[:, None] if th.ndim == 1 else th
        if th.ndim != 2 or th.shape[0] != self.nseg or not 1 <= th.shape[1] <= 4:
            raise ValueError(f"depth exceedance of a stream: thresholds must be [nseg] or [nseg, K] with nseg = {self.nseg} and K <= 4: "
                             f"got {th.shape}")
        return np.ascontiguousarray(th, dtype=self.dtype)

    def stream_set_depth_exceedance(self, th="bankfull"):
        """The streams on this plan keep, on the device and over ALL their days, the threshold exceedance of every row's DEPTH
        against ``th`` -- [nseg] or [nseg, K] (K <= 4) in row order, metres, or "bankfull" (``bankfull_depth()``: the steps a row
        is out of bank): steps over, first and last step, longest run, the steps counted on over the days and a run carried over a
        day's end (trmc_stream_set_depth_exceedance; ``stream_depth_exceedance`` fetches).  The depth is what ``stage`` and the
        full result hand out: a reservoir row's is its pool's elevation, a boundary row's 0.  A second accumulator beside
        ``stream_set_exceedance``'s, with a threshold table of its own (``set_thresholds`` is not touched): a stream may keep both.
        Such a stream writes every step's depth, as one with ``stream_set_stage`` does, and ``stream_begin`` refuses what it
        refuses for stage.  Declared before ``stream_begin``; it stays until the next call; ``None`` withdraws it."""
        th = self.stream_depth_thresholds(th)
        if self.engine != "levels":
            raise ValueError("a stream of days runs on the level engine: its depth exceedance needs engine='levels'")
        _lib.check(_lib.lib().trmc_stream_set_depth_exceedance(self._h, 0 if th is None else th.shape[1], _lib.ptr(th)))
        self._stream_depth_levels = 0 if th is None else th.shape[1]

    def stream_depth_exceedance(self, parts=("steps_over", "first_step", "last_step", "longest_run")):
        """The depth exceedance over all days of the stream in progress that have been handed over so far
        (trmc_stream_depth_exceedance, synchronous): a dict with ``"days"`` and, of ``steps_over``, ``first_step``, ``last_step``
        and ``longest_run``, the parts asked for -- int64 [nseg, K] arrays in row order, the steps 1-based from the stream's first
        step, as ``window_exceedance("depth")`` defines them over the days' depths one after the other."""
        parts = (parts,) if isinstance(parts, str) else tuple(parts or ())
        unknown = [p for p in parts if p not in self.WINDOW_EXCEEDANCE_PARTS]
        if unknown:
            raise ValueError(f"unknown part(s) of a stream's depth exceedance {unknown}: one of {list(self.WINDOW_EXCEEDANCE_PARTS)}")
        if not parts:
            raise ValueError("stream_depth_exceedance: no part asked for")
        k = getattr(self, "_stream_depth_levels", 0)
        out = {name: (np.empty((self.nseg, k), np.int64) if name in parts else None) for name in self.WINDOW_EXCEEDANCE_PARTS}
        days = C.c_int64(0)
        _lib.check(_lib.lib().trmc_stream_depth_exceedance(self._h, *(_lib.ptr(out[name]) for name in self.WINDOW_EXCEEDANCE_PARTS), C.byref(days)))
        res = {"days": int(days.value)}
        res.update((name, a) for name, a in out.items() if a is not None)
        return res

    def stream_depth_exceedance_kernel_ms(self):
        """device time (ms) of the last day's fold into the stream's depth exceedance, from events around the kernel
        (trmc_stream_depth_exceedance_kernel_ms; waits for it)"""
        return self._kernel_ms(_lib.lib().trmc_stream_depth_exceedance_kernel_ms)

    @staticmethod
    def stream_courant_limit(limit):
        """``limit`` of a stream's Courant number, checked: a real number (returned as a float) or None; ValueError otherwise."""
        if limit is None:
            return None
        if isinstance(limit, (bool, str, bytes)) or not isinstance(limit, (int, float, np.integer, np.floating)):
            raise ValueError(f"courant: the limit cn is counted against must be a real number (or None), got {limit!r}")
        return float(limit)

    def stream_set_courant(self, limit=1.0):
        """The streams on this plan keep, on the device and over ALL their days, every row's Courant number cn = ck dt / dx: the
        highest, the step it was first reached at and the number of steps with cn > ``limit`` -- ``window_courant_summary`` with
        the steps counted on over the days (trmc_stream_set_courant; ``stream_courant`` fetches).  Such a stream writes every
        step's depth, as one with ``stream_set_stage`` does, and ``stream_begin`` refuses what it refuses for stage.  Declared
        before ``stream_begin``; it stays until the next call; ``None`` withdraws it."""
        limit = self.stream_courant_limit(limit)
        if self.engine != "levels":
            raise ValueError("a stream of days runs on the level engine: its Courant number needs engine='levels'")
        _lib.check(_lib.lib().trmc_stream_set_courant(self._h, int(limit is not None), 0.0 if limit is None else limit))
        self._stream_courant = limit

    def stream_courant(self):
        """The Courant number over all days of the stream in progress that have been handed over so far (trmc_stream_courant,
        synchronous): a dict with ``"days"``, ``"peak_cn"`` (plan dtype), ``"peak_cn_step"`` and ``"steps_over"`` (int64, the steps
        1-based from the stream's first step) -- [nseg] arrays in row order, as ``window_courant_summary`` defines them over the
        days one after the other.  Reservoir and boundary rows: (0, 1, 0)."""
        peak, step, over = np.empty(self.nseg, self.dtype), np.empty(self.nseg, np.int64), np.empty(self.nseg, np.int64)
        days = C.c_int64(0)
        _lib.check(_lib.lib().trmc_stream_courant(self._h, _lib.ptr(peak), _lib.ptr(step), _lib.ptr(over), C.byref(days)))
        return {"days": int(days.value), "peak_cn": peak, "peak_cn_step": step, "steps_over": over}

    def stream_courant_kernel_ms(self):
        """device time (ms) of the last day's fold into the stream's Courant number, from events around the kernel
        (trmc_stream_courant_kernel_ms; waits for it)"""
        return self._kernel_ms(_lib.lib().trmc_stream_courant_kernel_ms)

    @staticmethod
    def velocity_thresholds(th, nseg, what="velocity of a stream", rows="nseg"):
        """``thresholds`` of a stream's velocity against ``nseg`` rows, checked -- the one rule ``stream_set_velocity`` and
        ``RouteStream(velocity=)`` share: None (no velocity), True (the peak and its step only; returned as True), or [nseg] /
        [nseg, K] with K <= 4, m/s (returned [nseg, K]); ValueError otherwise."""
        if th is None or th is True:
            return th
        if isinstance(th, (bool, str, bytes)):
            raise ValueError(f"{what}: None, True or thresholds [{rows}] or [{rows}, K], got {th!r}")
        th = np.asarray(th)
        th = th[:, None] if th.ndim == 1 else th
        if th.ndim != 2 or th.shape[0] != nseg or not 1 <= th.shape[1] <= 4:
            raise ValueError(f"{what}: thresholds must be [{rows}] or [{rows}, K] with {rows} = {nseg} and K <= 4: got {th.shape}")
        return th

    def stream_set_velocity(self, thresholds=True):
        """The streams on this plan keep, on the device and over ALL their days, every row's peak velocity and the step it was
        first reached at -- ``window_summary(("peak_velocity",))`` with the steps counted on over the days -- and, with
        ``thresholds`` [nseg] or [nseg, K] (K <= 4) in row order, m/s, the threshold exceedance of the velocity as
        ``window_exceedance("velocity")`` defines it: steps over, first and last step, longest run, a run carried over a day's end
        (trmc_stream_set_velocity; ``stream_velocity`` fetches).  ``True``: the peak and its step only.  The velocity is column 1
        of the same days routed as windows: 0 where a step had no flow, at reservoir rows and at boundary rows.  A fourth
        accumulator beside the flow exceedance, the depth exceedance and the Courant number; a stream may keep them all.  The
        step loop forms no velocity for it: such a stream writes every step's depth, as one with ``stream_set_stage`` does, and
        ``stream_begin`` refuses what it refuses for stage.  Declared before ``stream_begin``; it stays until the next call;
        ``None`` withdraws it."""
        th = self.velocity_thresholds(thresholds, self.nseg)
        if th is None and (self.engine != "levels" or getattr(self, "_stream_velocity", None) is None):
            return                                                  # (withdrawing nothing is no error, on either engine)
        if self.engine != "levels":
            raise ValueError("a stream of days runs on the level engine: its velocity needs engine='levels'")
        if th is not None and th is not True:
            th = np.ascontiguousarray(th, dtype=self.dtype)
        k = 0 if th is None or th is True else th.shape[1]
        _lib.check(_lib.lib().trmc_stream_set_velocity(self._h, int(th is not None), k, _lib.ptr(th) if k else None))
        self._stream_velocity = None if th is None else k

    def stream_velocity(self):
        """The velocity over all days of the stream in progress that have been handed over so far (trmc_stream_velocity,
        synchronous): a dict with ``"days"``, ``"peak_velocity"`` (plan dtype) and ``"peak_velocity_step"`` (int64, 1-based from
        the stream's first step) -- [nseg] arrays in row order -- and, where the declaration had thresholds, ``"steps_over"``,
        ``"first_step"``, ``"last_step"`` and ``"longest_run"``, int64 [nseg, K].  Reservoir and boundary rows: v = 0, so (0, 1)."""
        k = getattr(self, "_stream_velocity", None) or 0
        peak, step = np.empty(self.nseg, self.dtype), np.empty(self.nseg, np.int64)
        parts = [np.empty((self.nseg, k), np.int64) if k else None for _ in self.WINDOW_EXCEEDANCE_PARTS]
        days = C.c_int64(0)
        _lib.check(_lib.lib().trmc_stream_velocity(self._h, _lib.ptr(peak), _lib.ptr(step), *(_lib.ptr(a) if k else None for a in parts),
                                                   C.byref(days)))
        res = {"days": int(days.value), "peak_velocity": peak, "peak_velocity_step": step}
        if k:
            res.update(zip(self.WINDOW_EXCEEDANCE_PARTS, parts))
        return res

    def stream_velocity_kernel_ms(self):
        """device time (ms) of the last day's fold into the stream's velocity, from events around the kernel
        (trmc_stream_velocity_kernel_ms; waits for it)"""
        return self._kernel_ms(_lib.lib().trmc_stream_velocity_kernel_ms)

    def stream_gather(self, day, rowset, device_ptr, stream=0):
        """Flows of a row set over `day` [rows, nsteps] into device memory (trmc_stream_gather)."""
        _lib.check(_lib.lib().trmc_stream_gather(self._h, int(day), int(rowset), C.c_void_p(device_ptr), C.c_void_p(stream or 0)))

    def stream_boundary(self, day, device_ptr, src_row_stride, index_ptr=None, stream=0):
        """The boundary rows' flows of `day` from a block of hydrographs in device memory (trmc_stream_boundary)."""
        _lib.check(_lib.lib().trmc_stream_boundary(self._h, int(day), C.c_void_p(device_ptr), int(src_row_stride),
                                                   C.c_void_p(index_ptr or 0), C.c_void_p(stream or 0)))

    def stream_gather_host(self, day, rowset):
        """The same through the host: [rows, nsteps] (a stream whose ranks exchange with host collectives)."""
        from . import comm as X
        n = self._rowset_n[rowset]
        if n == 0:
            return np.zeros((0, self._nsteps), dtype=self.dtype)
        dev = self.info()["device"]
        buf = X.DeviceBuffer(dev, n * self._nsteps * np.dtype(self.dtype).itemsize)
        st = self.stream()
        # (the gather on the stream the download is queued on: behind the launches of both compute streams, whichever of them
        # the stream's last launch is on)
        self.stream_gather(day, rowset, buf.ptr, stream=st)
        return buf.download((n, self._nsteps), self.dtype, stream=st)

    def stream_boundary_host(self, day, flows):
        """The boundary rows' flows of `day` [nboundary, nsteps] from a host array."""
        from . import comm as X
        flows = np.ascontiguousarray(flows, dtype=self.dtype)
        if flows.shape != (self.nboundary, self._nsteps):
            raise ValueError("boundary flows must be [nboundary, nsteps]")
        if self.nboundary == 0:
            return
        buf = X.DeviceBuffer.from_array(self.info()["device"], flows)
        self._stream_keep[("boundary", int(day))] = buf          # (alive until the fill has run)
        for k in [k for k in self._stream_keep if isinstance(k, tuple) and k[1] < day - 8]:
            del self._stream_keep[k]
        self.stream_boundary(day, buf.ptr, self._nsteps)

    def stream_advance(self, ntiles):
        """Queue the next ``ntiles`` launches of the stream without a new day (the rows still under way move on)."""
        _lib.check(_lib.lib().trmc_stream_advance(self._h, int(ntiles)))

    def stream_flush(self):
        _lib.check(_lib.lib().trmc_stream_flush(self._h))

    def stream_wait(self, day):
        _lib.check(_lib.lib().trmc_stream_wait(self._h, int(day)))

    def stream_info(self):
        v = [C.c_int32(0) for _ in range(5)] + [C.c_int64(0) for _ in range(3)]
        _lib.check(_lib.lib().trmc_stream_info(self._h, *[C.byref(x) for x in v]))
        names = ("slots", "tiles_per_day", "lag_max", "wide_levels", "cluster_levels", "days_pushed", "days_complete", "launches")
        return {k: x.value for k, x in zip(names, v)}

    def stream_day_ms(self, day):
        """device ms between the first and the last launch of the day's push on the slices' stream (trmc_stream_day_ms)"""
        ms = C.c_double(0)
        _lib.check(_lib.lib().trmc_stream_day_ms(self._h, int(day), C.byref(ms)))
        return ms.value

    def stream_end(self):
        _lib.check(_lib.lib().trmc_stream_end(self._h))
        self._stream_keep = {}

    def stream(self):
        """hipStream_t of the plan as an integer (what troute_amd.comm's event / stream calls and the collectives take)."""
        s = C.c_void_p(0)
        _lib.check(_lib.lib().trmc_plan_stream(self._h, C.byref(s)))
        return s.value or 0

    def rowset(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        rid = C.c_int32(-1)
        _lib.check(_lib.lib().trmc_rowset_create(self._h, _lib.ptr(rows), rows.shape[0], C.byref(rid)))
        if not hasattr(self, "_rowset_n"):
            self._rowset_n = {}
        self._rowset_n[rid.value] = int(rows.shape[0])
        return rid.value

    def gather_flow_range(self, rowset, t_begin, t_end, device_ptr, stride):
        _lib.check(_lib.lib().trmc_gather_flow_range(self._h, rowset, int(t_begin), int(t_end),
                                                     C.c_void_p(device_ptr), int(stride)))

    def set_boundary_flow_range(self, t_begin, t_end, device_ptr, stride, stream=None, index_ptr=None):
        """index_ptr: device int64 [nboundary], the source row of every boundary row (None: row b <- source row b)"""
        _lib.check(_lib.lib().trmc_set_boundary_flow_range_indexed(self._h, int(t_begin), int(t_end),
                                                                   C.c_void_p(device_ptr), int(stride),
                                                                   C.c_void_p(index_ptr) if index_ptr else None,
                                                                   C.c_void_p(stream) if stream else None))

    def set_lag(self, lag_of_row):
        """Rows with lag L are routed L launches behind the others (include/trmc.h trmc_plan_set_lag)."""
        lag = None if lag_of_row is None else np.ascontiguousarray(lag_of_row, dtype=np.int32)
        if lag is not None and lag.shape != (self.nseg,):
            raise ValueError("lag_of_row must be [nseg]")
        _lib.check(_lib.lib().trmc_plan_set_lag(self._h, _lib.ptr(lag)))
        self.maxlag = 0 if lag is None else int(lag.max(initial=0))

    def download_fvd(self, stride=1, rowset=None):
        """fvd [nseg, nsteps // stride, 3]: every `stride`-th step (the steps stride, 2 stride, ... counted from 1), decimated
        on the device (trmc_download_fvd_strided); stride = 1: the whole result.  rowset (``rowset(rows)``): the rows of that
        set only, in its order (trmc_download_fvd_rowset)."""
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1")
        if rowset is not None:
            out = _lib.result_empty((self._rowset_n[rowset], self._nsteps // stride, 3), self.dtype)
            if out.size:
                _lib.check(_lib.lib().trmc_download_fvd_rowset(self._h, stride, int(rowset), _lib.ptr(out)))
            return out
        out = _lib.result_empty((self.nseg, self._nsteps // stride, 3), self.dtype)
        if out.size:
            _lib.check(_lib.lib().trmc_download_fvd_strided(self._h, stride, _lib.ptr(out)))
        return out

    # window_summary's parts -> the arrays each brings (value arrays in the plan's dtype, steps int32), in trmc_window_summary's order
    WINDOW_SUMMARY_PARTS = {"peak": ("peak_flow", "peak_step"), "mean": ("mean_flow",), "peak_depth": ("peak_depth", "peak_depth_step"),
                            "peak_velocity": ("peak_velocity", "peak_velocity_step")}

    @staticmethod
    def _tile(fn, precision):
        """(rows, steps) from one of the library's trmc_window_*_tile"""
        rows, steps = C.c_int32(0), C.c_int32(0)
        _lib.check(fn(int(precision), C.byref(rows), C.byref(steps)))
        return rows.value, steps.value

    def _kernel_ms(self, fn):
        """milliseconds from one of the library's trmc_window_*_kernel_ms"""
        ms = C.c_double(0)
        _lib.check(fn(self._h, C.byref(ms)))
        return ms.value

    @staticmethod
    def _column_block(columns):
        """ONE block for the arrays of a window's product (page-locked and pooled when it is large, like a downloaded result), each
        a view of it on a 256-byte boundary: {name: array} from (name, dtype, shape) triples."""
        columns = [(name, np.dtype(dtype), shape, int(np.prod(shape)) * np.dtype(dtype).itemsize) for name, dtype, shape in columns]
        block = _lib.result_empty((sum(-(-nbytes // 256) * 256 for *_, nbytes in columns),), np.uint8)
        out, at = {}, 0
        for name, dtype, shape, nbytes in columns:
            out[name] = block[at:at + nbytes].view(dtype).reshape(shape)
            at += -(-nbytes // 256) * 256
        return out

    @staticmethod
    def window_summary_tile(precision=32):
        """(rows, steps) of the reduction kernel's tile for a precision (trmc_window_summary_tile)"""
        return RoutingPlan._tile(_lib.lib().trmc_window_summary_tile, precision)

    def window_summary(self, parts=("peak", "mean", "peak_depth", "peak_velocity"), rowset=None):
        """Per-row summary of the last window, reduced on the device over EVERY step of its result (trmc_window_summary): a dict
        with ``peak_flow`` / ``peak_step`` ("peak"), ``mean_flow`` ("mean"), ``peak_depth`` / ``peak_depth_step`` ("peak_depth") and
        ``peak_velocity`` / ``peak_velocity_step`` ("peak_velocity") -- the parts asked for only.  Values [rows] in the plan's
        dtype, steps int32, 1-based, the first of equal peaks; the first five are a stream day's summary of the same names, bit
        for bit.  rowset (``rowset(rows)``): the rows of that set, in its order."""
        parts = (parts,) if isinstance(parts, str) else tuple(parts or ())
        unknown = [p for p in parts if p not in self.WINDOW_SUMMARY_PARTS]
        if unknown:
            raise ValueError(f"unknown part(s) of a window summary {unknown}: one of {sorted(self.WINDOW_SUMMARY_PARTS)}")
        if not parts:
            raise ValueError("window_summary: no part asked for")
        n = self.nseg if rowset is None else self._rowset_n[rowset]
        order = ("peak_flow", "peak_step", "mean_flow", "peak_depth", "peak_depth_step", "peak_velocity", "peak_velocity_step")
        asked = [name for part, names in self.WINDOW_SUMMARY_PARTS.items() if part in parts for name in names]
        out = self._column_block((name, np.int32 if name.endswith("_step") else self.dtype, (n,)) for name in order if name in asked)
        _lib.check(_lib.lib().trmc_window_summary(self._h, -1 if rowset is None else int(rowset), *(_lib.ptr(out.get(k)) for k in order)))
        return out

    def window_summary_kernel_ms(self):
        """device time (ms) of the last ``window_summary``'s kernel, from events around it (trmc_window_summary_kernel_ms)"""
        return self._kernel_ms(_lib.lib().trmc_window_summary_kernel_ms)

    @staticmethod
    def window_courant_tile(precision=32):
        """(rows, steps) of the Courant kernel's tile for a precision (trmc_window_courant_tile)"""
        return RoutingPlan._tile(_lib.lib().trmc_window_courant_tile, precision)

    def window_courant(self, stride=1, rowset=None):
        """Courant metrics of the last window [rows, nsteps // stride, 3] = (cn, ck, X) per kept step (the steps stride, 2 stride,
        ... counted from 1, as ``download_fvd``), recomputed on the device from the window's result, state and forcing in the
        plan's own arithmetic (trmc_window_courant).  Reservoir and boundary rows are zeros.  rowset (``rowset(rows)``): the rows
        of that set, in its order."""
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1")
        n = self.nseg if rowset is None else self._rowset_n[rowset]
        out = _lib.result_empty((n, (self._nsteps or 0) // stride, 3), self.dtype)
        # (an empty block is still asked for: the call's refusals -- nothing routed, a stream in progress -- hold for it too)
        _lib.check(_lib.lib().trmc_window_courant(self._h, -1 if rowset is None else int(rowset), stride, _lib.ptr(out) if out.size else None))
        return out

    def window_courant_summary(self, limit=1.0, rowset=None):
        """Per row of the last window: ``peak_cn`` (the highest Courant number, plan dtype), ``peak_cn_step`` (the 1-based step it
        was first reached at, int32) and ``steps_over`` (steps with cn > limit, int32), reduced on the device over every step
        (trmc_window_courant_summary).  Where cn > 1, dt is too long for that reach's dx."""
        n = self.nseg if rowset is None else self._rowset_n[rowset]
        out = {"peak_cn": _lib.result_empty((n,), self.dtype), "peak_cn_step": _lib.result_empty((n,), np.int32),
               "steps_over": _lib.result_empty((n,), np.int32)}
        _lib.check(_lib.lib().trmc_window_courant_summary(self._h, -1 if rowset is None else int(rowset), float(limit),
                                                          *(_lib.ptr(v) for v in out.values())))
        return out

    def window_courant_kernel_ms(self):
        """device time (ms) of the last ``window_courant`` / ``window_courant_summary``'s kernel (trmc_window_courant_kernel_ms)"""
        return self._kernel_ms(_lib.lib().trmc_window_courant_kernel_ms)

    # window_exceedance's parts, in trmc_window_exceedance's order
    WINDOW_EXCEEDANCE_PARTS = ("steps_over", "first_step", "last_step", "longest_run")

    @staticmethod
    def window_exceedance_tile(precision=32):
        """(rows, steps) of the exceedance kernel's tile for a precision (trmc_window_exceedance_tile)"""
        return RoutingPlan._tile(_lib.lib().trmc_window_exceedance_tile, precision)

    def set_thresholds(self, th):
        """Thresholds of every row, [nseg] (one level) or [nseg, K] with K <= 4, cast to the plan's dtype and kept on the device
        until replaced (trmc_plan_set_thresholds); ``None`` clears them.  Per plan object: a ``clone`` has none until set."""
        if th is None:
            _lib.check(_lib.lib().trmc_plan_set_thresholds(self._h, 0, None))
            self._th_levels = 0
            return
        th = np.asarray(th)
        if th.ndim == 1:
            th = th[:, None]
        if th.ndim != 2 or th.shape[0] != self.nseg:
            raise ValueError(f"thresholds must be [nseg] or [nseg, K] with nseg = {self.nseg}: got {th.shape}")
        if not 1 <= th.shape[1] <= 4:
            raise ValueError(f"thresholds: 1 to 4 levels a row, got {th.shape[1]}")
        th = np.ascontiguousarray(th, dtype=self.dtype)
        _lib.check(_lib.lib().trmc_plan_set_thresholds(self._h, th.shape[1], _lib.ptr(th)))
        self._th_levels = th.shape[1]

    def window_exceedance(self, quantity="flow", parts=WINDOW_EXCEEDANCE_PARTS, rowset=None):
        """Per row of the last window and per level of ``set_thresholds``: ``steps_over`` (steps t with x[t] > threshold, compared
        in the plan's dtype; a NaN on either side is not over, nor is equality), ``first_step`` and ``last_step`` (the first and the
        last such t, 1-based, 0 if none) and ``longest_run`` (the longest run of consecutive such steps) of ``quantity`` ("flow",
        "velocity" or "depth"), reduced on the device over EVERY step of the result (trmc_window_exceedance): a dict of int32
        [rows, K] arrays, the parts asked for only.  rowset (``rowset(rows)``): the rows of that set, in its order, each against
        the thresholds of the row it names."""
        if quantity not in _lib.X_NAMES:
            raise ValueError(f"unknown quantity {quantity!r}: one of {sorted(_lib.X_NAMES)}")
        parts = (parts,) if isinstance(parts, str) else tuple(parts or ())
        unknown = [p for p in parts if p not in self.WINDOW_EXCEEDANCE_PARTS]
        if unknown:
            raise ValueError(f"unknown part(s) of a window exceedance {unknown}: one of {list(self.WINDOW_EXCEEDANCE_PARTS)}")
        if not parts:
            raise ValueError("window_exceedance: no part asked for")
        n = self.nseg if rowset is None else self._rowset_n[rowset]
        k = getattr(self, "_th_levels", 0)
        order = self.WINDOW_EXCEEDANCE_PARTS
        out = self._column_block((name, np.int32, (n, k)) for name in order if name in parts)
        # (without thresholds the arrays are empty and the library refuses the call)
        _lib.check(_lib.lib().trmc_window_exceedance(self._h, -1 if rowset is None else int(rowset), _lib.X_NAMES[quantity],
                                                     *(_lib.ptr(out.get(name)) for name in order)))
        return out

    def window_exceedance_kernel_ms(self):
        """device time (ms) of the last ``window_exceedance``'s kernel, from events around it (trmc_window_exceedance_kernel_ms)"""
        return self._kernel_ms(_lib.lib().trmc_window_exceedance_kernel_ms)

    def bankfull_depth(self):
        """[nseg] in the plan's dtype: the bankfull depth the step kernels use, +inf on rows that route no Muskingum-Cunge step
        (boundary rows, reservoirs) -- trmc_plan_bankfull_depth.  ``set_thresholds(plan.bankfull_depth())`` and
        ``window_exceedance("depth")``: the steps a row was out of bank."""
        out = np.empty((self.nseg,), self.dtype)
        _lib.check(_lib.lib().trmc_plan_bankfull_depth(self._h, _lib.ptr(out) if out.size else None))
        return out

    def set_nan_is_zero(self, on=True):
        """uploads of forcing and state: NaN -> 0 on the device (trmc_plan_set_nan_is_zero)"""
        _lib.check(_lib.lib().trmc_plan_set_nan_is_zero(self._h, int(bool(on))))

    def download_final_state(self):
        out = _lib.result_empty((self.nseg, 3), self.dtype)
        _lib.check(_lib.lib().trmc_download_final_state(self._h, _lib.ptr(out)))
        return out

    def download_iterations(self):
        """uint8 [nseg]: secant iterations each row spent on the last routed timestep (diagnostic)."""
        out = np.zeros(self.nseg, dtype=np.uint8)
        _lib.check(_lib.lib().trmc_download_iterations(self._h, _lib.ptr(out)))
        return out

    def collect_cost(self, enable=True):
        """Sum min(secant iterations, 3) per row over the timesteps of the windows routed from now on (the cost
        hint of ``RoutingPlan(cost_hint=...)``); off by default."""
        _lib.check(_lib.lib().trmc_plan_collect_cost(self._h, int(bool(enable))))

    def download_cost(self):
        """(uint16 [nseg] cost sums of the last window, its number of timesteps)"""
        out = np.zeros(self.nseg, dtype=np.uint16)
        n = C.c_int32(0)
        _lib.check(_lib.lib().trmc_download_cost(self._h, _lib.ptr(out), C.byref(n)))
        return out, n.value

    def gather_flow_rows_resident(self, rows):
        """Gather into plan-owned HBM (no host copy); download_gathered() fetches it later."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        self._gathered_shape = (rows.shape[0], self._nsteps)
        _lib.check(_lib.lib().trmc_gather_flow_rows(self._h, _lib.ptr(rows), rows.shape[0], None, 1))

    def download_gathered(self):
        out = _lib.result_empty(self._gathered_shape, self.dtype)
        if out.size:
            _lib.check(_lib.lib().trmc_download_gathered(self._h, _lib.ptr(out)))
        return out

    def hot_rows(self):
        """Diagnosis (trmc_plan_hot_rows): rows the tiles have routed from the hot list so far, all windows together."""
        n = C.c_int64(0)
        _lib.check(_lib.lib().trmc_plan_hot_rows(self._h, C.byref(n)))
        return n.value

    def hot_state(self):
        """Diagnosis (trmc_plan_hot_state): the hot lists as the launches queued so far leave them -- ``cap`` entries per list,
        ``hot_home`` blocks that take the list in the next launch, ``counts`` [3] lengths as attempted appends (above ``cap``: the
        list overflowed), ``cur_next`` the list the next launch reads, and the build's ``tile_block`` and ``wave_max``."""
        cap, home, cur, blk, wmax = (C.c_int32(0) for _ in range(5))
        counts = (C.c_int32 * 3)()
        _lib.check(_lib.lib().trmc_plan_hot_state(self._h, C.byref(cap), C.byref(home), counts, C.byref(cur), C.byref(blk),
                                                  C.byref(wmax)))
        return {"cap": cap.value, "hot_home": home.value, "counts": [int(c) for c in counts], "cur_next": cur.value,
                "tile_block": blk.value, "wave_max": wmax.value}

    def set_output_stride(self, stride):
        """Windows begun from now on write every `stride`-th step of (q, v, d) aside as they go (trmc_plan_set_output_stride):
        what ``fetch_begin(..., output_stride=stride)`` then copies without another pass over the result; 0 / None: off."""
        _lib.check(_lib.lib().trmc_plan_set_output_stride(self._h, int(stride or 0)))

    def set_stamps(self, nwindows=8):
        """Diagnosis (trmc_plan_set_stamps): returns a page-locked uint64 array [nwindows, 4] that window k since this call
        fills (row k % nwindows) with the device clock (100 MHz) at: tiles begin, last tile ended, tail begins, last step
        launch ended.  nwindows = 0 switches it off."""
        if not nwindows:
            _lib.check(_lib.lib().trmc_plan_set_stamps(self._h, None, 0))
            self._stamps = None
            return None
        ring = _lib.result_empty((int(nwindows), 4), np.uint64, always_pinned=True)
        ring[...] = 0
        _lib.check(_lib.lib().trmc_plan_set_stamps(self._h, _lib.ptr(ring), int(nwindows)))
        self._stamps = ring
        return ring

    def fetch_begin(self, rowset, want_state=True, output_stride=None):
        """Start the asynchronous fetch of a window's products (include/trmc.h trmc_fetch_begin): the hydrographs of a
        registered row set and / or the final state, into page-locked arrays; returns at once.  ``fetch_wait()`` hands the
        arrays over when the copy stream is through -- typically after the NEXT window has been queued.  The arrays come
        from a ring of three sets the plan keeps (all made at the first call: no allocation in a steady pipeline), so what
        ``fetch_wait()`` returned stays valid until the third fetch_begin() after it.

        output_stride = n: also every n-th step of (q, v, d) of every row, [nseg, nsteps // n, 3], decimated on the device
        and copied beside the next window (trmc_fetch_begin_fvd); ``fetch_wait()`` then returns three arrays."""
        nrows = 0 if rowset is None else self._rowset_n[rowset]
        stride = None if output_stride is None else int(output_stride)
        if stride is not None and stride < 1:
            raise ValueError("output_stride must be >= 1")
        shape = ((nrows, self._nsteps) if rowset is not None else None, (self.nseg, 3) if want_state else None,
                 None if stride is None else (self.nseg, self._nsteps // stride, 3))
        ring = getattr(self, "_fetch_ring", None)
        if ring is None or ring["shape"] != shape:
            ring = {"shape": shape, "k": 0,
                    "sets": [tuple(None if sh is None else _lib.result_empty(sh, self.dtype, always_pinned=True) for sh in shape)
                             for _ in range(3)]}
            self._fetch_ring = ring
        hyd, q0, fvd = ring["sets"][ring["k"] % 3]
        ring["k"] += 1
        rs = -1 if rowset is None else int(rowset)
        if stride is None:
            _lib.check(_lib.lib().trmc_fetch_begin(self._h, rs, _lib.ptr(hyd), _lib.ptr(q0)))
            self._fetch = (hyd, q0)
        else:
            _lib.check(_lib.lib().trmc_fetch_begin_fvd(self._h, rs, _lib.ptr(hyd), _lib.ptr(q0), stride,
                                                       _lib.ptr(fvd) if fvd.size else None))
            self._fetch = (hyd, q0, fvd)

    def fetch_wait(self):
        _lib.check(_lib.lib().trmc_fetch_wait(self._h))
        out, self._fetch = getattr(self, "_fetch", (None, None)), (None, None)
        return out

    def gather_flow_rows(self, rows, device_ptr=None):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if device_ptr is not None:
            _lib.check(_lib.lib().trmc_gather_flow_rows(self._h, _lib.ptr(rows), rows.shape[0],
                                                        C.c_void_p(device_ptr), 1))
            return None
        out = np.empty((rows.shape[0], self._nsteps), dtype=self.dtype)
        _lib.check(_lib.lib().trmc_gather_flow_rows(self._h, _lib.ptr(rows), rows.shape[0], _lib.ptr(out), 0))
        return out

    def route(self, nsteps, qts_subdivisions, assume_short_ts, qlat, q0, boundary_fvd=None):
        """upload + route + download: fvd [nseg, nsteps, 3]."""
        self.upload_forcing(nsteps, qlat, q0, boundary_fvd)
        self.route_device(nsteps, qts_subdivisions, assume_short_ts)
        return self.download_fvd()


def segments(inputs, device=0, arithmetic="exact", with_iterations=False):
    """Batch of independent single-segment steps on the GPU.  inputs [n,15] -> [n,6] (and, with_iterations, the secant
    iterations of every step, int32 [n]).  arithmetic: "exact" | "tolerance" (include/trmc.h, trmc_plan_options)."""
    inputs = np.ascontiguousarray(inputs)
    if inputs.dtype == np.float32:
        precision = 32
    elif inputs.dtype == np.float64:
        precision = 64
    else:
        raise ValueError("inputs must be float32 or float64")
    if inputs.ndim != 2 or inputs.shape[1] != 15:
        raise ValueError("inputs must be [n, 15]")
    out = np.empty((inputs.shape[0], 6), dtype=inputs.dtype)
    iters = np.zeros(inputs.shape[0], dtype=np.int32) if with_iterations else None
    _lib.mark_hip_started()
    _lib.check(_lib.lib().trmc_segments_ex(device, precision, {"exact": _lib.ARITH_EXACT, "tolerance": _lib.ARITH_TOLERANCE}[arithmetic],
                                           inputs.shape[0], _lib.ptr(inputs), _lib.ptr(out), _lib.ptr(iters)))
    return (out, iters) if with_iterations else out


def reservoir_da_steps(kind, obs, time, fin, iin=None, device=0):
    """Batch of independent reservoir data-assimilation steps on the GPU (include/trmc.h trmc_reservoir_da_steps), through the
    device functions the step kernels call.  kind "hybrid": obs, time [n, ncol], fin [n, 12] -> [n, 6]; kind "rfc": obs
    [n, ncol], fin [n, 9], iin [n, 6] -> ([n, 3], timeseries_idx [n])."""
    hybrid = {"hybrid": True, "rfc": False}[kind]
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    fin = np.ascontiguousarray(fin, dtype=np.float32)
    n = fin.shape[0]
    if obs.ndim != 2 or obs.shape[0] != n or fin.shape != (n, 12 if hybrid else 9):
        raise ValueError("obs must be [n, ncol], fin [n, 12] (hybrid) or [n, 9] (rfc)")
    if hybrid:
        time = np.ascontiguousarray(time, dtype=np.float32)
        if time.shape != obs.shape:
            raise ValueError("time must have the shape of obs")
        iin = iout = None
    else:
        time = None
        iin = np.ascontiguousarray(iin, dtype=np.int32)
        if iin.shape != (n, 6):
            raise ValueError("iin must be [n, 6]")
        iout = np.zeros(n, dtype=np.int32)
    fout = np.zeros((n, 6 if hybrid else 3), dtype=np.float32)
    _lib.mark_hip_started()
    _lib.check(_lib.lib().trmc_reservoir_da_steps(device, _lib.RESERVOIR_DA_HYBRID if hybrid else _lib.RESERVOIR_DA_RFC, n,
                                                  obs.shape[1], _lib.ptr(obs), _lib.ptr(time), _lib.ptr(fin), _lib.ptr(iin),
                                                  _lib.ptr(fout), _lib.ptr(iout)))
    return fout if hybrid else (fout, iout)
