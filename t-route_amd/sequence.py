"""A SEQUENCE of routing windows ("days") on one network -- what an operational cycle does with the reference: every call of
``compute_nhd_routing_v02`` gets that window's ``qlat_values`` (mc_reach.pyx:173,:723) and starts from the state the window
before left (``AbstractNetwork.new_q0``, AbstractNetwork.py:177-191).  Here the windows follow each other on the device
without the host in between:

  * every day's forcing travels host -> device on a copy stream while the day before is being routed (page-locked memory,
    ``trmc_stage_forcing``);
  * the state is handed from day to day in HBM (``trmc_plan_chain_from`` between a plan and its clone on one GPU; the
    resident state of the merged plan on a rank of a multi-GPU job);
  * every day's products -- the outlet hydrographs and the final state, SURVEY 8d's throughput mode -- are copied to
    page-locked host arrays beside the next day's kernels (``trmc_fetch_begin``) and handed to the caller a day later.

One GPU (``world == 1``): the days take turns on the router's plan and a clone of it (ONE copy of topology and parameter
columns in HBM, two sets of window buffers), both in sequence mode (trmc_plan_options.sequence_mode), so that day w + 1's
leading levels run while day w's narrow levels are finishing.  The order in which a day's pieces are queued is what the
shared hardware queues need ("A sequence of days"): the window; BEHIND its last launch the gathers of its
products and their copy to the host; behind its set-up the forcing of the plan's NEXT day, two days ahead.

Several ranks (``ShardedRouter`` with a communicator): the same protocol on every rank's merged plan (its sub-basins plus
the time-skewed trunk it owns): the day's forcing of the rank's rows staged from page-locked memory, the cut-edge
hydrographs exchanged chunk by chunk (``ShardedRouter.route_on_device``), the outlet block gathered, the rank's final
state and the block fetched beside the next day.

Reference analogue of the loop: nwm_routing/__main__.py:1112-1226 (``nwm_route`` per run set, ``new_q0`` between them).
"""
import time

import numpy as np

from . import _lib
from . import stream_products as SP


def pinned_like(array):
    """A page-locked copy of a forcing array (what ``stage_forcing`` wants to copy from without a wait)."""
    out = _lib.result_empty(array.shape, array.dtype, always_pinned=True)
    out[...] = array
    return out


class DaySequence:
    """``DaySequence(router, nsteps, qts_subdivisions)`` then ``run(days, state0, steps, warmup)``.

    router : a ``ShardedRouter`` (one rank of a job of any size; ``enable_device_exchange`` done when world > 1)
    output_stride : None, or n -- every n-th step of every row's (q, v, d) with each day's products
    """

    def __init__(self, router, nsteps, qts_subdivisions, assume_short_ts=True, nchunks=None, hydrographs_on_every_rank=False,
                 output_stride=None, timeline=False):
        if not assume_short_ts:
            raise ValueError("a pipelined sequence of windows needs assume_short_ts (a day's leading levels run ahead of the "
                             "day before's narrow ones only there); route general-mode windows one by one")
        self.r = router
        self.nsteps, self.qts, self.nchunks = int(nsteps), int(qts_subdivisions), nchunks
        self.world = router.world
        self._hyd_everywhere = bool(hydrographs_on_every_rank)   # (default: the gathered outlet block goes to rank 0's host only)
        # every output_stride-th step of (q, v, d) of every row as a further product of each day -- what the reference's
        # writers take at stream_output_internal_frequency (nwm_routing/output.py:209-216) -- decimated on the device and
        # copied beside the next day (trmc_fetch_begin_fvd); on_day then gets a fourth argument
        self.output_stride = None if output_stride is None else int(output_stride)
        self._clone = None
        self._local_days = None
        self.timeline = [] if timeline else None            # (diagnosis: host time, in ms, at which each call of a day returned)
        if self.world == 1:
            p = router.plan0
            if p.engine != "levels":
                raise ValueError("the one-GPU sequence pipeline runs on the level engine (a plan created for assume_short_ts "
                                 "with a million rows or more, or engine='levels')")
            self._clone = p.clone()
            self.plans = [p, self._clone]
            for pl in self.plans:
                pl.set_sequence_mode(True)
            self.set_output_stride(self.output_stride)
            self._rs = [pl.rowset(router.my_out0_local) for pl in self.plans]

    def set_output_stride(self, stride):
        """(Between runs.)  None / 0: the days' products are the outlet hydrographs and the final state; n: also every n-th step
        of every row's (q, v, d) -- the plans are told, so that their windows write the kept steps aside as they go
        (trmc_plan_set_output_stride)."""
        stride = int(stride) if stride else None
        if self.world == 1 and (stride or self.output_stride):
            for pl in self.plans:
                pl.set_output_stride(stride or 0)
        self.output_stride = stride

    def close(self):
        if self._clone is not None:
            self._clone.close()
            self._clone = None
            self.r.plan0.set_sequence_mode(False)
            if self.output_stride:
                self.r.plan0.set_output_stride(0)
                self.output_stride = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------------------------------------------------------
    def prepare_days(self, days):
        """Multi-rank jobs: this rank's rows of every day in page-locked memory (where a caller would have read them from the
        forcing file to).  One GPU: the arrays as they are (they should be page-locked: ``pinned_like``)."""
        if self.world == 1:
            return list(days)
        rows = self.r.sequence_rows()
        return [pinned_like(np.ascontiguousarray(d[rows])) for d in days]

    def run(self, days, state0, steps, warmup=0, on_day=None, prepared=False):
        """Route ``warmup + steps`` consecutive days; day w takes ``days[w % len(days)]`` (global rows; a ring that is used in
        turn -- the state evolves on, no two windows are the same work) and starts from day w - 1's final state (day 0 from
        ``state0`` [nseg, 3], or from the router's resident state if None).  The clock covers the ``steps`` days after the
        warm-up ones, everything a day needs inside it.  ``on_day(w, hydrographs, final_state)`` -- with ``output_stride``
        ``on_day(w, hydrographs, final_state, fvd)``, fvd [rows, nsteps // output_stride, 3] (one GPU: all rows in the
        caller's order; a rank: a list with the block of its ``sequence_rows()``) -- is called as each day's products arrive
        on the host (arrays of a ring of three: copy what is kept).

        Returns {"el": wall seconds of the timed days, "ms_main": [per-day device ms], "day_ms": [host-observed periods],
        "hyd", "final": the last day's products, "days_routed", "last_plan"}."""
        days = list(days) if prepared else self.prepare_days(days)
        if self.world == 1:
            return self._run_one_gpu(days, state0, steps, warmup, on_day)
        return self._run_rank(days, state0, steps, warmup, on_day)

    # ---- one GPU: a plan and its clone ---------------------------------------------------------------------------------
    def _run_one_gpu(self, days, state0, steps, warmup, on_day):
        from . import comm as X
        plans, rs, nsteps, qts = self.plans, self._rs, self.nsteps, self.qts
        nd, total = len(days), warmup + steps
        dev = plans[0].info()["device"]

        tl, tl0 = self.timeline, time.perf_counter()
        rings = [p.set_stamps(16) for p in plans] if tl is not None else None   # (diagnosis: the device's own clock per window)

        def mark(what, w):
            if tl is not None:
                tl.append((round((time.perf_counter() - tl0) * 1e3, 2), what, w))

        def queue(p):
            p.route_begin(nsteps, qts, True)
            p.route_advance(nsteps)

        def after_window(i, w):
            """behind day w's set-up on plan i the forcing of the plan's next day (w + 2), behind its last launch its products to
            the host.  In this order: copies and the events behind them share ONE in-order hardware queue (the low-priority
            one), and the forcing queued behind a day's products would wait for their copy to end -- with the decimated result
            among them (14 ms) it then reached the device 5 ms after the day it is for should have begun."""
            if w + 2 < total:
                plans[i].stage_forcing(nsteps, days[(w + 2) % nd])
                mark("stage_forcing", w + 2)
            plans[i].fetch_begin(rs[i], True, self.output_stride)
            mark("fetch_begin", w)
        plans[0].upload_forcing(nsteps, days[0], state0)        # the first day the ordinary way (synchronous)
        if total > 1:
            plans[1].stage_forcing(nsteps, days[1 % nd])
        ms_main, ends, got = [], [], (None, None, None)

        def deliver(d):
            nonlocal got
            got = plans[d % 2].fetch_wait()                     # day d's products are on the host
            mark("fetch_wait", d)
            if on_day is not None:
                on_day(d, *got)
        # Products are handed over a day after their window -- or TWO days after it when every row's decimated series is
        # among them: that block (0.8 GB of a CONUS day) takes most of the next window to cross PCIe, and a host that waited
        # for it before queueing the day after would let the device run out of queued work once a day.  (A plan has one fetch
        # in flight: day w - 2's is waited for right before day w's begins, on the same plan.)
        lag = 2 if self.output_stride else 1
        t0 = time.perf_counter() if warmup == 0 else None       # (no warm-up day: the clock starts with day 0's window)
        queue(plans[0])
        after_window(0, 0)
        for w in range(1, total + 1):
            cur, prev = plans[w % 2], plans[(w - 1) % 2]
            if w < total:
                cur.chain_from(prev)                            # day w starts where day w - 1 ends: handed over in HBM
                mark("chained", w)
                queue(cur)
                mark("queued", w)
                if lag == 2 and w >= 2:
                    deliver(w - 2)
                after_window(w % 2, w)
            st = prev.route_end()                               # day w - 1 is through
            mark("route_end", w - 1)
            ends.append(time.perf_counter())
            if w - 1 >= warmup:
                ms_main.append(st["ms_main"])
            if lag == 1:
                deliver(w - 1)
            if w == warmup and warmup > 0:                      # the clock starts when the last warm-up day is through
                t0 = time.perf_counter()
        if lag == 2:
            for d in range(max(0, total - 2), total):
                deliver(d)
        X.device_synchronize(dev)
        el = time.perf_counter() - t0
        day_ms = [round((b - a) * 1e3, 2) for a, b in zip(ends[:-1], ends[1:])][max(0, warmup - 1):]
        if rings is not None:       # the last days on the device's clock (ms from the first of them): tiles begin / end, tail begins / ends
            first = max(0, total - 8)
            rows = [rings[d % 2][(d // 2) % 16].astype(np.int64) for d in range(first, total)]
            base = int(min(r[0] if r[0] else r[2] for r in rows))
            self.device_days = [(first + i, *[round((int(v) - base) / 1e5, 2) if v else None for v in r]) for i, r in enumerate(rows)]
            for p in plans:
                p.set_stamps(0)
        return {"el": el, "ms_main": ms_main, "hyd": got[0], "final": got[1], "fvd": got[2] if len(got) > 2 else None,
                "days_routed": total, "last_plan": plans[(total - 1) % 2], "day_ms": day_ms}

    # ---- one rank of a multi-GPU job: the merged plan, day after day ----------------------------------------------------------
    def _run_rank(self, days, state0, steps, warmup, on_day):
        r = self.r
        X, dev, comm = r._X, r._dev, r._comm
        nsteps, qts = self.nsteps, self.qts
        nd, total = len(days), warmup + steps
        r.begin_sequence(nsteps, days[0], state0, qts, self.nchunks)   # day 0's forcing and state, synchronously
        ms_main, ends, got = [], [], (None, None)

        def sync():
            X.device_synchronize(dev)
            comm.barrier()
        sync()
        t0 = time.perf_counter() if warmup == 0 else None
        for w in range(total):
            # day w: every hand-off in HBM (route_on_device's body); day w + 1's forcing is staged as soon as day w is queued
            # to its end -- it travels beside the window, and day w + 1 continues from the state day w leaves
            nxt = days[(w + 1) % nd] if w + 1 < total else None
            rows, hyd = r.route_staged(qts, self.nchunks, next_qlat=nxt)
            ends.append(time.perf_counter())
            if w >= warmup:
                ms_main.append(r.last_stats["phase0"]["ms_main"])
            if w >= 1:
                got = r.fetch_wait()                                # day w - 1's products (copied beside day w)
                if on_day is not None:
                    on_day(w - 1, *got)
            r.fetch_begin(hyd, want_hyd=(r.rank == 0 or self._hyd_everywhere), output_stride=self.output_stride)
            if w + 1 == warmup:                                     # the clock starts when the last warm-up day is through
                sync()
                t0 = time.perf_counter()
        got = r.fetch_wait()
        if on_day is not None:
            on_day(total - 1, *got)
        sync()
        el = time.perf_counter() - t0
        el = float(comm.all_reduce_max_host(np.array([el], dtype=np.float64))[0])
        day_ms = [round((b - a) * 1e3, 2) for a, b in zip(ends[:-1], ends[1:])][max(0, warmup - 1):]
        return {"el": el, "ms_main": ms_main, "hyd": got[0], "final": got[1], "fvd": got[2] if len(got) > 2 else None,
                "days_routed": total, "last_plan": r._state_plans[0], "day_ms": day_ms}


# ---- the parts of RouteStream.route: each keeps one thing from day to day ------------------------------------------------
def days_spanned(lag, tpd):
    """the days that a lag of ``lag`` tiles spans, at ``tpd`` tiles per day"""
    return -(-lag // tpd)


def ring_sizes(lmax_mine, lmax_all, tpd, want_fvd, low, slots_asked):
    """(slots asked of ``stream_begin``, days ``behind`` its push at which a day is delivered, days the host's staging ``ring``
    holds).  lmax_mine: the largest lag of this rank's rows, in tiles; lmax_all: of every rank's (None: one GPU).
    slots -- a day's (q, v, d) block takes most of a day to cross PCIe (0.79 GB of a CONUS day with hourly output: 14.5 ms): it is
    handed over a day later than the other products would be, so that the host never waits for a copy while the device runs out
    of queued days, and the ring holds a slot more for it.  Several ranks hand a day over in the same iteration -- when the rank
    whose rows run furthest behind (the trunk's owner) has it: a rank's ring must hold its days that long.
    behind -- a day's products are waited for a day after they were queued (the host then never waits for launches it has just
    queued: the device always holds a day of work); low (latency="low"): right after the day's own push, which is flushed.
    ring -- a staging buffer is read by the copy that the day's push queues, and only the delivery of a day makes the host wait
    for that copy: before day d is staged the days up to d - 1 - behind have been delivered, so their forcing has been read.  The
    ring of a day's forcing and tables must therefore be behind + 1 days deep -- with three, a host that ran ahead of the device
    (several ranks: the first delivery comes days after the first push) overwrote the forcing of a day not copied yet."""
    slots, later = slots_asked, 1 if want_fvd else 0
    if lmax_all is not None:
        slots = max(slots, days_spanned(lmax_all, tpd) + 3 + later)
    elif want_fvd:
        slots = max(slots, 3 + days_spanned(lmax_mine + 1, tpd))
    behind = 0 if low else days_spanned(lmax_mine if lmax_all is None else lmax_all, tpd) + 1 + later
    return slots, behind, max(3, behind + 1)


def _next_of(it, what, day):
    try:
        return next(it)
    except StopIteration:
        raise ValueError(f"{what} ended before the forcings (day {day})") from None


class ProductRing:
    """A stream's page-locked destinations: day d hands over into slot d % slots.  A slot holds one array per row of
    ``stream_products.PRODUCTS`` that the stream carries (``has``: what the rows' ``on`` ask for), under the row's name --
    nothing is allocated for a product the stream does not hand over."""

    def __init__(self, slots, plan_dtype, dims, has):
        carried = [p for p in SP.ALL if p.on is None or has.get(p.on)]
        self._slots = [{p.name: _lib.result_empty(SP.shape_of(p, dims), SP.dtype_of(p, plan_dtype), always_pinned=True) for p in carried}
                       for _ in range(slots)]
        self._keywords = [SP.push_keywords(a) for a in self._slots]
        self.parts = SP.SUMMARY[:len(self._keywords[0].get("summary", ()))]     # the parts a day's dict names (None: not asked for)

    def arrays(self, day):
        return self._slots[day % len(self._slots)]

    def keywords(self, day):        # (the slot as ``RoutingPlan.stream_push`` takes it)
        return self._keywords[day % len(self._slots)]


class ForcingStage:
    """Page-locked staging buffers for forcing that is not page-locked where it is: made when a day needs one, ``depth`` days deep."""

    def __init__(self, depth, shape, dtype):
        self.depth, self.shape, self.dtype, self._bufs = depth, shape, dtype, {}

    def pinned(self, day, q):
        if _lib.is_pinned(q) and q.dtype == self.dtype and q.flags.c_contiguous:
            return q
        if day % self.depth not in self._bufs:
            self._bufs[day % self.depth] = _lib.result_empty(self.shape, self.dtype, always_pinned=True)
        self._bufs[day % self.depth][...] = q
        return self._bufs[day % self.depth]


class GageCarry:
    """The gages' last observations from day to day, as between two calls of the window path: the values as they are, the times
    less the day's length.  ``nudging(day, usgs_values)``: the day's tables as ``stream_push(nudging=...)`` takes them, in
    page-locked arrays of a ring ``depth`` days deep; ``lastobs(day)``: (lastobs_times, lastobs_values) as that day left them, once."""

    def __init__(self, ngage, nsteps, dtype, routing_period, depth, lastobs=None, da_parameters=None):
        from .routing.fast_reach import simple_da
        self._resolve = simple_da.resolve_tables
        dap = {"da_decay_coefficient": 120.0, "routing_period": None, **(da_parameters or {})}
        self.nsteps, self.decay = nsteps, dap["da_decay_coefficient"]
        self.period = routing_period if dap["routing_period"] is None else dap["routing_period"]
        nan = np.full(ngage, np.nan, dtype=np.float32)
        self.lv, self.lt = (nan, nan.copy()) if lastobs is None else (np.asarray(x, dtype=np.float32) for x in lastobs[:2])
        if self.lv.shape != (ngage,) or self.lt.shape != (ngage,):
            raise ValueError("lastobs must be (lastobs_values [ngage], time_since_lastobs [ngage])")
        self.day_len = np.float32(nsteps * self.period)
        self._tabs = [[_lib.result_empty(s, t, always_pinned=True) for s, t in (
            ((ngage, nsteps), np.uint8), ((ngage, nsteps), dtype), ((ngage, nsteps), dtype), ((ngage,), dtype))] for _ in range(depth)]
        self._left = {}

    def nudging(self, day, usgs):
        mode, a, w, lt_fin, lv_fin = self._resolve(self.nsteps, self.period, self.decay, usgs, self.lv, self.lt)
        tabs = self._tabs[day % len(self._tabs)]
        tabs[0][...], tabs[1][...], tabs[2][...] = mode, a, w
        u = np.asarray(usgs, dtype=np.float32)
        tabs[3][...] = u[:, 0] if (u.ndim == 2 and u.shape[1] > 0) else np.nan     # (mc_reach.pyx:404-411)
        self._left[day] = (lt_fin, lv_fin)
        self.lv, self.lt = lv_fin, (lt_fin - self.day_len).astype(np.float32)      # (the next day counts from its own start)
        return tuple(tabs)

    def lastobs(self, day):
        return self._left.pop(day, (None, None))


class ReservoirDaCarry:
    """The host's copy of the state of every reservoir-DA table row, as the reference's loop hands it from run set to run set
    (mc_reach.pyx:820-837).  ``rda``: the router's declaration (kind, table_row, usgs, usace, rfc[, ids]); ``tuples(state, tsidx)``
    of the next day delivered: the three tuples that day left -- the device's values in a reservoir's rows, the others' times a day less."""

    def __init__(self, rda, nsteps, period):
        f32, i32 = (lambda a: np.array(a, dtype=np.float32)), (lambda a: np.array(a, dtype=np.int32))
        self.kind, self.trow = np.asarray(rda[0]).tolist(), np.asarray(rda[1], dtype=np.int64).tolist()
        n_of = [0 if t is None else len(t[0]) for t in rda[2:5]]
        ids = rda[5] if len(rda) > 5 else [np.arange(n) for n in n_of]
        self.hyb = [[i32(ids[k])] + ([f32(rda[2 + k][2])[:, j] for j in range(4)] if n_of[k] else [f32([])] * 4) for k in (0, 1)]
        self.rfc = [i32(ids[2]), f32(rda[4][1]) if n_of[2] else f32([]), i32(rda[4][2])[:, 0] if n_of[2] else i32([])]
        self.t_end = np.float32(np.float32(nsteps) * np.float32(period))

    def tuples(self, state, tsidx):
        hyb, rfc = self.hyb, self.rfc
        for times in (hyb[0][1], hyb[0][4], hyb[1][1], hyb[1][4], rfc[1]):
            times -= self.t_end
        for i, (kd, tr) in enumerate(zip(self.kind, self.trow)):
            if kd in (2, 3):
                for j in range(4):
                    hyb[kd - 2][1 + j][tr] = state[i, j]
            elif kd in (4, 5):
                rfc[1][tr], rfc[2][tr] = state[i, 0], tsidx[i]
        return tuple(tuple(x.copy() for x in t) for t in (hyb[0], hyb[1], rfc))     # (the caller's own: the carry moves on)


class CutExchange:
    """The daily exchange of the cut-edge hydrographs between ranks: ``exchange(day)``, when every rank's cut rows are through
    ``day`` -- gathered, all-gathered, into the trunk's boundary rows.  on_device: everything in HBM on the router's exchange
    stream, double-buffered; otherwise through the host (any communicator with ``all_gather_rows_host``)."""

    def __init__(self, router, plan, comm, on_device, nsteps):
        self.r, self.P, self.comm, self.on_device, self.nsteps = router, plan, comm, on_device, nsteps
        self.ncut = int(router.cut_rows.shape[0])
        if on_device:
            self.nbytes = max(router._max_cut, 1) * nsteps * np.dtype(plan.dtype).itemsize
            self.send = [router._X.DeviceBuffer(router._dev, self.nbytes) for _ in range(2)]
            self.recv = [router._X.DeviceBuffer(router._dev, router.world * self.nbytes) for _ in range(2)]

    def exchange(self, day):
        r, P = self.r, self.P
        if self.ncut == 0 or day < 0:
            return
        if not self.on_device:
            parts = self.comm.all_gather_rows_host(P.stream_gather_host(day, r._rsS_cut))
            if r.plan1 is not None:
                cut_q = np.zeros((self.ncut, self.nsteps), dtype=P.dtype)
                for k, blk in enumerate(parts):
                    cut_q[r.cut_owner == k] = blk
                P.stream_boundary_host(day, cut_q[r.b_cut_index])
            return
        send, recv = self.send[day % 2], self.recv[day % 2]
        P.stream_gather(day, r._rsS_cut, send.ptr, stream=r._sc)
        self.comm.all_gather(send.ptr, recv.ptr, self.nbytes, r._sc)
        if r.plan1 is not None:
            P.stream_boundary(day, recv.ptr, self.nsteps, index_ptr=r._d_b_index.ptr, stream=r._sc)


class RouteStream:
    """The product's run-set loop (the reference: ``for run in run_sets: nwm_route(...) -> compute_nhd_routing_v02(...); new_q0;
    assemble_forcings(next)``, nwm_routing/__main__.py:195-333) as an iterator over days::

        router = ShardedRouter(to, params, ..., stream=True)
        with RouteStream(router, nsteps, qts_subdivisions) as rs:
            for day, hydrographs, final_state in rs.route(forcings, state0):
                ...

    ``forcings``: any iterable of [nseg, nq] arrays (global rows; page-locked ones -- ``pinned_like`` -- are copied from where
    they are, others through a page-locked ring); it is consumed as far ahead as the device can take days and may yield late.
    Every day's products come back in order: the outlet hydrographs [noutlets, nsteps] (rows ``outlet_rows``; on rank 0 of a
    multi-rank job, or everywhere with ``hydrographs_on_every_rank``), the final state ([nseg, 3]; a rank of a multi-rank job:
    of its ``rows``), with ``output_stride=n`` also every n-th step of (q, v, d) of those rows.  The arrays belong to a ring:
    copy what is kept beyond the next few days.

    ``summary=("peak", "mean")`` (or one of them): every tuple ends in a dict with the day's peak flow, the 1-based step at which
    it was first reached (int32) and the mean flow, under the names of ``stream_products.SUMMARY`` -- [rows] ring arrays over
    this rank's ``rows`` in the order of the final state, formed on the device from ALL nsteps flows of the day (include/trmc.h,
    trmc_stream_set_summary; None for what was not asked).  A router with reservoirs or gages: its trailing dict gains these
    keys.  ``"peak_depth"`` adds the table's two further parts: the highest depth of the day -- the pool's water elevation at a
    reservoir row, (0, 1) at a rank's boundary copies, which nobody routes -- and the step it was first reached at, carried by
    the tile kernels through every step (a router with ``reservoir_da``: NotImplementedError).  ``"total"`` (with at least one
    of the others) keeps the maximum and the mean of the whole forecast on the device: ``rs.total`` holds
    ``RoutingPlan.stream_summary_total()`` -- ``"days"`` and the same keys over this rank's ``rows``, the steps int64 and 1-based
    from the stream's first step -- once ``route()`` has yielded its last day; ``daily_summary=False`` then leaves the per-day
    dict out (the tuples of ``summary=None``) and no per-day summary array crosses to the host.  ``np.maximum`` over the days'
    ``peak_flow`` equals ``rs.total["peak_flow"]`` only while no day's peak is a NaN: the totals fold ``if (pk_D > pk)``, which a
    NaN day after day 0 never wins and a NaN on day 0 never loses (``np.fmax``, or the fold itself, otherwise).

    ``exceedance=("flow", thresholds)``: the device also keeps, over ALL days of the stream, every row's threshold exceedance --
    ``thresholds`` [rows] or [rows, K] (K <= 4) in the router's row order, a rank of a multi-rank job taking its own ``rows`` of
    them as it does of ``state0``; they are set on the plan that streams (``RoutingPlan.set_thresholds``).  ``rs.exceedance`` holds
    ``RoutingPlan.stream_exceedance()`` -- ``"days"`` and int64 [rows, K] ``steps_over``, ``first_step``, ``last_step``,
    ``longest_run`` over this rank's ``rows``, the steps 1-based from the stream's first step and a run carried over a day's end
    -- once ``route()`` has yielded its last day, next to ``rs.total``.  It is not a product of the day: the tuples do not change.
    Flow only ("depth", "velocity", "bankfull": NotImplementedError -- route the day in question as a window).

    ``depth_exceedance=thresholds`` or ``depth_exceedance="bankfull"``: the device also keeps, over ALL days of the stream, every
    row's threshold exceedance of DEPTH -- how long a reach is out of bank or over an action / flood stage, when it first goes over,
    the longest continuous inundation of the forecast.  ``thresholds`` [rows] or [rows, K] (K <= 4), metres, in the router's row
    order, a rank of a multi-rank job taking its own ``rows`` of them as ``exceedance=`` does; ``"bankfull"`` takes
    ``bankfull_depth()`` of the plan that streams: +inf where a row has no compound channel to leave (a reservoir) or is a rank's
    boundary copy, so such a row is never over.  ``rs.depth_exceedance`` holds ``RoutingPlan.stream_depth_exceedance()`` --
    ``"days"`` and int64 [rows, K] ``steps_over``, ``first_step``, ``last_step``, ``longest_run`` over this rank's ``rows``, the
    steps 1-based from the stream's first step and a run carried over a day's end -- once ``route()`` has yielded its last day,
    next to ``rs.exceedance``.  The depth is the one ``stage=True`` and ``full_output`` hand out: the pool's water elevation at a
    reservoir row, the step's own depth at a gage row, 0 at a rank's boundary copies (which report what a depth of 0 gives).  A
    second accumulator with a threshold table of its own: ``exceedance=`` and ``depth_exceedance=`` may be asked for together.
    Several ranks are supported -- the fold needs a row's own depth only, which every rank holds for its own rows.  Such a stream
    writes every step's depth as one with ``stage=True`` does; a router with ``reservoir_da``: NotImplementedError.  It is not a
    product of the day: the tuples do not change.

    ``courant=limit``: the device also keeps, over ALL days of the stream, every row's Courant number cn = ck dt / dx -- the
    highest, the step it was first reached at and the number of steps with cn > ``limit``: ``rs.courant`` holds
    ``RoutingPlan.stream_courant()`` -- ``"days"``, ``"peak_cn"``, ``"peak_cn_step"`` and ``"steps_over"`` over this rank's
    ``rows``, the steps int64 and 1-based from the stream's first step, ``window_courant_summary``'s definition over the days one
    after the other -- over the days handed over so far while ``route()`` runs (None before the first) and over all of them once
    it has yielded its last day.  It is not a product of the day: the tuples do not change.  Such a stream writes every step's
    depth as one with ``stage=True`` does, with stage's limits: one rank only, no ``reservoir_da`` (NotImplementedError).

    ``velocity=True`` or ``velocity=thresholds``: the device also keeps, over ALL days of the stream, every row's peak velocity and
    the step it was first reached at and, with ``thresholds`` [rows] or [rows, K] (K <= 4), m/s, in the router's row order, the
    threshold exceedance of the velocity -- the quantity ``exceedance=("velocity", ...)`` goes on refusing, because it is not a
    quantity of the flow accumulator but a FOURTH accumulator with a table of its own, which may run beside the other three.
    ``rs.velocity`` holds ``RoutingPlan.stream_velocity()`` -- ``"days"``, ``"peak_velocity"``, ``"peak_velocity_step"`` and, with
    thresholds, int64 [rows, K] ``steps_over``, ``first_step``, ``last_step``, ``longest_run``, the steps 1-based from the stream's
    first step and a run carried over a day's end -- over the days handed over so far while ``route()`` runs (None before the first)
    and over all of them once it has yielded its last day.  The velocity is column 1 of the same days routed as windows
    (``window_summary(("peak_velocity",))``, ``window_exceedance("velocity")`` over the days one after the other): 0 where a step
    had no flow and at reservoir rows.  The step loop still forms no velocity: a fold kernel re-forms it once per day from the
    depths, so such a stream writes every step's depth as one with ``stage=True`` does, with stage's limits: one rank only, no
    ``reservoir_da`` (NotImplementedError).  It is not a product of the day: the tuples do not change.

    ``stage=True``: every day also carries STAGE HYDROGRAPHS -- the depth of every step at the rows of its hydrographs: the
    trailing dict gains ``"stage"``, a ring array [len(outlet_rows), nsteps] in the hydrographs' row order (a reservoir row: its
    pool's elevation; nudging changes a gage's flow only).  The tile kernels then write a slot's depth plane at every step
    instead of at a tile's last one, and the hydrographs' gather kernel forms the array from it (include/trmc.h,
    trmc_stream_set_stage).  One rank only: with several, the outlets' stage would have to be gathered over the ranks as the
    hydrographs are, which nothing does yet -- NotImplementedError; so is a router with ``reservoir_da``.

    Underneath is ONE stream of tile launches (include/trmc.h, trmc_stream_*): the tile index runs on over the days, every
    launch routes every row through the next K steps of its own place in the stream -- a row deep in the network works on an
    earlier tile than the headwaters, possibly of an earlier day -- so a day costs nsteps / K launches and nothing else, and a
    day's products are complete ``lag`` launches after its first row finished it.  ``latency="low"`` flushes after every day
    (each day's products right after its push, at the price of the partly filled launches a single window has).

    Several ranks: every rank streams its sub-basins and small networks; the trunk of the dominant basin rides in its owner's
    stream a day or two behind, and the cut-edge hydrographs are exchanged ONCE PER DAY (an all-gather on the exchange
    stream, ``comm``) when every rank's cut rows are through that day -- SURVEY 8e's "upstream piece finishes, sends the
    tailwater hydrograph", with the order DAG resolved by the trunk's lag instead of by waiting.
    """

    PACKED_ON_RANKS = ("packed days on several ranks: the join on the feature id is made for ONE plan's rows -- a rank's own rows and "
                       "its boundary copies of other ranks' rows would each need a join of their own, which nothing builds yet; unpack "
                       "on the host (nhd_io.unpack_packed) and pass float days")

    def __init__(self, router, nsteps, qts_subdivisions, output_stride=None, full_output=False, slots=0, latency="throughput",
                 hydrographs_on_every_rank=False, comm=None, exchange=None, reservoir_da_ncol=None, summary=None,
                 daily_summary=True, velocity=None, depth_exceedance=None, courant=None, packed_forcing=None, stage=False,
                 exceedance=None):
        """comm / exchange (several ranks): the communicator -- default: the one given to ``router.enable_device_exchange`` -- and
        how the daily cut-edge hydrographs travel: "device" (gather kernel -> all-gather on the exchange stream -> boundary rows,
        everything in HBM: RCCL over xGMI) or "host" (through ``comm.all_gather_rows_host``: any communicator with that method,
        ``all_reduce_max_host`` and ``barrier`` -- a transport without device collectives; the days of slack the trunk's lag gives
        cover the round trip).  Default: "device" when the router has a device exchange, else "host".
        reservoir_da_ncol (a router with ``reservoir_da``): the most columns (usgs, usace, rfc) a day's tables may have; default:
        as many as the declared tables.
        packed_forcing: the ids of the router's rows, int64 [router.nseg] -- ``route`` then takes a day's forcing as a dict of
        ``nhd_io.chrtout_packed`` as well as a float array, and the device decodes and joins it (``RoutingPlan.stream_push(packed=)``).
        The FIRST day of such a stream, if it is packed, declares the files' feature axis and packing facts; a stream that begins
        with float days declares them here: ``(row_ids, packed)`` with any dict of those files.  One rank only."""
        self._rda_ncol = reservoir_da_ncol
        self._pk_ids = self._pk_like = None
        if packed_forcing is not None:
            if router.world > 1:
                raise NotImplementedError(self.PACKED_ON_RANKS)
            ids, like = packed_forcing if isinstance(packed_forcing, tuple) else (packed_forcing, None)
            self._pk_ids, self._pk_like = np.asarray(ids, dtype=np.int64), like
            if self._pk_ids.shape != (router.nseg,):
                raise ValueError(f"packed_forcing: the ids of the router's rows, [{router.nseg}]: got {self._pk_ids.shape}")
        from .plan import RoutingPlan
        self._cou_limit = RoutingPlan.stream_courant_limit(courant)
        self._courant = None
        if self._cou_limit is not None and router.world > 1:
            raise NotImplementedError("courant= on several ranks: the Courant number needs every step's depth of a row and of the rows above "
                                      "it, which a rank holds for its own rows only -- as for stage=True, nothing gathers it over the ranks")
        if self._cou_limit is not None and getattr(router, "_reservoir_da", None) is not None:
            raise NotImplementedError("courant= with reservoir data assimilation: the tile kernels of such a stream do not write the depth "
                                      "plane at every step (as for stage=True)")
        self._vel_th = self._velocity = None
        if velocity is not None and velocity is not False:
            self._vel_th = RoutingPlan.velocity_thresholds(velocity, router.nseg, what="velocity", rows="rows")
            if router.world > 1:
                raise NotImplementedError("velocity= on several ranks: the velocity needs every step's depth of a row and the flows of the "
                                          "rows above it, which a rank holds for its own rows only -- as for courant=, nothing gathers it "
                                          "over the ranks")
            if getattr(router, "_reservoir_da", None) is not None:
                raise NotImplementedError("velocity= with reservoir data assimilation: the tile kernels of such a stream do not write the "
                                          "depth plane at every step (as for stage=True)")
        self.stage = bool(stage)
        if self.stage and router.world > 1:
            raise NotImplementedError("stage=True on several ranks: a day's stage covers the rows of its hydrographs, which every rank holds a "
                                      "part of -- the parts are gathered over the ranks for the flows only")
        if self.stage and getattr(router, "_reservoir_da", None) is not None:
            raise NotImplementedError("stage=True with reservoir data assimilation: the tile kernels of such a stream do not write the depth "
                                      "plane at every step (as for summary 'peak_depth')")
        summary = (summary,) if isinstance(summary, str) else tuple(summary or ())
        if any(w not in _lib.SUMMARY_NAMES for w in summary):
            raise ValueError("summary: an iterable of 'peak' and / or 'mean', 'peak_depth', 'total', or None")
        if "total" in summary and len(set(summary)) < 2:
            raise ValueError("summary: 'total' needs at least one of 'peak', 'mean', 'peak_depth'")
        if not daily_summary and "total" not in summary:
            raise ValueError("daily_summary=False leaves nothing of a summary without 'total'")
        self.summary = summary
        self.daily_summary = bool(daily_summary)
        self.total = None
        self.exceedance = None
        self._exc_th = None
        if exceedance is not None:
            try:
                quantity, th = exceedance
            except (TypeError, ValueError):
                raise ValueError("exceedance: (\"flow\", thresholds)") from None
            if isinstance(th, str):     # (the drop-in's ("depth", "bankfull"): a depth)
                quantity = th if quantity in _lib.X_NAMES else quantity
            RoutingPlan.stream_exceedance_quantity(quantity)
            th = np.asarray(th)
            th = th[:, None] if th.ndim == 1 else th
            if th.ndim != 2 or th.shape[0] != router.nseg or not 1 <= th.shape[1] <= 4:
                raise ValueError(f"exceedance: thresholds must be [rows] or [rows, K] with rows = {router.nseg} and K <= 4: got {th.shape}")
            self._exc_th = th
        self.depth_exceedance = None
        self._dex_th = None
        if depth_exceedance is not None:
            if isinstance(depth_exceedance, str):
                if depth_exceedance != "bankfull":
                    raise ValueError(f"depth_exceedance: thresholds [rows] or [rows, K], or 'bankfull': got {depth_exceedance!r}")
                self._dex_th = "bankfull"       # (bankfull_depth() of the plan that streams: route())
            else:
                th = np.asarray(depth_exceedance)
                th = th[:, None] if th.ndim == 1 else th
                if th.ndim != 2 or th.shape[0] != router.nseg or not 1 <= th.shape[1] <= 4:
                    raise ValueError(f"depth_exceedance: thresholds must be [rows] or [rows, K] with rows = {router.nseg} and K <= 4: got {th.shape}")
                self._dex_th = th
            if getattr(router, "_reservoir_da", None) is not None:
                raise NotImplementedError("depth_exceedance= with reservoir data assimilation: the tile kernels of such a stream do not write "
                                          "the depth plane at every step (as for stage=True)")
        if latency not in ("throughput", "low"):
            raise ValueError("latency must be 'throughput' or 'low'")
        self.r = router
        self.comm = comm if comm is not None else getattr(router, "_comm", None)
        self.exchange = exchange or ("device" if getattr(router, "_X", None) is not None else "host")
        if self.exchange not in ("device", "host"):
            raise ValueError("exchange must be 'device' or 'host'")
        if router.world > 1 and self.comm is None:
            raise ValueError("several ranks need a communicator (router.enable_device_exchange(comm), or comm=...)")
        self.nsteps, self.qts = int(nsteps), int(qts_subdivisions)
        self.output_stride = int(output_stride) if output_stride else 0
        self.full_output = bool(full_output)
        self.slots, self.latency = int(slots), latency
        self.world, self.rank = router.world, router.rank
        self._hyd_everywhere = bool(hydrographs_on_every_rank)
        self.plan = None
        self.info = None
        self.last_info = None
        self._dc = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.plan is not None and self.info is not None:
            try:
                self.plan.stream_end()
            except Exception:
                pass
        self.info = None

    # ------------------------------------------------------------------------------------------------------------------
    def _setup(self):
        """the plan, the trunk's lag (every rank must agree on it: the largest lag among ALL ranks' cut rows decides how many
        days after a day its cut-edge hydrographs can be exchanged), the row sets"""
        r = self.r
        K = None
        if self.world == 1:
            P = r.stream_plan(0)
            self._dc = 0
        else:
            comm = self.comm
            # (the cut rows are rows of plan0 -- the sub-basins -- whose order does not depend on the trunk: their lag is known
            # before the merged plan is built, so that plan is built once, with the lag the trunk needs)
            lag0, _, _ = r.plan0.lags()
            mine = int(lag0[r.my_cut_local].max()) if r.my_cut_local.size else 0
            pmax = int(comm.all_reduce_max_host(np.array([mine], dtype=np.float64))[0])
            tpd = self.nsteps // self._tile_steps(r.plan0)
            dc = days_spanned(pmax + 1, tpd)                # days after which every rank's cut rows are through a day
            P = r.stream_plan((dc + 1) * tpd)               # ... and the tiles the trunk must run behind for that
            self._dc = dc
        self.plan = P
        self.rows = r._rowsS
        return P

    def _tile_steps(self, P):
        return int(getattr(P, "tile_steps", 16))

    @property
    def courant(self):
        """the Courant number over the days handed over so far (``courant=limit``; see the class), None before the first"""
        if self._cou_limit is not None and self.info is not None and self.plan.stream_info()["days_complete"] > 0:
            self._courant = self.plan.stream_courant()
        return self._courant

    @property
    def velocity(self):
        """the peak velocity and the velocity exceedance over the days handed over so far (``velocity=``; see the class), None
        before the first"""
        if self._vel_th is not None and self.info is not None and self.plan.stream_info()["days_complete"] > 0:
            self._velocity = self.plan.stream_velocity()
        return self._velocity

    @property
    def outlet_rows(self):
        """global rows of the hydrographs handed out (ascending)"""
        return self._out_rows

    def prepare_days(self, days):
        """This rank's rows of every day in page-locked memory (where a rank of a real job reads them from the forcing files to);
        pass ``prepared=True`` to ``route`` with such arrays.  One GPU: page-locked copies of the arrays."""
        if self.plan is None:
            self._setup()
        rows = self.rows
        local = rows.shape[0] != self.r.nseg or self.world > 1
        return [pinned_like(np.ascontiguousarray(d[rows] if local else d, dtype=self.plan.dtype)) for d in days]

    def run(self, days, state0, steps, warmup=0, on_day=None, prepared=False):
        """Measurement form (bench.py, tools/sim_ranks.py): route ``warmup + steps`` consecutive days -- day w takes
        ``days[w % len(days)]`` -- and time the ``steps`` days pushed after the warm-up ones: the device is drained (and the ranks
        meet at a barrier) before the first of them is pushed and after the last of them has been, so the clock covers exactly
        ``steps`` days of launches, each carrying every row (the stream is full: ``warmup`` is raised to the days the rows' lag
        spans), the forcing of those days on its way in and the products of as many earlier days on their way out.  What brings
        the last days to their end afterwards (the flush) is outside the clock, as the work of the warm-up days' last rows is
        inside it.  Returns {"el": seconds, "days_routed", "warmup", "hyd", "final", "fvd": the last day's products, "info"}."""
        from . import comm as X
        if self.plan is None:
            self._setup()
        days = list(days) if prepared else self.prepare_days(days)
        P, multi = self.plan, self.world > 1
        lag, _, _ = P.lags()
        tpd = self.nsteps // self._tile_steps(P)
        fill = ring_sizes(int(lag.max(initial=0)), None, tpd, bool(self.output_stride or self.full_output), False, 0)[1] + (self._dc + 1 if multi else 0)
        if multi:
            fill = int(self.comm.all_reduce_max_host(np.array([fill], dtype=np.float64))[0])
        wu = max(int(warmup), fill)
        total, nd = wu + int(steps), len(days)
        dev = P.info()["device"]
        marks = {}
        comm = self.comm

        def meet():
            if dev >= 0:
                X.device_synchronize(dev)
            if multi:
                self.comm.barrier()

        def feed():
            for w in range(total):
                if w == wu:
                    meet()
                    marks["t0"] = time.perf_counter()
                yield days[w % nd]
            meet()
            marks["t1"] = time.perf_counter()
        last, push_ms = None, []
        for item in self.route(feed(), state0, prepared=True):
            if on_day is not None:
                on_day(*item)
            if item[0] >= wu and self.info is not None:
                try:                                        # (device time of the day's own launches on the slices' stream)
                    push_ms.append(P.stream_day_ms(item[0]))
                except (RuntimeError, ValueError):
                    pass
            last = item
        el = marks["t1"] - marks["t0"]
        if multi:
            el = float(self.comm.all_reduce_max_host(np.array([el], dtype=np.float64))[0])
        return {"el": el, "days_routed": total, "warmup": wu, "hyd": last[1], "final": last[2],
                "fvd": last[3] if len(last) > 3 and not isinstance(last[3], dict) else None, "info": self.last_info, "push_ms": push_ms}

    def route(self, forcings, state0=None, prepared=False, observations=None, lastobs=None, da_parameters=None, reservoir_da=None):
        """generator of (day, hydrographs, final_state[, fvd][, dict]) -- see the class (``summary``) and below.  prepared: the arrays hold this rank's rows only
        (``prepare_days``).  A day's forcing is the float array [rows, nq] or -- ``RouteStream(..., packed_forcing=row_ids)``, one rank -- a
        dict of ``nhd_io.chrtout_packed`` whose raw columns the device decodes and joins to the rows (include/trmc.h,
        trmc_stream_push_day_packed); the two kinds may alternate.

        A router with reservoirs or gages (``ShardedRouter(..., stream=True, reservoirs=..., gages=...)``): every tuple has one more
        trailing element, a dict {"reservoir_inflow": [nres, nsteps] (the reference's upstream_array rows; None without
        reservoirs), "nudge": [ngage, nsteps], "lastobs": (lastobs_times, lastobs_values) as the day left them (None, None without
        gages)} -- arrays of the ring as well.  ``observations``: an iterable parallel to ``forcings``, a day's ``usgs_values``
        [ngage, gage_maxtimestep] (NaN = missing) indexed by the day's own timestep, as ``simple_da.resolve_tables`` takes them;
        ``lastobs`` = (lastobs_values_init, time_since_lastobs_init) of the first day (default: none known).  Every day's tables
        are resolved on the host as the drop-in resolves a window's, a gage row starts a day from the day's first observation
        (column 0, where it is not NaN: mc_reach.pyx:404-411), and the last observations go from day to day as between two
        calls of the window path: the values as they are, the times less the day's length.  ``da_parameters``:
        {"da_decay_coefficient": 120.0, "routing_period": the router's dt}.

        A router with ``reservoir_da`` (reservoir types 2-5): ``reservoir_da`` is an iterable parallel to ``forcings`` that yields
        each day's tables ``(usgs, usace, rfc[, rfc_reset_idx])`` as ``RoutingPlan.stream_push`` takes them (times from the day's
        start; the state is the device's), and the dict gains "reservoir_da": the three state tuples the day left, in the layout
        of elements [4], [5], [7] of ``compute_network_structured`` 's result -- (ids, update_time, prev_persisted_flow,
        persistence_index, persistence_update_time) for usgs and usace, (ids, update_time, timeseries_idx) for rfc, the times
        counted from the next day's start -- which a caller writes back into its ``*_param_df`` as ``update_after_compute``
        does.  Rows of a table that no reservoir of the router uses pass through as the loop passes them."""
        multi, low = self.world > 1, self.latency == "low"
        if low and multi:
            raise ValueError("latency='low' is a one-GPU option")
        r, nsteps = self.r, self.nsteps
        P = self.plan if self.plan is not None else self._setup()
        res, gages, rda = (getattr(r, a, None) for a in ("_reservoirs", "_gages", "_reservoir_da"))
        nres, ngage = 0 if res is None else res[0].shape[0], 0 if gages is None else gages.shape[0]
        if reservoir_da is not None and rda is None:
            raise ValueError("reservoir_da needs a router with data-assimilation reservoirs (ShardedRouter(..., stream=True, "
                             "reservoirs=..., reservoir_da=...))")
        if rda is not None and reservoir_da is None:
            raise ValueError("the router has data-assimilation reservoirs: route(..., reservoir_da=...) must yield every day's tables")
        if observations is not None and not ngage:
            raise ValueError("observations need a router with gages (ShardedRouter(..., stream=True, gages=rows))")
        if ngage and observations is None:
            raise ValueError("the router has gages: route(..., observations=...) must yield every day's usgs_values")
        want_fvd = bool(self.output_stride or self.full_output)
        lmax_mine = int(P.lags()[0].max(initial=0))
        lmax_all = int(self.comm.all_reduce_max_host(np.array([lmax_mine], dtype=np.float64))[0]) if multi else None
        slots, behind, depth = ring_sizes(lmax_mine, lmax_all, nsteps // self._tile_steps(P), want_fvd, low, self.slots)
        rdac = ReservoirDaCarry(rda, nsteps, res[2]) if rda is not None else None
        gage = GageCarry(ngage, nsteps, P.dtype, float(r._mk["params"][0, _lib.PARAM_COLS.index("dt")]), depth, lastobs,
                         da_parameters) if ngage else None
        it, obs_it, rda_it = (None if x is None else iter(x) for x in (forcings, observations, reservoir_da))
        nxt = next(it, None)
        if nxt is None:
            return
        rows, local = self.rows, multi or self.rows.shape[0] != r.nseg
        pick = local and not prepared                       # (the forcings hold global rows: this rank's are picked out)
        q0 = None if state0 is None else np.ascontiguousarray(state0[rows] if (local and state0.shape[0] == r.nseg) else state0, dtype=P.dtype)
        # days as packed CHRTOUT columns (the class' ``packed_forcing``): the first day's dict, or the constructor's, is the declaration
        pk_like = nxt if isinstance(nxt, dict) else self._pk_like
        if pk_like is not None and multi:
            raise NotImplementedError(self.PACKED_ON_RANKS)
        if pk_like is not None and self._pk_ids is None:
            raise ValueError("a packed day needs the ids of the router's rows: RouteStream(..., packed_forcing=row_ids)")
        nq = nxt["raw_a"].shape[0] if isinstance(nxt, dict) else nxt.shape[1]
        first = np.zeros((rows.shape[0], nq), P.dtype) if isinstance(nxt, dict) else np.ascontiguousarray(nxt[rows] if pick else nxt, dtype=P.dtype)
        P.upload_forcing(nsteps, first, q0)                    # the state and the shape of the forcing (a stream reads no more of it)
        if pk_like is not None:
            P.stream_set_packed_forcing(pk_like, self._pk_ids[rows])
        elif getattr(P, "_stream_packed", None) is not None:   # (an earlier stream's declaration is withdrawn, as its summary is)
            P.stream_set_packed_forcing(None)
        raw_stage = None
        if self.summary or getattr(P, "_stream_summary", 0):   # (the declaration outlives a stream: an earlier one's is withdrawn)
            P.stream_set_summary(self.summary)
        if self._exc_th is not None:                           # (on the plan that streams: this rank's rows of them)
            P.set_thresholds(self._exc_th[rows])
            P.stream_set_exceedance("flow")
        elif getattr(P, "_stream_exceedance", -1) >= 0:        # (an earlier stream's declaration is withdrawn, as its summary is)
            P.stream_set_exceedance(None)
        self.exceedance = None
        if self.stage or getattr(P, "_stream_stage", False):   # (likewise)
            P.stream_set_stage(self.stage)
        if self._cou_limit is not None or getattr(P, "_stream_courant", None) is not None:
            P.stream_set_courant(self._cou_limit)
        self._courant = None
        if self._dex_th is not None:                           # (a table of the stream's own: this rank's rows of the thresholds)
            P.stream_set_depth_exceedance("bankfull" if isinstance(self._dex_th, str) else self._dex_th[rows])
        elif getattr(P, "_stream_depth_levels", 0) > 0:        # (an earlier stream's declaration is withdrawn)
            P.stream_set_depth_exceedance(None)
        self.depth_exceedance = None
        if self._vel_th is not None:
            P.stream_set_velocity(self._vel_th)
        elif getattr(P, "_stream_velocity", None) is not None: # (an earlier stream's declaration is withdrawn)
            P.stream_set_velocity(None)
        self._velocity = None
        P.stream_begin(nsteps, self.qts, slots=slots, full_output=self.full_output and not self.output_stride, output_stride=self.output_stride,
                       **({} if rda is None else {"reservoir_da": True if self._rda_ncol is None else self._rda_ncol}))
        self.info = info = P.stream_info()
        self.total = None
        daily = bool(self.summary) and self.daily_summary
        ring = ProductRing(info["slots"], P.dtype,
                           {"rows": rows.shape[0], "nsteps": nsteps, "keep": nsteps // self.output_stride if self.output_stride else nsteps,
                            "outlets": max(r._outS_global.shape[0], 1), "nres": nres, "ngage": ngage},
                           {"fvd": want_fvd, "ngage": ngage, "nres": nres, "rda": rda is not None, "stage": self.stage,
                            **{w: daily for w in self.summary}})
        stage = ForcingStage(depth, (rows.shape[0], nq), P.dtype)
        xch = CutExchange(r, P, self.comm, self.exchange == "device", nsteps) if multi else None
        self._out_rows, self._order = (None, None) if multi else (np.sort(r._outS_global), np.argsort(r._outS_global, kind="stable"))
        extras = res is not None or gages is not None
        d = delivered = 0
        while nxt is not None:
            more = {"nudging": gage.nudging(d, _next_of(obs_it, "observations", d)) if gage else None} if extras else {}
            if rdac is not None:
                more["reservoir_da"] = _next_of(rda_it, "reservoir_da", d)
            if isinstance(nxt, dict):   # (a packed day: its raw columns, page-locked, in place of the float array)
                if pk_like is None:
                    raise ValueError("a packed day in a stream that began with float days: declare the files with "
                                     "RouteStream(..., packed_forcing=(row_ids, packed))")
                if raw_stage is None:
                    raw_stage = [ForcingStage(depth, nxt["raw_a"].shape, np.int32) for _ in range(2)]
                raw = {k: None if nxt.get(k) is None else s.pinned(d, nxt[k]) for k, s in zip(("raw_a", "raw_b"), raw_stage)}
                P.stream_push(packed=raw, rowset=r._rsS_out, **ring.keywords(d), **more)
            else:
                P.stream_push(stage.pinned(d, nxt[rows] if pick else nxt), rowset=r._rsS_out, **ring.keywords(d), **more)
            if low:
                P.stream_flush()
            if xch is not None:
                xch.exchange(d - self._dc)
            while delivered <= d - behind:
                yield self._deliver(delivered, ring, gage, rdac, extras)
                delivered += 1
            d += 1
            nxt = next(it, None)
        # the days still under way: no new day starts, the stream advances a day's launches at a time (the exchange of the last
        # days' cut-edge hydrographs between them), until every day has been queued to its end
        for k in range(self._dc):       # (0 on one GPU)
            P.stream_advance(info["tiles_per_day"])
            xch.exchange(d + k - self._dc)
        P.stream_flush()
        if "total" in self.summary:     # (every day has been handed over on the device: the totals of the whole stream)
            self.total = P.stream_summary_total()
        if self._exc_th is not None:    # (... and the exceedance over all of its steps)
            self.exceedance = P.stream_exceedance()
        if self._cou_limit is not None: # (... and the Courant number)
            self._courant = P.stream_courant()
        if self._dex_th is not None:    # (... and the depth exceedance)
            self.depth_exceedance = P.stream_depth_exceedance()
        if self._vel_th is not None:    # (... and the velocity)
            self._velocity = P.stream_velocity()
        while delivered < d:
            yield self._deliver(delivered, ring, gage, rdac, extras)
            delivered += 1
        self.last_info = P.stream_info()
        P.stream_end()
        self.info = None

    def _deliver(self, day, ring, gage, rdac, extras):
        """day's tuple, once its products are on the host (days are delivered in order: the carries move on with them)"""
        self.plan.stream_wait(day)
        a = ring.arrays(day)
        hyd, fin, fvd = a["hyd"][:self.r._outS_global.shape[0]], a["q0"], a.get("fvd")
        if self.world > 1:
            parts = self.comm.all_gather_rows_host(np.ascontiguousarray(hyd))
            if self._order is None:
                own = np.ascontiguousarray(self.r._outS_global.astype(np.int64)[:, None])
                rows_all = np.concatenate(self.comm.all_gather_rows_host(own))[:, 0]
                self._order = np.argsort(rows_all, kind="stable")
                self._out_rows = rows_all[self._order]
            hyd = np.concatenate(parts, 0)[self._order] if (self.rank == 0 or self._hyd_everywhere) else None
            fin, fvd = [fin], [fvd]
        else:
            hyd = hyd[self._order]
        item = (day, hyd, fin, fvd) if "fvd" in a else (day, hyd, fin)
        more = {p.name: a.get(p.name) for p in SP.RECORDS} if extras else {}    # (reservoirs and gages: the day's records)
        if extras:
            more["lastobs"] = gage.lastobs(day) if gage is not None else (None, None)
            if rdac is not None:
                more["reservoir_da"] = rdac.tuples(a["reservoir_da_state"], a["reservoir_da_tsidx"])
        more.update((p.name, a.get(p.name)) for p in ring.parts)
        if self.stage:      # (the hydrographs' rows, in their order)
            more["stage"] = a["stage"][:self.r._outS_global.shape[0]][self._order]
        return item + (more,) if (extras or ring.parts or self.stage) else item

