"""A stream of windows (trmc_stream_*) against the same days routed one by one on the same plan: every day's final state of every
row and the hydrographs of sampled rows bit for bit, and what a day costs either way.
  python tools/stream_probe.py [--nseg N] [--days D] [--wide-min-rows R] [--hint] [--stride n] [--full]
                               [--reservoirs N --gages M]   level-pool waterbodies and nudged gages scattered over the network
                               [--reservoir-da N]           N of those waterbodies are of types 2-5 (hybrid persistence, RFC series)
                                                            with synthetic tables: their data assimilation rides in the stream
                               [--summary]                  every day's per-row peak flow, step of the peak and mean flow as stream
                                                            products (trmc_stream_set_summary); checked against the host's reduction
                                                            of the one-by-one day's full result where that fits (nseg * 288 <= 2^26)
                               [--summary-depth]            ... and the peak depth with its step (carried by the tile kernels)
                               [--summary-total]            the totals over the days on the device, fetched once at the end; the
                                                            days' own summary arrays then stay on the device
                               [--exceedance K]             the threshold exceedance of every row's flow over ALL days of the stream at
                                                            K levels (trmc_stream_set_exceedance), fetched once at the end; checked
                                                            against the numpy loop over the one-by-one days' flows where that fits
                               [--depth-exceedance K]       the threshold exceedance of every row's DEPTH over ALL days of the stream at K
                                                            levels (trmc_stream_set_depth_exceedance): quantiles of the one-by-one days'
                                                            depths where they are known, else multiples of the bankfull depth; checked
                                                            against the numpy loop where that fits; the fold kernel's time from events
                               [--depth-bankfull]           ... at ONE level, the plan's bankfull depth: the steps a row is out of bank
                               [--courant LIMIT]            the stream is run twice, without and with every row's Courant number over the
                                                            whole stream (trmc_stream_set_courant): peak, its step, steps with cn > LIMIT;
                                                            checked against the fold of the one-by-one days' window_courant_summary;
                                                            the fold kernel's time from events
                               [--velocity K]               every row's peak velocity and its step over ALL days of the stream and the
                                                            exceedance of K (0..4; 0: the peak only) velocity levels
                                                            (trmc_stream_set_velocity): quantiles of the one-by-one days' velocities
                                                            where they are known, else 0.5, 1, 1.5, 2 m/s; the peak checked against the
                                                            fold of the one-by-one days' window_summary, the figures against the numpy
                                                            rule on the days' velocities where that fits; the fold kernel's time from events
                               [--stage]                    stage hydrographs: the depth of every step at the rows of the day's row set
                                                            (trmc_stream_set_stage); checked against column 2 of the one-by-one
                                                            day's full result where that fits (nseg * 288 <= 2^26)
                               [--outlets]                  the row set of the hydrographs (and of --stage) is the networks' outlets
                                                            instead of 3000 sampled rows"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from troute_amd import synthetic as S                     # noqa: E402
from troute_amd.plan import RoutingPlan                   # noqa: E402
from troute_amd import _lib                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nseg", type=int, default=S.CONUS_NSEG)
ap.add_argument("--days", type=int, default=8)
ap.add_argument("--wide-min-rows", type=int, default=0)
ap.add_argument("--wide-k", type=int, default=0)
ap.add_argument("--wide-levels", type=int, default=0)
ap.add_argument("--split", type=int, default=0)
ap.add_argument("--hint", action="store_true")
ap.add_argument("--stride", type=int, default=0)
ap.add_argument("--full", action="store_true")
ap.add_argument("--no-check", action="store_true")
ap.add_argument("--slots", type=int, default=0)
ap.add_argument("--velocity-on-demand", type=int, default=0)
ap.add_argument("--later", type=int, default=0, help="hand a day over this many days later than its last row allows (and hold as many more slots)")
ap.add_argument("--reservoirs", type=int, default=0, help="level-pool reservoirs scattered over the network (rows with an upstream row)")
ap.add_argument("--reservoir-da", type=int, default=0, help="so many of the --reservoirs are of types 2, 3, 4, 5 in turn, with synthetic tables")
ap.add_argument("--summary", action="store_true", help="per-row peak flow, step of the peak and mean flow of every day as stream products")
ap.add_argument("--summary-depth", action="store_true", help="the day's peak depth and its step as well (with or without --summary)")
ap.add_argument("--summary-total", action="store_true", help="the totals over the days of the stream; no per-day summary array crosses to the host")
ap.add_argument("--exceedance", type=int, default=0, metavar="K", help="exceedance of K (1..4) flow thresholds a row over the whole stream, kept on the device")
ap.add_argument("--depth-exceedance", type=int, default=0, metavar="K", help="exceedance of K (1..4) depth thresholds a row over the whole stream, kept on the device")
ap.add_argument("--depth-bankfull", action="store_true", help="the depth exceedance against the plan's bankfull depth (one level): out of bank")
ap.add_argument("--courant", type=float, default=None, metavar="LIMIT", help="every row's Courant number over the whole stream (peak, its step, steps with cn > LIMIT), kept on the device")
ap.add_argument("--velocity", type=int, default=-1, metavar="K", help="peak velocity and its step over the whole stream and the exceedance of K (0..4) velocity levels, kept on the device")
ap.add_argument("--stage", action="store_true", help="the depth of every step at the rows of the row set as a stream product")
ap.add_argument("--outlets", action="store_true", help="the row set: every network's outlet (default: 3000 sampled rows)")
ap.add_argument("--packed", type=int, default=0, metavar="V", help="the days arrive as packed CHRTOUT columns of V (1 or 2) int32 variables on a permuted feature axis and the device decodes and joins "
                                                                     "them; the host time to form the float forcing from the same columns is printed beside it")
ap.add_argument("--gages", type=int, default=0, help="nudged gages scattered over the network (observations: 70 %% valid, lognormal)")
a = ap.parse_args()
if a.reservoir_da > a.reservoirs:
    ap.error("--reservoir-da counts among the --reservoirs")
if a.summary_total and not (a.summary or a.summary_depth):
    ap.error("--summary-total totals --summary and / or --summary-depth")
if not 0 <= a.exceedance <= 4:
    ap.error("--exceedance: 1 to 4 levels (0: none)")
if not 0 <= a.depth_exceedance <= 4:
    ap.error("--depth-exceedance: 1 to 4 levels (0: none)")
if a.depth_bankfull and a.depth_exceedance > 1:
    ap.error("--depth-bankfull is one level")
if a.depth_bankfull:
    a.depth_exceedance = 1
if a.depth_exceedance and a.reservoir_da:
    ap.error("--depth-exceedance: not with --reservoir-da (the tile kernels of such a stream do not write the depth plane)")
if not -1 <= a.velocity <= 4:
    ap.error("--velocity: 0 to 4 levels (0: the peak and its step only)")
if a.velocity >= 0 and a.reservoir_da:
    ap.error("--velocity: not with --reservoir-da (the tile kernels of such a stream do not write the depth plane)")
_lib.single_hw_queue_per_priority("stream_probe")
nnet = S.CONUS_NNET if a.nseg == S.CONUS_NSEG else max(1, a.nseg // 185)
net = S.generate(a.nseg, nnet, cache_dir=os.environ.get("TRMC_SYNTH_CACHE", "/tmp"))
n = a.nseg
up_ptr, up_idx = S.upstream_csr(net["to"])
nsteps, qts = 288, 12
days = [net["qlat"]]
for d in range(1, min(a.days, 4)):
    days.append(S.forcing(n, previous=days[-1], seed=S.DEFAULT_SEED + 1 + d))
packed_days = None
if a.packed:
    # every day quantised to packed columns (scale 1e-5, one variable or the sum of two) on a feature axis that is a permutation of
    # the rows; the days routed are the floats the host rule forms from them -- timed, since that is what the device's decode replaces
    if a.packed not in (1, 2):
        ap.error("--packed: 1 or 2 variables")
    from troute_amd import nhd_io                         # noqa: E402
    scale, nan = float(np.float32(1e-5)), float("nan")
    feature_id = np.random.default_rng(29).permutation(np.arange(n, dtype=np.int64))     # (row r has the id r)
    col = np.argsort(feature_id, kind="stable")
    packed_days, host_ms = [], []
    for i, q in enumerate(days):
        raw = _lib.result_empty((q.shape[1], n), np.int32, always_pinned=True)
        raw[:, col] = np.minimum(np.rint(q.T.astype(np.float64) / scale), 2.0 ** 30).astype(np.int32)
        raw_b = None
        if a.packed == 2:
            raw_b = _lib.result_empty(raw.shape, np.int32, always_pinned=True)
            raw_b[...] = raw // 3
            raw -= raw_b
        pack = np.array([scale, 0.0, -999900000.0, nan, 0.0, 2000000000.0])
        packed_days.append({"feature_id": feature_id, "raw_a": raw, "raw_b": raw_b, "pack_a": pack, "pack_b": pack if raw_b is not None else None})
        t0 = time.perf_counter()
        host = nhd_io.unpack_packed(packed_days[-1])                     # the mask, scale and offset, the sum: float64 [nq, nfeat]
        days[i] = np.ascontiguousarray(host[:, col].T, dtype=np.float32) # the join on the feature id, row order, the cast
        host_ms.append((time.perf_counter() - t0) * 1e3)
    print(f"packed: {a.packed} variable(s) [{days[0].shape[1]}][{n}] int32 a day; forming the float forcing on the host (unpack_packed + the join + "
          f"the cast): median {np.median(host_ms):.1f} ms a day {np.round(host_ms, 1).tolist()}", flush=True)
pinned = []
for q in days:
    b = _lib.result_empty(q.shape, q.dtype, always_pinned=True)
    b[...] = q
    pinned.append(b)
q0 = np.zeros((n, 3), np.float32)
rng = np.random.default_rng(5)
sample = np.sort(rng.choice(n, min(n, 3000), replace=False))
if a.outlets:
    sample = np.flatnonzero(np.asarray(net["to"]) < 0)
# reservoirs and gages: synthetic level-pool parameters (oracle.LP_PAR order), every day's nudging tables resolved beforehand
lakes = gages = par = None
tabs = []
if a.reservoirs or a.gages:
    from troute_amd.routing.fast_reach import simple_da as DA          # noqa: E402
    has_up = np.flatnonzero(np.diff(up_ptr) > 0)
    lakes = np.sort(rng.choice(has_up, a.reservoirs, replace=False)) if a.reservoirs else np.zeros(0, np.int64)
    rest = np.setdiff1d(np.arange(n), lakes)
    gages = np.sort(rng.choice(rest, a.gages, replace=False)) if a.gages else np.zeros(0, np.int64)
    nl = lakes.shape[0]
    par = np.stack([rng.uniform(0.2, 5.0, nl), np.full(nl, 113.0), rng.uniform(0.5, 4.0, nl), np.full(nl, 0.1), np.full(nl, 100.0),
                    np.full(nl, 0.4), np.full(nl, 110.0), rng.uniform(10.0, 60.0, nl), np.full(nl, 10.0)], 1).astype(np.float32)
    q0[lakes, 2] = rng.uniform(104.0, 111.0, nl).astype(np.float32)     # the pools' elevations live in the depth slot
    if a.reservoir_da:
        # types 2, 3, 4, 5 in turn; the same observations every day (times from the day's start: 24 h back to 24 h on, every 15
        # minutes), a forecast series of 48 hourly values
        nda = a.reservoir_da
        da_kind = np.zeros(nl, np.int32)
        da_kind[np.sort(rng.choice(nl, nda, replace=False))] = 2 + np.arange(nda) % 4
        da_trow = np.zeros(nl, np.int32)
        da_n = [int(np.count_nonzero(da_kind == 2)), int(np.count_nonzero(da_kind == 3)), int(np.count_nonzero(da_kind >= 4))]
        for sel in (da_kind == 2, da_kind == 3, da_kind >= 4):
            da_trow[sel] = np.arange(np.count_nonzero(sel))
        da_time = (np.arange(193, dtype=np.float32) - 96) * np.float32(900.0)
        da_obs = []
        for k in range(2):
            o = rng.lognormal(np.log(2.0), 1.0, (da_n[k], 193)).astype(np.float32)
            o[rng.random(o.shape) < 0.2] = np.nan
            da_obs.append(o)
        da_series = rng.lognormal(np.log(2.0), 1.0, (da_n[2], 48)).astype(np.float32)
        da_t_end = np.float32(np.float32(nsteps) * np.float32(300.0))

        def da_tables(state=None, tsidx=None):
            """(usgs, usace, rfc) as set_reservoir_da takes them; state / tsidx [nres]: what the day before left (None: the start)"""
            out = []
            for k in range(2):
                st = np.tile(np.array([0.0, 1.0, 0.0, 0.0], np.float32), (da_n[k], 1))
                if state is not None:
                    st[da_trow[da_kind == 2 + k]] = state[da_kind == 2 + k]
                out.append((da_obs[k], da_time, st) if da_n[k] else None)
            ut = np.zeros(da_n[2], np.float32)
            ipar = np.tile(np.array([0, 47, 1, 3600, 10], np.int32), (da_n[2], 1))
            if state is not None:
                ut[da_trow[da_kind >= 4]] = state[da_kind >= 4, 0]
                ipar[da_trow[da_kind >= 4], 0] = tsidx[da_kind >= 4]
            out.append((da_series, ut, ipar) if da_n[2] else None)
            return out
    t0 = time.perf_counter()
    for d in range(len(days) if a.gages else 0):
        usgs = rng.lognormal(np.log(0.5), 1.0, (a.gages, nsteps + 1)).astype(np.float32)
        usgs[rng.random(usgs.shape) < 0.3] = np.nan
        nan = np.full(a.gages, np.nan, np.float32)
        mode, ta, tw, _, _ = DA.resolve_tables(nsteps, 300.0, 120.0, usgs, nan, nan)
        tabs.append(tuple(_lib.result_empty(x.shape, x.dtype, always_pinned=True) for x in (mode, ta, tw)))
        for dst, src in zip(tabs[-1], (mode, ta, tw)):
            dst[...] = src
    if a.gages:
        print(f"nudging tables of {a.gages} gages resolved on the host: {(time.perf_counter() - t0) / len(days):.2f} s per day", flush=True)


def summary_of(q):
    """(peak_flow, peak_step, mean_flow) of flows q [rows, nsteps] as include/trmc.h defines them"""
    peak, step = peak_of(q)
    return peak, step, np.cumsum(q, axis=1, dtype=q.dtype)[:, -1] / q.dtype.type(q.shape[1])


def peak_of(q):
    peak, step = q[:, 0].copy(), np.ones(q.shape[0], np.int32)
    for t in range(1, q.shape[1]):
        m = q[:, t] > peak
        peak[m] = q[m, t]
        step[m] = t + 1
    return peak, step


def exceedance_of(x, th):
    """steps over, first step, last step, longest run [rows, K] (int64) of x [rows, steps] against th [rows, K]: include/trmc.h"""
    count, first, last, longest, run = (np.zeros(th.shape, np.int64) for _ in range(5))
    with np.errstate(invalid="ignore"):
        for t in range(1, x.shape[1] + 1):
            over = x[:, t - 1][:, None] > th
            count = count + over
            first = np.where(over & (first == 0), t, first)
            last = np.where(over, t, last)
            run = np.where(over, run + 1, 0)
            longest = np.maximum(longest, run)
    return {"steps_over": count, "first_step": first, "last_step": last, "longest_run": longest}


any_summary = a.summary or a.summary_depth
check_exc = a.exceedance and not a.no_check and n * nsteps * a.days <= 1 << 26
ref_q = []
check_dex = a.depth_exceedance and not a.no_check and n * nsteps * a.days <= 1 << 26
ref_d = []
daily = any_summary and not a.summary_total
check_summary = any_summary and not a.no_check and n * nsteps <= 1 << 26
ref_sum = []
check_stage = a.stage and not a.no_check and n * nsteps <= 1 << 26
ref_stage = []
check_cou = a.courant is not None and not a.no_check and not a.reservoir_da     # (the same days' window summaries, folded over the days)
ref_cou = []
check_vel = a.velocity >= 0 and not a.no_check                                     # (the peak: the same days' window summaries, folded)
check_velx = check_vel and a.velocity > 0 and n * nsteps * a.days <= 1 << 26         # (the figures: the numpy rule on the days' velocities)
ref_vel, ref_v = [], []
opts = {"wide_min_rows": a.wide_min_rows, "wide_k": a.wide_k, "cluster_rows": 128, "wide_levels": a.wide_levels, "stream_split": a.split, "velocity_on_demand": a.velocity_on_demand}
hint = None
if a.hint:
    with RoutingPlan(up_ptr, up_idx, net["params"], assume_short_ts=True, engine="levels", options=opts) as p:
        p.upload_forcing(nsteps, days[0], q0)
        p.route_device(nsteps, qts, True)
        p.upload_forcing(nsteps, days[1 % len(days)], None)
        p.collect_cost(True)
        p.route_device(nsteps, qts, True)
        cost, ns = p.download_cost()
        hint = np.minimum(255, (cost.astype(np.float64) * 16 / ns).round()).astype(np.uint8)
with RoutingPlan(up_ptr, up_idx, net["params"], assume_short_ts=True, engine="levels", cost_hint=hint, options=opts) as p:
    rs = p.rowset(sample)
    ref = []
    if lakes is not None:
        if lakes.size:
            p.set_reservoirs(lakes, par, 300.0)
        if gages.size:
            p.stream_set_gages(gages)
    da_state = da_tsidx = None
    if not a.no_check:
        t0 = time.perf_counter()
        for d in range(a.days):
            if a.reservoir_da:              # (the state through the host, the times less the day's length: mc_reach.pyx:820-837)
                p.set_reservoir_da(da_kind, da_trow, *da_tables(da_state, da_tsidx))
            # (set_reservoir_da stages a new window: the state the last one left goes in again explicitly)
            p.upload_forcing(nsteps, days[d % len(days)], q0 if d == 0 else (ref[-1][0] if a.reservoir_da else None))
            if tabs:
                p.set_nudging(nsteps, gages, *tabs[d % len(days)])
            st = p.route_device(nsteps, qts, True)
            fin = p.download_final_state()
            hyd = p.gather_flow_rows(sample)
            fvd = p.download_fvd(a.stride or 1) if (a.stride or a.full) else None
            if check_summary:
                full = fvd if (a.full and not a.stride) else p.download_fvd()
                ref_sum.append(summary_of(np.ascontiguousarray(full[:, :, 0])) + peak_of(np.ascontiguousarray(full[:, :, 2])))
            if check_stage:
                ref_stage.append(np.ascontiguousarray((fvd if (a.full and not a.stride) else p.download_fvd())[sample, :, 2]))
            if check_exc:
                ref_q.append(np.ascontiguousarray((full if check_summary else p.download_fvd())[:, :, 0]))
            if check_dex:
                ref_d.append(np.ascontiguousarray((fvd if (a.full and not a.stride) else p.download_fvd())[:, :, 2]))
            if check_cou:
                ref_cou.append(p.window_courant_summary(a.courant))
            if check_vel:
                ref_vel.append(p.window_summary(("peak_velocity",)))
            if check_velx:
                ref_v.append(np.ascontiguousarray((fvd if (a.full and not a.stride) else p.download_fvd())[:, :, 1]))
            if a.reservoir_da:
                da_state, da_tsidx = p.download_reservoir_da()
                da_state[da_kind != 0, 0] -= da_t_end
                da_state[(da_kind == 2) | (da_kind == 3), 3] -= da_t_end
            ref.append((fin, hyd, fvd, p.download_reservoir_inflow() if a.reservoirs else None, p.download_nudge() if tabs else None,
                        (da_state.copy(), da_tsidx.copy()) if a.reservoir_da else None))
        print(f"one by one: {(time.perf_counter() - t0) / a.days * 1e3:.2f} ms per day (host loop, downloads included); window ms_main {st['ms_main']:.2f}", flush=True)
    # the stream -- with --courant LIMIT twice: without the Courant number, then with it (the same days, every check both times)
    for cou_on in ((False, True) if a.courant is not None else (False,)):
        if a.courant is not None:
            print("-- the stream " + ("WITH" if cou_on else "WITHOUT") + " the Courant number", flush=True)
        if a.reservoir_da:
            p.set_reservoir_da(da_kind, da_trow, *da_tables())
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_set_summary((("peak", "mean") if a.summary else ()) + (("peak_depth",) if a.summary_depth else ())
                             + (("total",) if a.summary_total else ()) or None)
        if a.stage:
            p.stream_set_stage(True)
        if a.packed:
            p.stream_set_packed_forcing(packed_days[0], np.arange(n, dtype=np.int64))
        if a.courant is not None:
            p.stream_set_courant(a.courant if cou_on else None)
        if a.exceedance:
            # a row's levels: quantiles of its own flows over the stream where they are known (the check), else multiples of its forcing
            if check_exc:
                exc_x = np.concatenate(ref_q, axis=1)
                exc_th = np.quantile(exc_x.astype(np.float64), (0.5, 0.25, 0.9, 0.75)[:a.exceedance], axis=1).T.astype(np.float32)
            else:
                exc_th = days[0].mean(axis=1, dtype=np.float32)[:, None] * np.array([1, 10, 100, 1000], np.float32)[None, :a.exceedance]
            p.set_thresholds(exc_th)
            p.stream_set_exceedance("flow")
        if a.depth_exceedance:
            # a row's levels: its bankfull depth; or quantiles of its own depths over the stream where they are known (the check),
            # else multiples of its bankfull depth
            if check_dex:
                dex_x = np.concatenate(ref_d, axis=1)
            if a.depth_bankfull:
                dex_th = p.bankfull_depth()[:, None]
            elif check_dex:
                dex_th = np.quantile(dex_x.astype(np.float64), (0.5, 0.25, 0.9, 0.75)[:a.depth_exceedance], axis=1).T.astype(np.float32)
            else:
                dex_th = p.bankfull_depth()[:, None] * np.array([1, 0.5, 0.25, 0.125], np.float32)[None, :a.depth_exceedance]
            p.stream_set_depth_exceedance(dex_th)
        if a.velocity >= 0:
            # a row's levels: quantiles of its own velocities over the stream where they are known (the check), else fixed speeds
            vel_th = None
            if check_velx:
                vel_x = np.concatenate(ref_v, axis=1)
                vel_th = np.quantile(vel_x.astype(np.float64), (0.5, 0.25, 0.9, 0.75)[:a.velocity], axis=1).T.astype(np.float32)
            elif a.velocity > 0:
                vel_th = np.tile(np.array([0.5, 1.0, 1.5, 2.0], np.float32)[None, :a.velocity], (n, 1))
            p.stream_set_velocity(True if vel_th is None else vel_th)
        p.stream_begin(nsteps, qts, reservoir_da=bool(a.reservoir_da) or None, slots=a.slots + a.later if a.slots else (a.later and 2 + -(-(int(p.lags()[0].max(initial=0)) + 1) // (nsteps // p.tile_steps)) + a.later), full_output=a.full and not a.stride, output_stride=a.stride)
        info = p.stream_info()
        print("stream:", info, flush=True)
        D = info["slots"]
        hyds = [_lib.result_empty((sample.shape[0], nsteps), np.float32, always_pinned=True) for _ in range(D)]
        fins = [_lib.result_empty((n, 3), np.float32, always_pinned=True) for _ in range(D)]
        keep = nsteps // a.stride if a.stride else nsteps
        fvds = [_lib.result_empty((n, keep, 3), np.float32, always_pinned=True) for _ in range(D)] if (a.stride or a.full) else [None] * D
        rins = [_lib.result_empty((a.reservoirs, nsteps), np.float32, always_pinned=True) if a.reservoirs else None for _ in range(D)]
        nuds = [_lib.result_empty((a.gages, nsteps), np.float32, always_pinned=True) if tabs else None for _ in range(D)]
        rdas = [(_lib.result_empty((a.reservoirs, 4), np.float32, always_pinned=True), _lib.result_empty((a.reservoirs,), np.int32, always_pinned=True))
                if a.reservoir_da else None for _ in range(D)]
        sums = [(_lib.result_empty((n,), np.float32, always_pinned=True), _lib.result_empty((n,), np.int32, always_pinned=True),
                 _lib.result_empty((n,), np.float32, always_pinned=True)) if (a.summary and daily) else ((None, None, None) if daily else None)
                for _ in range(D)]
        if daily and a.summary_depth:
            sums = [s + (_lib.result_empty((n,), np.float32, always_pinned=True), _lib.result_empty((n,), np.int32, always_pinned=True)) for s in sums]
        stgs = [_lib.result_empty((sample.shape[0], nsteps), np.float32, always_pinned=True) if a.stage else None for _ in range(D)]
        da_day = da_tables() if a.reservoir_da else None
        got = []
        behind = (info["lag_max"] + info["tiles_per_day"]) // info["tiles_per_day"] + a.later
        ok = True
        marks = []

        def take(e):
            global ok
            p.stream_wait(e)
            marks.append(time.perf_counter())
            if a.no_check:
                return
            fin, hyd, fvd, rin, nud, rda = ref[e]
            if rda is not None and not (np.array_equal(rda[0].view(np.uint32), rdas[e % D][0].view(np.uint32)) and np.array_equal(rda[1], rdas[e % D][1])):
                ok = False
                print(f"   day {e}: reservoir data-assimilation state differs", flush=True)
            for name, x, y in (("reservoir inflow", rin, rins[e % D]), ("nudge", nud, nuds[e % D])):
                if x is not None and not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                    ok = False
                    print(f"   day {e}: {name} differs", flush=True)
            if check_summary and daily and not all(y is None or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ref_sum[e], sums[e % D])):
                ok = False
                print(f"   day {e}: summary differs", flush=True)
            if check_stage and not np.array_equal(ref_stage[e].view(np.uint32), stgs[e % D].view(np.uint32)):
                ok = False
                print(f"   day {e}: stage differs", flush=True)
            s1 = np.array_equal(fin.view(np.uint32), fins[e % D].view(np.uint32))
            s2 = np.array_equal(hyd.view(np.uint32), hyds[e % D].view(np.uint32))
            s3 = fvd is None or np.array_equal(np.ascontiguousarray(fvd).view(np.uint32), fvds[e % D].view(np.uint32))
            if not (s1 and s2 and s3):
                ok = False
                print(f"   day {e}: final state {s1} hydrographs {s2} fvd {s3}", flush=True)
        t0 = time.perf_counter()
        for d in range(a.days):
            p.stream_push(None if a.packed else pinned[d % len(days)], packed=packed_days[d % len(days)] if a.packed else None, rowset=rs, hyd=hyds[d % D], q0=fins[d % D], fvd=fvds[d % D],
                          nudging=tabs[d % len(days)] if tabs else None, nudge=nuds[d % D], reservoir_inflow=rins[d % D], reservoir_da=da_day, reservoir_da_state=rdas[d % D], summary=sums[d % D], **({"stage": stgs[d % D]} if a.stage else {}))
            e = d - behind
            if e >= 0:
                take(e)
        p.stream_flush()
        for e in range(max(0, a.days - behind), a.days):
            take(e)
        el = time.perf_counter() - t0
        if a.summary_total:
            tot = p.stream_summary_total()
            print(f"   totals over {tot['days']} days fetched in {(time.perf_counter() - t0 - el) * 1e3:.2f} ms: {sorted(k for k in tot if k != 'days')}", flush=True)
            if check_summary:
                for kf, ks, i in (("peak_flow", "peak_step", 0), ("peak_depth", "peak_depth_step", 3)):
                    if kf in tot:
                        pk, st = ref_sum[0][i].copy(), ref_sum[0][i + 1].astype(np.int64)
                        for e in range(1, a.days):
                            m = ref_sum[e][i] > pk
                            pk[m], st[m] = ref_sum[e][i][m], e * nsteps + ref_sum[e][i + 1][m]
                        if not (np.array_equal(pk.view(np.uint32), tot[kf].view(np.uint32)) and np.array_equal(st, tot[ks])):
                            ok = False
                            print(f"   totals: {kf} differs", flush=True)
                if "mean_flow" in tot:
                    m = ref_sum[0][2].copy()
                    for e in range(1, a.days):
                        m = m + ref_sum[e][2]
                    if not np.array_equal((m / np.float32(a.days)).view(np.uint32), tot["mean_flow"].view(np.uint32)):
                        ok = False
                        print("   totals: mean_flow differs", flush=True)
        if a.exceedance:
            t1 = time.perf_counter()
            exc = p.stream_exceedance()
            print(f"   exceedance at {a.exceedance} level(s) over {exc['days']} days fetched in {(time.perf_counter() - t1) * 1e3:.2f} ms: "
                  f"{int(np.count_nonzero(exc['steps_over']))} of {exc['steps_over'].size} (row, level) pairs went over, longest run {int(exc['longest_run'].max())} steps;",
                  "not checked (no check asked for, or too large for a host loop)" if not check_exc else "", flush=True)
            if check_exc:
                want = exceedance_of(exc_x, exc_th)
                same = exc["days"] == a.days and all(np.array_equal(exc[k], want[k]) for k in want)
                ok = ok and same
                print("   exceedance equals the numpy loop over the one-by-one days' flows:", same, flush=True)
        if a.depth_exceedance:
            fold_ms = p.stream_depth_exceedance_kernel_ms()
            print(f"   the last day's depth fold (k_stream_exceed_depth, from the {'full result' if a.full and not a.stride else 'depth plane'}), "
                  f"from events around the kernel: {fold_ms:.3f} ms", flush=True)
            t1 = time.perf_counter()
            dex = p.stream_depth_exceedance()
            print(f"   depth exceedance at {a.depth_exceedance} level(s){' (bankfull)' if a.depth_bankfull else ''} over {dex['days']} days fetched in "
                  f"{(time.perf_counter() - t1) * 1e3:.2f} ms: {int(np.count_nonzero(dex['steps_over']))} of {dex['steps_over'].size} (row, level) pairs went "
                  f"over, longest run {int(dex['longest_run'].max())} steps;",
                  "not checked (no check asked for, or too large for a host loop)" if not check_dex else "", flush=True)
            if check_dex:
                want = exceedance_of(dex_x, np.ascontiguousarray(dex_th))
                same = dex["days"] == a.days and all(np.array_equal(dex[k], want[k]) for k in want)
                ok = ok and same
                print("   depth exceedance equals the numpy loop over the one-by-one days' depths:", same, flush=True)
        if cou_on:
            fold_ms = p.stream_courant_kernel_ms()
            print(f"   the last day's fold (k_stream_courant), from events around the kernel: {fold_ms:.3f} ms", flush=True)
            t1 = time.perf_counter()
            cou = p.stream_courant()
            print(f"   Courant number over {cou['days']} days fetched in {(time.perf_counter() - t1) * 1e3:.2f} ms: highest cn {float(np.nanmax(cou['peak_cn'])):.3f}, "
                  f"{int(np.count_nonzero(cou['steps_over']))} of {n} rows went over {a.courant};", "" if check_cou else "not checked", flush=True)
            if check_cou:
                pk, st, ov = ref_cou[0]["peak_cn"].copy(), ref_cou[0]["peak_cn_step"].astype(np.int64), ref_cou[0]["steps_over"].astype(np.int64)
                for e in range(1, a.days):          # (the fold of the days' window summaries: a later day wins only with a greater peak)
                    m = ref_cou[e]["peak_cn"] > pk
                    pk[m], st[m] = ref_cou[e]["peak_cn"][m], e * nsteps + ref_cou[e]["peak_cn_step"][m]
                    ov += ref_cou[e]["steps_over"]
                same = (cou["days"] == a.days and np.array_equal(pk.view(np.uint32), cou["peak_cn"].view(np.uint32)) and np.array_equal(st, cou["peak_cn_step"])
                        and np.array_equal(ov, cou["steps_over"]))
                ok = ok and same
                print("   Courant number equals the fold of the one-by-one days' window_courant_summary:", same, flush=True)
        if a.velocity >= 0:
            fold_ms = p.stream_velocity_kernel_ms()
            gb = ((2 * nsteps + nsteps // qts) * n * 4 + up_idx.shape[0] * nsteps * 4) / 1e9   # flow, depth, forcing, every upstream flow: read once
            print(f"   the last day's velocity fold (k_stream_velocity, depths from the {'full result' if a.full and not a.stride else 'depth plane'}), from "
                  f"events around the kernel: {fold_ms:.3f} ms; its bytes ({gb:.3f} GB) take {gb / 8e3 * 1e3:.3f} ms at 8 TB/s", flush=True)
            t1 = time.perf_counter()
            vel = p.stream_velocity()
            print(f"   velocity at {a.velocity} level(s) over {vel['days']} days fetched in {(time.perf_counter() - t1) * 1e3:.2f} ms: highest "
                  f"{float(np.nanmax(vel['peak_velocity'])):.3f} m/s"
                  + (f", {int(np.count_nonzero(vel['steps_over']))} of {vel['steps_over'].size} (row, level) pairs went over" if a.velocity else "") + ";",
                  "" if check_vel else "not checked", flush=True)
            if check_vel:
                pk, st = ref_vel[0]["peak_velocity"].copy(), ref_vel[0]["peak_velocity_step"].astype(np.int64)
                for e in range(1, a.days):          # (the fold of the days' window summaries: a later day wins only with a greater peak)
                    m = ref_vel[e]["peak_velocity"] > pk
                    pk[m], st[m] = ref_vel[e]["peak_velocity"][m], e * nsteps + ref_vel[e]["peak_velocity_step"][m]
                same = vel["days"] == a.days and np.array_equal(pk.view(np.uint32), vel["peak_velocity"].view(np.uint32)) and np.array_equal(st, vel["peak_velocity_step"])
                ok = ok and same
                print("   peak velocity equals the fold of the one-by-one days' window_summary:", same, flush=True)
            if check_velx:
                want = exceedance_of(vel_x, np.ascontiguousarray(vel_th))
                same = all(np.array_equal(vel[k], want[k]) for k in want)
                ok = ok and same
                print("   velocity exceedance equals the numpy rule over the one-by-one days' velocities:", same, flush=True)
        if a.packed:
            nq = days[0].shape[1]
            gb = (a.packed * nq * n * 4 + n * 4 + nq * n * 4) / 1e9     # the raw values once, feat_of_pos, the forcing stored
            print(f"   the last day's decode (k_ingest_packed_day), from events around the kernel: {p.stream_packed_forcing_kernel_ms():.3f} ms; its bytes "
                  f"({gb:.3f} GB: {a.packed} x [{nq}][{n}] int32 read once, the join, [{nq}][{n}] fp32 stored) take {gb / 8e3 * 1e3:.3f} ms at 8 TB/s", flush=True)
        dev_ms = [p.stream_day_ms(e) for e in range(max(behind + 1, a.days - D + 1), a.days)]    # (days pushed into a full stream, still in the ring)
        p.stream_end()
        if dev_ms:
            print(f"   device time of a day's own launches on the slices' stream: median {np.median(dev_ms):.2f} ms over {len(dev_ms)} days {np.round(dev_ms, 2).tolist()}", flush=True)
        per = np.diff(marks) * 1e3
        print(f"stream: {el / a.days * 1e3:.2f} ms per day over {a.days} days (fill and drain included); between deliveries {np.round(per, 2).tolist()}", flush=True)
        if any_summary:
            print("   summary (" + ", ".join((["peak flow, step of the peak, mean flow"] if a.summary else []) + (["peak depth and its step"] if a.summary_depth else []))
                  + " of every row" + ("; totals only" if a.summary_total else "") + "):",
                  "checked against the host's reduction of every day's full result" if check_summary else "not checked (no check asked for, or too large for a host reduction)", flush=True)
        if a.stage:
            print(f"   stage of every step at the {sample.shape[0]} rows of the row set:",
                  "checked against column 2 of every day's full result" if check_stage else "not checked (no check asked for, or too large)", flush=True)
        print("   launches", p.stream_info()["launches"], " every day bit-identical to the days routed one by one:", ok if not a.no_check else "not checked", flush=True)
