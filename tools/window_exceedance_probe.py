"""What a window's threshold exceedance costs on the device (RoutingPlan.window_exceedance, trmc_window_exceedance) beside the
per-row summary of the same window (RoutingPlan.window_summary), which reads the same bytes with the same tiling and is the
yardstick: one plan at synthetic CONUS size, one window, then ROUNDS interleaved rounds of (s) window_summary, (x1) window_exceedance
of the flow with one level, (x4) with four levels -- each kernel alone, from the events around it.  Medians, the spread, and every
kernel's time against its bytes at 8 TB/s.
  python tools/window_exceedance_probe.py [--nseg N] [--rounds 5] [--engine auto|levels|flow] [--short] [--check]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from troute_amd import synthetic as S                     # noqa: E402
from troute_amd.plan import RoutingPlan                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nseg", type=int, default=S.CONUS_NSEG)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--engine", default="auto")
ap.add_argument("--short", action="store_true", help="assume_short_ts (default: the general mode)")
ap.add_argument("--check", action="store_true", help="compare steps_over / first_step / last_step with numpy over the full block (small --nseg only)")
a = ap.parse_args()
nnet = S.CONUS_NNET if a.nseg == S.CONUS_NSEG else max(1, a.nseg // 185)
net = S.generate(a.nseg, nnet, cache_dir=os.environ.get("TRMC_SYNTH_CACHE", "/tmp"))
n = a.nseg
up_ptr, up_idx = S.upstream_csr(net["to"])
nsteps, qts = 288, 12
qlat = np.ascontiguousarray(net["qlat"][:, :nsteps // qts])
q0 = np.zeros((n, 3), np.float32)
short = bool(a.short)

with RoutingPlan(up_ptr, up_idx, net["params"], assume_short_ts=short, engine=a.engine) as p:
    print(f"engine {p.engine}, {n} rows x {nsteps} steps, assume_short_ts={short}", flush=True)
    p.upload_forcing(nsteps, qlat, q0)
    p.route_device(nsteps, qts, short)
    peak = p.window_summary(("peak",))["peak_flow"]
    # levels a forecaster might set: fractions of the window's own peak, so every level is crossed by part of the rows
    th4 = np.ascontiguousarray(peak[:, None] * np.array([0.25, 0.5, 0.75, 0.9], np.float32)[None, :])
    th1 = np.ascontiguousarray(th4[:, 1])
    if a.check:
        q = np.ascontiguousarray(p.download_fvd()[:, :, 0])
        p.set_thresholds(th4)
        got = p.window_exceedance("flow")
        over = q[:, :, None] > th4[:, None, :]
        t = np.arange(1, nsteps + 1, dtype=np.int32)[None, :, None]
        ok = (np.array_equal(got["steps_over"], over.sum(1)) and np.array_equal(got["first_step"], np.where(over, t, nsteps + 1).min(1) % (nsteps + 1))
              and np.array_equal(got["last_step"], np.where(over, t, 0).max(1)))
        print("steps_over, first_step, last_step == numpy over the full block:", ok, flush=True)
    for th in (th1, th4):                                  # (warm-up: scratch, events, the pinned pool of the results)
        p.set_thresholds(th)
        p.window_exceedance("flow")
    Sm, X1, X4 = [], [], []
    for _ in range(a.rounds):
        p.window_summary()
        Sm.append(p.window_summary_kernel_ms())
        p.set_thresholds(th1)
        p.window_exceedance("flow")
        X1.append(p.window_exceedance_kernel_ms())
        p.set_thresholds(th4)
        p.window_exceedance("flow")
        X4.append(p.window_exceedance_kernel_ms())
    nbytes = n * nsteps * 3 * 4
    floor = nbytes / 8e12 * 1e3
    for name, v in (("(s)  k_window_summary, all seven parts", Sm), ("(x1) k_window_exceed, flow, K = 1     ", X1), ("(x4) k_window_exceed, flow, K = 4     ", X4)):
        m = float(np.median(v))
        print(f"{name} ms: {' '.join(f'{x:.3f}' for x in v)}   median {m:.3f}  min {min(v):.3f}  max {max(v):.3f}   "
              f"{nbytes / m / 1e9:.2f} TB/s, {m / floor:.2f} x the floor of {floor:.3f} ms at 8 TB/s")
    ms = float(np.median(Sm))
    print(f"against the summary kernel: K = 1 {np.median(X1) / ms:.3f} x, K = 4 {np.median(X4) / ms:.3f} x; the summary's own spread "
          f"{(max(Sm) - min(Sm)) / ms:.3f} of its median")
