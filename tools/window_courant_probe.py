"""What a window's Courant metrics cost (RoutingPlan.window_courant / window_courant_summary, trmc_window_courant) against the
window they are recomputed from: one plan at synthetic CONUS size in the general mode (no assume_short_ts), ROUNDS rounds of the
window (its device time, trmc_stats ms_total), the summary kernel, the block's kernel at stride 1 and at stride 12, in turn -- the
kernels' times from the events around them.  The pass does a window's arithmetic once with no dependent chain: a kernel that takes
longer than the window's own device time has the wrong layout.
  python tools/window_courant_probe.py [--nseg N] [--rounds 5] [--engine auto|levels|flow] [--short] [--no-block]"""
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
ap.add_argument("--no-block", action="store_true", help="skip the stride-1 block (9.4 GB to the host at CONUS size)")
a = ap.parse_args()
nnet = S.CONUS_NNET if a.nseg == S.CONUS_NSEG else max(1, a.nseg // 185)
net = S.generate(a.nseg, nnet, cache_dir=os.environ.get("TRMC_SYNTH_CACHE", "/tmp"))
n = a.nseg
up_ptr, up_idx = S.upstream_csr(net["to"])
nsteps, qts, stride = 288, 12, 12
qlat = np.ascontiguousarray(net["qlat"][:, :nsteps // qts])
q0 = np.zeros((n, 3), np.float32)
short = bool(a.short)

with RoutingPlan(up_ptr, up_idx, net["params"], assume_short_ts=short, engine=a.engine) as p:
    print(f"engine {p.engine}, {n} rows x {nsteps} steps, assume_short_ts={short}", flush=True)
    W, Ks, K1, K12 = [], [], [], []
    for r in range(a.rounds + 1):                         # (round 0: warm-up -- buffers, the pinned pool of the downloads)
        p.upload_forcing(nsteps, qlat, q0)
        p.route_device(nsteps, qts, short)
        w = p.stats()["ms_total"]
        s = p.window_courant_summary(1.0)
        ks = p.window_courant_kernel_ms()
        p.window_courant(stride)
        k12 = p.window_courant_kernel_ms()
        k1 = float("nan")
        if not a.no_block:
            p.window_courant(1)
            k1 = p.window_courant_kernel_ms()
        if r:
            W.append(w), Ks.append(ks), K12.append(k12), K1.append(k1)
    med = lambda v: float(np.median(v))                    # noqa: E731
    fmt = lambda v: " ".join(f"{x:.2f}" for x in v)        # noqa: E731
    print(f"window, device time (trmc_stats ms_total)        ms: {fmt(W)}   median {med(W):.2f}")
    print(f"k_window_courant, summary                        ms: {fmt(Ks)}   median {med(Ks):.2f}   ({med(Ks) / med(W):.2f} x the window)")
    print(f"k_window_courant, block at stride 1              ms: {fmt(K1)}   median {med(K1):.2f}   ({med(K1) / med(W):.2f} x the window)")
    print(f"k_window_courant, block at stride {stride:<2d}             ms: {fmt(K12)}   median {med(K12):.2f}   ({med(K12) / med(W):.2f} x the window)")
    over = s["steps_over"]
    print(f"rows with cn > 1 at some step: {int((over > 0).sum())} of {n}; highest cn {float(np.nanmax(s['peak_cn'])):.3g}")
