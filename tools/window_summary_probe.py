"""What a window's per-row summary costs (RoutingPlan.window_summary, trmc_window_summary) against the only other way a single
window hands back per-reach information, the hourly block (download_fvd(12)): one plan at synthetic CONUS size in the general mode
(no assume_short_ts), ROUNDS rounds of (a) the window alone, (b) the window + window_summary() of all seven parts, (c) the window +
download_fvd(12), in turn; (d) the reduction kernel alone, from the events around it.  Medians, the (b) / (c) ratio of what each
adds to the window, and the kernel's time against its bytes at 8 TB/s.
  python tools/window_summary_probe.py [--nseg N] [--rounds 5] [--engine auto|levels|flow] [--short] [--check]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from troute_amd import synthetic as S                     # noqa: E402
from troute_amd.plan import RoutingPlan                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nseg", type=int, default=S.CONUS_NSEG)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--engine", default="auto")
ap.add_argument("--short", action="store_true", help="assume_short_ts (default: the general mode)")
ap.add_argument("--check", action="store_true", help="compare the summary with numpy over the full block (small --nseg only)")
a = ap.parse_args()
nnet = S.CONUS_NNET if a.nseg == S.CONUS_NSEG else max(1, a.nseg // 185)
net = S.generate(a.nseg, nnet, cache_dir=os.environ.get("TRMC_SYNTH_CACHE", "/tmp"))
n = a.nseg
up_ptr, up_idx = S.upstream_csr(net["to"])
nsteps, qts, stride = 288, 12, 12
qlat = np.ascontiguousarray(net["qlat"][:, :nsteps // qts])
q0 = np.zeros((n, 3), np.float32)
short = bool(a.short)


def window(p):
    p.upload_forcing(nsteps, qlat, q0)
    return p.route_device(nsteps, qts, short)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


with RoutingPlan(up_ptr, up_idx, net["params"], assume_short_ts=short, engine=a.engine) as p:
    print(f"engine {p.engine}, {n} rows x {nsteps} steps, assume_short_ts={short}", flush=True)
    window(p)                                             # (warm-up: buffers, the pinned pool of the downloads)
    p.window_summary()
    p.download_fvd(stride)
    if a.check:
        fvd = p.download_fvd()
        got = p.window_summary()
        q = np.ascontiguousarray(fvd[:, :, 0])
        ok = np.array_equal(got["mean_flow"].view(np.uint32), (np.cumsum(q, axis=1, dtype=np.float32)[:, -1] / np.float32(nsteps)).view(np.uint32))
        for name, c in (("peak_flow", 0), ("peak_velocity", 1), ("peak_depth", 2)):
            x = fvd[:, :, c]
            at = np.argmax(x, axis=1)                     # (the first of equal values)
            step = name.replace("_flow", "") + "_step"
            ok = ok and np.array_equal(got[name].view(np.uint32), x[np.arange(n), at].view(np.uint32)) and np.array_equal(got[step], at + 1)
        print("summary == numpy over the full block:", ok, flush=True)
    A, B, Cc, K, Bs, Cs = [], [], [], [], [], []
    for _ in range(a.rounds):
        A.append(timed(lambda: window(p)))
        t = timed(lambda: window(p))
        s = timed(p.window_summary)
        B.append(t + s)
        Bs.append(s)
        K.append(p.window_summary_kernel_ms())
        t = timed(lambda: window(p))
        s = timed(lambda: p.download_fvd(stride))
        Cc.append(t + s)
        Cs.append(s)
    med = lambda v: float(np.median(v))                    # noqa: E731
    fmt = lambda v: " ".join(f"{x:.2f}" for x in v)        # noqa: E731
    print(f"(a) window alone (upload + route, host wall)      ms: {fmt(A)}   median {med(A):.2f}")
    print(f"(b) window + window_summary(all seven parts)      ms: {fmt(B)}   median {med(B):.2f}   (the call alone: median {med(Bs):.2f})")
    print(f"(c) window + download_fvd({stride})                     ms: {fmt(Cc)}   median {med(Cc):.2f}   (the call alone: median {med(Cs):.2f})")
    print(f"(d) k_window_summary alone (events)               ms: {fmt(K)}   median {med(K):.3f}")
    nbytes = n * nsteps * 3 * 4
    floor = nbytes / 8e12 * 1e3
    print(f"(b) / (c) = {med(B) / med(Cc):.3f}; what each adds to the window: summary {med(Bs):.2f} ms, hourly block {med(Cs):.2f} ms "
          f"(ratio {med(Bs) / med(Cs):.3f})")
    print(f"kernel: {nbytes / 1e9:.2f} GB read in {med(K):.3f} ms = {nbytes / med(K) / 1e9:.2f} TB/s, {med(K) / floor:.2f} x the floor of "
          f"{floor:.3f} ms at 8 TB/s")
