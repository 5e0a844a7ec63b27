"""TRMC_ARITH_TOLERANCE (include/trmc.h, trmc_plan_options.arithmetic): the Muskingum-Cunge step on the hardware's
log2 / exp2 / reciprocal / square-root instructions instead of the bit-reproducible restatements -- NOT bit-comparable with
the reference, so what is asserted here is the STATED TOLERANCE, against the same references the bit-exact path is pinned to
(the reference Fortran's kernel vectors, the LowerColorado goldens, the reference routed on the CPU at full CONUS size).

Stated tolerance (the numbers asserted below; measured distributions: profiles/r05_tolerance_report.json):
  * one segment-step (f90:8-186) on the reference's own population of kernel vectors (tests/golden/kernel_vectors.npz: the
    ranges of its test suite, many far outside any river) against the reference Fortran's bits: 99 % of the q / velocity /
    depth values within rtol 2e-5 + atol 1e-7, 99.8 % within rtol 1e-3 + atol 1e-6, at most 0.1 % of the steps beyond
    rtol 3e-2 + atol 1e-4.  The tail is the secant iteration's, not the arithmetic's: where it needs ten or fifty iterations
    (or never settles and leaves by its depth floor, f90:120-122) a last-place difference in a residual moves the exit, and
    the 1 % exit test (f90:83) lets the depth land anywhere in its band -- the reference's own kernel as shipped scatters by
    3.5e-2 at its 99th percentile on the same vectors for that reason (finding 2).  Nothing routed stays
    exactly nothing; every result is finite where the reference's is;
  * a routed window with assume_short_ts (the reference's configured mode) against the reference Fortran: at least 99.9 % of
    all (row, step) flows within rtol 1e-4 + atol 1e-6 m3/s, at least 99.99 % within rtol 3e-2 + atol 1e-4, every one within
    rtol 1e-1 + atol 1e-3 (measured on CONUS, 7.9e8 flows: 99.9955 %, 100 %, largest relative difference 5.6e-2 on 517 of
    2.7 M rows; LowerColorado: every flow within 5.2e-5);
  * without assume_short_ts the reference recurrence itself amplifies last-place differences from a cold start (the reason
    det_pow.h exists: "close" is not testable there) -- tolerance arithmetic runs in that mode, and no tolerance is claimed:
    the test only records the distribution and asserts finiteness and the bulk.
Every test writes its measured distribution into gpurun_out/tolerance_report.json (profiles/r05_tolerance_report.json is
the copy of the round's run).
"""
import json
import os

import numpy as np
import pytest

import helpers as H
from oracle import oracle as O
from troute_amd.plan import RoutingPlan, segments

pytestmark = pytest.mark.gpu

RTOL_STEP, ATOL_STEP, FRAC_STEP = 2e-5, 1e-7, 0.99
RTOL_STEP2, ATOL_STEP2, FRAC_STEP2 = 1e-3, 1e-6, 0.998
RTOL_FLIP = 3e-2
RTOL_DAY, ATOL_DAY, FRAC_DAY = 1e-4, 1e-6, 0.999
RTOL_ANY, ATOL_ANY, FRAC_ANY = 3e-2, 1e-4, 0.9999
RTOL_MAX, ATOL_MAX = 1e-1, 1e-3
REPORT = os.path.join(os.path.dirname(H.GOLDEN.rstrip("/")).rsplit("/tests", 1)[0], "gpurun_out", "tolerance_report.json")


def record(key, value):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    d = {}
    if os.path.exists(REPORT):
        try:
            d = json.load(open(REPORT))
        except Exception:
            d = {}
    d[key] = value
    json.dump(d, open(REPORT, "w"), indent=1, sort_keys=True)


def distribution(got, want, rtol, atol):
    """error of `got` against `want` in units of the bound atol + rtol |want|: what fraction is inside, the 99th / 99.9th
    percentile and the maximum of the plain relative error where the reference is not tiny"""
    got = np.asarray(got, np.float64).ravel()
    want = np.asarray(want, np.float64).ravel()
    err = np.abs(got - want)
    inside = err <= atol + rtol * np.abs(want)
    big = np.abs(want) > 100 * atol
    rel = err[big] / np.abs(want[big])
    return {"n": int(want.size), "inside": float(inside.mean()), "outside": int((~inside).sum()),
            "rel_p99": float(np.quantile(rel, 0.99)) if rel.size else 0.0,
            "rel_p999": float(np.quantile(rel, 0.999)) if rel.size else 0.0,
            "rel_max": float(rel.max()) if rel.size else 0.0, "abs_max": float(err.max()) if err.size else 0.0}


def test_segment_step_within_the_stated_tolerance_of_the_reference_fortran():
    """The 12 026 kernel vectors of the reference Fortran (tests/golden/kernel_vectors.npz, the fixture the bit-exact test
    uses -- drawn over the ranges of the reference's own test suite), against the reference's bits."""
    kv = H.load_kernel_vectors()
    x = np.ascontiguousarray(kv["inputs_f64"].astype(np.float32))
    ex, ie = segments(x, arithmetic="exact", with_iterations=True)
    assert np.array_equal(ex.view(np.uint32), kv["ref_qj0_f32"].view(np.uint32))        # (the reference's bits)
    tl, it = segments(x, arithmetic="tolerance", with_iterations=True)
    ok = np.isfinite(ex).all(axis=1)
    e3, t3 = ex[ok][:, :3], tl[ok][:, :3]
    d1 = distribution(t3, e3, RTOL_STEP, ATOL_STEP)
    d2 = distribution(t3, e3, RTOL_STEP2, ATOL_STEP2)
    beyond = (np.abs(t3.astype(np.float64) - e3) > ATOL_ANY + RTOL_FLIP * np.abs(e3)).any(axis=1)
    rel = np.abs(t3.astype(np.float64) - e3) / np.maximum(np.abs(e3), 1e-3)
    record("segment_step", {
        "steps": int(ok.sum()), "iteration_count_differs": int((ie[ok] != it[ok]).sum()),
        "within_rtol_2e-5": d1, "within_rtol_1e-3": d2, "steps_beyond_rtol_3e-2": int(beyond.sum()),
        "rel_quantiles": {str(q): float(np.quantile(rel, q)) for q in (0.5, 0.9, 0.99, 0.999, 0.9999, 1.0)},
        "courant": distribution(tl[ok][:, 3:5], ex[ok][:, 3:5], RTOL_STEP2, ATOL_STEP2)})
    assert np.isfinite(tl[ok]).all()
    assert d1["inside"] >= FRAC_STEP and d2["inside"] >= FRAC_STEP2, (d1, d2)
    assert beyond.sum() <= 0.001 * ok.sum(), int(beyond.sum())
    dry = ok & (ie == 0)                                  # nothing routed stays exactly nothing
    assert dry.any() and np.array_equal(tl[dry][:, :3], ex[dry][:, :3])


@pytest.mark.parametrize("engine", ["flow", "levels", "levels-wide"])
@pytest.mark.parametrize("short", [True, False])
def test_lowercolorado_within_the_stated_tolerance_of_the_reference_golden(short, engine, monkeypatch):
    """LowerColorado 11 248 segments x 288 steps, both timestep modes, every engine, against the reference Fortran golden."""
    monkeypatch.setenv("TRMC_ENGINE", engine.split("-")[0])
    if engine.endswith("-wide"):
        monkeypatch.setenv("TRMC_WIDE_MIN_ROWS", "32")
        monkeypatch.setenv("TRMC_WIDE_K", "8")
        monkeypatch.setenv("TRMC_MID_MIN_ROWS", "8")
    lc = H.LowerColorado()
    up_ptr, up_idx = lc.csr()
    with RoutingPlan(up_ptr, up_idx, lc.params9, assume_short_ts=short, options={"arithmetic": "tolerance"}) as plan:
        assert plan.arithmetic == "tolerance"
        fvd = plan.route(288, lc.qts, short, lc.qlat, lc.q0)
        assert plan.stats()["arithmetic"] == 1
    with RoutingPlan(up_ptr, up_idx, lc.params9, assume_short_ts=short) as plan:
        exact = plan.route(288, lc.qts, short, lc.qlat, lc.q0)
    g = lc.golden()
    tag = "shortts" if short else "fullts"
    assert np.array_equal(exact[:, g["tsel"] - 1, :].view(np.uint32), g[f"{tag}_f32_tsel"].view(np.uint32))   # (the reference's bits)
    d_q = distribution(fvd[:, :, 0], exact[:, :, 0], RTOL_DAY, ATOL_DAY)
    d_any = distribution(fvd[:, :, 0], exact[:, :, 0], RTOL_ANY, ATOL_ANY)
    d_d = distribution(fvd[:, :, 2], exact[:, :, 2], RTOL_DAY, 1e-5)
    d_v = distribution(fvd[:, :, 1], exact[:, :, 1], RTOL_DAY, 1e-5)
    record(f"lowercolorado_{tag}_{engine}", {"flow": d_q, "depth": d_d, "velocity": d_v})
    assert np.isfinite(fvd).all()
    if short:
        d_max = distribution(fvd[:, :, 0], exact[:, :, 0], RTOL_MAX, ATOL_MAX)
        assert d_q["inside"] >= FRAC_DAY and d_any["inside"] >= FRAC_ANY and d_max["inside"] == 1.0, (d_q, d_any, d_max)
    else:
        # without the short-timestep assumption the reference recurrence amplifies differences from a cold start (det_pow.h;
        # SURVEY section 0): no tolerance is claimed, the distribution is recorded, the bulk asserted
        assert d_q["inside"] >= 0.7, d_q


def test_conus_every_segment_within_the_stated_tolerance_of_the_reference():
    """All 2 729 077 segments of the timed configuration through the three bench days (N-1 cold, N, N+1 warm) in tolerance
    arithmetic, day N+1 against the reference Fortran routed on the CPU (oracle.reference_windows, as the bit-exact test):
    the flow of every row at every step, and the final state; plus, against the bit-exact plan on the same days, on how
    many rows the last step's iteration count differs."""
    from troute_amd import synthetic
    net = synthetic.generate(cache_dir=os.environ.get("TRMC_CACHE", "/tmp/trmc_cache"))
    to, params = net["to"], net["params"]
    up_ptr, up_idx = synthetic.upstream_csr(to)
    nseg = to.shape[0]
    nsteps, qts = 288, 12
    qlat_s = net["qlat"]
    qlat_a = synthetic.forcing(nseg, qlat_s.shape[1], synthetic.DEFAULT_SEED + 1, previous=qlat_s)
    qlat_b = synthetic.forcing(nseg, qlat_s.shape[1], synthetic.DEFAULT_SEED + 2, previous=qlat_a)
    q0 = np.zeros((nseg, 3), np.float32)
    ref = O.reference_windows(to, params, (qlat_s, qlat_a, qlat_b), q0, nsteps, qts, True)
    out = {}
    iters = {}
    for arith in ("tolerance", "exact"):
        with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, options={"arithmetic": arith}) as plan:
            assert plan.engine == "levels"
            plan.upload_forcing(nsteps, qlat_s, q0)
            plan.route_device(nsteps, qts, True)
            plan.upload_forcing(nsteps, qlat_a, None)
            plan.route_device(nsteps, qts, True)
            plan.upload_forcing(nsteps, qlat_b, None)
            st = plan.route_device(nsteps, qts, True)
            iters[arith] = plan.download_iterations()
            if arith == "tolerance":
                q = np.ascontiguousarray(plan.download_fvd().reshape(nseg, nsteps, 3)[:, :, 0])
                final = plan.download_final_state()
                ms_tol = st["ms_main"]
            else:
                ms_exact = st["ms_main"]
    want = ref["q"][:, 1:]
    rep = {"segments": int(nseg), "steps": nsteps, "ms_main_tolerance": ms_tol, "ms_main_exact": ms_exact,
           "last_step_iteration_count_differs": int((iters["tolerance"] != iters["exact"]).sum())}
    inside_day = 0
    inside_any = 0
    inside_max = 0
    rel_max = 0.0
    rows_touched = 0
    for lo in range(0, nseg, 200000):
        g, w = q[lo:lo + 200000].astype(np.float64), want[lo:lo + 200000].astype(np.float64)
        err = np.abs(g - w)
        ok = err <= ATOL_DAY + RTOL_DAY * np.abs(w)
        inside_day += int(ok.sum())
        inside_any += int((err <= ATOL_ANY + RTOL_ANY * np.abs(w)).sum())
        inside_max += int((err <= ATOL_MAX + RTOL_MAX * np.abs(w)).sum())
        rows_touched += int((~ok).any(axis=1).sum())
        big = np.abs(w) > 1e-4
        if big.any():
            rel_max = max(rel_max, float((err[big] / np.abs(w[big])).max()))
    total = nseg * nsteps
    rep.update({"flows": total, "inside_rtol1e-4": inside_day / total, "outside_rtol1e-4": total - inside_day,
                "rows_with_a_flow_outside": rows_touched, "inside_rtol3e-2": inside_any / total, "inside_rtol1e-1": inside_max / total,
                "rel_max": rel_max,
                "final_state": distribution(final[:, [0, 2]], ref["state"][:, [0, 2]], RTOL_DAY, ATOL_DAY)})
    record("conus_day_n_plus_1", rep)
    assert np.isfinite(q).all()
    assert rep["inside_rtol1e-4"] >= FRAC_DAY and rep["inside_rtol3e-2"] >= FRAC_ANY and rep["inside_rtol1e-1"] == 1.0, rep


def test_conus_stream_within_the_stated_tolerance_of_the_reference():
    """The stream of days in tolerance arithmetic at full size (ShardedRouter(stream=True, options={"arithmetic": "tolerance"}),
    products only: the TOL + LAZYV instances of k_mc_tile / k_mc_ctile): the three bench days from the cold start, every day's
    outlet hydrographs and the last day's final state, against the reference Fortran routed on the CPU day by day; then the
    same days with the last one as a full result -- the flow of every row at every step within the stated tolerance."""
    from troute_amd import _lib, synthetic
    from troute_amd.distributed import ShardedRouter
    from troute_amd.sequence import pinned_like
    net = synthetic.generate(cache_dir=os.environ.get("TRMC_CACHE", "/tmp/trmc_cache"))
    to, params = net["to"], net["params"]
    nseg = to.shape[0]
    nsteps, qts = 288, 12
    qlat_s = net["qlat"]
    qlat_a = synthetic.forcing(nseg, qlat_s.shape[1], synthetic.DEFAULT_SEED + 1, previous=qlat_s)
    qlat_b = synthetic.forcing(nseg, qlat_s.shape[1], synthetic.DEFAULT_SEED + 2, previous=qlat_a)
    days = [qlat_s, qlat_a, qlat_b]
    q0 = np.zeros((nseg, 3), np.float32)
    s = ShardedRouter(to, params, stream=True, options={"arithmetic": "tolerance"})
    P = s.stream_plan(0)
    assert P.arithmetic == "tolerance"
    lag, W, C = P.lags()
    assert W > 0 and C > 0
    rows, prod, _, info = H.stream_days(s, lambda k: days[k], nsteps, qts, q0, ndays=len(days))
    P.upload_forcing(nsteps, days[0], q0)
    P.stream_begin(nsteps, qts, full_output=True)
    full = _lib.result_empty((nseg, nsteps, 3), np.float32, always_pinned=True)
    for d in range(len(days)):
        P.stream_push(pinned_like(days[d]), fvd=full if d == len(days) - 1 else None)
    P.stream_flush()
    P.stream_wait(len(days) - 1)
    P.stream_end()
    s.close()
    rep = {"segments": int(nseg), "steps": nsteps, "days": len(days), "wide_levels": W, "cluster_levels": C,
           "tiles_per_day": info["tiles_per_day"]}
    for w, (q, state, _) in enumerate(H.reference_day_by_day(to, params, days, q0, nsteps, qts)):
        want = q[rows, 1:]
        d_day = distribution(prod[w][0], want, RTOL_DAY, ATOL_DAY)
        d_any = distribution(prod[w][0], want, RTOL_ANY, ATOL_ANY)
        d_max = distribution(prod[w][0], want, RTOL_MAX, ATOL_MAX)
        rep[f"day{w}_outlets"] = {"within_rtol1e-4": d_day, "inside_rtol3e-2": d_any["inside"], "inside_rtol1e-1": d_max["inside"]}
        assert np.isfinite(prod[w][0]).all() and np.isfinite(prod[w][1]).all(), w
        assert d_day["inside"] >= FRAC_DAY and d_any["inside"] >= FRAC_ANY and d_max["inside"] == 1.0, (w, d_day, d_any, d_max)
        if w == len(days) - 1:
            inside = [0, 0, 0]
            for lo in range(0, nseg, 200000):
                g, t = full[lo:lo + 200000, :, 0].astype(np.float64), q[lo:lo + 200000, 1:].astype(np.float64)
                err = np.abs(g - t)
                for i, (rt, at) in enumerate(((RTOL_DAY, ATOL_DAY), (RTOL_ANY, ATOL_ANY), (RTOL_MAX, ATOL_MAX))):
                    inside[i] += int((err <= at + rt * np.abs(t)).sum())
            total = nseg * nsteps
            rep.update({"flows": total, "inside_rtol1e-4": inside[0] / total, "inside_rtol3e-2": inside[1] / total,
                        "inside_rtol1e-1": inside[2] / total,
                        "final_state": distribution(prod[w][1][:, [0, 2]], state[:, [0, 2]], RTOL_DAY, ATOL_DAY),
                        "final_flow": distribution(prod[w][1][:, 0], state[:, 0], RTOL_DAY, ATOL_DAY)})
            assert np.isfinite(full[:, :, 0]).all()
            assert_full = rep["inside_rtol1e-4"] >= FRAC_DAY and rep["inside_rtol3e-2"] >= FRAC_ANY and rep["inside_rtol1e-1"] == 1.0
            record("conus_stream_products_only", rep)
            assert assert_full, rep
            assert rep["final_flow"]["inside"] >= FRAC_DAY, rep["final_flow"]
        del q
