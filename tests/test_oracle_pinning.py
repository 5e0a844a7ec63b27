"""The oracle is only worth something if it IS the reference: pin it.

Every check here runs on CPU.  Fixtures were produced by tests/golden/make_fixtures.py from the
reference Fortran compiled in the dev container (oracle/Makefile `ref`); when those builds are
present (dev container) the live comparison runs too.
"""
import hashlib
import os

import numpy as np
import pytest

import helpers as H
from oracle import oracle as O

KV = H.load_kernel_vectors()
X64 = KV["inputs_f64"]
X32 = X64.astype(np.float32)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_restatement_equals_reference_fortran_fp32_bitwise():
    """12 026 vectors (KATs, the reference's own seed-16 generator, CONUS-like states, branch edge
    cases): restated kernel == reference Fortran with the canonical Qj_0 = 0, bit for bit, NaNs included."""
    got = O.segments(X32)
    assert np.array_equal(bits(got), bits(KV["ref_qj0_f32"]))


def test_restatement_equals_reference_fortran_fp64_bitwise():
    got = O.segments(X32.astype(np.float64))
    assert np.array_equal(bits(got), bits(KV["ref_qj0_f64"]))


def test_equals_unmodified_wrfhydro_original_where_semantics_coincide():
    """src/kernel/muskingum/test_MC_kernel.py:36-40 asserts T-Route kernel == WRF-Hydro original.
    The two differ by design only when quc is the sole positive flow (MUSKINGCUNGE.f90:96 vs
    NOLOOP.f90:73-74) or the flood-plain guards (twcc<=0, ncc<=0) fire; everywhere else the
    restatement must reproduce the UNMODIFIED original bit for bit."""
    got = O.segments(X32)[:, :3]
    wrf = KV["wrf_f32"]
    c = {k: X32[:, i] for i, k in enumerate(O.IN_COLS)}
    same_sem = ((c["ql"] > 0) | (c["qup"] > 0) | (c["qdp"] > 0)) & (c["twcc"] > 0) & (c["ncc"] > 0)
    same_sem &= np.isfinite(got).all(1)
    assert same_sem.sum() > 11000
    assert np.array_equal(bits(got[same_sem]), bits(wrf[same_sem]))


def test_reference_kats():
    """Known answers printed in mc_sseg_stime_NOLOOP_demo.py:196-205,:234-248 (their last digits are
    compiler-dependent: gfortran there, amdflang here -- 1e-7 relative in fp32, 5e-8 in fp64)."""
    tags = KV["tags"]
    i32 = int(np.flatnonzero(tags == "kat_lowflow_f32")[0])
    exp32 = np.array([0.7570106983184814, 0.12373604625463486, 0.02334451675415039])
    got = O.segments(X32[i32:i32 + 1])[0, :3].astype(np.float64)
    assert np.allclose(got, exp32, rtol=2e-7, atol=0)
    i64 = int(np.flatnonzero(tags == "kat_lowflow_f64in")[0])
    exp64 = np.array([0.7570107902354513, 0.12373606306742324, 0.02334451646521419])
    got64 = O.segments(X64[i64:i64 + 1])[0, :3]
    assert np.allclose(got64, exp64, rtol=5e-8, atol=0)
    assert got64[2] == exp64[2]          # depth reproduces to the last bit


def test_as_shipped_kernel_is_only_statistically_comparable():
    """The shipped routine reads Qj_0 uninitialised (SURVEY finding 2): its output depends on call
    history, so it can only bound the canonical semantics statistically."""
    a = O.segments(X32)[:, :3]
    s = KV["ref_asshipped_f32"][:, :3]
    ok = np.isfinite(a).all(1) & np.isfinite(s).all(1)
    rel = (np.abs(a - s) / np.maximum(np.abs(a), 1e-30)).max(1)
    tags = KV["tags"]
    # the reference's own generator in its intended ranges: identical on all 5000 vectors
    m = ok & (tags == "refgen_mapped")
    assert m.sum() == 5000 and (rel[m] == 0).all()
    # CONUS-like low-flow states: the stale Qj_0 leaks into X on the first secant pass
    m = ok & (tags == "realistic")
    assert (rel[m] == 0).mean() > 0.7
    assert np.quantile(rel[m], 0.9) < 1e-2


def fresh_vectors():
    """100 000 of the kernel vectors drawn again with their flows jittered (seeded)"""
    rng = np.random.default_rng(123)
    n = 100_000
    x = X32[rng.integers(0, X32.shape[0], n)].copy()
    x[:, 1:5] *= rng.uniform(0.5, 2.0, (n, 4)).astype(np.float32)     # jitter the flows
    x[:, 14] *= rng.uniform(0.5, 2.0, n).astype(np.float32)
    return x


def digest(a):
    """SHA-256 of the bits of an output array (what tests/golden/make_ref_recordings.py records of the reference's)"""
    return hashlib.sha256(bits(np.ascontiguousarray(a)).tobytes()).hexdigest()


def test_live_against_ref_builds_on_fresh_vectors():
    """restated kernel == reference Fortran (canonical Qj_0) on fresh vectors, fp32 and fp64, bit for bit: against the digest
    of the reference's outputs recorded in tests/golden/reference_recordings.npz, and live where oracle/_ref is present"""
    rec = np.load(os.path.join(H.GOLDEN, "reference_recordings.npz"))
    x = fresh_vectors()
    for xs, sfx in ((x, "f32"), (x.astype(np.float64), "f64")):
        got = O.segments(xs)
        assert digest(got) == str(rec["fresh_vectors_sha256_" + sfx])
        name = f"libmc_ref_qj0_{sfx}.so"
        if O.have_ref(name):
            assert np.array_equal(bits(got), bits(O.ref_segments(xs, name)))


@pytest.mark.parametrize("short", [True, False])
def test_network_loop_equals_reference_kernel_driven_golden(short):
    """LowerColorado_TX MC-only, 11 248 segments x 288 steps: the restated loop (mc_reach.pyx:492-750)
    with the restated kernel equals the golden produced by calling the reference Fortran symbol per
    segment -- bit for bit at 12 time slices for every segment and at every step for 100 probes."""
    lc = H.LowerColorado()
    g = lc.golden()
    reaches, ups = lc.row_lists()
    tag = "shortts" if short else "fullts"
    fvd = O.network(lc.nts, lc.qts, reaches, ups, lc.params9, lc.q0, lc.qlat, short)
    assert np.array_equal(bits(np.ascontiguousarray(fvd[:, g["tsel"], :])), bits(g[f"{tag}_f32_tsel"]))
    assert np.array_equal(bits(np.ascontiguousarray(fvd[g["probes"]])), bits(g[f"{tag}_f32_probes"]))


def test_network_loop_fp64_golden():
    lc = H.LowerColorado()
    g = lc.golden()
    reaches, ups = lc.row_lists()
    fvd = O.network(lc.nts, lc.qts, reaches, ups, lc.params9.astype(np.float64), lc.q0, lc.qlat, True)
    assert np.array_equal(bits(np.ascontiguousarray(fvd[:, lc.nts, :])), bits(g["shortts_f64_final"]))
    assert np.array_equal(bits(np.ascontiguousarray(fvd[g["probes"]])), bits(g["shortts_f64_probes"]))


def test_segmentwise_driver_equals_reachwise():
    """A reach is just consecutive single-upstream segments: driving the loop segment by segment in
    level order is bit-identical to driving it reach by reach (what lets the GPU forget reaches)."""
    from troute_amd.plan import topology_levels
    from troute_amd.routing.fast_reach.mc_reach import _flatten_network
    lc = H.LowerColorado()
    reaches, ups = lc.row_lists()
    up_ptr, up_idx, in_reach = _flatten_network([(r, 0) for r in lc.reaches], lc.rconn, lc.ids)
    assert in_reach.all()
    lvl, _, _ = topology_levels(up_ptr, up_idx)
    for short in (True, False):
        a = O.network(36, lc.qts, reaches, ups, lc.params9, lc.q0, lc.qlat, short)
        b = O.network_by_segment(36, lc.qts, up_ptr, up_idx, lvl, lc.params9, lc.q0, lc.qlat, short)
        assert np.array_equal(bits(a), bits(b))


# ---- the bit-reproducible power the GPU uses ------------------------------------------------------
def test_det_powf_equals_this_libm_powf_strided_exhaustive():
    """det_pow.h (restated glibc 2.35 powf) against this machine's libm powf over every 61st float bit
    pattern (70 M patterns x 2 exponents incl. zeros, subnormals, infinities, NaNs, negatives).
    The full 2^32 sweep (stride 1, about a minute) was run when the fixtures were made: 0 mismatches."""
    import subprocess
    import tempfile
    root = H.GOLDEN.rsplit("/tests/", 1)[0]
    with tempfile.TemporaryDirectory() as td:
        exe = f"{td}/powf_exh"
        mfma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", *mfma, "-fopenmp", f"{root}/tests/powf_exhaustive.c",
                               "-lm", "-o", exe])
        out = subprocess.run([exe, "61"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count(" 0 mismatches") == 3


def test_det_powf_special_values():
    sp = np.array([0.0, -0.0, np.inf, np.nan, -1.0, 1e-45, 1.0, -np.inf], np.float32)
    got = O.det_powf(sp, np.float32(2) / np.float32(3))
    assert got[0] == 0 and got[1] == 0 and np.isinf(got[2]) and np.isnan(got[3]) and np.isnan(got[4])
    assert got[5] > 0 and got[6] == 1.0 and np.isinf(got[7]) and got[7] > 0


def test_det_instantiation_is_bitwise_the_libm_instantiation():
    """Same restated algorithm, libm powf swapped for det_pow.h: identical bits everywhere (kernel
    vectors and the LowerColorado network in both timestep modes) -- hence identical to the reference
    Fortran goldens, which the libm instantiation is pinned to above."""
    assert np.array_equal(bits(O.segments(X32)), bits(O.segments(X32, det=True)))
    lc = H.LowerColorado()
    g = lc.golden()
    reaches, ups = lc.row_lists()
    for short, tag in ((True, "shortts"), (False, "fullts")):
        d = O.network(lc.nts, lc.qts, reaches, ups, lc.params9, lc.q0, lc.qlat, short, det=True)
        assert np.array_equal(bits(np.ascontiguousarray(d[:, g["tsel"], :])), bits(g[f"{tag}_f32_tsel"]))
        assert np.array_equal(bits(np.ascontiguousarray(d[g["probes"]])), bits(g[f"{tag}_f32_probes"]))


def test_full_timestep_mode_is_chaotic_from_cold_start():
    """Documents WHY full-timestep parity is asserted bit-exactly (against the det oracle) instead of
    by tolerance: the reference recurrence amplifies a 1e-13 relative forcing change to O(1)
    differences within a few steps of a cold start, in fp64."""
    lc = H.LowerColorado()
    reaches, ups = lc.row_lists()
    p = lc.params9.astype(np.float64)
    ql = lc.qlat.astype(np.float64)
    a = O.network(24, lc.qts, reaches, ups, p, lc.q0, ql, False)
    b = O.network(24, lc.qts, reaches, ups, p, lc.q0, ql * (1 + 1e-13), False)
    rel = np.abs(a - b)[:, 1:, 0] / np.maximum(np.abs(a[:, 1:, 0]), 1e-9)
    assert rel.max() > 1.0
    a = O.network(24, lc.qts, reaches, ups, p, lc.q0, ql, True)
    b = O.network(24, lc.qts, reaches, ups, p, lc.q0, ql * (1 + 1e-13), True)
    rel = np.abs(a - b)[:, 1:, 0] / np.maximum(np.abs(a[:, 1:, 0]), 1e-9)
    assert rel.max() < 1e-9


def test_cpu_baseline_driver_equals_the_network_loop():
    """bench.py's CPU baseline (oracle/cpu_baseline.c: ordered sub-networks, C + OpenMP around a kernel symbol) routes
    the same flows and depths as the restated reference loop -- with the reference Fortran kernel where oracle/_ref is
    built, and with the restatement behind the same signature."""
    import helpers as H
    from troute_amd.synthetic import upstream_csr
    rng = np.random.default_rng(3)
    n = 5000
    to = np.array([rng.integers(i + 1, min(n, i + 60)) if (i + 1 < n and rng.random() > 0.002) else -1 for i in range(n)])
    perm = rng.permutation(n)
    to_r = np.full(n, -1, np.int64)
    to_r[perm] = np.where(to >= 0, perm[np.maximum(to, 0)], -1)
    up_ptr, up_idx = upstream_csr(to_r)
    p = np.stack([np.full(n, 300.0), rng.uniform(300, 3000, n), rng.uniform(1, 9, n), np.zeros(n), np.zeros(n),
                  np.full(n, 0.06), np.full(n, 0.12), rng.uniform(0.2, 1.5, n), rng.uniform(1e-3, 2e-2, n)], 1)
    p[:, 3] = p[:, 2] * 5 / 3
    p[:, 4] = 3 * p[:, 3]
    p = p.astype(np.float32)
    qlat = rng.uniform(0, 0.05, (n, 2)).astype(np.float32)
    q0 = np.zeros((n, 3), np.float32)
    nsteps, qts = 18, 12
    order_ptr, job_ptr, rows = O.ordered_subnetworks(to_r, target=400)
    assert sorted(rows.tolist()) == list(range(n)) and order_ptr[-1] == job_ptr.shape[0] - 1 and order_ptr.shape[0] > 2
    assert (np.diff(job_ptr) <= 400).all()
    from troute_amd.plan import topology_levels
    lvl, _, _ = topology_levels(up_ptr, up_idx)
    for short in (True, False):
        want = O.network_by_segment(nsteps, qts, up_ptr, up_idx, lvl, p, q0, qlat, short)
        names = [None] + (["libmc_ref_qj0_f32.so"] if O.have_ref("libmc_ref_qj0_f32.so") else [])
        for name in names:
            q, d, done, nthreads = O.cpu_baseline_route(nsteps, qts, short, order_ptr, job_ptr, rows, up_ptr, up_idx, p, qlat,
                                                        q0, ref_name=name, nthreads=4)
            assert done == n * nsteps
            assert np.array_equal(q.view(np.uint32), np.ascontiguousarray(want[:, :, 0]).view(np.uint32)), (short, name)
            assert np.array_equal(d.view(np.uint32), np.ascontiguousarray(want[:, -1, 2]).view(np.uint32))
