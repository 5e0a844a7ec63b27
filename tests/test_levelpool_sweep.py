"""The level pool in every regime, on the CPU: reference Fortran (recorded, and live where oracle/_ref is present) -> oracle ->
the classifying restatement of tests/levelpool_cases.py, and the census of the sweep as conditions.  The device side is
tests/test_gpu_levelpool_sweep.py."""
import ctypes as C
import functools
import os

import numpy as np

import helpers as H
import levelpool_cases as LC
from oracle import oracle as O

MIN_COUNT = 20


@functools.lru_cache(maxsize=None)
def recording():
    rec = np.load(os.path.join(H.GOLDEN, "levelpool_sweep.npz"))
    return rec["outflow"], rec["elevation"], rec["sha256"]


@functools.lru_cache(maxsize=None)
def oracle_sweep():
    return LC.oracle_sweep()


@functools.lru_cache(maxsize=None)
def classified():
    par, dt, h0, inflows = LC.sweep_arrays()
    return par, LC.classify_series(par, dt, h0, inflows)


def test_the_recording_is_of_these_inputs():
    q, h, sha = recording()
    assert q.dtype == h.dtype == np.float32 and q.shape == h.shape == (len(LC.sweep_cases()), LC.SWEEP_STEPS)
    assert np.array_equal(sha, LC.input_hashes())
    names = [c[0] for c in LC.sweep_cases()]
    assert len(set(names)) == len(names)


def test_oracle_levelpool_equals_reference_fortran_on_the_sweep():
    """every case and every step: the recorded bits where they are finite, a NaN where the reference has one; and the same
    against the reference build itself where it is present"""
    q, h = oracle_sweep()
    wants = [recording()[:2]]
    if O.have_ref("liblp_ref.so"):
        wants.append(LC.reference_sweep(C.CDLL(O.ref_path("liblp_ref.so"))))
    for want_q, want_h in wants:
        for k, case in enumerate(LC.sweep_cases()):
            assert LC.same(q[k], want_q[k]) and LC.same(h[k], want_h[k]), case[0]
    assert np.isnan(wants[0][0]).any() and np.isinf(wants[0][0]).sum() == 0      # (the sweep does reach NaN, and never an infinity)


def test_classify_equals_the_oracle_on_the_sweep():
    """the restatement that names the branches computes the oracle's outflow and elevation on every step"""
    q, h = oracle_sweep()
    _, s = classified()
    for k, case in enumerate(LC.sweep_cases()):
        assert LC.same(s["outflow"][k], q[k]) and LC.same(s["elevation"][k], h[k]), case[0]


def test_classify_of_one_pool_and_of_many_agree():
    name, par, dt, h0, inflows = LC.sweep_cases()[1234]
    one = LC.classify(par, dt, h0, inflows[0])
    _, s = classified()
    assert one["branch"].shape == (4,) and one["outflow"].shape == ()
    assert LC.same(one["outflow"], s["outflow"][1234, 0]) and np.array_equal(one["branch"], s["branch"][1234, 0])


def test_census_of_the_sweep_meets_its_conditions():
    """Conditions, not measurements: the sweep is chosen so that the reference's recording alone reaches every stage x branch
    cell, every start -> end crossing and every tag at least MIN_COUNT times (classify reproduces the recording bit for bit:
    the two tests above, so its labels are labels of the recorded steps).

    Two cells cannot be reached by construction and are asserted EMPTY instead: `overtop` with the weir depth unclipped at
    stage 1 and at the final evaluation.  There the pool is evaluated at the elevation the overtopping test reads
    (h_eval == h_top), so the branch needs H > maxh with fl(H - we) <= fl(maxh - we).  Every triple of the sweep has
    0 <= we <= maxh: H - we and maxh - we are then no larger than H, their exact values differ by at least one ulp of H,
    hence by at least one ulp of either result, and rounding keeps them apart -- H > maxh forces dh onto maxWeirDepth.
    Stages 2 and 3 do reach it: a pool that overtopped at the start of the step and has drained below the crest since."""
    par, s = classified()
    assert LC.same(s["outflow"], recording()[0]) and LC.same(s["elevation"], recording()[1])
    c = LC.census(par, s)
    print(LC.census_table(c))
    assert all(0 <= p[LC._P["weir_elevation"]] <= p[LC._P["max_depth"]] for p in par)
    for (stage, branch), n in c["cells"].items():
        if branch == "overtop" and stage in ("stage1", "final"):
            assert n == 0, (stage, branch, n)
        else:
            assert n >= MIN_COUNT, (stage, branch, n)
    assert len(c["crossings"]) == 12
    for crossing, n in c["crossings"].items():
        assert n >= MIN_COUNT, (crossing, n)
    assert set(c["tags"]) == set(LC.TAGS)
    for tag, n in c["tags"].items():
        assert n >= MIN_COUNT, (tag, n)


def test_cold_start_on_the_crest_does_not_overtop():
    """ifd = 1 puts the pool on max_depth exactly (oe + (maxh - oe) * 1 in float32), and the reference's strict > keeps it
    out of the overtopping branch"""
    hits = 0
    for k, (name, par, dt, h0, inflows) in enumerate(LC.sweep_cases()):
        if "/ifd=1.0/" in name:
            assert h0 == par[LC._P["max_depth"]], name
            assert classified()[1]["branch"][k, 0, 0] < LC.OVERTOP, name
            hits += 1
    assert hits >= MIN_COUNT
