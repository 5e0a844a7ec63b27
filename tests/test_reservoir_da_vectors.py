"""Reservoir data-assimilation steps (hybrid persistence, RFC series) against the reference functions' recorded returns:
tests/golden/reservoir_da_vectors.npz (tests/golden/make_reservoir_da_fixtures.py), through the batch entry point that runs
the device functions of the step kernels (csrc/reservoir_da.hpp, trmc_reservoir_da_steps)."""
import os

import numpy as np
import pytest

import helpers as H

VEC = np.load(os.path.join(H.GOLDEN, "reservoir_da_vectors.npz"))

BRANCHES = ("obs_inside_window", "obs_outside_window", "obs_not_found", "tick_below_limit", "tick_above_limit", "nan_persisted",
            "storage_negative_outflow", "storage_max_reached", "storage_deficit", "storage_final_clamp", "max_storage_override",
            "rfc_index_advance", "rfc_expired", "rfc_negative_recovered", "rfc_negative_not_recovered_type4",
            "rfc_negative_not_recovered_type5")


def test_vectors_cover_every_branch():
    counts = dict(zip(VEC["branch_names"].tolist(), VEC["branch_counts"].tolist()))
    for b in BRANCHES:
        assert counts.get(b, 0) > 0, b
    assert VEC["hybrid_in"].shape[0] >= 2000 and VEC["rfc_in"].shape[0] >= 2000
    assert VEC["hybrid_in"].dtype == np.float32 and VEC["hybrid_out"].dtype == np.float32


@pytest.mark.gpu
def test_gpu_hybrid_steps_bit_identical_to_reference():
    from troute_amd.plan import reservoir_da_steps
    got = reservoir_da_steps("hybrid", VEC["hybrid_obs"], VEC["hybrid_time"], VEC["hybrid_in"])
    want = VEC["hybrid_out"]
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.gpu
def test_gpu_rfc_steps_bit_identical_to_reference():
    from troute_amd.plan import reservoir_da_steps
    got, idx = reservoir_da_steps("rfc", VEC["rfc_series"], None, VEC["rfc_in"], VEC["rfc_iin"])
    want = VEC["rfc_out"]
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1) | (idx != VEC["rfc_idx"]))
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.gpu
def test_gpu_batch_entry_validates_its_arguments():
    from troute_amd.plan import reservoir_da_steps
    with pytest.raises(ValueError):
        reservoir_da_steps("hybrid", np.zeros((2, 0), np.float32), np.zeros((2, 0), np.float32), np.zeros((2, 12), np.float32))
