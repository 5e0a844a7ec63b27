#!/usr/bin/env python3
"""Recorded outputs of the reference Fortran level pool over the sweep of tests/levelpool_cases.py, made in the dev container
only (needs oracle/_ref/liblp_ref.so: oracle/Makefile `ref`).

Writes tests/golden/levelpool_sweep.npz:
  outflow / elevation   [cases, steps] float32: what run_lp (bind_lp.f90 -> LEVELPOOL_PHYSICS) returned, NaN included
  sha256                [cases, 32] uint8: SHA-256 of each case's inputs; the inputs themselves are not stored, the
                        generator (levelpool_cases.sweep_cases) makes them again
Every case runs on two fresh handles of the reference, which must agree bit for bit (NaN for NaN) before anything is
recorded.  The census that tests/test_levelpool_sweep.py sets conditions on is printed from the recording: the classifying
restatement must reproduce the recorded bits first.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import oracle as O  # noqa: E402
import levelpool_cases as LC  # noqa: E402


def main():
    if not O.have_ref("liblp_ref.so"):
        raise SystemExit("oracle/_ref lacks liblp_ref.so: run `make -C oracle ref` where the reference sources are")
    lp = C.CDLL(O.ref_path("liblp_ref.so"))
    q, h = LC.reference_sweep(lp)
    q2, h2 = LC.reference_sweep(lp)
    assert LC.same(q2, q) and LC.same(h2, h), "two fresh handles of the reference disagree"
    par, dt, h0, inflows = LC.sweep_arrays()
    s = LC.classify_series(par, dt, h0, inflows)
    assert LC.same(s["outflow"], q) and LC.same(s["elevation"], h), "the classifying restatement is not the reference"
    path = os.path.join(HERE, "levelpool_sweep.npz")
    np.savez_compressed(path, outflow=q, elevation=h, sha256=LC.input_hashes())
    print(LC.census_table(LC.census(par, s)))
    print(f"{q.shape[0]} cases x {q.shape[1]} steps, {int(np.isnan(q).any(axis=1).sum())} cases with a NaN, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
