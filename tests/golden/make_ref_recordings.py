#!/usr/bin/env python3
"""Recorded outputs of the reference builds for the tests that also compare against them live, made in the dev container only
(needs oracle/_ref: oracle/Makefile `ref`).

Writes tests/golden/reference_recordings.npz:
  fresh_vectors_sha256_f32 / _f64   SHA-256 of the bits of the reference Fortran kernel's outputs (libmc_ref_qj0_f32.so /
                                    _f64.so) over tests/test_oracle_pinning.py's fresh_vectors() -- 100 000 rows x 6 outputs
                                    are too large to store, their digest pins them bit for bit
  levelpool_out / levelpool_h       [lakes, periods] float32: the reference level pool's (liblp_ref.so) outflow and water
                                    elevation over tests/test_reservoirs.py's levelpool_cases()
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
import test_oracle_pinning as P  # noqa: E402
import test_reservoirs as R  # noqa: E402


def main():
    names = ("libmc_ref_qj0_f32.so", "libmc_ref_qj0_f64.so", "liblp_ref.so")
    missing = [n for n in names if not O.have_ref(n)]
    if missing:
        raise SystemExit(f"oracle/_ref lacks {missing}: run `make -C oracle ref` where the reference sources are")
    x = P.fresh_vectors()
    out = {"fresh_vectors_sha256_f32": np.array(P.digest(O.ref_segments(x, names[0]))),
           "fresh_vectors_sha256_f64": np.array(P.digest(O.ref_segments(x.astype(np.float64), names[1])))}
    out["levelpool_out"], out["levelpool_h"] = R.reference_levelpool_runs(C.CDLL(O.ref_path(names[2])))
    path = os.path.join(HERE, "reference_recordings.npz")
    np.savez_compressed(path, **out)
    print(path, {k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
