#!/usr/bin/env python3
"""ONE call of the reference Fortran's c_diffnw (oracle/_ref/libdiff_ref.so), in a process of its own.

    python tests/golden/diffusive_ref_child.py INPUTS.npz OUTPUTS.npz

INPUTS.npz holds the arguments of the call as in_<name> (tests/diffusive_cases.py::ARG_ORDER); OUTPUTS.npz receives out_q,
out_elv and out_depth.  c_diffnw carries state from one call to the next, so a process that has called it once is spent:
this one exits.  It opens no GPU and has nothing preloaded; parents start it with subprocess.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import diffusive_cases as DC  # noqa: E402


def main():
    src, dst = sys.argv[1:3]
    z = np.load(src)
    ins = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libdiff_ref.so"))
    lib.c_diffnw.restype = None
    _, outs = DC.call_c(lib, "c_diffnw", ins)
    np.savez(dst, **{n: np.ascontiguousarray(o) for n, o in zip(DC.OUT_NAMES, outs)})


if __name__ == "__main__":
    main()
