"""Randomised parity sweeps of the diffusive solver (developer tool), on synthetic mainstems the goldens do not reach.

    python tools/fuzz_diffusive.py --seconds 240 [--seed 1]                  (GPU box)
    python tools/fuzz_diffusive.py --reference --seconds 600 [--seed 1]      (CPU only; needs oracle/_ref/libdiff_ref.so)

Default mode: the device's parallel time loop against the host instantiation of the same source (oracle/libdw_oracle.so),
bit for bit.  Every round draws a domain from tests/diffusive_cases.py::long_mainstem -- 3 to 260 mainstem reaches in series
with a side branch and tributary junctions, so both chain-state homes are taken (LDS for the short ones, global memory for
the long) -- then scales flows (x 0.05 ... x 40: from nearly dry to far over bank, so that the table windows of the depth
solve wander and are re-centred), roughness and the tributary hydrographs, and every fourth round forces the narrow 5-row
windows or the global-memory chain state (TRDW_WINDOW_ROWS / TRDW_CHAIN_GLOBAL).

--reference: the host instantiation against the REFERENCE FORTRAN, bit for bit, over the wider draws of
tests/diffusive_cases.py::widened_draw (flows x 0.01 ... x 200, roughness x 0.4 ... x 4, slopes x 0.05 / x 20 on every fifth
domain, a prescribed depth series at the tailwater on every third).  c_diffnw carries state from one call to the next -- 911
such domains called one after the other in ONE process gave 158 "differences", all on the reference's side (it differed from
its own first answer when asked again; the host never did) -- so every domain goes to a fresh child process
(tests/golden/diffusive_ref_child.py), and a domain that differs is sent to a second child before it is reported: two
children that agree with each other and not with the host mean a misreading in diffusive_core.hpp.

Both modes print the number of rounds and of differing domains; exit code 1 on any differing bit.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diffusive_cases as DC                                       # noqa: E402


def host_oracle():
    import ctypes as C
    from oracle import oracle as O
    O.build()
    return C.CDLL(os.path.join(ROOT, "oracle", "libdw_oracle.so"))


def against_reference(a):
    from concurrent.futures import ThreadPoolExecutor
    host = host_oracle()
    t_end = time.time() + a.seconds
    seed, rounds, bad, unrepeatable, nonfinite, nodes_total = a.seed, 0, 0, 0, 0, 0

    def one(s):
        ins, knobs = DC.widened_draw(s)
        return s, ins, knobs, DC.reference_in_child(ins)

    with ThreadPoolExecutor(a.jobs) as pool:
        while time.time() < t_end:
            for s, ins, knobs, ref in pool.map(one, range(seed, seed + 4 * a.jobs)):
                rc, got = DC.call_c(host, "dw_oracle_diffnw", ins)
                ok = rc == 0 and all(DC.same_bits(g, r) for g, r in zip(got, ref))
                verdict = "ok"
                if not ok:
                    again = DC.reference_in_child(ins)
                    if all(DC.same_bits(x, y) for x, y in zip(ref, again)):
                        bad += 1
                        verdict = "DIFF (two reference processes agree with each other)"
                    else:
                        unrepeatable += 1
                        verdict = "reference not repeatable across fresh processes"
                fin = bool(all(np.isfinite(r).all() for r in ref))
                nonfinite += 0 if fin else 1
                nodes_total += DC.mainstem_nodes(ins)
                rounds += 1
                if verdict != "ok" or not fin or rounds % 50 == 0:
                    print(f"seed {s:5d} nmain {knobs['nmain']:3d} flow x{knobs['flow']:8.3f} n x{knobs['rough']:4.2f} "
                          f"slope x{knobs['slope']:5.2f} option 1 {knobs['opt1']} depth max {np.nanmax(ref[2]):8.2f} "
                          f"finite {fin} {verdict}", flush=True)
            seed += 4 * a.jobs
    print(f"fuzz_diffusive --reference: {rounds} domains, {nodes_total} mainstem nodes, {nonfinite} with non-finite results "
          f"in the reference run, {unrepeatable} not repeatable across fresh reference processes, {bad} differing")
    sys.exit(1 if bad or unrepeatable else 0)


def against_device(a):
    from troute_amd.routing.fast_reach import diffusive as D
    host = host_oracle()
    t_end = time.time() + a.seconds
    seed, rounds, bad, nodes_total, nonfinite = a.seed, 0, 0, 0, 0
    while time.time() < t_end:
        rng = np.random.default_rng(10_000 + seed)
        nmain = int(rng.choice([3, 5, 8, 13, 21, 40, 80, 150, 220, 260]))
        ins = DC.long_mainstem(nmain=nmain, seed=seed)
        scale = float(np.exp(rng.uniform(np.log(0.05), np.log(40.0))))
        ins["iniq"] = ins["iniq"] * scale
        ins["qtrib_g"] = ins["qtrib_g"] * scale * float(rng.uniform(0.5, 3.0))
        ins["qlat_g"] = ins["qlat_g"] * scale
        f = float(rng.uniform(0.6, 2.5))
        ins["mann_ar_g"] = ins["mann_ar_g"] * f
        ins["manncc_ar_g"] = ins["manncc_ar_g"] * f
        env = {}
        if seed % 4 == 1:
            env["TRDW_WINDOW_ROWS"] = "5"
        elif seed % 4 == 3:
            env["TRDW_CHAIN_GLOBAL"] = "1"
        rc, want = DC.call_c(host, "dw_oracle_diffnw", ins)
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            got = D.compute_diffusive(ins)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        ok = rc == 0 and all(DC.same_bits(g, w) for g, w in zip(got, want))
        fin = bool(np.isfinite(want[0]).all())
        nonfinite += 0 if fin else 1
        nodes = int(ins["frnw_g"][:, 0].sum())
        nodes_total += nodes
        rounds += 1
        bad += 0 if ok else 1
        print(f"seed {seed:4d} reaches {int(ins['nrch_g']):4d} nodes {nodes:5d} flow x{scale:7.3f} n x{f:4.2f} "
              f"{' '.join(f'{k}={v}' for k, v in env.items()) or '-':22s} depth max {np.nanmax(want[2]):7.2f} "
              f"finite {fin} {'ok' if ok else 'DIFF'}", flush=True)
        seed += 1
    print(f"fuzz_diffusive: {rounds} domains, {nodes_total} nodes, {nonfinite} with non-finite results in the host run, "
          f"{bad} differing")
    sys.exit(1 if bad else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reference", action="store_true", help="host restatement against the reference Fortran (CPU only)")
    ap.add_argument("--jobs", type=int, default=8, help="--reference: child processes at a time")
    a = ap.parse_args()
    (against_reference if a.reference else against_device)(a)


if __name__ == "__main__":
    main()
