#!/usr/bin/env python3
"""Counters per day of the timed STREAM in a rocprofv3 --pmc database (e.g. `rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES -- python
bench.py --steps 6 --warmup 1 --headline-only`): the full launches of the last stream (the selection of tools/stream_timeline.py),
mean per launch x tiles per day, per kernel.    python tools/stream_counters.py results.db"""
import sqlite3
import sys

con = sqlite3.connect(sys.argv[1])
tpd = 18
rows = con.execute(
    "select d.id, s.kernel_name, d.start from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id "
    "order by d.start").fetchall()
pm = {}
for did, name, v in con.execute(
        "select d.id, p.name, sum(e.value) from rocpd_pmc_event e join rocpd_info_pmc p on e.pmc_id = p.id "
        "join rocpd_kernel_dispatch d on d.event_id = e.event_id group by d.id, p.name"):
    pm.setdefault(did, {})[name] = v


def short(n):
    for k in ("k_mc_ctile", "k_mc_tile", "k_init_state", "k_prep_qlat"):
        if k in n:
            return k
    return n[:24]


rows = [(did, short(n), n) for did, n, _ in rows]
i0 = max(i for i, r in enumerate(rows) if r[1] == "k_init_state")
win = rows[i0:]
tiles = [r for r in win if r[1] == "k_mc_tile"]
ctiles = [r for r in win if r[1] == "k_mc_ctile"]
days = sum(1 for r in win if r[1] == "k_prep_qlat")
lag = len(tiles) - days * tpd
lo, hi = min(len(tiles) - lag - tpd, max(lag, tpd)), len(tiles) - lag
print(f"last stream: {days} days, {len(tiles)} k_mc_tile / {len(ctiles)} k_mc_ctile launches, steady state {lo}..{hi - 1}")
tot = {}
for name, ks in (("k_mc_tile", tiles), ("k_mc_ctile", ctiles)):
    sel = ks[lo:hi]
    inst = sorted(set(n for _, _, n in sel))
    cs = sorted(set(c for r in sel for c in pm.get(r[0], {})))
    for c in cs:
        vals = [pm[r[0]][c] for r in sel if c in pm.get(r[0], {})]
        per_day = sum(vals) / len(vals) * tpd
        tot[c] = tot.get(c, 0) + per_day
        print(f"  {name:11s} {c:16s} per launch {sum(vals) / len(vals) / 1e6:9.2f} M  per day {per_day / 1e9:7.3f} x 10^9   ({len(vals)} launches)")
    print(f"      instance(s): {inst}")
for c, v in tot.items():
    print(f"  both kernels {c:16s} per day {v / 1e9:7.3f} x 10^9")
