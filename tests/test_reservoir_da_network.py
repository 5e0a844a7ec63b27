"""Hybrid-persistence (types 2, 3) and RFC (types 4, 5) reservoirs inside the network loop, on the device: the LowerColorado
domain collapsed at waterbodies against tests/golden/reservoir_da_network*.npz -- the reference's time x reach loop restated
in Python around the reference's own data-assimilation functions (tests/golden/make_reservoir_da_fixtures.py)."""
import os

import numpy as np
import pytest

import helpers as H
import test_reservoirs as TR

NET = np.load(os.path.join(H.GOLDEN, "reservoir_da_network.npz"))
NET_GENERAL = np.load(os.path.join(H.GOLDEN, "reservoir_da_network_general.npz"))
NTS = int(NET["nts"])
ENGINES = H.TABLE_ENGINES          # (helpers.set_engine: what each of them routes the window with)


def golden(short, key):
    return (NET if short else NET_GENERAL)[("short" if short else "general") + "_long_" + key]


def da_case(nts, short):
    return dict(case=TR.reservoir_case(), nts=nts, short=short)


def tables(t_shift=0.0, state=None, rfc_rows=None, order_by_lake=False):
    """the 23 reservoir data-assimilation arguments of compute_network_structured from the fixture's tables; t_shift: seconds
    the window starts after the fixture's t0 (observation times are relative to the window's start); state: the (usgs, usace,
    rfc) tuples a window before returned"""
    out = []
    for k, name in enumerate(("usgs", "usace")):
        obs, idx, time = NET[f"{name}_obs"], NET[f"{name}_idx"], NET[f"{name}_time"] - np.float32(t_shift)
        if state is None:
            ut, prev, index, put = NET[f"{name}_update_time"], NET[f"{name}_prev"], NET[f"{name}_index"], NET[f"{name}_put"]
        else:
            sidx, ut, prev, index, put = state[k]
            assert np.array_equal(sidx, idx)
        o = np.argsort(idx, kind="stable") if order_by_lake else np.arange(len(idx))
        out += [obs[o], idx[o], time, ut[o], prev[o], put[o], index[o]]
    rows = np.arange(len(NET["rfc_idx"])) if rfc_rows is None else np.asarray(rfc_rows)
    if state is None:
        ut, ts_idx = NET["rfc_update_time"], NET["rfc_ts_idx"]
    else:
        sidx, ut, ts_idx = state[2]
        assert np.array_equal(sidx, NET["rfc_idx"])
    out += [NET["rfc_obs"][rows], NET["rfc_idx"][rows], NET["rfc_total"][rows], [""] * len(rows), NET["rfc_use"][rows], ts_idx[rows],
            ut[rows], NET["rfc_da_dt"][rows], NET["rfc_days"][rows]]
    return out


def da_args(c, types=None, tables_=None, q0=None, ql=None, rfc_rows=None, order_by_lake=False, with_tables=True):
    from troute_amd.routing.fast_reach.mc_reach import mc_only_args
    lc, ids, dv, ql0, q00, reaches, net, lakes, wbody_cols, lakeset, _ = c["case"]
    args = mc_only_args(c["nts"], lc.dt, lc.qts, reaches, net, ids, lc.data_cols, dv, q00 if q0 is None else q0,
                        ql0 if ql is None else ql, assume_short_ts=c["short"])
    args[3] = [(r, 1 if r[0] in lakeset else 0) for r in reaches]
    args[10] = lakes.tolist()
    args[11] = wbody_cols if "wbody_cols" not in c else c["wbody_cols"]
    args[13] = np.asarray(NET["types"] if types is None else types, np.int32).reshape(-1, 1)
    args[14] = True
    if with_tables:
        args[23:46] = tables(rfc_rows=rfc_rows, order_by_lake=order_by_lake) if tables_ is None else tables_
    return args[:57]          # (positional through assume_short_ts)


def check_against_golden(r, short, nts_from=0, nts_to=NTS):
    """rows stored in full, every 12th step of every row, the lakes' inflow series -- steps (nts_from, nts_to] of the long window"""
    n = r[1].shape[0]
    fvd = r[1].reshape(n, nts_to - nts_from, 3)
    full = golden(short, "full")[:, nts_from:nts_to]
    assert np.array_equal(fvd[NET["full_rows"]].view(np.uint32), full.view(np.uint32))
    dec = golden(short, "dec")                                   # steps 12, 24, ...
    keep = [k for k in range(dec.shape[1]) if nts_from < 12 * (k + 1) <= nts_to]
    got = fvd[:, [12 * (k + 1) - 1 - nts_from for k in keep]]
    assert np.array_equal(got.view(np.uint32), dec[:, keep].view(np.uint32))
    row = {int(s): i for i, s in enumerate(r[0])}
    lake_rows = np.array([row[int(l)] for l in NET["lakes"]])
    assert np.array_equal(r[6][lake_rows].view(np.uint32), golden(short, "inflow")[:, nts_from:nts_to].view(np.uint32))


def check_state(r, short):
    for j, name in ((4, "usgs"), (5, "usace"), (7, "rfc")):
        for i, a in enumerate(r[j]):
            want = golden(short, f"state_{name}_{i}")
            assert a.dtype == want.dtype and np.array_equal(a, want, equal_nan=True), (name, i, a, want)


@pytest.mark.gpu
@pytest.mark.parametrize("short,engine", ENGINES)
def test_gpu_reservoir_da_bit_identical_to_reference_loop(short, engine, monkeypatch):
    clusters = H.set_engine(engine, monkeypatch)
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    c = da_case(NTS, short)
    r = compute_network_structured(*da_args(c), from_files=False, return_stats=True)
    if clusters:
        H.cluster_stats(r[-1], engine, NTS)
    check_against_golden(r, short)
    check_state(r, short)
    assert set(NET["types"].tolist()) == {1, 2, 3, 4, 5}


@pytest.mark.gpu
@pytest.mark.parametrize("short", [True, False])
def test_gpu_empty_tables_and_demoted_types_equal_level_pool(short):
    """no table, every type demoted to 1 (what _prep_reservoir_da_dataframes does with empty DataFrames): today's result"""
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    c = da_case(24, short)
    demoted = compute_network_structured(*da_args(c, types=np.ones_like(NET["types"]), with_tables=False), from_files=False)
    args = da_args(c, with_tables=False)
    args[13], args[14] = np.ones((len(NET["types"]), 1), np.int32), False       # (as test_reservoirs routes level pools)
    plain = compute_network_structured(*args)
    assert np.array_equal(demoted[1].view(np.uint32), plain[1].view(np.uint32)) and np.array_equal(demoted[6], plain[6])
    for j in (4, 5, 7):
        assert all(len(a) == 0 for a in demoted[j])


@pytest.mark.gpu
@pytest.mark.parametrize("short,engine", [(True, None), (False, None), (True, "levels-mid"), (True, "levels-clusters"),
                                          (True, "levels-slices+clusters")])
def test_gpu_two_windows_equal_one_long_window(short, engine, monkeypatch):
    """the reference's run-set loop: window 2 starts from window 1's last column (new_q0), its final pool elevations and the
    state tuples it returned, with the observation times counted from the new start -- and lands on the one long window"""
    clusters = H.set_engine(engine, monkeypatch)
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    half = NTS // 2
    c = da_case(half, short)
    lc, ids, dv, ql, q0, reaches, net, lakes, wbody_cols, lakeset, _ = c["case"]
    r1 = compute_network_structured(*da_args(c), from_files=False, return_stats=True)
    if clusters:
        H.cluster_stats(r1[-1], engine, half)
    check_against_golden(r1, short, 0, half)
    n = len(ids)
    last = r1[1].reshape(n, half, 3)[:, -1]
    q0_2 = np.stack([last[:, 0], last[:, 0], last[:, 2]], axis=1).astype(np.float32)      # AbstractNetwork.new_q0
    row = {int(s): i for i, s in enumerate(ids)}
    lake_rows = np.array([row[int(l)] for l in lakes])
    wb2 = wbody_cols.copy()
    wb2[:, 9] = last[lake_rows, 0]                 # qd0 and h0 of the waterbodies (update_waterbody_water_elevation)
    wb2[:, 10] = last[lake_rows, 2]
    c2 = dict(c, wbody_cols=wb2)
    assert half % lc.qts == 0
    ql2 = ql[:, half // lc.qts:]
    t2 = tables(t_shift=half * lc.dt, state=(r1[4], r1[5], r1[7]))
    r2 = compute_network_structured(*da_args(c2, tables_=t2, q0=q0_2, ql=ql2), from_files=False, return_stats=True)
    if clusters:
        H.cluster_stats(r2[-1], engine, half)
    check_against_golden(r2, short, half, NTS)
    check_state(r2, short)


@pytest.mark.gpu
def test_gpu_reservoir_da_refusals():
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    c = da_case(12, True)
    with pytest.raises(NotImplementedError, match="from_files=True"):
        compute_network_structured(*da_args(c))                                     # (from_files defaults to True)
    with pytest.raises(NotImplementedError, match="precision 64"):
        compute_network_structured(*da_args(c), from_files=False, precision=64)
    t = NET["types"].copy()
    t[t == 1] = 6
    with pytest.raises(NotImplementedError, match="reservoir type 6"):
        compute_network_structured(*da_args(c, types=t), from_files=False)
