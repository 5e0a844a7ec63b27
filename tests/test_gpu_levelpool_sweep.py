"""THE LEVEL POOL IN EVERY REGIME ON EVERY KERNEL THAT STEPS IT (csrc/levelpool.hpp; its call sites: k_mc_step, the tile row of
k_mc_tile / k_mc_ctile, both sites of the dataflow kernel, the day stream).  One small network of independent basins
headwater(s) -> lake A -> channel -> lake B -> outlet channel (levelpool_cases.network_case: 68 basins, about 400 rows, 48
steps) whose pools fill from dead, drain through the orifice and the weir, overtop and come back within a step or two; the
expected values are the oracle's (oracle.network_by_segment(..., det=True, res=)), bit for bit.

What the case reaches is a condition, checked WITHOUT a device (test_the_device_case_meets_its_conditions): every value of
the oracle is finite -- the classes of the CPU sweep that produce NaN stay there, no NaN is handed to the secant iteration of
a row below a lake -- and the census of the lakes' steps, taken from the oracle's inflow record through
levelpool_cases.classify, holds every branch at stage 1 and at the final evaluation, every start -> end crossing, both zero
coefficients the drop-in can carry (it fixes dam_length at 10), area = 0 and every exact edge at least three times on the
upper lakes and on the lower lakes; and the pools that part `dh > 0` from `dh >= 0` (levelpool_cases.dry_weir_basin).

Precision 64 is out of scope: the oracle restates reservoirs for float32 only (oracle._res_struct), as the reference has
them, so there is nothing to hold a double-precision pool against."""
import numpy as np
import pytest

import helpers as H
import levelpool_cases as LC
from oracle import oracle as O

bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731


def test_the_device_case_meets_its_conditions():
    c = LC.network_case()
    assert c.lakes.shape[0] == 2 * (len(LC.NET_BASINS) + len(LC.NET_DRY_WEIR_BASINS)) and 300 < c.n < 450
    assert np.count_nonzero(np.diff(c.up_ptr)[c.lakes] == 2) >= 5          # lakes below a junction of two headwaters
    cold = LC.network_cold()
    long_ts = LC.route_oracle(c, LC.NET_STEPS, c.qlat, c.q0, c.h0, short=False)
    for what, arrays in (("window", (c.fvd, c.inflow, c.h_final)), ("window, long timestep", long_ts),
                         ("cold start", (cold.fvd, cold.inflow, cold.h_final)),
                         ("days", [a for day in LC.network_days() for a in day])):
        assert all(np.isfinite(a).all() for a in arrays), what
    for lower in (False, True):
        cen = LC.lake_census(c, c.fvd, c.inflow, c.is_b == lower)
        print("lake B" if lower else "lake A")
        print(LC.census_table(cen))
        for key, n in LC.network_needs(cen).items():
            assert n >= LC.NET_MIN_COUNT, (lower, key, n)
    assert LC.dry_weir_steps(c, c.fvd) >= 4 * LC.NET_STEPS               # four pools that never leave the crest of their dry weir
    # the cold starts: ifd = 1 lands on the crest exactly and does not overtop; all three fractions occur
    on_crest = cold.ifd == 1
    assert np.array_equal(cold.h0[on_crest], cold.par[on_crest, 1]) and on_crest.sum() >= 40
    assert sorted(set(cold.ifd.tolist())) == [0.0, 0.5, 1.0]
    s = LC.classify_series(cold.par, np.full(cold.lakes.shape[0], LC.NET_DT, np.float32), cold.h0, cold.inflow)
    assert (s["branch"][on_crest, 0, 0] < LC.OVERTOP).all()


# ---- the drop-in on every engine ---------------------------------------------------------------------------------------------
def dropin_args(c, short, h0_column):
    """compute_network_structured's arguments for the case: every row a reach of its own (lakes must be), ids = rows"""
    from troute_amd.routing.fast_reach.mc_reach import mc_only_args
    order = np.argsort(c.level, kind="stable")
    reaches = [[int(r)] for r in order]
    net = {r: list(c.ups[r]) for r in range(c.n)}
    ids = np.arange(c.n, dtype=np.int64)
    cols = dict(zip(O.PARAM_COLS, c.params.T), alt=np.zeros(c.n, np.float32))
    dv = np.stack([cols[k] for k in H.DATA_COLS], 1).astype(np.float32)
    lakeset = set(c.lakes.tolist())
    args = mc_only_args(LC.NET_STEPS, LC.NET_DT, LC.NET_QTS, reaches, net, ids, np.array(H.DATA_COLS, dtype=object), dv,
                        np.zeros((c.n, 3), np.float32), c.qlat, assume_short_ts=short)
    args[3] = [(r, 1 if r[0] in lakeset else 0) for r in reaches]
    args[10] = c.lakes.tolist()
    nres = c.lakes.shape[0]
    ifd = getattr(c, "ifd", np.zeros(nres))
    #   LkArea LkMxE OrificeA OrificeC OrificeE WeirC WeirE WeirL ifd qd0 h0
    args[11] = np.concatenate([c.par[:, :8].astype(np.float64), np.asarray(ifd, np.float64)[:, None], np.zeros((nres, 1)),
                               np.asarray(h0_column, np.float64)[:, None]], 1)
    args[13] = np.ones((nres, 1), np.int32)
    args[14] = False
    return args


def assert_window(r, c, fvd_want, inflow_want, h_final):
    fvd = r[1].reshape(c.n, LC.NET_STEPS, 3)
    bad = np.flatnonzero((bits(fvd) != bits(fvd_want)).reshape(c.n, -1).any(axis=1))
    assert bad.size == 0, ("rows", bad[:16].tolist(), "lakes among them", np.intersect1d(bad, c.lakes)[:16].tolist())
    assert np.array_equal(bits(r[6][c.lakes]), bits(inflow_want))         # upstream_array rows of the lakes
    assert not fvd[c.lakes, :, 1].any()                                   # velocity slot of a reservoir row
    assert np.array_equal(bits(fvd[c.lakes, -1, 2]), bits(h_final))       # final pool elevations


@pytest.mark.gpu
@pytest.mark.parametrize("short,engine", H.TABLE_ENGINES)
def test_gpu_levelpool_regimes_bit_identical_to_oracle(short, engine, monkeypatch):
    """engine: helpers.set_engine -- both sites of the dataflow kernel, k_mc_step, k_mc_tile in one and two tiers, k_mc_ctile
    with and without slices (levels of 81 .. 45 rows are slices there, the last level of 9 rows a cluster level).  Warm
    start: the exact bits of every starting elevation in the waterbody table's h0 column."""
    clusters = H.set_engine(engine, monkeypatch)
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    c = LC.network_case()
    want = (c.fvd, c.inflow, c.h_final) if short else LC.route_oracle(c, LC.NET_STEPS, c.qlat, c.q0, c.h0, short=False)
    r = compute_network_structured(*dropin_args(c, short, c.h0), return_stats=True)
    if clusters:
        H.cluster_stats(r[-1], engine, LC.NET_STEPS)
    assert_window(r, c, *want)


@pytest.mark.gpu
def test_gpu_levelpool_cold_starts_through_the_dropin():
    """h0 = -1e9 in the waterbody table: the drop-in forms oe + (maxh - oe) * ifd in float32 (init_levelpool_reach), ifd in
    {0, 0.5, 1}; a pool started at ifd = 1 stands on the crest exactly and must not overtop"""
    from troute_amd.routing.fast_reach.mc_reach import compute_network_structured
    c = LC.network_cold()
    r = compute_network_structured(*dropin_args(c, True, np.full(c.lakes.shape[0], -1.0e9)))
    assert_window(r, c, c.fvd, c.inflow, c.h_final)


# ---- the day stream ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_levelpool_regimes_in_a_stream_of_three_days():
    """the same case as three days of 16 steps at plan level (slices and a cluster level, 4 steps per launch): every day's
    block, reservoir_inflow product and final state against the oracle routed day by day with the elevations carried over"""
    from troute_amd import _lib
    from troute_amd.plan import RoutingPlan
    from troute_amd.sequence import pinned_like
    c = LC.network_case()
    days = LC.network_days()
    nres, ns = c.lakes.shape[0], LC.NET_DAY_STEPS
    with RoutingPlan(c.up_ptr, c.up_idx, c.params, assume_short_ts=True, engine="levels",
                     options={"cluster_rows": 24, "wide_min_rows": 32, "wide_k": 4}) as p:
        p.set_reservoirs(c.lakes, c.par, LC.NET_DT)
        p.upload_forcing(ns, days[0][0], c.q0)
        p.stream_begin(ns, LC.NET_QTS, slots=LC.NET_DAYS, full_output=True)
        info = p.stream_info()
        assert info["slots"] >= LC.NET_DAYS and info["wide_levels"] > 0 and info["cluster_levels"] > 0, info
        outs = [(_lib.result_empty((c.n, ns, 3), np.float32, always_pinned=True),
                 _lib.result_empty((nres, ns), np.float32, always_pinned=True),
                 _lib.result_empty((c.n, 3), np.float32, always_pinned=True)) for _ in range(LC.NET_DAYS)]
        for d, (ql, _, _, _) in enumerate(days):
            p.stream_push(pinned_like(ql), fvd=outs[d][0], reservoir_inflow=outs[d][1], q0=outs[d][2])
        p.stream_flush()
        for d, (_, fvd, inflow, state) in enumerate(days):
            p.stream_wait(d)
            bad = np.flatnonzero((bits(outs[d][0]) != bits(fvd)).reshape(c.n, -1).any(axis=1))
            assert bad.size == 0, (d, bad[:16].tolist())
            assert np.array_equal(bits(outs[d][1]), bits(inflow)), d
            assert np.array_equal(bits(outs[d][2]), bits(state)), d
            assert not outs[d][0][c.lakes, :, 1].any()
        p.stream_end()
