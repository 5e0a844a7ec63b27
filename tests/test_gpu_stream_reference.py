"""A stream of days at the STREAM'S OWN plan options (ShardedRouter(..., stream=True) with no options: cluster_rows 128,
wide_min_rows 1024, wide_levels 32, 16 steps per tile) against the reference, value by value, day after day with the state
handed on as new_q0 does (AbstractNetwork.py:177-191) -- the kernels bench.py times (products only: the LAZYV instances of
k_mc_tile / k_mc_ctile), the hourly block and the full result, on a network where the defaults give slices AND clusters, and
at the edges of the stream: forcing columns against the tile boundaries, the cluster and slice thresholds, a ring of day
slots deeper than eight days, forcing from ordinary (pageable) host memory."""
import numpy as np
import pytest

import helpers as H
from oracle import oracle as O
from test_gpu_parity import assert_bit_identical, synth_inputs
from troute_amd import _lib, synthetic
from troute_amd.distributed import ShardedRouter, restrict_csr
from troute_amd.plan import topology_levels
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu


def oracle_days(to, params, days, q0, nsteps, qts):
    """the oracle's (q, v, d) of every day [nseg, nsteps + 1, 3], chained as new_q0 does"""
    up_ptr, up_idx = synthetic.upstream_csr(to)
    lvl, _, _ = topology_levels(up_ptr, up_idx)
    state, out = np.ascontiguousarray(q0), []
    for ql in days:
        w = O.network_by_segment(nsteps, qts, up_ptr, up_idx, lvl, params, state, ql, True, det=params.dtype == np.float32)
        out.append(w)
        state = np.ascontiguousarray(w[:, -1, :][:, [0, 0, 2]])
    return out


def check_days(rows, got, want, stride=None, full=False, what=""):
    """every day's products against the oracle's (q, v, d) of that day"""
    for w, ref in enumerate(want):
        assert_bit_identical(got[w][0], ref[rows, 1:, 0], f"{what} day {w}: outlet hydrographs")
        assert_bit_identical(got[w][1], ref[:, -1, :][:, [0, 0, 2]], f"{what} day {w}: final state")
        if stride:
            assert_bit_identical(got[w][2], ref[:, 1:][:, stride - 1::stride], f"{what} day {w}: every {stride}th (q, v, d)")
        if full:
            assert_bit_identical(got[w][2], ref[:, 1:], f"{what} day {w}: every (q, v, d)")


def chains(lengths):
    """a forest of unbranched chains of the given lengths (row i flows into row i + 1 of its chain)"""
    parts, base = [], 0
    for n in lengths:
        t = np.arange(base + 1, base + n + 1, dtype=np.int64)
        t[-1] = -1
        parts.append(t)
        base += n
    return np.concatenate(parts)


# ---- B. a mid-size CONUS-shaped network at the stream's defaults, cost-hinted, against the reference ----------------------
NSTEPS_B, QTS_B = 96, 12            # 8 forcing columns of 12 steps across 6 tiles of 16: columns change inside tiles


@pytest.fixture(scope="module")
def mid():
    net = synthetic.generate(nseg=120000, nnet=120, seed=7, nq=NSTEPS_B // QTS_B)
    to, params = net["to"], net["params"]
    nseg = to.shape[0]
    q0 = np.zeros((nseg, 3), np.float32)
    qlat_s = net["qlat"]
    qlat_a = synthetic.forcing(nseg, qlat_s.shape[1], 8, previous=qlat_s)
    # the tuning window of bench.py: day N-1 cold, day N warm with cost collection; the stream starts from day N's state
    r = ShardedRouter(to, params, assume_short_ts=True)
    r.upload(NSTEPS_B, qlat_s, q0)
    r.route_resident(QTS_B, True)
    r.upload(NSTEPS_B, qlat_a, None)
    r.collect_cost(True)
    r.route_resident(QTS_B, True)
    hint = r.iteration_hint()
    state_n = r.plan0.download_final_state()
    r.close()
    rng = np.random.default_rng(9)
    bf = (params[:, 3] - params[:, 2]) * params[:, 7] / 2       # bankfull depth (tw - bw) / (2 z), z = 1 / cs

    def day(k, prev):
        """persistent days, then independently redrawn ones, a flood day, an all-zero day, then persistent again"""
        if k in (3, 4):
            return synthetic.forcing(nseg, qlat_s.shape[1], 100 + k)
        if k == 5:
            return (prev * np.float32(400.0) + rng.uniform(0, 30, prev.shape)).astype(np.float32)
        if k == 6:
            return np.zeros_like(prev)
        return synthetic.forcing(nseg, qlat_s.shape[1], 100 + k, previous=prev if prev.any() else qlat_a)
    days = []

    def make_day(k):
        if k >= len(days):
            days.append(day(k, days[-1] if days else qlat_a))
        return days[k]
    return dict(to=to, params=params, hint=hint, state_n=state_n, make_day=make_day, days=days, bf=bf)


def test_mid_stream_at_its_own_options_equals_the_reference_every_day(mid):
    """Products only (the timed instances), the hourly block and the full result of the same days on ONE cost-hinted stream
    router at the stream's defaults: every day's outlet hydrographs, final state and kept (q, v, d) against the reference
    routed on the CPU (the reference Fortran's flows of every row at every step; its velocity and depth series by exact
    checksums), through persistent, redrawn, flood and all-zero days, the ring of day slots wrapping."""
    to, params = mid["to"], mid["params"]
    r = ShardedRouter(to, params, cost_hint=mid["hint"], stream=True)
    P = r.stream_plan(0)
    lag, W, C = P.lags()
    assert W > 0 and C > 0
    hot0 = P.hot_rows()
    rows, prod, days, info = H.stream_days(r, mid["make_day"], NSTEPS_B, QTS_B, mid["state_n"], extra=2, min_days=8)
    hot1 = P.hot_rows()
    assert hot1 > hot0, "the stream never routed a row from the hot list"
    assert info["tiles_per_day"] == NSTEPS_B // 16 and info["wide_levels"] == W and info["cluster_levels"] == C
    assert len(days) >= 8                                         # (every regime of the day sequence is among them)
    _, hourly, _, _ = H.stream_days(r, lambda k: days[k], NSTEPS_B, QTS_B, mid["state_n"], ndays=len(days), output_stride=12)
    _, full, _, _ = H.stream_days(r, lambda k: days[k], NSTEPS_B, QTS_B, mid["state_n"], ndays=len(days), full_output=True)
    r.close()
    over = 0
    for w, (q, state, (chk_v, chk_d)) in enumerate(H.reference_day_by_day(to, params, days, mid["state_n"], NSTEPS_B, QTS_B,
                                                                          checksums=True)):
        assert_bit_identical(prod[w][0], q[rows, 1:], f"day {w}: outlet hydrographs (products only)")
        assert_bit_identical(prod[w][1], state, f"day {w}: final state (products only)")
        assert_bit_identical(hourly[w][0], prod[w][0], f"day {w}: outlet hydrographs (hourly)")
        assert_bit_identical(hourly[w][1], state, f"day {w}: final state (hourly)")
        assert_bit_identical(hourly[w][2][:, :, 0], q[:, 12::12], f"day {w}: hourly flows")
        assert_bit_identical(full[w][2][:, :, 0], q[:, 1:], f"day {w}: every flow")
        assert np.array_equal(O.series_checksum(full[w][2][:, :, 1]), chk_v), f"day {w}: velocity series of some row"
        assert np.array_equal(O.series_checksum(full[w][2][:, :, 2]), chk_d), f"day {w}: depth series of some row"
        assert_bit_identical(hourly[w][2][:, :, 1:], full[w][2][:, 11::12, 1:], f"day {w}: hourly velocity and depth")
        assert_bit_identical(full[w][1], state, f"day {w}: final state (full result)")
        if w == 5:
            over = int((full[w][2][:, :, 2] > mid["bf"][:, None]).any(axis=1).sum())
        if w == 6:
            assert np.all(days[w] == 0)
    assert over > 100, over                                      # (the flood day goes over bank)
    print(f"\nmid stream: W={W} C={C} tiles_per_day={info['tiles_per_day']} slots={info['slots']} lag_max={info['lag_max']} "
          f"days={len(days)} hot_rows {hot0}->{hot1} over_bank_rows={over}")


def test_mid_stream_fp64_products_only_equals_the_fp64_oracle(mid):
    """The fp64 products-only stream (k_mc_tile<double, ..., LAZYV>) on the same network through stream_push(hyd=, q0=), the
    ring wrapping, against the fp64 oracle: the rows of a sample of whole networks (independent networks do not interact),
    their outlet hydrographs and final state every day."""
    to, params = mid["to"], mid["params"]
    days = [mid["make_day"](k) for k in range(9)]
    up_ptr, up_idx = synthetic.upstream_csr(to)
    from troute_amd import sharding
    _, lab = np.unique(sharding.outlet_of(to), return_inverse=True)
    sizes = np.bincount(lab)
    keep = np.argsort(sizes)[:-1]                                # every network but the largest: the second one's deep levels
    sample = np.flatnonzero(np.isin(lab, keep))                  # are in the clusters too
    assert 20000 < sample.size < 80000
    r = ShardedRouter(to, params, cost_hint=mid["hint"], stream=True, precision=64)
    P = r.stream_plan(0)
    assert P.dtype == np.float64
    lag, W, C = P.lags()
    assert W > 0 and C > 0
    assert np.array_equal(r.rows0, np.arange(to.shape[0]))
    outl = r.my_out0_local
    rs = P.rowset(outl)
    state0 = mid["state_n"].astype(np.float64)
    P.upload_forcing(NSTEPS_B, days[0].astype(np.float64), state0)
    P.stream_begin(NSTEPS_B, QTS_B)
    info = P.stream_info()
    D, tpd = info["slots"], info["tiles_per_day"]
    behind = -(-info["lag_max"] // tpd) + 1                     # (a day is through this many pushes later: RouteStream)
    assert len(days) >= D + 2, D
    hyds = [_lib.result_empty((outl.size, NSTEPS_B), np.float64, always_pinned=True) for _ in range(D)]
    fins = [_lib.result_empty((to.shape[0], 3), np.float64, always_pinned=True) for _ in range(D)]
    got = {}
    done = 0
    for d, q in enumerate(days):
        P.stream_push(pinned_like(q.astype(np.float64)), rowset=rs, hyd=hyds[d % D], q0=fins[d % D])
        while done <= d - behind:
            P.stream_wait(done)
            got[done] = (hyds[done % D].copy(), fins[done % D].copy())
            done += 1
    P.stream_flush()
    while done < len(days):
        P.stream_wait(done)
        got[done] = (hyds[done % D].copy(), fins[done % D].copy())
        done += 1
    P.stream_end()
    r.close()
    g2l = np.full(to.shape[0], -1, np.int64)
    g2l[sample] = np.arange(sample.size)
    lp, li = restrict_csr(up_ptr, up_idx, sample, g2l)
    lvl, _, _ = topology_levels(lp, li)
    out_pos = np.flatnonzero(np.isin(outl, sample))
    state = np.ascontiguousarray(state0[sample])
    for w, ql in enumerate(days):
        want = O.network_by_segment(NSTEPS_B, QTS_B, lp, li, lvl, params[sample].astype(np.float64), state,
                                    ql[sample].astype(np.float64), True)
        state = np.ascontiguousarray(want[:, -1, :][:, [0, 0, 2]])
        assert_bit_identical(got[w][1][sample], state, f"fp64 day {w}: final state")
        assert_bit_identical(got[w][0][out_pos], want[g2l[outl[out_pos]], 1:, 0], f"fp64 day {w}: outlet hydrographs")
    print(f"\nfp64 stream: W={W} C={C} tiles_per_day={info['tiles_per_day']} slots={D} days={len(days)} sample={sample.size}")


# ---- C. the edges of the stream, small, against the oracle -------------------------------------------------------------------
def edge_case(case):
    """(to, params, q0, make_day, nsteps, qts, RouteStream kwargs, pinned, what to assert of the plan)"""
    rng = np.random.default_rng(EDGES.index(case))
    nsteps, qts, kw, pinned, expect = 48, 12, {}, True, {}
    if case == "nsteps16":
        t2 = H.random_network(rng, 3000)
        to = np.concatenate([chains([2500]), np.where(t2 >= 0, t2 + 2500, -1)])
        nsteps, qts, expect = 16, 4, {"slots_over": 8}
    elif case.startswith("qts"):
        to = H.random_network(rng, 6000)
        qts = {"qts1": 1, "qts3": 3, "qts16": 16, "qtsN": nsteps}[case]
    elif case.startswith("stride"):
        to = H.random_network(rng, 6000)
        kw = {"output_stride": int(case[6:])}
    elif case == "chains":
        to = chains([127, 128, 129, 127, 128, 129, 1500, 1])
        expect = {"C": True}
    elif case in ("level1023", "level1024"):
        to = chains([12] * int(case[5:]))
        expect = {"W": int(case[5:]) >= 1024}
    elif case == "levels_over_32":
        to = chains([34] * 1030)
        kw, expect = {"ndays": 3}, {"W32": True}
    elif case == "zero":
        to = H.random_network(rng, 6000)
    elif case == "dt":
        to = H.random_network(rng, 6000)
    elif case == "pageable":
        to = H.random_network(rng, 6000)
        pinned = False
    nseg = to.shape[0]
    nq = -(-nsteps // qts)
    params, _, q0 = synth_inputs(rng, nseg, nq, dt_uniform=case != "dt")
    if case == "zero":
        q0[:] = 0

    def make_day(k):
        if case == "zero":
            return np.zeros((nseg, nq), np.float32)
        return synth_inputs(np.random.default_rng(1000 + k), nseg, nq)[1]
    return to, params, q0, make_day, nsteps, qts, kw, pinned, expect


EDGES = ["nsteps16", "qts1", "qts3", "qts16", "qtsN", "stride3", "stride12", "stride16", "chains", "level1023", "level1024",
         "levels_over_32", "zero", "dt", "pageable"]


@pytest.mark.parametrize("case", EDGES)
def test_stream_edges_equal_the_oracle(case):
    to, params, q0, make_day, nsteps, qts, kw, pinned, expect = edge_case(case)
    r = ShardedRouter(to, params, stream=True)
    lag, W, C = r.stream_plan(0).lags()
    rows, got, days, info = H.stream_days(r, make_day, nsteps, qts, q0, pinned=pinned, **kw)
    r.close()
    want = oracle_days(to, params, days, q0, nsteps, qts)
    check_days(rows, got, want, stride=kw.get("output_stride"), what=case)
    if "W" in expect:
        assert (W > 0) == expect["W"], W
    if "W32" in expect:
        assert W == 32, W
    if "C" in expect:
        assert C > 1, C
    if "slots_over" in expect:
        assert info["tiles_per_day"] == 1 and info["slots"] > expect["slots_over"], info
    if case == "zero":
        for w in range(len(days)):
            assert not bits_any(got[w][0]) and not bits_any(got[w][1]), w
    print(f"\n{case}: W={W} C={C} tiles_per_day={info['tiles_per_day']} slots={info['slots']} lag_max={info['lag_max']} days={len(days)}")


def bits_any(a):
    return np.ascontiguousarray(a).view(np.uint32).any()


def test_stream_around_the_fast_division_guard_equals_the_oracle():
    """The inputs of test_extreme_parameters_and_depths_around_the_fast_division_guard (parameters over the whole admitted
    range, depths on both sides of the per-call test) through a stream at its defaults, the rows the oracle keeps finite
    compared; then one parameter outside the range, which switches the plan to plain divisions."""
    from test_gpu_parity import extreme_inputs
    nsteps, qts = 48, 16
    to, params, qlat, q0 = extreme_inputs(np.random.default_rng(78), 12000)
    params2 = params.copy()
    params2[0, 2] = np.float32(2.0 ** 18)
    params2[0, 3] = np.float32(2.0 ** 19)
    for par in (params, params2):
        r = ShardedRouter(to, par, stream=True)
        rows, got, days, info = H.stream_days(r, lambda k: (qlat * np.float32(0.5 + 0.25 * k)).astype(np.float32), nsteps, qts, q0,
                                            extra=1)
        r.close()
        want = oracle_days(to, par, days, q0, nsteps, qts)
        fin = np.ones(to.shape[0], bool)
        for w, ref in enumerate(want):
            fin &= np.isfinite(ref).all(axis=(1, 2))
            assert fin.mean() > 0.98
            assert_bit_identical(got[w][1][fin], ref[fin, -1, :][:, [0, 0, 2]], f"day {w}: final state of the finite rows")
            ok = fin[rows]
            assert_bit_identical(got[w][0][ok], ref[rows[ok], 1:, 0], f"day {w}: outlet hydrographs of the finite rows")
