"""The inputs of tests/test_gpu_guard_edges.py really sit on the edges of the guards -- checked without a GPU.

For every fixture of the GPU test: the plain-division oracle routes it, `guard_edges.census` classifies every (row, step) with
the host mirrors of params_sane, coef_guard and fast_ok, and every class the builders meant to produce must be there, at least
MIN_PAIRS times; the mirrors must give the verdict the builder intended on every directed row; and the oracle's result must be
finite on every row (at most 1 % of the rows may be excluded, the cap of the extreme-parameter test in test_gpu_parity.py).
This is what keeps the GPU test from passing on inputs that have drifted off the edges."""
import numpy as np
import pytest

import guard_edges as G
from oracle import oracle as O

MIN_PAIRS = 8        # (row, step) pairs -- or rows at the first step, or (row, column) pairs -- every intended class must reach
MAX_EXCLUDED = 0.01  # share of rows whose oracle result may be non-finite


def finite_rows(res):
    return np.isfinite(res[:, 1:, :]).all(axis=(1, 2))


def check_finite(fx, short=True):
    fin = finite_rows(fx.oracle(short))
    print(f"{fx.name} short={short}: finite on {int(fin.sum())} of {fin.size} rows")
    assert fin.mean() >= 1.0 - MAX_EXCLUDED, (fx.name, short, float(fin.mean()))
    return fin


def test_forcing_values_sit_where_they_are_meant_to():
    v = G.forcing_values()
    dt = G.F(300.0)
    n4 = {k: G.F(x) * dt for k, x in v.items()}
    print({k: float(x).hex() for k, x in n4.items()})
    assert n4["+edge"] == G.N4_LO and n4["-edge"] == -G.N4_LO
    assert n4["+below"] == G.down(G.N4_LO)          # one unit in the last place below the bound, exactly
    assert n4["-below"] == -n4["+below"]
    assert G.u32(n4["+0"]) == 0 and G.u32(n4["-0"]) == 0x80000000
    for i, name in enumerate(G.FORCING):
        assert G.forcing_class(dt, v[name]) == i, name
        assert bool(G.coef_guard(dt, v[name])) == G.FORCING_PASSES[name], name
    # dt outside its own range fails the guard whatever the forcing
    assert not G.coef_guard(G.down(G.DT_LO), G.F(1.0)) and not G.coef_guard(G.up(G.DT_HI), G.F(1e-3))
    assert G.coef_guard(G.DT_LO, G.F(1.0)) and G.coef_guard(G.DT_HI, G.F(1e-3))


def test_starting_depths_sit_on_the_bounds_of_fast_ok():
    far = np.array([G.F(1e6)])
    for name, (d, ok) in G.start_depths().items():
        s = G.fast_ok_start(np.array([d]), far, np.array([G.F(18.0)]))
        assert bool(s["ok0"][0] and s["ok1"][0]) == ok, name
    sd = G.start_depths()
    at = lambda name: G.fast_ok_start(np.array([sd[name][0]]), far, far)  # noqa: E731
    assert at("h0=lo")["h0"][0] == G.H_LO and at("h0=lo+1ulp")["h0"][0] == G.up(G.H_LO)
    # the nearest h_0 below the bound: two units below it, and the next depth up already gives the bound
    assert at("h0=lo-2ulp")["h0"][0] == G.down(G.H_LO, 2) and G.up(sd["h0=lo-2ulp"][0]) * G.F(0.67) >= G.H_LO
    assert at("h=hi")["h"][0] == G.H_HI and at("h=hi-1ulp")["h"][0] == G.down(G.H_HI) and at("h=hi+1ulp")["h"][0] == G.up(G.H_HI)
    for fp in (True, False):
        p = G.bank_channel(fp)[None, :]
        bfd = G.bankfull(p)
        assert bfd[0] == G.BFD_EXACT
        for name, d in G.bank_depths().items():
            s = G.fast_ok_start(np.array([d]), bfd, p[:, G.P_TWCC])
            k = G.BANK_EDGES[name]
            assert s["raw0"][0] == G.F(k * 2.0 ** -32), name
            # with a flood plain an over-bank depth inside (0, 2**-30) fails; without one the trapezoid goes on and it holds
            assert bool(s["ok0"][0]) == (not fp or k in (0, 4)), (name, fp)
            assert bool(s["ok1"][0]), (name, fp)


def test_parameter_variants_and_the_rows_one_ulp_outside():
    for label, p in G.bound_variants():
        assert G.params_sane(p[None, :])[0], label
    assert len(G.bound_variants()) == 2 * len(G.SWEPT) + 4 + 5
    for name, side in G.OUTSIDE_CASES:
        out, twin = G.outside(name, side), G.outside(name, side, inside=True)
        sane = G.params_sane(out.params)
        assert not sane[G.OUTSIDE_ROW] and sane.sum() == G.OUTSIDE_NSEG - 1, (name, side)
        assert G.params_sane(twin.params).all(), (name, side)
        differ = np.argwhere(G.u32(out.params) != G.u32(twin.params))
        assert differ.tolist() == [[G.OUTSIDE_ROW, G.BOUNDS[name][0]]], (name, side)
        col = G.BOUNDS[name][0]
        bound = G.BOUNDS[name][1 if side == "lo" else 2]
        assert twin.params[G.OUTSIDE_ROW, col] == bound
        assert out.params[G.OUTSIDE_ROW, col] == (G.down(bound) if side == "lo" else G.up(bound))
        for short in (True, False):
            for fx in (out, twin):
                fin = finite_rows(fx.oracle(short))
                assert fin.all(), (fx.name, short, np.flatnonzero(~fin))


def day_state(day):
    """the state the stream of days hands day `day`: new_q0 = (q_T, q_T, depth_T) of the day before, from the oracle"""
    state = G.interleaved(0).q0
    for d in range(day):
        fx = G.interleaved(d)
        res = fx.oracle(True) if d == 0 else fx.oracle(True, qlat=fx.qlat, q0=state)
        state = np.ascontiguousarray(np.stack([res[:, -1, 0], res[:, -1, 0], res[:, -1, 2]], axis=1))
    return state


@pytest.mark.parametrize("day", [0, 1, 2])
def test_interleaved_fixture_census(day):
    fx = G.interleaved(day)
    q0 = day_state(day)
    assert G.params_sane(fx.params).all()
    # the forcing is what the schedule says, and every ordered pair of classes meets between consecutive columns
    dt = np.broadcast_to(fx.params[:, G.P_DT][:, None], fx.qlat.shape)
    assert np.array_equal(G.forcing_class(dt, fx.qlat), fx.cls)
    assert np.array_equal(G.coef_guard(dt, fx.qlat), np.array([G.FORCING_PASSES[n] for n in G.FORCING])[fx.cls])
    pairs = G.pair_census(fx.params, fx.qlat)
    print("ordered class pairs, fewest (row, column) pairs:", int(pairs.min()))
    assert pairs.min() >= MIN_PAIRS
    # a change of class at every column boundary, i.e. at steps 4, 7, ..., 22: inside, first and last in a tile for tiles of 7 and,
    # under the level skew, of 8 steps
    changes = (fx.cls[:, 1:] != fx.cls[:, :-1]).sum(axis=0)
    assert (changes >= 100 * MIN_PAIRS).all(), changes
    assert (fx.cls == fx.cls[:, :1]).all(axis=1).sum() >= 10 * MIN_PAIRS      # rows that keep one class for the whole window
    for short in (True, False):
        if day and not short:
            continue        # (the stream of days routes short timesteps only)
        res = fx.oracle(short) if day == 0 else fx.oracle(True, qlat=fx.qlat, q0=q0)
        fin = finite_rows(res)
        print(f"{fx.name} short={short}: finite on {int(fin.sum())} of {fin.size} rows")
        assert fin.mean() >= 1.0 - MAX_EXCLUDED
        c = G.census(fx.params, fx.qlat, q0, res, fx.qts)
        print(fx.name, short, c)
        for name in G.FORCING:
            assert c["ql:" + name] >= MIN_PAIRS, name
        for name in ("guard:pass", "guard:fail", "fast:both", "fast:neither-or-one", "inbank-fast", "over-bank", "h0<lo", "h>hi", "flow"):
            assert c[name] >= MIN_PAIRS, name
        if day:
            continue
        flags = G.census_flags(fx.params, fx.qlat, fx.q0, res, fx.qts)
        first = {k: v[:, 0] for k, v in flags.items()}
        # the directed depths: at the first step every such row is in the class it was built for (and the step is solved)
        want = {"depth:h0=lo": "h0=lo", "depth:h0=lo-2ulp": "h0=lo-2ulp", "depth:h0=lo+1ulp": "h0=lo+1ulp", "depth:h=hi": "h=hi",
                "depth:h=hi-1ulp": "h=hi-1ulp", "depth:h=hi+1ulp": "h=hi+1ulp", "depth:dry": "h0<lo", "depth:h0<<lo": "h0<lo",
                "depth:ordinary": "fast:both"}
        for kind in ("flood-plain", "extended"):
            want[f"depth:over0=0:{kind}"] = "over0=0@bank"
            want[f"depth:over0=1ulp:{kind}"] = "over0=1ulp"
            want[f"depth:over0=2ulp:{kind}"] = f"over0-tiny:{kind}"
            want[f"depth:over0=lo:{kind}"] = f"over0=lo:{kind}"
        assert set(want) == {k for k in fx.intent if k.startswith("depth:")}
        for label, flag in want.items():
            rows = fx.intent[label]
            assert rows.size >= MIN_PAIRS and first[flag][rows].all() and first["flow"][rows].all(), (label, rows.size)
            assert fin[rows].all(), label
        sd = G.start_depths()
        for label, (_, ok) in sd.items():
            rows = fx.intent["depth:" + label]
            assert (first["fast:both"][rows] == ok).all(), label
        for kind, fp in (("flood-plain", True), ("extended", False)):
            for edge, k in G.BANK_EDGES.items():
                rows = fx.intent[f"depth:{edge}:{kind}"]
                assert (first["fast:both"][rows] == (not fp or k in (0, 4))).all(), (edge, kind)
        # the parameter variants: each on at least MIN_PAIRS rows, every one of them finite
        for label, _ in G.bound_variants():
            rows = fx.intent["par:" + label]
            assert rows.size >= MIN_PAIRS and fin[rows].all(), label
        # the rows built for the retry branch of the secant loop enter it at the first step (more than 100 iterations)
        rows = fx.intent["retry"]
        _, iters = O.segments(G.step_inputs(fx, res, 1, rows), return_iters=True, det=True)
        print("retry rows, iterations of the first step:", iters.tolist())
        assert rows.size >= MIN_PAIRS and (iters > 100).all() and fin[rows].all()
        # the negative forcing larger than the routed water empties rows (the -w clamp and the q_lo select), the smaller one does not
        q = res[:, 1:, 0]
        big, small = flags["ql:-big"] & flags["flow"], flags["ql:-small"] & flags["flow"]
        assert (q[big] == 0).sum() >= MIN_PAIRS and (q[small] > 0).sum() >= MIN_PAIRS


@pytest.mark.parametrize("name", G.UNIFORM_CLASSES)
def test_uniform_fixture_census(name):
    fx = G.uniform(name)
    assert G.params_sane(fx.params).all()
    for short in (True, False):
        fin = check_finite(fx, short)
        assert fin.all()
        flags = G.census_flags(fx.params, fx.qlat, fx.q0, fx.oracle(short), fx.qts)
        c = {k: int(v.sum()) for k, v in flags.items()}
        print(fx.name, short, c)
        assert c["ql:" + name] == G.NSEG * G.NSTEPS
        assert c["guard:pass" if G.FORCING_PASSES[name] else "guard:fail"] == G.NSEG * G.NSTEPS
        # every row in bank and in fast_ok's range at the first step, and solved: every wavefront takes the uniform branch there
        assert flags["inbank-fast"][:, 0].all() and flags["flow"][:, 0].all()


def test_single_steps_are_finite_and_reach_the_retry_branch():
    x, labels = G.single_steps()
    out, iters = O.segments(x, return_iters=True, det=True)
    whole = np.isfinite(out).all(axis=1)
    print(f"{x.shape[0]} directed single steps, at most {int(iters.max())} secant iterations, {int((iters > 100).sum())} of them in the "
          f"retry branch; every output finite on {int(whole.sum())} rows")
    # the step's own outputs (flow, velocity, depth, weighting factor) are finite on EVERY row; the unguarded Courant outputs of
    # this entry point (celerity, Courant number) are NaN for a dry result and for ncc == 0, in the reference as here -- the
    # GPU test compares those rows too, and asks for the same non-finite elements
    assert np.isfinite(out[:, [0, 1, 2, 5]]).all()
    assert whole.mean() > 0.9
    out64 = O.segments(x.astype(np.float64))
    assert np.isfinite(out64[:, [0, 1, 2, 5]]).all()
    assert x.shape[0] == len(labels) and x.shape[0] >= 1000
    # every forcing class, parameter variant and depth is there, with the verdict meant for it
    fc = G.forcing_class(x[:, 0], x[:, 4])
    assert np.array_equal(fc, np.array([G.FORCING.index(lab[1]) for lab in labels]))
    assert len({lab[0] for lab in labels}) == len(G.bound_variants()) + 3
    assert G.params_sane(x[:, [0, 5, 6, 7, 8, 9, 10, 11, 12]]).all()
    # the retry branch of the secant loop (more than 100 iterations; csrc/mc_segment.hpp, step_solve) IS reached: by the all-low
    # channel with n4 on the bound and right below it
    assert (iters > 100).sum() >= 2
    assert {labels[i][:2] for i in np.flatnonzero(iters > 100)} >= {("all-lo", "+edge"), ("all-lo", "+below")}


def test_fp64_oracle_of_the_interleaved_fixture_is_finite():
    fx = G.interleaved(0)
    assert finite_rows(fx.oracle(True, 64)).mean() >= 1.0 - MAX_EXCLUDED
