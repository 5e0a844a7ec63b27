"""THE TILE SCHEDULER'S RARE PATHS (csrc/kernels_levels.inc mc_tile_rows; csrc/host_levels.inc tile_setup / tile_args / tile_turn;
csrc/stream.inc stream_launch).  Which thread routes which row of a wide tile is decided inside the launch: the in-block partition
by cost class, the three rotating hot lists with their stamp columns, the hot blocks at the front of the grid -- and, for a stream,
which of two launches on which of two streams routes a slice (stream_split).  A mistake there routes a row twice in a tile or not
at all: a plausible wrong hydrograph without a fault.  Every case here

  * compares the device's (q, v, d) BIT FOR BIT with the CPU oracle (oracle.network_by_segment(..., det=True): oracle.network with
    every row its own reach; chained day by day with new_q0's rule for consecutive windows and for streams), and
  * PROVES from the library's own report which path ran: RoutingPlan.hot_state() (trmc_plan_hot_state: the lists' lengths as
    attempted appends, their capacity, the hot blocks of the next launch), hot_rows(), stream_info()["launches"], levels().

1. a hot list that OVERFLOWS: more rows end a tile hot than a list holds -- the rest stay with their blocks, unstamped;
2. the WAVEFRONT VERDICT: a wavefront with TRMC_HOT_WAVE_MAX hot rows or more keeps them, one with fewer lists them;
3. hot_wave_rows: 8, 16, 32, 64 rows of the list per wavefront of the hot blocks, and the values outside 1..64;
4. stream_split: the slices from level s on in a launch of their own on the clusters' stream;
5. tail_sort = -1: the per-level order below the tiled levels of a hinted short-timestep plan.

The constants (threads per tile block, TRMC_HOT_WAVE_MAX, a list's capacity) are the build's, read through hot_state()."""
import functools

import numpy as np
import pytest

import guard_edges as GE
import test_gpu_ctile_block as CB
import test_gpu_stream_reservoirs_nudging as SRN
import test_gpu_tile_lean_loop as LL
import test_gpu_window_api as WA
from oracle import oracle as O
from troute_amd import _lib
from troute_amd.plan import RoutingPlan, topology_levels
from troute_amd.sequence import pinned_like

pytestmark = pytest.mark.gpu

K, QTS = 4, 4            # steps per tile launch; steps per forcing column (cases 1 and 2)
NT = 4                   # tiles of their windows: 16 steps


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def new_q0(w):
    """the state a window hands on (AbstractNetwork.new_q0): (q_T, q_T, d_T) of w [n, nsteps, 3]"""
    return np.ascontiguousarray(np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], 1))


def oracle_window(net, nsteps, qts, state, ql, dtype=np.float32):
    """[n, nsteps, 3]: the CPU restatement of the reference loop (fp32: with the deterministic power, what the device restates)"""
    up_ptr, up_idx, level, params = net
    kw = {"det": True} if dtype == np.float32 else {}
    w = O.network_by_segment(nsteps, qts, up_ptr, up_idx, level, params.astype(dtype), state.astype(dtype), ql.astype(dtype), True, **kw)
    w = np.ascontiguousarray(w[:, 1:, :])
    w.setflags(write=False)
    return w


# ---- cases 1 and 2: one wide level of independent rows, flooded BY POSITION -----------------------------------------------------
FLOOD = 300.0            # m3/s of lateral inflow into a channel a few metres wide: far over bank


@functools.lru_cache(maxsize=None)
def wide_level(rows):
    """`rows` headwaters that are their own outlets (test_gpu_tile_lean_loop.test_one_wide_level_that_ends_in_a_short_block)"""
    rng = np.random.default_rng(rows)
    to = np.full(rows, -1, np.int64)
    up_ptr, up_idx = CB.csr_of(to)
    p = np.stack([np.full(rows, 300.0), rng.uniform(500, 1500, rows), rng.uniform(2, 10, rows), np.zeros(rows), np.zeros(rows),
                  np.full(rows, 0.06), np.full(rows, 0.12), rng.uniform(0.3, 1.0, rows), rng.uniform(0.001, 0.02, rows)], 1)
    p[:, 3] = p[:, 2] * 5 / 3
    p[:, 4] = p[:, 3] * 3
    p = p.astype(np.float32)
    level = topology_levels(up_ptr, up_idx)[0]
    assert not level.any()
    for a in (up_ptr, up_idx, level, p):
        a.setflags(write=False)
    return up_ptr, up_idx, level, p


OPTS_WIDE = {"wide_min_rows": 1, "wide_k": K}


def open_wide(rows, precision=32, **extra):
    """no cost hint, level engine, TRMC_PLAN_SHORT_TS"""
    up_ptr, up_idx, level, p = wide_level(rows)
    return RoutingPlan(up_ptr, up_idx, p, assume_short_ts=True, engine="levels", precision=precision, options={**OPTS_WIDE, **extra})


def flood_by_wave(plan, per_wave):
    """the rows at the first per_wave[k] positions of wavefront k (64 consecutive positions of the level): bool [rows]"""
    lvl, pos = plan.levels()
    n = pos.shape[0]
    assert not lvl.any() and sorted(pos.tolist()) == list(range(n))   # (one level; it begins at position 0)
    assert len(per_wave) == -(-n // 64)
    row_of_pos = np.argsort(pos)
    wet = np.zeros(n, bool)
    for k, m in enumerate(per_wave):
        assert 0 <= m <= min(64, n - 64 * k)
        wet[row_of_pos[64 * k:64 * k + m]] = True
    return wet


def flood_inputs(rows, wet, nq):
    """flooded rows: FLOOD in every column, from the state the oracle reaches after 32 steps of it (from an empty channel the
    secant iteration takes some ten steps to find the flood's depth: the rows must be over bank from the FIRST step on); every
    other row: no forcing, no state -- class 0, no flow"""
    ql = np.zeros((rows, max(nq, 8)), np.float32)
    ql[wet] = np.float32(FLOOD)
    q0 = new_q0(oracle_window(wide_level(rows), 32, QTS, np.zeros((rows, 3), np.float32), ql[:, :8]))
    assert not q0[~wet].any()
    return np.ascontiguousarray(ql[:, :nq]), q0


def check_classes(rows, wet, want):
    """the kernel's own rule (class = min(iterations, 3) + 4 if over bank; hot: class >= 3): a flooded row is over bank at EVERY
    step with a clear margin, so it ends every tile in class >= 4; every other row never has any flow: class 0"""
    bfd = GE.bankfull(wide_level(rows)[3])
    assert np.all(np.isfinite(bfd)) and np.all(bfd > 0)
    for w in want:
        assert np.all(w[wet][:, :, 2] > 1.5 * bfd[wet, None]), float((w[wet][:, :, 2] / bfd[wet, None]).min())
        assert not w[~wet].any()


def prefix_windows(rows, ql, q0, want, precision=32, **extra):
    """WHAT EVERY LAUNCH OF A WINDOW READ.  All tiles of a window are queued at once, so the lists cannot be looked at between
    them.  But a window's last launch appends nothing (a row that finishes a window is not listed unless the plan is in a
    stream) and clears only the list after next: the list it READ is still there afterwards, at (cur_next + 2) % 3.  The forcing
    is constant in time, so a window of m tiles on a fresh plan is the first m launches of the window of NT tiles (and its result
    the first m K steps of the oracle's); m = 1 .. NT gives, for launch m - 1, the length of the list it read and -- hot_rows()
    being a running total -- the rows it routed from the list.  Returns (read [NT], routed [NT], cap, the state of a fresh plan)."""
    dt = np.float32 if precision == 32 else np.float64
    read, total, cap, fresh = [], [0], None, None
    for m in range(1, NT + 1):
        with open_wide(rows, precision, **extra) as plan:
            if m == 1:
                fresh = plan.hot_state()
            plan.upload_forcing(m * K, ql[:, :m].astype(dt), q0.astype(dt))
            stats = plan.route_device(m * K, QTS, True)
            assert stats["wide_levels"] == 1 and stats["wide_k"] == K and stats["wide_launches"] == m, stats
            assert np.array_equal(bits(plan.download_fvd()), bits(want[:, :m * K])), m
            st = plan.hot_state()
            assert st["cur_next"] == m % 3 and st["cap"] > 0
            cap = st["cap"]
            read.append(st["counts"][(st["cur_next"] + 2) % 3])
            total.append(plan.hot_rows())
    return read, np.diff(total).tolist(), cap, fresh


def listed_under_the_partition(hot_per_block, block, wave_max):
    """From a plan's second tile on the threads of a block take its rows by descending class: the block's h hot rows (not
    stamped) sit in its first threads, 64 to a wavefront.  A wavefront with 0 < hot rows < wave_max lists them."""
    n = 0
    for h in hot_per_block:
        for w in range(block // 64):
            in_wave = max(0, min(64, h - 64 * w))
            if 0 < in_wave < wave_max:
                n += in_wave
    return n


def cap_of(rows, block):
    """tile_setup: a list holds a 32nd of the tiled rows, in whole blocks, one block at least"""
    return max(block, -(-(rows // 32) // block) * block)


ROWS_OVER = 2048 + 2     # (a short last block of two rows: the partition's `none`, the s >= s_end exit)


@pytest.mark.parametrize("precision", [32, 64])
def test_a_hot_list_that_overflows_leaves_the_rest_with_their_blocks(precision):
    """15 flooded rows in every wavefront of 64 positions, 482 in all, into lists of 128 (rows / 32, in whole blocks).

    THE SEQUENCE, from the kernel's rules.  Launch 1 of a fresh plan: one class everywhere, the partition deals a block's rows
    in the order of one LDS counter -- a wavefront's 64 lanes draw 64 consecutive numbers, so the wavefronts of a block may trade
    places but each keeps its 64 positions and its 15 hot rows; 15 < TRMC_HOT_WAVE_MAX: EVERY flooded row is appended.  The list
    read by launch 2 has length 482 > cap: cap rows are stored and stamped, the others stay with their blocks.  Launch 2 routes
    min(482, cap) = cap rows from the list; every one of them is listed again (a row from the list always is), so the list launch
    3 reads holds cap at least -- and more wherever a block's unstamped hot rows are fewer than TRMC_HOT_WAVE_MAX, which depends
    on which appends won and is not asserted -- and so on: the launches of the first window route 0, cap, cap, cap rows from the
    lists.  The window's last launch lists nothing, so the second window's first launch reads an empty list; by then the classes
    of the tile before put a block's flooded rows into its first threads: 30 of them in the first wavefront of every full block of
    128 (>= TRMC_HOT_WAVE_MAX: kept), 2 in the short last block (listed): 0, 2, 2, 2."""
    dt = np.float32 if precision == 32 else np.float64
    rows = ROWS_OVER
    net = wide_level(rows)
    with open_wide(rows, precision) as probe:
        hs = probe.hot_state()
        block, wave_max = hs["tile_block"], hs["wave_max"]
        assert hs["cap"] == 0 and hs["counts"] == [0, 0, 0] and hs["cur_next"] == 0      # (no tiled window yet: no lists)
        assert block % 64 == 0 and 15 < wave_max <= 64
        nwaves = -(-rows // 64)
        per_wave = [min(15, rows - 64 * k) for k in range(nwaves)]
        wet = flood_by_wave(probe, per_wave)
        _, pos = probe.levels()
    nwet = int(wet.sum())
    cap = cap_of(rows, block)
    assert nwet == sum(per_wave) > cap and rows % block != 0, (nwet, cap)
    ql, q0 = flood_inputs(rows, wet, NT)
    w1 = oracle_window(net, NT * K, QTS, q0, ql, dt)
    w2 = oracle_window(net, NT * K, QTS, new_q0(w1), ql, dt)
    check_classes(rows, wet, (w1, w2))

    # (b), (c): launch by launch
    read, routed, cap_seen, _ = prefix_windows(rows, ql, q0, w1, precision)
    assert cap_seen == cap
    assert read[0] == 0 and read[1] == nwet > cap, read          # (b) the list overflowed: every flooded row asked for a place
    assert all(r >= cap for r in read[2:]), read                 # (the stored rows list themselves again, whoever else does)
    assert routed == [min(r, cap) for r in read] == [0, cap, cap, cap], (routed, read)

    # (a), (c), (d): two consecutive windows on one plan, the second from the state on the device; the cost every row collected
    hot_per_block = np.bincount(pos[wet] // block, minlength=-(-rows // block)).tolist()
    again = listed_under_the_partition(hot_per_block, block, wave_max)
    assert 0 < again <= cap
    got = {}
    for hot in (1, -1):
        with open_wide(rows, precision, hot_rows=hot) as plan:
            plan.collect_cost(True)
            res = []
            for k, (state, want) in enumerate(((q0, w1), (None, w2))):
                before = plan.hot_rows()
                plan.upload_forcing(NT * K, ql.astype(dt), None if state is None else state.astype(dt))
                stats = plan.route_device(NT * K, QTS, True)
                assert stats["wide_launches"] == NT and stats["wide_segment_steps"] == rows * NT * K, stats
                fvd = plan.download_fvd()
                assert fvd.dtype == dt and np.array_equal(bits(fvd), bits(want)), (hot, k)
                cost, nts = plan.download_cost()
                assert nts == NT * K
                res.append(cost)
                st = plan.hot_state()
                if hot > 0:
                    assert st["cap"] == cap and st["cur_next"] == (NT * (k + 1)) % 3
                    last_read = st["counts"][(st["cur_next"] + 2) % 3]
                    assert (last_read >= cap) if k == 0 else (last_read == again), (k, st)
                    assert plan.hot_rows() - before == (3 * cap if k == 0 else 3 * again), (k, plan.hot_rows(), before)
                else:
                    assert st["cap"] == 0 and plan.hot_rows() == 0
            got[hot] = res
    # (d) one addition per routing of a row and tile: a row routed twice in a launch would have counted twice.  Every step of a
    # flooded row is over bank (4) with one iteration at least; the others never iterate
    for k in range(2):
        assert np.array_equal(got[1][k], got[-1][k]), k
        assert not got[1][k][~wet].any() and np.all(got[1][k][wet] >= 5 * NT * K) and np.all(got[1][k][wet] <= 7 * NT * K)


@pytest.mark.parametrize("full_output", [False, True], ids=["products", "full_output"])
def test_an_overflowing_list_carries_over_the_days_of_a_stream(full_output):
    """The same rows and forcing as a stream of three days on a fresh plan in cluster order, twice (the second stream picks the lists up where the
    first left them).  In a stream a row that ends a day is listed like any other (seq_slots > 1): from the second launch on every
    launch reads a list of cap rows at least -- the rows routed from a list always list themselves again -- so the plan's launches
    route 0, cap, cap, ... rows from the lists over both streams, the day's ends included."""
    rows, ndays = ROWS_OVER, 3
    net = wide_level(rows)
    want = []
    with open_wide(rows, cluster_rows=64) as plan:       # (a stream needs a plan in cluster order; here it has no cluster: W = 1)
        block = plan.hot_state()["tile_block"]
        nwaves = -(-rows // 64)
        wet = flood_by_wave(plan, [min(15, rows - 64 * k) for k in range(nwaves)])
        ql, q0 = flood_inputs(rows, wet, NT)
        state = q0
        for d in range(ndays):
            want.append(oracle_window(net, NT * K, QTS, state, ql))
            state = new_q0(want[-1])
        check_classes(rows, wet, want)
        cap = cap_of(rows, block)
        rs = plan.rowset(np.arange(rows))
        launches = 0
        for turn in range(2):
            plan.upload_forcing(NT * K, ql, q0)
            plan.stream_begin(NT * K, QTS, full_output=full_output)
            keep, out = [pinned_like(ql) for _ in range(ndays)], []
            for d in range(ndays):
                hyd = _lib.result_empty((rows, NT * K), np.float32, always_pinned=True)
                fin = _lib.result_empty((rows, 3), np.float32, always_pinned=True)
                blk = _lib.result_empty((rows, NT * K, 3), np.float32, always_pinned=True) if full_output else None
                plan.stream_push(keep[d], rowset=rs, hyd=hyd, q0=fin, fvd=blk)
                out.append((hyd, fin, blk))
            plan.stream_flush()
            for d in range(ndays):
                plan.stream_wait(d)
            info = plan.stream_info()
            plan.stream_end()
            assert info["wide_levels"] == 1 and info["cluster_levels"] == 0 and info["launches"] == ndays * NT, info
            launches += info["launches"]
            for d, (hyd, fin, blk) in enumerate(out):
                assert np.array_equal(bits(hyd), bits(want[d][:, :, 0])), (turn, d)
                assert np.array_equal(bits(fin), bits(new_q0(want[d]))), (turn, d)
                if full_output:
                    assert np.array_equal(bits(blk), bits(want[d])), (turn, d)
            st = plan.hot_state()
            assert st["cap"] == cap and st["cur_next"] == launches % 3
            assert st["counts"][st["cur_next"]] >= cap, st                      # (what the day's last launch appended: carried on)
            assert plan.hot_rows() == cap * (launches - 1), (turn, plan.hot_rows(), cap, launches)


def test_a_wavefront_keeps_its_hot_rows_from_the_threshold_on():
    """Eight wavefronts of one level with MAX - 2, MAX - 1, MAX, MAX + 1, 0, 1, 63, 64 flooded positions (MAX =
    TRMC_HOT_WAVE_MAX).  Launch 1 (one class: every wavefront routes its own 64 positions, see the overflow test) lists the rows
    of the wavefronts with fewer than MAX: (MAX - 2) + (MAX - 1) + 0 + 1.  They fit the list, so all are stamped; from launch 2 on
    they are routed from the list and list themselves again, and the partition gathers every block's other flooded rows -- MAX
    and MAX + 1, 63 and 64: MAX at least per block -- in the block's first threads, 64 to a wavefront, MAX at least in every
    wavefront that holds any: kept.  The length stays where it is."""
    with open_wide(512) as probe:
        hs = probe.hot_state()
        block, wmax = hs["tile_block"], hs["wave_max"]
        per_wave = [wmax - 2, wmax - 1, wmax, wmax + 1, 0, 1, 63, 64]
        assert 2 <= wmax <= 62 and block in (64, 128, 256, 512)
        wet = flood_by_wave(probe, per_wave)
    rows = 512
    net = wide_level(rows)
    ql, q0 = flood_inputs(rows, wet, NT)
    want = oracle_window(net, NT * K, QTS, q0, ql)
    check_classes(rows, wet, (want,))
    listed = sum(m for m in per_wave if m < wmax)
    read, routed, cap, _ = prefix_windows(rows, ql, q0, want)
    assert listed == 2 * wmax - 2 <= cap
    assert read == [0, listed, listed, listed], (read, listed)
    assert routed == read


# ---- case 3: hot_wave_rows ------------------------------------------------------------------------------------------------------
FOREST_STEPS, FOREST_QTS = 48, 12
FOREST_OPTS = {"wide_min_rows": 64, "wide_k": 4}


@functools.lru_cache(maxsize=None)
def flooded_forest():
    """the network, the flooded forcing and the three windows of test_gpu_window_api.
    test_hot_rows_are_routed_by_blocks_of_their_own_and_change_nothing, with the oracle's three results"""
    to, ups, up_ptr, up_idx, p, qlat, q0 = WA.small_forest(nseg=6000)
    rng = np.random.default_rng(5)
    qlat = qlat.copy()
    qlat[rng.uniform(0, 1, qlat.shape[0]) < 0.08] *= np.float32(400.0)
    level = topology_levels(up_ptr, up_idx)[0]
    net = (up_ptr, up_idx, level, p)
    forcing = [qlat] + [(qlat * np.float32(1.0 + 0.5 * (k + 1))).astype(np.float32) for k in range(2)]
    want, state = [], q0
    for ql in forcing:
        want.append(oracle_window(net, FOREST_STEPS, FOREST_QTS, state, ql))
        state = new_q0(want[-1])
    return net, forcing, q0, want


@pytest.mark.parametrize("h", [8, 16, 32, 64, 0, 65, -3])
def test_hot_wave_rows_changes_who_routes_a_listed_row_and_nothing_else(h):
    """hot_wave_rows = H: a wavefront of the hot blocks takes H entries of the list (i = wave * H + lane, lanes >= H leave), so
    the launch needs ceil(cap / (H * wavefronts per block)) hot blocks.  Outside 1..64: 0 and anything below is the default 64,
    anything above is 64 (include/trmc.h).  Three windows of the flooded forest from the state on the device, and the lean-loop
    network (slices over clusters) as a stream of two days, bit for bit against the oracle."""
    net, forcing, q0, want = flooded_forest()
    up_ptr, up_idx, level, p = net
    eff = 64 if h <= 0 else min(h, 64)
    with RoutingPlan(up_ptr, up_idx, p, assume_short_ts=True, engine="levels", options={**FOREST_OPTS, "hot_wave_rows": h}) as plan:
        for k, ql in enumerate(forcing):
            plan.upload_forcing(FOREST_STEPS, ql, q0 if k == 0 else None)
            stats = plan.route_device(FOREST_STEPS, FOREST_QTS, True)
            assert stats["wide_levels"] > 0 and stats["wide_k"] == 4, stats
            assert np.array_equal(bits(plan.download_fvd()), bits(want[k])), (h, k)
        st = plan.hot_state()
        tiled = int(np.count_nonzero(level < stats["wide_levels"]))
        assert st["cap"] == cap_of(tiled, st["tile_block"]), (st, tiled)
        assert st["hot_home"] == -(-st["cap"] // (eff * (st["tile_block"] // 64))), (h, st)
        assert plan.hot_rows() > 0
    lean = LL.oracle_days()
    with RoutingPlan(*LL.inputs()[:2], LL.inputs()[3], assume_short_ts=True, engine="levels", options={**LL.OPTS, "hot_wave_rows": h}) as plan:
        LL.check_paths(plan)
        got = LL.stream(plan, full_output=True)
        for d in range(2):
            LL.check_products(got[d], lean[d], d)
            assert np.array_equal(bits(got[d][2]), bits(lean[d])), (h, d)
        st = plan.hot_state()
        assert st["hot_home"] == -(-st["cap"] // (eff * (st["tile_block"] // 64))) and plan.hot_rows() > 0, (h, st)


# ---- case 4: stream_split -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lean_chain(ndays):
    """the lean-loop network's two days in turn, `ndays` days by the oracle with the state handed on"""
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    state, out = q0, []
    for i in range(ndays):
        out.append(oracle_window((up_ptr, up_idx, level, params), LL.NSTEPS, LL.QTS, state, days[i % 2]))
        state = new_q0(out[-1])
    return out


def lean_stream(plan, extra, full_output, output_stride):
    """slots + `extra` days through a stream at plan level (the ring of day slots wraps); per day (hydrographs of every row,
    final state, the (q, v, d) block or None), stream_info at the end"""
    up_ptr, up_idx, level, params, days, q0 = LL.inputs()
    n, ns = params.shape[0], LL.NSTEPS
    rs = plan.rowset(np.arange(n))
    plan.upload_forcing(ns, days[0], q0)
    plan.stream_begin(ns, LL.QTS, full_output=full_output, output_stride=output_stride)
    slots = plan.stream_info()["slots"]
    ndays = slots + extra
    kept = ns // output_stride if output_stride else ns
    keep, out = [pinned_like(days[i % 2]) for i in range(ndays)], []
    for d in range(ndays):
        if d >= slots:                                    # (a slot's last day leaves before the slot is pushed into again)
            if plan.stream_info()["days_complete"] <= d - slots:
                plan.stream_flush()
            plan.stream_wait(d - slots)
        hyd = _lib.result_empty((n, ns), np.float32, always_pinned=True)
        st = _lib.result_empty((n, 3), np.float32, always_pinned=True)
        blk = _lib.result_empty((n, kept, 3), np.float32, always_pinned=True) if (full_output or output_stride) else None
        plan.stream_push(keep[d], rowset=rs, hyd=hyd, q0=st, fvd=blk)
        out.append((hyd, st, blk))
    plan.stream_flush()
    for d in range(ndays - slots, ndays):                 # (the days before them were waited for above)
        plan.stream_wait(d)
    info = plan.stream_info()
    plan.stream_end()
    assert info["days_complete"] == ndays == info["slots"] + extra, info
    return out, info


@pytest.mark.parametrize("full_output,stride", [(False, 0), (True, 4)], ids=["products", "full_output-stride-4"])
def test_stream_split_moves_slices_to_the_clusters_stream_and_changes_nothing(full_output, stride):
    """The lean-loop network: W = 3 slices over clusters.  stream_split = s, 0 < s < W: the slices from level s on are a launch of
    their own on the clusters' stream, behind an event of the tile stream's launch before -- one launch more per tile index:
    stream_info's count differs from the unsplit stream's, which is the proof that the split ran.  s >= W is ignored: the unsplit
    count.  slots + 2 days, so the ring of day slots wraps; every day against the oracle."""
    base = None
    for s in (0, 1, 2, 3, 8):
        with RoutingPlan(*LL.inputs()[:2], LL.inputs()[3], assume_short_ts=True, engine="levels", options={**LL.OPTS, "stream_split": s}) as plan:
            lag, W, C = plan.lags()
            assert W == 3 and C >= 2
            got, info = lean_stream(plan, 2, full_output, stride)
            assert plan.hot_rows() > 0
        want = lean_chain(len(got))
        for d, day in enumerate(got):
            LL.check_products(day, want[d], (s, d))
            if stride:
                kept = np.ascontiguousarray(want[d][:, stride - 1::stride])
                assert day[2].shape == kept.shape and np.any(kept[:, :, 1] != 0)
                assert np.array_equal(bits(day[2]), bits(kept)), (s, d)
        if s == 0:
            base = info
            continue
        assert (info["slots"], info["tiles_per_day"], info["lag_max"]) == (base["slots"], base["tiles_per_day"], base["lag_max"])
        if 0 < s < W:
            assert info["launches"] > base["launches"], (s, info, base)
        else:
            assert info["launches"] == base["launches"], (s, info, base)


def test_stream_split_with_a_reservoir_in_the_split_slices_and_a_gage_in_the_clusters():
    """the lakes and gages of test_gpu_stream_reservoirs_nudging (level pools in the slices at level s and deeper -- routed by the
    split-off launch -- and in the clusters, nudged gages in both parts), slots + 2 days with stream_split = 1: every day's full
    result, reservoir inflows, nudges and final state against the oracle's level pool and simple_da"""
    s = 1
    c3 = SRN.case()
    tpd = SRN.NSTEPS // SRN.K
    slots = 2 + -(-(c3.W + c3.C) // tpd)                 # (trmc_stream_begin: 2 + ceil((lag_max + 1) / tiles_per_day))
    key = (5000, 77, slots + 2)
    c = SRN.case(*key)
    assert c.W > s and np.count_nonzero((c.lag[c.lakes] >= s) & (c.lag[c.lakes] < c.W)) >= 1 and np.count_nonzero(c.lag[c.gages] >= c.W) >= 1
    tabs, _ = SRN.day_tables(c, len(c.days))
    want = SRN.oracle_days(key)
    launches = {}
    for split in (0, s):
        with SRN.open_plan(c, 32, {"stream_split": split}) as p:
            got, info = SRN.stream_days(p, c, tabs)
            launches[split] = p.stream_info()["launches"]          # (the ended stream's count)
            assert info["slots"] == slots and len(got) == slots + 2, info
        SRN.assert_days_equal(got, [(w[0], w[1], w[2], new_q0(w[0])) for w in want], f"oracle, split {split}")
    assert launches[s] > launches[0] > 0, launches               # (the split-off launches ran)


# ---- case 5: tail_sort ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hinted_forest():
    to, ups, up_ptr, up_idx, p, qlat, q0 = WA.small_forest()
    level = topology_levels(up_ptr, up_idx)[0]
    hint = np.random.default_rng(9).integers(0, 4, to.shape[0]).astype(np.uint8)
    want = oracle_window((up_ptr, up_idx, level, p), 16, 4, q0, qlat)
    return up_ptr, up_idx, level, p, qlat, q0, hint, want


@pytest.mark.parametrize("mid", [False, True], ids=["wide", "wide+mid"])
def test_tail_sort_off_keeps_the_per_level_order_below_the_tiled_levels(mid):
    """A hinted short-timestep plan of the level engine without clusters orders the rows below its tiled levels by cost; tail_sort
    = -1 keeps their per-level order.  The two plans place some row of the tail differently (the option did something) and every
    row of the tiled levels alike; a window on either -- wide tiles over one-step launches, and with the second tier between them
    -- equals the oracle."""
    up_ptr, up_idx, level, p, qlat, q0, hint, want = hinted_forest()
    opts = {"wide_min_rows": 64, "wide_k": 4, "cluster_rows": 0, **({"mid_min_rows": 8, "mid_k": 2} if mid else {"mid_min_rows": -1})}
    pos, tiled = {}, None
    for ts in (0, -1):
        with RoutingPlan(up_ptr, up_idx, p, assume_short_ts=True, engine="levels", cost_hint=hint, options={**opts, "tail_sort": ts}) as plan:
            lvl, pos[ts] = plan.levels()
            assert np.array_equal(lvl, level)
            plan.upload_forcing(16, qlat, q0)
            stats = plan.route_device(16, 4, True)
            assert stats["wide_levels"] > 0 and (stats["mid_levels"] > 0) == mid, stats
            t = stats["wide_levels"] + stats["mid_levels"]
            assert tiled in (None, t) and t < level.max()
            tiled = t
            assert np.array_equal(bits(plan.download_fvd()), bits(want)), ts
    tail = level >= tiled
    assert np.array_equal(pos[0][~tail], pos[-1][~tail])
    assert np.count_nonzero(pos[0][tail] != pos[-1][tail]) > 0
    assert sorted(pos[0][tail].tolist()) == sorted(pos[-1][tail].tolist())
