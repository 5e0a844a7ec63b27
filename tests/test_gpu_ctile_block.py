"""CLUSTER BLOCKS wider than a cluster (csrc/k_mc_ctile.inc kCtileBlock, csrc/topology.hpp cluster_block_rows): the plan packs
whole clusters of one cluster level into blocks of the width of k_mc_ctile's workgroup, whose threads take the block's rows by cost
class.  Which thread routes a row enters no result -- so every shape the packing can produce is compared bit for bit with the
oracle (the CPU restatement of the reference loop), at the smallest sizes that have the shape: every row a cluster row
(wide_min_rows < 0: no slices), fp32, short timestep, a few tiles of 8 steps."""
import numpy as np
import pytest

from oracle import oracle as O
from troute_amd import _lib
from troute_amd.distributed import ShardedRouter
from troute_amd.plan import RoutingPlan, csr_from_lists
from troute_amd.sequence import RouteStream, pinned_like

pytestmark = pytest.mark.gpu
K = 8   # steps per tile launch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- networks as to[row] (-1: outlet), labels shuffled ---------------------------------------------------------------------
def _shuffled(to, rng):
    n = to.shape[0]
    perm = rng.permutation(n)
    out = np.full(n, -1, np.int64)
    out[perm] = np.where(to >= 0, perm[np.maximum(to, 0)], -1)
    return out


def forest(sizes, rng):
    """one random tree per entry (junctions of up to three rows), every tree smaller than a cluster: ONE cluster level"""
    to, base = [], 0
    for n in sizes:
        t, nup = np.full(n, -1, np.int64), np.zeros(n, np.int64)
        for i in range(1, n):
            j = int(rng.integers(0, i))
            while nup[j] >= 3:
                j = (j + 1) % i
            t[i] = base + j
            nup[j] += 1
        to.append(t)
        base += n
    return _shuffled(np.concatenate(to), rng)


def chains(lengths, rng):
    to, base = [], 0
    for n in lengths:
        t = base + np.arange(1, n + 1, dtype=np.int64)
        t[-1] = -1
        to.append(t)
        base += n
    return _shuffled(np.concatenate(to), rng)


def csr_of(to):
    ups = [[] for _ in range(to.shape[0])]
    for i, d in enumerate(to.tolist()):
        if d >= 0:
            ups[d].append(i)
    return csr_from_lists(ups)


def inputs(rng, n, nq=4, wet=None):
    """channel parameters, lateral inflow, initial state; wet: rows whose inflow is 100 x the others' (they go over bank and take
    more secant iterations: other cost classes)"""
    p = np.stack([np.full(n, 300.0), rng.uniform(200, 4000, n), rng.uniform(0.5, 20, n), np.zeros(n), np.zeros(n),
                  rng.choice([0.04, 0.05, 0.06], n), np.zeros(n), rng.uniform(0.1, 2.0, n),
                  np.exp(rng.uniform(np.log(1e-4), np.log(0.1), n))], 1)
    p[:, 3] = p[:, 2] * 5 / 3
    p[:, 4] = p[:, 3] * 3
    p[:, 6] = 2 * p[:, 5]
    ql = rng.uniform(0.0, 0.05, (n, nq))
    if wet is not None:
        ql[wet] *= 100.0
    q0 = np.stack([rng.uniform(0, 2, n), rng.uniform(0, 2, n), rng.uniform(0, 1, n)], 1)
    return p.astype(np.float32), ql.astype(np.float32), q0.astype(np.float32)


_width = []


def block_width():
    """the library's cluster block width (a build-time constant: any plan in cluster order reports it)"""
    if not _width:
        up_ptr, up_idx = csr_from_lists([[], [0]])
        with RoutingPlan(up_ptr, up_idx, np.ones((2, 9), np.float32), assume_short_ts=True, engine="levels",
                         options={"cluster_rows": 128, "wide_min_rows": -1}) as p:
            _width.append(p.cluster_blocks()[1])
        assert _width[0] % 64 == 0 and 128 <= _width[0] <= 1024
    return _width[0]


def shape_of(plan, up_ptr, up_idx, cluster_rows):
    """THE packing invariant, from the plan itself: no cluster block holds more rows than the block width, a block is a run of
    consecutive positions of one lag, every cluster (the rows joined by edges between rows of equal lag) lies inside one block,
    every other edge comes from a row that runs ahead.  Returns (rows per block, clusters per block, lag per block)."""
    blk, width, nb = plan.cluster_blocks()
    lag, W, C = plan.lags()
    _, pos = plan.levels()
    n = blk.shape[0]
    assert width == block_width() and W == 0 and np.all(blk >= 0) and nb == blk.max() + 1
    rows = np.bincount(blk, minlength=nb)
    assert rows.min() >= 1 and rows.max() <= width
    order = np.argsort(pos)
    assert np.all(np.diff(blk[order]) >= 0) and np.all(np.diff(lag[order]) >= 0)
    first = np.r_[0, np.flatnonzero(np.diff(blk[order])) + 1]
    lag_b = lag[order][first]
    assert np.array_equal(np.maximum.reduceat(lag[order], first), lag_b) and np.array_equal(np.minimum.reduceat(lag[order], first), lag_b)
    down = np.repeat(np.arange(n), np.diff(up_ptr))
    same = lag[up_idx] == lag[down]
    assert np.all(blk[up_idx][same] == blk[down][same])
    assert np.all(lag[up_idx][~same] < lag[down][~same])
    root = np.arange(n)

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x
    for u, d in zip(up_idx[same].tolist(), down[same].tolist()):
        root[find(u)] = find(d)
    roots = np.array([find(r) for r in range(n)])
    assert np.bincount(roots).max() <= cluster_rows
    ncl = np.array([np.unique(roots[blk == b]).shape[0] for b in range(nb)])
    return rows, ncl, lag_b


def stream_full(up_ptr, up_idx, params, days, q0, nsteps, qts, cluster_rows, check):
    """the days as a stream with every (q, v, d) of every row, each against the oracle, the state handed on as new_q0 does"""
    n = params.shape[0]
    with RoutingPlan(up_ptr, up_idx, params, assume_short_ts=True, engine="levels",
                     options={"cluster_rows": cluster_rows, "wide_min_rows": -1, "wide_k": K}) as p:
        lvl, _ = p.levels()
        check(*shape_of(p, up_ptr, up_idx, cluster_rows))
        p.upload_forcing(nsteps, days[0], q0)
        p.stream_begin(nsteps, qts, full_output=True)
        D = p.stream_info()["slots"]
        outs = [_lib.result_empty((n, nsteps, 3), np.float32, always_pinned=True) for _ in range(D)]
        keep = [pinned_like(q) for q in days]
        for d, q in enumerate(keep):
            p.stream_push(q, fvd=outs[d % D])
        p.stream_flush()
        state, wants = q0, []
        for d, q in enumerate(days):
            p.stream_wait(d)
            want = O.network_by_segment(nsteps, qts, up_ptr, up_idx, lvl, params, state, q, True, det=True)[:, 1:, :]
            assert np.array_equal(bits(outs[d % D]), bits(want)), d
            state = np.stack([want[:, -1, 0], want[:, -1, 0], want[:, -1, 2]], 1)
            wants.append(want)
        p.stream_end()
    return wants


def many_small_clusters(width, rng):
    """cluster sizes 5..40 that sum to three blocks and 37 rows"""
    total, sizes = 3 * width + 37, []
    while sum(sizes) < total - 45:
        sizes.append(int(rng.integers(5, 41)))
    rest = total - sum(sizes)
    sizes += [rest - 20, 20] if rest > 40 else [rest]
    assert sum(sizes) == total and 5 <= min(sizes) and max(sizes) <= 40
    return sizes


def test_many_clusters_per_block():
    """one cluster level of small clusters: blocks of more than four clusters, the level's last block short of one wavefront"""
    rng = np.random.default_rng(5)
    to = forest(many_small_clusters(block_width(), rng), rng)
    up_ptr, up_idx = csr_of(to)
    params, ql, q0 = inputs(rng, to.shape[0])

    def check(rows, ncl, lag_b):
        assert np.all(lag_b == 0) and rows.shape[0] >= 2
        assert ncl.max() > 4 and rows.max() > 128 - 40 and 0 < rows[-1] < 64
    stream_full(up_ptr, up_idx, params, [ql, (ql * 1.5).astype(np.float32)], q0, 32, 8, 128, check)


def test_clusters_as_large_as_blocks():
    """three chains of four and a bit cluster levels, every cluster but the last of exactly cluster_rows rows (two of them fill a
    block of the narrowest build): clusters of one level share a block -- the LDS slots of the second begin behind the first's --
    and every cluster's head reads its inflow from the block of the level above through the plane"""
    rng = np.random.default_rng(6)
    cr = min(128, block_width() // 2)
    to = chains([4 * cr + 17] * 3, rng)
    up_ptr, up_idx = csr_of(to)
    params, ql, q0 = inputs(rng, to.shape[0])

    def check(rows, ncl, lag_b):
        assert lag_b.max() == 4                                              # five cluster levels
        full = lag_b < 4
        assert ncl[full].max() >= 2 and np.all(rows[full] % cr == 0) and np.all(rows[~full] % 17 == 0)
    stream_full(up_ptr, up_idx, params, [ql, (ql * 0.5).astype(np.float32)], q0, 48, 12, cr, check)


def test_a_level_of_one_row():
    """a chain of 2 * 16 + 1 rows in clusters of 16: the last cluster level is one block of one row (and the threads of all its
    other wavefronts only keep the barriers); beside it, trees that end at the first level"""
    rng = np.random.default_rng(7)
    to_c, to_f = chains([33], rng), forest([9, 16, 3, 1, 12], rng)
    to = np.concatenate([to_c, np.where(to_f >= 0, to_f + 33, -1)])
    up_ptr, up_idx = csr_of(to)
    params, ql, q0 = inputs(rng, to.shape[0])

    def check(rows, ncl, lag_b):
        assert lag_b.tolist()[-1] == 2 and rows[-1] == 1 and np.count_nonzero(lag_b == 2) == 1
    stream_full(up_ptr, up_idx, params, [ql, (ql * 2).astype(np.float32)], q0, 32, 8, 16, check)


def test_mixed_cost_classes_products_only_equals_full_output_and_oracle():
    """a tenth of the rows with 100 x the lateral inflow: rows of several cost classes in every block, so from the second tile on
    the in-block partition deals threads over all the block's wavefronts.  Three days through RouteStream, products only: the
    outlet hydrographs and final states are those of the full-output pass, which is the oracle's, bit for bit."""
    rng = np.random.default_rng(8)
    width = block_width()
    sizes = many_small_clusters(width, rng) + [100, 128, 77]
    to_f, to_c = forest(sizes, rng), chains([2 * 128 + 50, 128 + 9], rng)
    to = np.concatenate([to_f, np.where(to_c >= 0, to_c + to_f.shape[0], -1)])
    n = to.shape[0]
    up_ptr, up_idx = csr_of(to)
    wet = rng.random(n) < 0.1
    params, ql, q0 = inputs(rng, n, wet=wet)
    nsteps, qts = 48, 12
    days = [ql, (ql * 1.7).astype(np.float32), (ql * 0.3).astype(np.float32)]

    def check(rows, ncl, lag_b):
        assert lag_b.max() == 2 and rows.max() > 64 and np.count_nonzero(lag_b == 0) >= 2
    wants = stream_full(up_ptr, up_idx, params, days, q0, nsteps, qts, 128, check)
    r = ShardedRouter(to, params, stream=True, options={"cluster_rows": 128, "wide_min_rows": -1, "wide_k": K})
    got = {}
    with RouteStream(r, nsteps, qts) as rs:
        for item in rs.route(iter(days), q0):
            got[item[0]] = tuple(None if x is None else np.array(x, copy=True) for x in item[1:])
        rows = np.array(rs.outlet_rows, copy=True)
    assert sorted(got) == [0, 1, 2]
    for d in range(3):
        w = wants[d]
        assert np.array_equal(bits(got[d][0]), bits(w[rows, :, 0])), d
        assert np.array_equal(bits(got[d][1]), bits(np.stack([w[:, -1, 0], w[:, -1, 0], w[:, -1, 2]], 1))), d
    r.close()
