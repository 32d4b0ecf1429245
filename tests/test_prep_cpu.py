"""CPU companion of test_prep_arrays.py: the numpy restatement of the graph and target preparation
(prep_helpers.py) checked on its own, and the coverage preconditions of every fixture the GPU
tests use -- conditions on the restatement, so a later edit of a generator cannot silently take a
code path out of the GPU tests.

1. The directed roundings against a brute-force search over all 65,536 halves.
2. The leaf rule and the kappa fixpoint against a scalar pure-Python version on small graphs.
3. hub_segments against the per-row definition.
4. The fixtures' preconditions (test_prep_arrays.py sections A, B, C).
"""
import math

import numpy as np
import pytest

import oracle
import prep_helpers as ph
from helpers import random_topology_graphml


# ----------------------------------------------------------------------------------------------
# 1. roundings
# ----------------------------------------------------------------------------------------------
def _all_halves():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    vals = bits.view(np.float16).astype(np.float64)
    return np.unique(vals[~np.isnan(vals)])  # ascending, -inf .. +inf, one zero


def _bits(vals, x):
    """bits of the half values vals; a zero takes x's sign"""
    b = vals.astype(np.float16).view(np.uint16).astype(np.uint32)
    return np.where((vals == 0) & np.signbit(x), 0x8000, b)


def brute_floor(x):
    H = _all_halves()
    return _bits(H[np.searchsorted(H, x, side="right") - 1], x)


def brute_ceil(x):
    H = _all_halves()
    return _bits(H[np.searchsorted(H, x, side="left")], x)


def rounding_inputs():
    rng = np.random.default_rng(5)
    tiny = 2.0 ** -24  # the smallest half subnormal
    edges = [0.0, -0.0, tiny, -tiny, 65504.0, -65504.0, np.inf, -np.inf, 65520.0, -65520.0,
             2.0 ** -14, -2.0 ** -14, 1.0, -1.0, 1e300, -1e300, 5e-324, -5e-324]
    near = []
    for e in edges:
        if np.isfinite(e):
            near += [np.nextafter(e, np.inf), np.nextafter(e, -np.inf)]
    halves = _all_halves()
    halves = halves[np.isfinite(halves)]
    pick = rng.choice(halves, 4000)
    rnd = np.concatenate([
        rng.uniform(-70000, 70000, 20000), rng.uniform(-1e-4, 1e-4, 20000),
        rng.uniform(-2e-7, 2e-7, 20000), 10.0 ** rng.uniform(-12, 12, 20000),
        -(10.0 ** rng.uniform(-12, 12, 20000)), rng.uniform(1, 100, 5000) * 2.0 ** -30,
        pick, np.nextafter(pick, np.inf), np.nextafter(pick, -np.inf),
        (pick + rng.choice(halves, 4000)) / 2])  # midpoints of halves and around them
    return np.concatenate([np.asarray(edges + near), rnd])


def test_half_roundings_against_a_search_over_every_half():
    x = rounding_inputs()
    fl, ce = brute_floor(x), brute_ceil(x)
    # the bounds hold, and no half lies between the bound and x
    assert bool((ph.half_value(fl) <= x).all()) and bool((ph.half_value(ce) >= x).all())
    want_dn = np.where(fl == 0x7C00, 0x7BFF, fl)  # a rounded-down bound is never +inf
    want_up = np.where(ce == 0xFC00, 0xFBFF, ce)  # a rounded-up bound is never -inf
    assert np.array_equal(ph.half_dn(x), want_dn)
    assert np.array_equal(ph.half_up(x), want_up)
    assert np.array_equal(ph.half_down(x), fl)    # kfix_store's: +inf stays
    nan = np.asarray([np.nan])
    assert ph.half_dn(nan)[0] == 0xFC00 and ph.half_up(nan)[0] == 0x7C00
    assert ph.half_down(nan)[0] == 0xFC00
    # the named edges
    tiny = 2.0 ** -24
    assert list(ph.half_dn(np.asarray([0.0, -0.0, -1e-30, 1e-30, tiny, np.inf, -70000.0]))) == \
        [0x0000, 0x8000, 0x8001, 0x0000, 0x0001, 0x7BFF, 0xFC00]
    assert list(ph.half_up(np.asarray([0.0, -0.0, 1e-30, -1e-30, -tiny, -np.inf, 70000.0]))) == \
        [0x0000, 0x8000, 0x0001, 0x8000, 0x8001, 0xFBFF, 0x7C00]
    assert list(ph.half_down(np.asarray([np.inf, 70000.0]))) == [0x7C00, 0x7BFF]


def test_f32_rounding_and_order_images():
    x = rounding_inputs()
    x = np.concatenate([x, [3.5e38, -3.5e38, 1e39, -1e39]])
    f = ph.f32_dn(x)
    assert bool((f.astype(np.float64) <= x).all())
    with np.errstate(over="ignore"):
        up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    assert bool((up[np.isfinite(x)] > x[np.isfinite(x)]).all())
    assert ph.f32_dn(np.asarray([np.nan]))[0] == -np.inf
    # the order images sort like the values; only radix_f32 merges the zeros
    s = np.unique(f[f != 0])
    assert bool((np.diff(ph.f32_order(s).astype(np.int64)) > 0).all())
    assert bool((np.diff(ph.radix_f32(s).astype(np.int64)) > 0).all())
    z = np.asarray([-0.0, 0.0], np.float32)
    assert ph.f32_order(z)[0] < ph.f32_order(z)[1]
    assert ph.radix_f32(z)[0] == ph.radix_f32(z)[1]


# ----------------------------------------------------------------------------------------------
# 2. leaf rule and fixpoint, scalar
# ----------------------------------------------------------------------------------------------
def small_graph(seed, directed):
    data = random_topology_graphml(n_routers=18, n_poi=9, extra=14, seed=seed, directed=directed)
    g = oracle.read_graphml(data)
    ea, va = g["eattrs"], g["vattrs"]
    graph = (g["V"], g["eu"], g["ev"], np.asarray(ea["latency"], np.float64),
             np.asarray(ea["packetloss"], np.float64), np.asarray(va["packetloss"], np.float64))
    return graph, [i for i, t in enumerate(va["type"]) if t != "pop"]


def scalar_targets(R, targets, leaf, nit):
    """rows as Python lists; every step a Python float operation"""
    V, out = R["V"], R["out"]
    rp = [int(x) for x in out.rowptr]
    col, w = [int(x) for x in out.col], [float(x) for x in out.w]
    pot = [float(x) for x in R["pot"]]
    eff, dead, peeled = set(targets), set(), 0
    if leaf:
        for t in targets:
            if rp[t + 1] - rp[t] == 1:
                u = col[rp[t]]
                if u != t and rp[u + 1] - rp[u] > 1:
                    eff.discard(t)
                    dead.add(t)
                    peeled += 1
        for t in dead:
            eff.add(col[rp[t]])
    K = [math.inf if x in dead else
         min([w[k] - pot[col[k]] for k in range(rp[x], rp[x + 1])], default=math.inf)
         for x in range(V)]
    for _ in range(nit):
        Kt = [-math.inf if x in eff else K[x] for x in range(V)]
        new = []
        for x in range(V):
            m = math.inf
            for k in range(rp[x], rp[x + 1]):
                kap = w[k] - pot[col[k]]
                ky = (Kt[col[k]] + w[k] * (1.0 - 2e-5)) - 1e-9
                m = min(m, ky if ky > kap else kap)
            new.append(math.inf if x in dead else m)
        K = new
    return eff, dead, peeled, K


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("nit", [0, 1, 6])
@pytest.mark.parametrize("leaf", [True, False])
def test_fixpoint_and_leaf_rule_against_scalar_code(seed, nit, leaf):
    graph, poi = small_graph(seed, False)
    assert graph[0] <= 30
    R = ph.restate(graph)
    targets = sorted(int(R["inv"][v]) for v in poi[:6])
    T = ph.restate_targets(R, targets, leaf=leaf, nit=nit)
    eff, dead, peeled, K = scalar_targets(R, targets, leaf, nit)
    assert T["peeled"] == peeled and (not leaf or peeled > 0)
    assert set(np.nonzero(T["tmask"])[0].tolist()) == eff
    if leaf:
        assert set(np.nonzero(T["deadmask"])[0].tolist()) == dead
        rec = T["tleaf"]
        assert [int(t) for t in rec[:, 0]] == targets
        assert set(int(t) for t in rec[rec[:, 1] != ph.NO_LEAF, 0]) == dead
    Kn = T["kfix"][:R["V"]]
    assert np.array_equal(Kn.view(np.uint64), np.asarray(K, np.float64).view(np.uint64))
    Kt = T["kfix"][R["V"]:]
    assert bool((Kt[sorted(eff)] == -np.inf).all())
    rest = np.setdiff1d(np.arange(R["V"]), sorted(eff))
    assert np.array_equal(Kt[rest].view(np.uint64), Kn[rest].view(np.uint64))


def test_directed_restatement_keeps_every_target():
    graph, poi = small_graph(4, True)
    R = ph.restate(graph, True)
    targets = sorted(int(R["inv"][v]) for v in poi[:6])
    T = ph.restate_targets(R, targets, leaf=True)
    assert T["peeled"] == 0 and "tleaf" not in T and T["state"]["leaf"] == 0
    eff, dead, peeled, K = scalar_targets(R, targets, False, ph.TARGET_KAPPA)
    assert np.array_equal(T["kfix"][:R["V"]].view(np.uint64),
                          np.asarray(K, np.float64).view(np.uint64))


def test_restated_rows_and_sorted_copy_are_consistent():
    """Structure of the restatement itself on a small multigraph with ties: rows ascending by
    (neighbour, edge id), the copy a permutation of each row ascending in kappa, the tree a tree."""
    data, graph = ph.multigraph()
    R = ph.restate(graph)
    out = R["out"]
    key = out.row.astype(np.int64) << 40 | out.col.astype(np.int64) << 20 | out.eid
    assert bool((np.diff(key) >= 0).all()) and bool((out.eid < 2 ** 20).all())
    par = R["spt_parent"].astype(np.int64)
    assert par[0] == 0xFFFFFFFF and int((par == 0xFFFFFFFF).sum()) == 1
    v = np.arange(1, R["V"])
    assert bool((R["pot"][par[v]] < R["pot"][v]).all())
    rows = np.repeat(np.arange(R["V"]), np.diff(out.rowptr))
    k = R["kap"]
    same = rows[1:] == rows[:-1]
    assert bool((k[1:][same] >= k[:-1][same]).all())
    a = np.lexsort((R["adjk"][:, 0] & 0x3FFFFFFF, R["adjk"][:, 2], R["adjk"][:, 3], rows))
    b = np.lexsort((R["adj"][:, 0], R["adj"][:, 2], R["adj"][:, 3], rows))
    assert np.array_equal(R["adjk"][a][:, 1:], R["adj"][b][:, 1:])


# ----------------------------------------------------------------------------------------------
# 3. hub segments
# ----------------------------------------------------------------------------------------------
def test_hub_segments_cover_every_row_once():
    n = np.asarray([0, 1, 4095, 4096, 4097, 8192, 8193, 0, 12288, 3])
    rp = np.concatenate([[0], np.cumsum(n)])
    seg, multi = ph.hub_segments(rp, len(n))
    for v in range(len(n)):
        s = seg[seg[:, 0] == v, 1].astype(np.int64)
        assert len(s) == max(1, -(-int(n[v]) // ph.HUB_SEG))
        assert list(s) == [int(rp[v]) + ph.HUB_SEG * i for i in range(len(s))]
    assert [tuple(int(x) for x in m) for m in multi] == \
        [(4, 4, 2, 0), (5, 6, 2, 0), (6, 8, 3, 0), (8, 12, 3, 0)]
    assert bool((np.diff(seg[:, 0].astype(np.int64)) >= 0).all())


# ----------------------------------------------------------------------------------------------
# 4. coverage preconditions
# ----------------------------------------------------------------------------------------------
def fields(R):
    f = (R["adj_out"] if R["directed"] else R["adj"])[:, 1]
    return f >> 16, f & 0xFFFF


def test_preconditions_rounding_range_dn30():
    """real x 2^-30: pi fields among the half subnormals and at 0x0001; kappa0 fields of both
    signs, with the +-0 -> 0x8001 step taken."""
    R = ph.domain_restated("real_dn30")
    hi, lo = fields(R)
    assert bool(((hi > 0) & (hi < 0x0400)).any()) and bool((hi == 0x0001).any())
    assert bool((lo == 0x8001).any())
    pos = (lo & 0x8000) == 0
    assert bool(pos.any()) and bool((~pos).any())
    # the step itself: a kappa0 in (-2^-24, 0) rounds to zero first
    k0 = R["kap0d"]
    assert bool(((k0 < 0) & (k0 > -2.0 ** -24)).any())


@pytest.mark.parametrize("directed", [False, True])
def test_preconditions_rounding_range_up30(directed):
    """real x 2^30: pi past 65504 (field +inf), kappa0 below -65504 (field -inf)."""
    R = ph.domain_restated("real_up30", directed)
    hi, lo = fields(R)
    assert bool((hi == 0x7C00).any()) and bool((lo == 0xFC00).any())


def test_preconditions_int_domain_has_several_tight_parents():
    R = ph.domain_restated("int")
    assert int((R["tight_parents"] >= 2).sum()) >= 10


@pytest.mark.parametrize("directed", [False, True])
def test_preconditions_shapes(directed):
    R = ph.shapes_restated(directed)
    V = R["V"]
    assert V > ph.GROUP_HUBS
    seg, multi = R["hub_seg"], R["hub_multi"]
    rp = R["out"].rowptr
    n = np.diff(rp)
    if not directed:
        assert sorted(n[:4].tolist()) == sorted(ph.HUB_ROWS)
        assert len(multi) >= 3
        # a row cut at exactly a segment end, one of a single full segment, one just past it
        assert bool((n[multi[:, 0]] % ph.HUB_SEG == 0).any())
        assert ph.HUB_SEG in n[:4] and ph.HUB_SEG + 1 in n[:4]
    else:
        # one hub is long only in its in-row: the tree's segments are the in-rows' own
        nin = np.diff(R["inn"].rowptr)
        assert len(multi) >= 2
        assert int(((nin > ph.HUB_SEG) & (n <= ph.HUB_SEG)).sum()) == 1
        iseg, imulti = ph.hub_segments(R["inn"].rowptr, ph.GROUP_HUBS)
        assert len(imulti) >= 3 and bool((nin[imulti[:, 0]] % ph.HUB_SEG == 0).any())
    # tail rows: a thread each; the 4-wide loop taken 0, 1 and 2 times with every remainder
    tail = n[ph.GROUP_HUBS:]
    assert set(range(1, 10)) <= set(tail.tolist())
    # several self loops on one vertex, different latencies, the lowest edge id not the first made
    _, eu, ev, elat, _, _ = ph.shapes_graph(directed)[1]
    loops = np.nonzero((eu == ev) & (eu == ph.SELF_LOOP_AT))[0]
    assert len(loops) == 4 and len(set(elat[loops].tolist())) == 4
    assert R["self_lat"][R["inv"][ph.SELF_LOOP_AT]] == elat[loops.min()]
    assert elat[loops.min()] != elat[loops].min() or elat[loops.min()] != elat[loops].max()
    # edge ids shuffled: not grouped by vertex
    assert not bool((np.diff(eu[:1000]) >= 0).all())


def shape_targets(R, poi):
    return sorted(int(R["inv"][ph.shapes_poi_vertex(k)]) for k in poi)


def test_preconditions_targets_on_the_shapes_graph():
    R = ph.shapes_restated()
    for poi in (ph.SHAPE_SET1, ph.SHAPE_SET2):
        tg = shape_targets(R, poi)
        T = ph.restate_targets(R, tg)
        n = np.diff(R["out"].rowptr)
        # peeled targets, a target that is not peeled, a pendant vertex that is no target
        assert 0 < T["peeled"] < len(tg)
        pend = np.nonzero(n == 1)[0]
        assert len(np.setdiff1d(pend, tg)) > 0
        # a target of the effective set on a row cut in several segments
        multi_rows = R["hub_multi"][:, 0].astype(np.int64)
        rows = R["out"].row
        on_multi = np.isin(rows, multi_rows) & T["tmask"][R["out"].col]
        assert bool(on_multi.any())
        # the iterates move, and rows of every sort class change their order
        assert ph.iterates_differ(T)
        cls = ph.resort_classes(R, T)
        assert cls["wave"] > 0 and cls["block"] > 0 and cls["big"] > 0, cls
    # the second set drops targets of the first and adds others
    assert set(ph.SHAPE_SET1) - set(ph.SHAPE_SET2) and set(ph.SHAPE_SET2) - set(ph.SHAPE_SET1)
    # the stale-key path matters: the two sets' copies differ
    T1 = ph.restate_targets(R, shape_targets(R, ph.SHAPE_SET1))
    T2 = ph.restate_targets(R, shape_targets(R, ph.SHAPE_SET2))
    assert not np.array_equal(T1["adjk"], T2["adjk"]) and not np.array_equal(T1["kap"], T2["kap"])


def test_preconditions_targets_on_the_domain_graph():
    R = ph.domain_restated("real")
    tg = sorted(int(R["inv"][v]) for v in ph.domain_targets("real"))
    T = ph.restate_targets(R, tg)
    n = np.diff(R["out"].rowptr)
    assert T["peeled"] > 0
    assert len(np.setdiff1d(np.nonzero(n == 1)[0], tg)) > 0  # a pendant non-target
    assert ph.iterates_differ(T)
    cls = ph.resort_classes(R, T)
    assert cls["wave"] > 0
