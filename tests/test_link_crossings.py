"""GPU tests of the link crossings (shdtopo_link_crossings, topo_cross.hip): the hops of a set of
flows that go over a watched edge or arrive at a watched vertex, compared exactly -- the records
byte for byte -- with records derived from the CPU oracle's chains (crossing_helpers.
ExpectedCrossings over load_helpers.ExpectedLoad: g.dijkstra for the parents, g.get_eid for each
hop's edge).  The watch sets follow one recipe over the oracle's loads (crossing_helpers.
watch_recipe); conditions on the inputs are asserted from the oracle's records.  Every graph has at
most 700 vertices.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from crossing_helpers import (DIAMOND_POI, ExpectedCrossings, check_crossings, check_stats,
                              diamond_case, diamond_graphml, parallel_groups_on_chains,
                              watch_recipe)
from helpers import random_topology_graphml
from load_helpers import (TRANSIT_POI, ExpectedLoad, all_pairs, check_load, long_chain_graphml,
                          pairs_crossing_ties, pinned, random_hosts, tie_grid_graphml,
                          transit_grid_graphml)
from shadow_amd import _lib

pytestmark = pytest.mark.gpu
NSRC = 5


# ------------------------------------------------------------------------------------------
# expected values, computed once per graph and shared (never modified)
# ------------------------------------------------------------------------------------------
def tie_grid_weights():
    return np.random.default_rng(21).integers(1, 2**40, 420, endpoint=True).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def tie_grid_expected(directed, verts):
    """6 sources x 70 destinations on the tie grid, random weights in [1, 2^40], the recipe's
    watches: (ExpectedLoad, ExpectedCrossings, edges, vertices)."""
    g = oracle.OGraph.from_graphml(tie_grid_graphml(directed))
    v = np.asarray(verts, np.int32)
    sv, dv = np.repeat(v[:6], 70), np.tile(v, 6)
    exp = ExpectedLoad(g, sv, dv, tie_grid_weights(), v)
    edges, vertices = watch_recipe(exp, sv, dv)
    return exp, ExpectedCrossings(g, exp, tie_grid_weights(), edges, vertices), edges, vertices


@functools.lru_cache(maxsize=None)
def transit_expected(directed, verts):
    g = oracle.OGraph.from_graphml(transit_grid_graphml(directed))
    v = np.asarray(verts, np.int32)
    sv, dv = np.repeat(v[:6], len(v)), np.tile(v, 6)
    exp = ExpectedLoad(g, sv, dv, None, v)
    edges, vertices = watch_recipe(exp, sv, dv)
    return exp, ExpectedCrossings(g, exp, None, edges, vertices), edges, vertices


def real_graphml():
    return random_topology_graphml(600, 60, 2400, seed=3)


def real_flows(av, aip):
    """The flow recipe of test_link_load_batch.py: NSRC sources x every attached vertex, then
    duplicates and self pairs, weights up to 2^40.  Returns (sip, dip, sv, dv, w)."""
    k = len(av)
    si = np.concatenate([np.repeat(np.arange(NSRC), k), [0, 0, 1, 3, 3, 2], [0, 1, 2]])
    di = np.concatenate([np.tile(np.arange(k), NSRC), [9, 9, 8, 7, 7, 11], [0, 1, 2]])
    w = np.random.default_rng(33).integers(1, 2**40, len(si), endpoint=True).astype(np.uint64)
    w[:3] = [2**40, 1, 2**40 - 1]
    return aip[si], aip[di], av[si], av[di], w


@functools.lru_cache(maxsize=None)
def real_expected(av):
    """The real-latency flows plus one unattached source as the call's last request:
    (ExpectedLoad, ExpectedCrossings of the n + 1 requests, edges, vertices, chains over ties)."""
    g = oracle.OGraph.from_graphml(real_graphml())
    v = np.asarray(av, np.int32)
    sip, dip, sv, dv, w = real_flows(v, np.zeros(len(v), np.uint32))
    exp = ExpectedLoad(g, sv, dv, w, v)
    edges, vertices = watch_recipe(exp, sv, dv)
    xc = ExpectedCrossings(g, exp, w, edges, vertices, flows=np.arange(len(sv)), n=len(sv) + 1)
    return exp, xc, edges, vertices, pairs_crossing_ties(g, exp)


def real_case(options=()):
    top, g, av, aip = random_hosts(real_graphml(), 300, options)
    sip, dip, sv, dv, w = real_flows(av, aip)
    exp, xc, edges, vertices, crossing = real_expected(tuple(int(v) for v in av))
    assert crossing == 0  # input condition: no requested chain crosses a tie
    stranger = sa.ip_to_network("10.9.8.7")
    sip = np.concatenate([sip, [stranger]]).astype(np.uint32)
    dip = np.concatenate([dip, [aip[0]]]).astype(np.uint32)
    w = np.concatenate([w, [2**39]]).astype(np.uint64)
    return top, sip, dip, w, exp, xc, edges, vertices


def bytes_equal(a, b):
    assert a["total"] == b["total"]
    for k in ("offsets", "records", "count", "weight"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------
# 1, 2. crossings against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int_keys", [0, 1])
@pytest.mark.parametrize("directed", [False, True])
def test_tie_grid_crossings(directed, int_keys):
    top, g, ips, verts = pinned(tie_grid_graphml(directed), 70, [("replay_int_keys", int_keys)])
    assert top.is_directed == directed
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp, xc, edges, vertices = tie_grid_expected(directed, tuple(int(v) for v in verts))
    # conditions on the input (from the oracle's records), not on the code under test
    assert xc.flows_with_several() >= 150, xc.flows_with_several()
    assert xc.both >= 90, xc.both
    assert xc.flows_without_any() >= 1
    if directed:
        assert xc.reverse_crossings() == 0
    else:
        assert xc.reverse_crossings() >= 50, xc.reverse_crossings()
    out = top.link_crossings(sip, dip, edges, vertices, tie_grid_weights())
    check_crossings(out, xc)
    cs = top.link_crossings_stats()
    check_stats(cs, xc, sources=6)
    assert cs["chunks"] == 1 and cs["kernel_ms"] > 0


@pytest.mark.parametrize("directed", [False, True])
def test_transit_grid_crossings(directed):
    """Destinations on other destinations' chains."""
    top, g, ips, verts = pinned(transit_grid_graphml(directed), TRANSIT_POI)
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp, xc, edges, vertices = transit_expected(directed, tuple(int(v) for v in verts))
    assert exp.transit_destinations() >= 80
    assert xc.flows_with_several() >= 150 and xc.both >= 90 and xc.flows_without_any() >= 1
    if directed:
        assert xc.reverse_crossings() == 0
    else:
        assert xc.reverse_crossings() >= 1
    out = top.link_crossings(sip, dip, edges, vertices)
    check_crossings(out, xc)
    check_stats(top.link_crossings_stats(), xc, sources=6)


# ------------------------------------------------------------------------------------------
# 3. the backward fill at its longest, and the cap rule
# ------------------------------------------------------------------------------------------
def test_long_chain_every_hop_is_watched_and_the_cap_rule():
    top, g, ips, verts = pinned(long_chain_graphml(), 3)
    sip, dip, sv, dv = all_pairs(ips, verts, 3)
    sip, dip = np.ascontiguousarray(sip), np.ascontiguousarray(dip)
    w = np.asarray([3, 5, 7, 11, 13, 17, 19, 23, 29], np.uint64) << np.uint64(33)
    exp = ExpectedLoad(g, sv, dv, w, verts)
    assert exp.hops.reshape(3, 3).tolist() == [[1, 201, 102], [201, 1, 101], [102, 101, 1]]
    edges, vertices = np.arange(g.E), np.arange(g.V)
    xc = ExpectedCrossings(g, exp, w, edges, vertices)
    assert np.array_equal(xc.per_flow, 2 * exp.hops) and xc.total == 2 * int(exp.hops.sum())
    out = top.link_crossings(sip, dip, edges, vertices, w)
    check_crossings(out, xc)
    rec = out["records"]
    for i in range(9):  # in hop order, the edge record of a hop before its vertex record
        r = rec[xc.offsets[i]:xc.offsets[i + 1]]
        assert np.array_equal(r["hop"], np.repeat(np.arange(exp.hops[i]), 2))
        assert np.all(r["watch"][0::2] < g.E) and np.all(r["watch"][1::2] >= g.E)
    # a cap in the middle of a 201-hop flow: only the flows that fit are written
    i = 3
    assert xc.per_flow[i] == 402
    cap = int(xc.offsets[i]) + 201
    part = top.link_crossings(sip, dip, edges, vertices, w, cap=cap)
    want = xc.fitting(cap)
    assert len(want) == xc.offsets[i]
    assert part["records"].tobytes() == want.tobytes()
    assert part["total"] == xc.total and np.array_equal(part["offsets"], xc.offsets)
    assert np.array_equal(part["count"], xc.count) and np.array_equal(part["weight"], xc.weight)
    # the tail of the buffer, from the first flow that does not fit on, is untouched
    lib, _ = _lib.load()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    buf = np.full(4 * (xc.total + 8), -7, np.int32)
    we, wv = edges.astype(np.int32), vertices.astype(np.int32)
    r = lib.shdtopo_link_crossings(top._h, p(sip), p(dip), p(w), 9, p(we), len(we), p(wv), len(wv),
                                   None, p(buf), cap, None, None)
    assert r == xc.total
    assert buf[:4 * len(want)].tobytes() == want.tobytes() and np.all(buf[4 * len(want):] == -7)


# ------------------------------------------------------------------------------------------
# 4. parallel edges: only the lowest id of a group is ever crossed
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
def test_multigraph_crossings_are_on_the_lowest_edge_id(directed):
    data = random_topology_graphml(n_routers=400, n_poi=40, extra=1600, seed=9, integer=True,
                                   directed=directed, parallel=400)
    top, g, av, aip = random_hosts(data, 120)
    sip, dip, sv, dv = all_pairs(aip, av, 6)
    exp = ExpectedLoad(g, sv, dv, None, av)
    groups = parallel_groups_on_chains(g, exp)
    assert len(groups) >= 10, len(groups)  # input condition
    groups = groups[:16]
    edges = [e for pair in groups for e in pair]  # lowest, higher, lowest, higher, ...
    xc = ExpectedCrossings(g, exp, None, edges, [])
    assert np.all(xc.count[0::2] > 0) and not xc.count[1::2].any()
    out = top.link_crossings(sip, dip, edges)
    check_crossings(out, xc)
    assert not np.isin(out["records"]["watch"], np.arange(1, len(edges), 2)).any()


# ------------------------------------------------------------------------------------------
# 5, 6. the batch path: chains from the batch kernel's pair records
# ------------------------------------------------------------------------------------------
def test_batch_path_equals_the_oracle_and_the_replay_path():
    top, sip, dip, w, exp, xc, edges, vertices = real_case()
    top.table()
    top.set_option("trace_batch", 0)
    try:
        a = top.link_crossings(sip, dip, edges, vertices, w)
        ca = top.link_crossings_stats()
    finally:
        top.set_option("trace_batch", 1)
    b = top.link_crossings(sip, dip, edges, vertices, w)
    cb = top.link_crossings_stats()
    check_crossings(b, xc)
    bytes_equal(a, b)
    check_stats(ca, xc, sources=NSRC, unattached=1)
    check_stats(cb, xc, sources=NSRC, unattached=1)
    assert cb["batch_sources"] == NSRC and cb["batch_fallback"] == 0
    assert cb["replay_ms"] == 0 and cb["batch_ms"] > 0
    assert ca["batch_sources"] == 0 and ca["batch_fallback"] == 0 and ca["batch_ms"] == 0
    # "load_walk" has no meaning here: the tree accumulation's option forces no replay
    top.set_option("load_walk", 0)
    try:
        c = top.link_crossings(sip, dip, edges, vertices, w)
        assert top.link_crossings_stats()["batch_sources"] == NSRC
    finally:
        top.set_option("load_walk", 1)
    bytes_equal(b, c)
    # vertex watches alone: the pair walk looks up no edge
    d = top.link_crossings(sip, dip, [], vertices, w)
    assert top.link_crossings_stats()["batch_sources"] == NSRC
    check_crossings(d, ExpectedCrossings(exp.g, exp, w[:-1], [], vertices, flows=xc.flows, n=xc.n))


def test_chunked_crossings_are_byte_identical():
    """Global offsets across chunks, and slot reuse by a second call on the same topology."""
    top, sip, dip, w, exp, xc, edges, vertices = real_case()
    top.table()
    a = top.link_crossings(sip, dip, edges, vertices, w)
    assert top.link_crossings_stats()["chunks"] == 1
    top.set_option("trace_chunk", 2)
    try:
        b = top.link_crossings(sip, dip, edges, vertices, w)
        cs = top.link_crossings_stats()
        assert cs["chunks"] == 3 and cs["sources"] == NSRC and cs["batch_sources"] == NSRC
    finally:
        top.set_option("trace_chunk", 0)
    bytes_equal(a, b)
    check_crossings(b, xc)


# ------------------------------------------------------------------------------------------
# 7. a chunk with both kinds of sources
# ------------------------------------------------------------------------------------------
def test_mixed_chunk_serves_both_chain_sources():
    top, g0, ips, verts = pinned(diamond_graphml(), DIAMOND_POI)
    g, free, tied = diamond_case(tuple(int(v) for v in verts))
    assert len(free) >= 2 and len(tied) >= 2, (len(free), len(tied))  # input condition
    src = sorted(free[:3] + tied[:3])
    ipof = {int(v): ip for ip, v in zip(ips, verts)}
    vs = sorted(ipof)
    sv = np.repeat(src, len(vs)).astype(np.int32)
    dv = np.tile(vs, len(src)).astype(np.int32)
    sip = np.asarray([ipof[int(v)] for v in sv], np.uint32)
    dip = np.asarray([ipof[int(v)] for v in dv], np.uint32)
    w = np.random.default_rng(7).integers(1, 2**40, len(sv)).astype(np.uint64)
    exp = ExpectedLoad(g, sv, dv, w, verts)
    edges, vertices = watch_recipe(exp, sv, dv)
    xc = ExpectedCrossings(g, exp, w, edges, vertices)
    assert xc.flows_with_several() >= 20 and xc.flows_without_any() >= 1
    top.table()
    out = top.link_crossings(sip, dip, edges, vertices, w)
    check_crossings(out, xc)
    cs = top.link_crossings_stats()
    check_stats(cs, xc, sources=len(src))
    assert cs["chunks"] == 1
    assert cs["batch_sources"] >= 1 and cs["batch_fallback"] >= 1
    assert cs["batch_sources"] + cs["batch_fallback"] == len(src)
    assert cs["replay_ms"] > 0 and cs["batch_ms"] > 0


# ------------------------------------------------------------------------------------------
# the call's contract
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    """The undirected tie grid with its table built, shared by the contract tests (none of them
    changes the topology; options are put back)."""
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70)
    top.table()
    return top, g, ips, verts


def test_edge_cases(grid):
    top, g, ips, verts = grid
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp, xc, edges, vertices = tie_grid_expected(False, tuple(int(v) for v in verts))
    w = tie_grid_weights()
    # the empty watch set: 0 crossings, every offset 0
    out = top.link_crossings(sip, dip, [], [], w)
    assert out["total"] == 0 and not out["offsets"].any() and len(out["offsets"]) == 421
    assert len(out["records"]) == 0 and len(out["count"]) == 0
    # no request
    out = top.link_crossings(sip[:0], dip[:0], edges, vertices)
    assert out["total"] == 0 and out["offsets"].tolist() == [0] and len(out["records"]) == 0
    assert not out["count"].any() and not out["weight"].any()
    # unsorted and duplicate requests: flow indices are the call's
    rng = np.random.default_rng(2)
    order = np.concatenate([rng.permutation(420), rng.integers(0, 420, 60)])
    e2 = ExpectedLoad(g, sv[order], dv[order], w[order], verts)
    x2 = ExpectedCrossings(g, e2, w[order], edges, vertices)
    assert x2.total > xc.total
    check_crossings(top.link_crossings(sip[order], dip[order], edges, vertices, w[order]), x2)
    # wrapping: two flows of weight 2^63 over one watched edge
    i = int(np.nonzero(sv != dv)[0][0])
    e = exp.edges[i][0]
    two = np.asarray([i, i])
    w63 = np.full(2, 2**63, np.uint64)
    out = top.link_crossings(sip[two], dip[two], [e], [], w63)
    assert out["total"] == 2 and out["count"].tolist() == [2] and out["weight"].tolist() == [0]
    assert out["records"]["flow"].tolist() == [0, 1]
    # a watched source vertex gets records only from self pairs (a route arrives nowhere at its
    # first vertex)
    s0 = int(verts[0])
    out = top.link_crossings(sip[:70], dip[:70], [], [s0])
    assert out["records"]["flow"].tolist() == np.nonzero(dv[:70] == s0)[0].tolist() == [0]
    assert out["records"]["hop"].tolist() == [0] and out["count"].tolist() == [1]


def test_watch_weights_equal_the_link_load(grid):
    """A cross-check, not the primary oracle: per watch the summed weight is the link load's."""
    top, g, ips, verts = grid
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp, xc, edges, vertices = tie_grid_expected(False, tuple(int(v) for v in verts))
    w = tie_grid_weights()
    out = top.link_crossings(sip, dip, edges, vertices, w)
    load = top.link_load(sip, dip, w)
    ne = len(edges)
    assert np.array_equal(out["weight"][:ne], (load["edge_fwd"] + load["edge_rev"])[edges])
    assert np.array_equal(out["weight"][ne:], load["vertex"][vertices])
    by = sa.crossings_by_watch(out)
    assert all(len(by[k]) == out["count"][k] for k in by)


def check_trace(tr, exp):
    """A trace's routes equal the oracle's chains (vertex by vertex, edge by edge)."""
    assert np.all(tr["status"] == 0) and np.array_equal(tr["hops"], exp.hops)
    for i in range(len(exp.verts)):
        o, h = int(tr["offset"][i]), int(tr["hops"][i])
        assert list(tr["vertices"][o:o + h + 1]) == exp.verts[i], i
        assert list(tr["edges"][o:o + h]) == exp.edges[i], i


@pytest.mark.parametrize("tie_free", [False, True])
def test_crossings_leave_stats_table_lazy_rows_traces_and_loads_alone(tie_free):
    if tie_free:
        top, g, av, ips = random_hosts(real_graphml(), 100)
        verts = av
    else:
        top, g, ips, verts = pinned(tie_grid_graphml(False), 70)
    assert top.latency_ip(ips[0], ips[1]) > 0  # builds the table, materialises a lazy row
    a0, lat0, rel0, hops0 = top.table()
    sip, dip, sv, dv = all_pairs(ips, verts, 4)
    exp = ExpectedLoad(g, sv, dv, None, verts)
    edges, vertices = watch_recipe(exp, sv, dv)
    xc = ExpectedCrossings(g, exp, None, edges, vertices)
    check_trace(top.trace_routes(sip, dip), exp)
    check_load(top.link_load(sip, dip), exp)
    st0, ts0, ls0 = top.stats(), top.trace_stats(), top.link_load_stats()
    lz0 = top.lazy_rows()
    lm0 = top.lazyMinimumLatency()
    check_crossings(top.link_crossings(sip, dip, edges, vertices), xc)
    assert top.stats() == st0 and top.trace_stats() == ts0 and top.link_load_stats() == ls0
    assert all(np.array_equal(x, y) for x, y in zip(top.lazy_rows(), lz0))
    assert top.lazyMinimumLatency() == lm0
    a1, lat1, rel1, hops1 = top.table()
    assert top.stats() == st0  # no rebuild
    assert np.array_equal(a0, a1) and np.array_equal(hops0, hops1)
    assert lat0.tobytes() == lat1.tobytes() and rel0.tobytes() == rel1.tobytes()
    check_trace(top.trace_routes(sip, dip), exp)  # the same slots, used again
    check_load(top.link_load(sip, dip), exp)
    check_crossings(top.link_crossings(sip, dip, edges, vertices), xc)
    assert top.stats() == st0


def test_multi_device_topology_answers_on_its_first_device():
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70, [("devices", 2)])
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp, xc, edges, vertices = tie_grid_expected(False, tuple(int(v) for v in verts))
    top.table()
    st0 = top.stats()
    assert st0["devices"] == 2
    check_crossings(top.link_crossings(sip, dip, edges, vertices, tie_grid_weights()), xc)
    assert top.stats() == st0
