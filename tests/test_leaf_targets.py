"""Leaf targets (option "leaf_targets"): an attached vertex with one non-loop edge
is resolved from its uplink -- d(t) = fl(d(u) + w), parent(t) = u -- instead of the graph search.

Every table is compared bit for bit with the CPU oracle and with the same topology built with
leaf_targets = 0.  Uplinks carry random latencies and non-zero random losses, so a misplaced or
missing factor of the reliability product shows.  The expected number of peeled targets is a
brute-force degree count over the test's own edge list.
"""
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import graphml_doc, host_ip
from load_helpers import ExpectedLoad, check_load
from test_trace import Expected, check_routes, check_table

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# graphs: (nodes, edges) lists; poi k has the type t<k>, so host k is pinned to it
# ------------------------------------------------------------------------------------------
def router_core(rng, n, extra, integer):
    lat = (lambda: int(rng.integers(1, 101))) if integer else (lambda: rng.uniform(1, 100))
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(n)]
    edges = [("pop-%d" % i, "pop-%d" % ((i + 1) % n), lat(), rng.uniform(0, 0.01))
             for i in range(n)] if n > 2 else []
    seen = set()
    while len(seen) < extra:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        key = (min(a, b), max(a, b))
        if a == b or abs(a - b) in (1, n - 1) or key in seen:
            continue
        seen.add(key)
        edges.append(("pop-%d" % a, "pop-%d" % b, lat(), rng.uniform(0, 0.01)))
    return nodes, edges


def uplink(rng, integer):
    """(latency, loss) of a poi edge: random, the loss never zero."""
    return (int(rng.integers(1, 21)) if integer else rng.uniform(1, 50)), rng.uniform(0.001, 0.05)


@functools.lru_cache(maxsize=None)
def mixed_graph(n_routers=600, n_poi=60, extra=2400, seed=41, integer=False):
    """Routers (a ring plus random edges) and poi in groups of six: a single uplink; two uplinks
    (not peeled); a single uplink to the router of the group's first poi (two poi on one router);
    a two-edge poi -- a router uplink plus the next poi -- and that next poi, a leaf whose only
    neighbour is the two-edge poi; a single uplink.  Every poi has a self loop."""
    rng = np.random.default_rng(seed)
    nodes, edges = router_core(rng, n_routers, extra, integer)
    nodes += [("poi-%d" % k, "t%d" % k, rng.uniform(0, 0.05)) for k in range(n_poi)]
    first = 0
    for k in range(n_poi):
        p = "poi-%d" % k
        r = int(rng.integers(0, n_routers))
        kind = k % 6
        if kind == 0:
            first = r
        if kind == 2:
            r = first
        if kind == 4:
            edges.append((p, "poi-%d" % (k - 1), *uplink(rng, integer)))
        else:
            edges.append((p, "pop-%d" % r, *uplink(rng, integer)))
        if kind == 1:
            edges.append((p, "pop-%d" % ((r + 7) % n_routers), *uplink(rng, integer)))
        edges.append((p, p, 1.0, 0.001 * (k + 1)))
    order = rng.permutation(len(edges))
    return nodes, [edges[i] for i in order]


@functools.lru_cache(maxsize=None)
def star_graph():
    """One router with 12 leaf poi: the router is every source's own uplink.  (Its row holds only
    peeled vertices.)"""
    rng = np.random.default_rng(43)
    nodes = [("pop-0", "pop", 0.0)] + [("poi-%d" % k, "t%d" % k, rng.uniform(0, 0.05))
                                       for k in range(12)]
    edges = []
    for k in range(12):
        edges.append(("poi-%d" % k, "pop-0", *uplink(rng, False)))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.002 * (k + 1)))
    return nodes, edges


@functools.lru_cache(maxsize=None)
def pendants_graph():
    """Two poi joined by a single edge (the only connected graph with two mutually pendant
    vertices), a self loop each."""
    rng = np.random.default_rng(47)
    nodes = [("poi-%d" % k, "t%d" % k, rng.uniform(0, 0.05)) for k in range(2)]
    edges = [("poi-0", "poi-1", *uplink(rng, False))]
    edges += [("poi-%d" % k, "poi-%d" % k, 1.0, 0.003) for k in range(2)]
    return nodes, edges


CHAIN = 60


@functools.lru_cache(maxsize=None)
def chain_graph():
    """A path of 60 routers, a leaf poi at each end and at routers 13, 30 and 44: routes of up to
    61 hops, beyond the epilogue's path buffer (kMaxHops = 48)."""
    rng = np.random.default_rng(53)
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(CHAIN)]
    at = (0, CHAIN - 1, 13, 30, 44)
    nodes += [("poi-%d" % k, "t%d" % k, 0.01 * (k + 1)) for k in range(len(at))]
    edges = [("pop-%d" % i, "pop-%d" % (i + 1), rng.uniform(1, 100), rng.uniform(0.001, 0.01))
             for i in range(CHAIN - 1)]
    for k, r in enumerate(at):
        edges.append(("poi-%d" % k, "pop-%d" % r, *uplink(rng, False)))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.001))
    order = rng.permutation(len(edges))
    return nodes, [edges[i] for i in order]


@functools.lru_cache(maxsize=None)
def directed_graph():
    """Routers on a ring in both directions plus random arcs, poi with one arc each way."""
    rng = np.random.default_rng(59)
    n = 200
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(n)]
    nodes += [("poi-%d" % k, "t%d" % k, rng.uniform(0, 0.05)) for k in range(24)]
    edges = []
    for i in range(n):
        edges.append(("pop-%d" % i, "pop-%d" % ((i + 1) % n), rng.uniform(1, 100), rng.uniform(0, 0.01)))
        edges.append(("pop-%d" % ((i + 1) % n), "pop-%d" % i, rng.uniform(1, 100), rng.uniform(0, 0.01)))
    seen = set()
    while len(seen) < 600:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a == b or abs(a - b) in (1, n - 1) or (a, b) in seen:
            continue
        seen.add((a, b))
        edges.append(("pop-%d" % a, "pop-%d" % b, rng.uniform(1, 100), rng.uniform(0, 0.01)))
    for k in range(24):
        r = "pop-%d" % int(rng.integers(0, n))
        edges.append(("poi-%d" % k, r, *uplink(rng, False)))
        edges.append((r, "poi-%d" % k, *uplink(rng, False)))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.001))
    order = rng.permutation(len(edges))
    return nodes, [edges[i] for i in order]


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def brute_force_peeled(graph, verts):
    """Attached vertices with exactly one non-loop edge whose other end has more than one."""
    nodes, edges = graph
    idx = {n[0]: i for i, n in enumerate(nodes)}
    nb = [[] for _ in nodes]
    for a, b, _, _ in edges:
        if a != b:
            nb[idx[a]].append(idx[b])
            nb[idx[b]].append(idx[a])
    return sum(1 for v in set(int(x) for x in verts)
               if len(nb[v]) == 1 and len(nb[nb[v][0]]) > 1)


def make(graph, options=(), directed=False):
    data = graphml_doc(*graph, directed)
    top = sa.Topology.from_buffer(data)
    for k, v in options:
        top.set_option(k, v)
    return top, data


def attach(tops, ks, graph):
    """Host k on poi k of every topology of tops; returns (ips, vertices)."""
    nodes = graph[0]
    idx = {n[0]: i for i, n in enumerate(nodes)}
    ips, verts = [], []
    for k in ks:
        st = (k * 2654435761 + 12345) & 0xFFFFFFFF
        for top in tops:
            v, _ = top.attach_ip(host_ip(k + 1), st, typeHint="t%d" % k)
            assert v == idx["poi-%d" % k]
        ips.append(host_ip(k + 1))
        verts.append(idx["poi-%d" % k])
    return ips, verts


def assert_tables(top, expect):
    a, lat, rel, hops = top.table()
    oa, olat, orel, ohops = expect
    assert np.array_equal(a, oa)
    assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64))
    assert np.array_equal(rel.view(np.uint64), orel.view(np.uint64))
    assert np.array_equal(hops, np.asarray(ohops).astype(np.uint16))
    return a, lat, rel, hops


def both_ways(graph, options, rounds, directed=False):
    """The topology with leaf_targets 1 and 0, hosts attached in `rounds`; after each round both
    tables equal the oracle's and peeled_targets the brute-force count (0 when off).  Returns the
    two topologies and (ips, verts)."""
    on, data = make(graph, options, directed)
    off, _ = make(graph, tuple(options) + (("leaf_targets", 0),), directed)
    g = oracle.OGraph.from_graphml(data)
    ips, verts = [], []
    for ks in rounds:
        i, v = attach((on, off), ks, graph)
        ips += i
        verts += v
        expect = g.table(verts)
        assert_tables(on, expect)
        assert_tables(off, expect)
        want = 0 if directed else brute_force_peeled(graph, verts)
        assert on.stats()["peeled_targets"] == want
        assert off.stats()["peeled_targets"] == 0
    return on, off, g, ips, verts


# ------------------------------------------------------------------------------------------
# 1. mixed attachment
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("skip,resort", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_mixed_attachment(integer, skip, resort):
    graph = mixed_graph(integer=integer)
    opts = (("target_skip", skip), ("target_resort", resort), ("tie_dense", 0), ("batch_fill", 8))
    # a late attach changes the target set (and the peeled set)
    on, off, g, ips, verts = both_ways(graph, opts, (range(0, 40), range(40, 60)))
    want = brute_force_peeled(graph, verts)
    assert want == 40  # per group of six: three single uplinks and the poi behind a poi
    # toggled on one topology, same target set: the copy's target-derived content is redone
    expect = g.table(verts)
    for leaf, n in ((0, 0), (1, want)):
        on.set_option("leaf_targets", leaf)
        on.rebuild()
        assert_tables(on, expect)
        assert on.stats()["peeled_targets"] == n


# ------------------------------------------------------------------------------------------
# 2. everything in LDS; the star
# ------------------------------------------------------------------------------------------
@gpu
def test_every_vertex_an_lds_hub():
    graph = mixed_graph(n_routers=40, n_poi=12, extra=60, seed=61)
    on, off, g, ips, verts = both_ways(graph, (("batch_fill", 8),), (range(12),))
    assert on.stats()["lds_hubs"] >= len(graph[0])
    assert on.stats()["peeled_targets"] == 8


@gpu
@pytest.mark.parametrize("skip", [1, 0])
def test_star_of_leaf_poi(skip):
    on, off, g, ips, verts = both_ways(star_graph(), (("target_skip", skip),), (range(12),))
    assert on.stats()["peeled_targets"] == 12


# ------------------------------------------------------------------------------------------
# 3. two pendants
# ------------------------------------------------------------------------------------------
@gpu
def test_two_mutually_pendant_poi():
    graph = pendants_graph()
    assert brute_force_peeled(graph, [0, 1]) == 0  # neither: each one's neighbour has one edge
    on, off, g, ips, verts = both_ways(graph, (), (range(2),))
    assert on.stats()["peeled_targets"] <= 1


# ------------------------------------------------------------------------------------------
# 4. long paths
# ------------------------------------------------------------------------------------------
@gpu
def test_long_paths_take_the_fallback():
    on, off, g, ips, verts = both_ways(chain_graph(), (), (range(5),))
    assert on.stats()["peeled_targets"] == 5
    assert on.stats()["long_paths"] > 0 and on.stats()["long_paths"] == off.stats()["long_paths"]


# ------------------------------------------------------------------------------------------
# 5. line reuse across batches
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("integer", [False, True])
def test_single_slot_line_reuse(integer):
    graph = mixed_graph(integer=integer)
    opts = (("slots", 1), ("batch_fill", 3), ("tie_dense", 0))
    both_ways(graph, opts, (range(0, 35), range(35, 60)))


# ------------------------------------------------------------------------------------------
# 6. keep launch: route traces and link load from the batch kernel's records
# ------------------------------------------------------------------------------------------
def trace_requests(ips, verts, src):
    """Every host of src to every host: destinations and sources that are peeled leaves, not
    peeled, and both; self pairs included."""
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    si = np.repeat(np.asarray(src), len(ips))
    di = np.tile(np.arange(len(ips)), len(src))
    return ips[si], ips[di], verts[si], verts[di]


@gpu
def test_keep_launch_routes_and_loads():
    graph = mixed_graph()
    on, off, g, ips, verts = both_ways(graph, (("batch_fill", 8),), (range(60),))
    # sources: a leaf, a two-uplink poi, the leaf sharing the first one's router, a two-edge poi,
    # the leaf behind it, a leaf
    src = [0, 1, 2, 3, 4, 5]
    sip, dip, sv, dv = trace_requests(ips, verts, src)
    exp = Expected(g, sv, dv, verts)
    routes = []
    for top in (on, off):
        tr = top.trace_routes(sip, dip)
        ts = top.trace_stats()
        assert ts["batch_sources"] + ts["batch_fallback"] == len(src) and ts["batch_sources"] > 0
        check_routes(tr, exp)
        check_table(top, tr, sv, dv)
        routes.append(tr)
    for k in ("offset", "hops", "status", "latency", "reliability", "vertices", "edges"):
        assert routes[0][k].tobytes() == routes[1][k].tobytes(), k
    w = np.random.default_rng(7).integers(1, 2**40, len(sip), endpoint=True).astype(np.uint64)
    lexp = ExpectedLoad(g, sv, dv, w, np.asarray(sorted(verts), np.int32))
    loads = []
    for top in (on, off):
        top.set_option("load_walk", 1)
        ld = top.link_load(sip, dip, w)
        assert top.link_load_stats()["batch_sources"] > 0
        check_load(ld, lexp)
        loads.append(ld)
    for k in ("edge_fwd", "edge_rev", "vertex"):
        assert loads[0][k].tobytes() == loads[1][k].tobytes(), k


# ------------------------------------------------------------------------------------------
# 7. directed topologies keep every target
# ------------------------------------------------------------------------------------------
@gpu
def test_directed_topology_peels_nothing():
    on, off, g, ips, verts = both_ways(directed_graph(), (("tie_dense", 0),), (range(24),),
                                       directed=True)
    assert on.is_directed and on.stats()["peeled_targets"] == 0
