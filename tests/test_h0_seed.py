"""Option "h0_seed" (DESIGN.md 4 item 2): the batch kernel's landmark bound d_j(h0) of source j
starts at the prepared d(s_j, h0), scaled up past the rounding of either summation order, instead
of +inf.  The seed only prunes work that can neither set nor tie a final value, so every table
must be what it was.

Every case builds the same topology with h0_seed 1 and 0 and compares both tables with the CPU
oracle bit for bit, and hops, getMinimumLatency, ambiguous_pairs and replay_rows with each other.
"""
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from shadow_amd import _lib as L
from helpers import attach_hosts, graphml_doc, host_ip
from load_helpers import ExpectedLoad, check_load
from test_leaf_targets import (assert_tables, attach, mixed_graph, router_core, trace_requests,
                               uplink)
from test_replay import _one_way_regions_graphml
from test_trace import Expected, check_routes, check_table

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def make_pair(data, options=()):
    """The topology twice: h0_seed 1 and 0, the other options alike."""
    tops = []
    for seed in (1, 0):
        top = sa.Topology.from_buffer(data)
        assert top is not None
        for k, v in options:
            top.set_option(k, v)
        top.set_option("h0_seed", seed)
        tops.append(top)
    return tops


def compare(on, off, g, verts):
    """Both tables equal the oracle's (so each other) bit for bit; the scalars agree."""
    expect = g.table(verts)
    ta = assert_tables(on, expect)
    tb = assert_tables(off, expect)
    for x, y in zip(ta, tb):
        assert x.tobytes() == y.tobytes()
    assert on.getMinimumLatency() == off.getMinimumLatency()
    so, sf = on.stats(), off.stats()
    for k in ("ambiguous_pairs", "replay_rows", "errors", "long_paths"):
        assert so[k] == sf[k], k
    assert so["errors"] == 0
    return so, sf


def graph_pair(graph, options, rounds, directed=False):
    data = graphml_doc(*graph, directed)
    on, off = make_pair(data, options)
    g = oracle.OGraph.from_graphml(data)
    ips, verts = [], []
    for ks in rounds:
        i, v = attach((on, off), ks, graph)
        ips += i
        verts += v
        so, sf = compare(on, off, g, verts)
    return on, off, g, ips, verts, so, sf


def host_seed(p, V):
    lib, _ = L.load()
    return float(lib.shdtopo_test_h0_seed(float(p), int(V)))


# ------------------------------------------------------------------------------------------
# 1. rounding direction: the prepared sum runs from h0, the kernel's from the source
# ------------------------------------------------------------------------------------------
PATH = 400
STAR = 40
PATH_POI = (PATH - 1, PATH - 1, PATH - 1, 377, 300, 211, 120, 61, 20, 1)  # the poi's routers


@functools.lru_cache(maxsize=None)
def rounding_graph():
    """A path of 400 routers, latencies 10^U(-3, 3) (full-mantissa draws), a star of 40 leaves on
    router 0 (the top hub, so h0), poi on the far end and along the path."""
    rng = np.random.default_rng(71)
    lat = 10.0 ** rng.uniform(-3, 3, PATH - 1)
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(PATH)]
    nodes += [("leaf-%d" % i, "pop", 0.0) for i in range(STAR)]
    nodes += [("poi-%d" % k, "t%d" % k, 0.01 * (k + 1)) for k in range(len(PATH_POI))]
    edges = [("pop-%d" % i, "pop-%d" % (i + 1), float(lat[i]), rng.uniform(0.001, 0.01))
             for i in range(PATH - 1)]
    edges += [("leaf-%d" % i, "pop-0", float(10.0 ** rng.uniform(-3, 3)), 0.001)
              for i in range(STAR)]
    ups = []
    for k, r in enumerate(PATH_POI):
        w = float(10.0 ** rng.uniform(-3, 3))
        ups.append(w)
        edges.append(("poi-%d" % k, "pop-%d" % r, w, rng.uniform(0.001, 0.05)))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.001))
    order = rng.permutation(len(edges))
    return (nodes, [edges[i] for i in order]), lat, ups


def fold(ws):
    s = 0.0
    for w in ws:
        s = s + float(w)  # one IEEE add per hop
    return s


@gpu
def test_rounding_direction():
    graph, lat, ups = rounding_graph()
    V = len(graph[0])
    # precondition (CPU): per source the sum from the source end (the kernel's d_j(h0)) and from
    # the h0 end (the preparation's pi(s)); they differ in their last bits for some source, and
    # every forward sum is <= the seed made from the backward one
    fwd, bwd = [], []
    for k, r in enumerate(PATH_POI):
        chain = list(lat[:r])  # edges pop-0 .. pop-r, from the h0 end
        bwd.append(fold(chain + [ups[k]]))
        fwd.append(fold([ups[k]] + chain[::-1]))
    assert any(f != b for f, b in zip(fwd, bwd))
    assert any(f > b for f, b in zip(fwd, bwd))  # the direction the seed's margin is for
    seeds = [host_seed(b, V) for b in bwd]
    assert all(f <= s for f, s in zip(fwd, seeds))
    on, off, g, ips, verts, so, sf = graph_pair(graph, (("batch_fill", 8),),
                                                (range(len(PATH_POI)),))
    # the model above is the library's: router 0 is h0 and pi(source) the backward sum
    prep = on.export_prep(["inv", "pot"])
    assert prep["inv"][0] == 0
    pot = prep["pot"][prep["inv"][np.asarray(verts)]]
    assert pot.view(np.uint64).tolist() == np.asarray(bwd).view(np.uint64).tolist()
    assert so["long_paths"] > 0  # routes of up to 400 hops


# ------------------------------------------------------------------------------------------
# 2. the source is h0, is adjacent to h0, is an LDS hub
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hub_sources_graph():
    """300 routers (a ring plus 600 random edges, degree ~6) and poi that are hubs themselves:
    poi-0 with 60 router edges (the top hub: h0), poi-1 on poi-0 and two routers, poi-2 with 30
    router edges, poi-3 .. poi-9 with a single uplink.  A self loop each."""
    rng = np.random.default_rng(73)
    nodes, edges = router_core(rng, 300, 600, False)
    nodes += [("poi-%d" % k, "t%d" % k, rng.uniform(0, 0.05)) for k in range(10)]
    for r in rng.choice(300, 60, replace=False):
        edges.append(("poi-0", "pop-%d" % int(r), *uplink(rng, False)))
    edges.append(("poi-1", "poi-0", *uplink(rng, False)))
    for r in rng.choice(300, 2, replace=False):
        edges.append(("poi-1", "pop-%d" % int(r), *uplink(rng, False)))
    for r in rng.choice(300, 30, replace=False):
        edges.append(("poi-2", "pop-%d" % int(r), *uplink(rng, False)))
    for k in range(3, 10):
        edges.append(("poi-%d" % k, "pop-%d" % int(rng.integers(0, 300)), *uplink(rng, False)))
    for k in range(10):
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.001 * (k + 1)))
    order = rng.permutation(len(edges))
    return nodes, [edges[i] for i in order]


@gpu
@pytest.mark.parametrize("fill", [8, 2])
def test_source_is_h0_adjacent_to_it_or_an_lds_hub(fill):
    graph = hub_sources_graph()
    opts = (("lds_hubs", 32), ("batch_fill", fill))
    on, off, g, ips, verts, so, sf = graph_pair(graph, opts, (range(10),))
    assert so["lds_hubs"] == 32 < len(graph[0])  # hubs in LDS and a tail in HBM
    inv = on.export_prep(["inv"])["inv"]
    assert inv[verts[0]] == 0        # poi-0 is h0: seed 0
    assert 0 < inv[verts[2]] < 32    # poi-2 is an LDS hub
    assert inv[verts[5]] >= 32       # a pendant poi lives in the tail


# ------------------------------------------------------------------------------------------
# 3. no route to h0
# ------------------------------------------------------------------------------------------
def test_second_component_is_refused_at_load():
    """A source without a route to h0 would get the seed +inf (test_h0_seed_cpu.py), but no such
    source reaches the kernel: an undirected graph with a second component is refused when it is
    loaded, as the reference refuses it (shd-topology.c:134-151)."""
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(6)]
    nodes += [("poi-%d" % k, "t%d" % k, 0.01) for k in range(4)]
    edges = [("pop-0", "pop-1", 3.0, 0.0), ("pop-1", "pop-2", 4.0, 0.0), ("pop-2", "pop-0", 5.0, 0.0),
             ("pop-3", "pop-4", 3.5, 0.0), ("pop-4", "pop-5", 4.5, 0.0),  # the second component
             ("poi-0", "pop-0", 1.0, 0.0), ("poi-1", "pop-2", 1.5, 0.0),
             ("poi-2", "pop-3", 2.0, 0.0), ("poi-3", "pop-5", 2.5, 0.0)]
    edges += [("poi-%d" % k, "poi-%d" % k, 1.0, 0.0) for k in range(4)]
    top = sa.Topology.from_buffer(graphml_doc(nodes, edges))
    assert top is None or not getattr(top, "_h", None)


@gpu
def test_directed_near_one_way_regions():
    """Seeds from the in-row distances d(v -> h0): huge for the sink region (one 5,000 ms arc
    out), small for the source region."""
    data = _one_way_regions_graphml()
    on, off = make_pair(data, (("tie_dense", 0),))
    g = oracle.OGraph.from_graphml(data)
    _, _, verts = attach_hosts(on, g, 90)
    _, _, verts2 = attach_hosts(off, g, 90)
    assert verts == verts2 and on.is_directed
    compare(on, off, g, verts)
    prep = on.export_prep(["inv", "pot_src"])
    ps = prep["pot_src"][prep["inv"][np.asarray(verts)]]
    assert bool(np.isfinite(ps).all()) and ps.max() > 5000.0 and ps.min() < 200.0


# ------------------------------------------------------------------------------------------
# 4. every vertex in LDS; one slot reused by every batch
# ------------------------------------------------------------------------------------------
@gpu
def test_every_vertex_an_lds_hub():
    graph = mixed_graph(n_routers=40, n_poi=12, extra=60, seed=61)
    on, off, g, ips, verts, so, sf = graph_pair(graph, (("batch_fill", 8),), (range(12),))
    assert so["lds_hubs"] >= len(graph[0])


@gpu
@pytest.mark.parametrize("integer", [False, True])
def test_single_slot_reused_by_every_batch(integer):
    """slots 1, three sources per batch: the workgroup's LDS seeds are rewritten 20 times; a late
    attach changes the batches' composition."""
    graph = mixed_graph(integer=integer)
    opts = (("slots", 1), ("batch_fill", 3), ("tie_dense", 0))
    graph_pair(graph, opts, (range(0, 35), range(35, 60)))


# ------------------------------------------------------------------------------------------
# 5. ties
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_graph():
    """mixed_graph's structure with every latency in {1, 2, 3}: most distances are tied."""
    nodes, edges = mixed_graph(n_routers=300, n_poi=60, extra=1200, seed=79, integer=True)
    return nodes, [(a, b, 1 + int(w) % 3, loss) for a, b, w, loss in edges]


@gpu
@pytest.mark.parametrize("skip", [1, 0])
def test_integer_ties(skip):
    """Tie bits and parents need every tight relaxation: the flagged rows and the ambiguous pairs
    are the same with and without the seed."""
    graph = tie_graph()
    opts = (("tie_dense", 0), ("batch_fill", 8), ("target_skip", skip))
    on, off, g, ips, verts, so, sf = graph_pair(graph, opts, (range(60),))
    assert so["ambiguous_pairs"] > 0 and so["replay_rows"] > 0


# ------------------------------------------------------------------------------------------
# 6. a small power-law synthetic; the seed must not disable pruning
# ------------------------------------------------------------------------------------------
def synthetic_tops(batch, seeds):
    """Topology.synthetic once per entry of seeds (the h0_seed option), the same hosts on each."""
    tops = []
    for s in seeds:
        top = sa.Topology.synthetic(seed=29, n_routers=4000, n_poi=96, n_edges=40000)
        top.set_option("batch", batch)
        top.set_option("batch_fill", batch)
        top.set_option("h0_seed", s)
        tops.append(top)
    st, verts = 1, []
    for k in range(400):  # several hosts per poi: ~90 of the 96 poi become sources
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        vs = {top.attach_ip(host_ip(k + 1), st, typeHint=("client", "relay")[k % 2])[0]
              for top in tops}
        assert len(vs) == 1
        verts.append(vs.pop())
    return tops, verts


@functools.lru_cache(maxsize=None)
def synthetic_oracle():
    import os
    import tempfile
    top = sa.Topology.synthetic(seed=29, n_routers=4000, n_poi=96, n_edges=40000)
    fd, path = tempfile.mkstemp(suffix=".graphml.xml")
    os.close(fd)
    try:
        top.write_graphml(path)
        return oracle.OGraph.from_graphml(path)
    finally:
        os.unlink(path)


@gpu
@pytest.mark.parametrize("batch", [8, 2])
def test_power_law_synthetic(batch):
    (on, off, off2), verts = synthetic_tops(batch, (1, 0, 0))
    g = synthetic_oracle()
    assert len(set(verts)) >= 64
    so, sf = compare(on, off, g, verts)
    assert_tables(off2, g.table(verts))
    sf2 = off2.stats()
    assert so["batch"] == batch
    # a guard against a seed that disables pruning, not a performance claim: the seeded build may
    # not exceed either seed-off build by more than those two differ from each other
    for k in ("expanded", "tail_relax"):
        a, b, c = so["events"][k], sf["events"][k], sf2["events"][k]
        spread = abs(b - c)
        print("h0_seed events %s batch %d: on %d, off %d and %d (spread %d)" % (k, batch, a, b, c,
                                                                                spread))
        assert b > 0 and c > 0
        assert a <= b + spread and a <= c + spread, k


# ------------------------------------------------------------------------------------------
# 7. keep launch: traces and link load from the batch kernel's records
# ------------------------------------------------------------------------------------------
@gpu
def test_keep_launch_routes_and_loads():
    graph = mixed_graph()
    on, off, g, ips, verts, so, sf = graph_pair(graph, (("batch_fill", 8),), (range(60),))
    src = [0, 1, 2, 3, 4, 5]
    sip, dip, sv, dv = trace_requests(ips, verts, src)
    exp = Expected(g, sv, dv, verts)
    routes = []
    for top in (on, off):
        tr = top.trace_routes(sip, dip)
        assert top.trace_stats()["batch_sources"] > 0
        check_routes(tr, exp)
        check_table(top, tr, sv, dv)
        routes.append(tr)
    for k in ("offset", "hops", "status", "latency", "reliability", "vertices", "edges"):
        assert routes[0][k].tobytes() == routes[1][k].tobytes(), k
    w = np.random.default_rng(7).integers(1, 2**40, len(sip), endpoint=True).astype(np.uint64)
    lexp = ExpectedLoad(g, sv, dv, w, np.asarray(sorted(verts), np.int32))
    loads = []
    for top in (on, off):
        ld = top.link_load(sip, dip, w)
        assert top.link_load_stats()["batch_sources"] > 0
        check_load(ld, lexp)
        loads.append(ld)
    for k in ("edge_fwd", "edge_rev", "vertex"):
        assert loads[0][k].tobytes() == loads[1][k].tobytes(), k


# ------------------------------------------------------------------------------------------
# 8. the option toggled between builds of one topology
# ------------------------------------------------------------------------------------------
@gpu
def test_option_toggled_between_builds():
    graph = mixed_graph()
    data = graphml_doc(*graph)
    top = sa.Topology.from_buffer(data)
    top.set_option("batch_fill", 8)
    g = oracle.OGraph.from_graphml(data)
    ips, verts = attach((top,), range(60), graph)
    expect = g.table(verts)
    for seed in (1, 0, 1):
        top.set_option("h0_seed", seed)
        top.rebuild()
        assert_tables(top, expect)
        assert top.stats()["errors"] == 0
