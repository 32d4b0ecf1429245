"""GPU tests of the link load (shdtopo_link_load, topo_load.hip): the weight a set of flows puts
on every edge (forward and reverse half) and vertex, compared exactly -- unsigned 64-bit sums --
with loads derived from the CPU oracle's chains (load_helpers.ExpectedLoad: g.dijkstra for the
parents, g.get_eid for each hop's edge).  Both implementations run: the leaf-to-root tree
accumulation (option load_walk = 0) and the per-request walk (1).  Every graph has at most 700
vertices.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import host_ip, random_topology_graphml
from load_helpers import (TRANSIT_POI, ExpectedLoad, all_pairs, check_load, long_chain_graphml,
                          pairs_crossing_ties, pinned, random_hosts, tie_grid_graphml,
                          transit_grid_graphml)
from shadow_amd import _lib

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# expected values, computed once per graph and shared (never modified)
# ------------------------------------------------------------------------------------------
def tie_grid_weights():
    return np.random.default_rng(21).integers(1, 2**40, 420, endpoint=True).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def tie_grid_expected(directed, verts):
    """6 sources x 70 destinations on the tie grid with random weights in [1, 2^40]."""
    g = oracle.OGraph.from_graphml(tie_grid_graphml(directed))
    v = np.asarray(verts, np.int32)
    exp = ExpectedLoad(g, np.repeat(v[:6], 70), np.tile(v, 6), tie_grid_weights(), v)
    return exp, pairs_crossing_ties(g, exp)


@functools.lru_cache(maxsize=None)
def transit_expected(directed, verts, nsrc):
    g = oracle.OGraph.from_graphml(transit_grid_graphml(directed))
    v = np.asarray(verts, np.int32)
    return ExpectedLoad(g, np.repeat(v[:nsrc], len(v)), np.tile(v, nsrc), None, v)


# ------------------------------------------------------------------------------------------
# loads against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("directed,int_keys", [(False, 1), (False, 0), (True, 1), (True, 0)])
def test_tie_grid_loads(directed, int_keys, walk):
    """Ties across most chains: at least 100 requested pairs cross a vertex whose parent igraph's
    pop order decides; weights up to 2^40."""
    top, g, ips, verts = pinned(tie_grid_graphml(directed), 70,
                                [("replay_int_keys", int_keys), ("load_walk", walk)])
    assert top.is_directed == directed
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp, crossing = tie_grid_expected(directed, tuple(int(v) for v in verts))
    assert crossing >= 100, crossing
    out = top.link_load(sip, dip, tie_grid_weights())
    check_load(out, exp)
    if directed:
        assert not out["edge_rev"].any()
    else:
        assert out["edge_rev"].any()
    ls = top.link_load_stats()
    assert ls["requests"] == 420 and ls["routed"] == 420 and ls["sources"] == 6
    assert ls["unattached"] == 0 and ls["broken"] == 0
    assert ls["hop_weight"] == exp.hop_weight
    assert ls["tree_vertices"] == (0 if walk else exp.tree_vertices)


@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("directed", [False, True])
def test_transit_grid_loads(directed, walk):
    """Destinations on other destinations' chains, and branching union trees."""
    top, g, ips, verts = pinned(transit_grid_graphml(directed), TRANSIT_POI,
                                [("load_walk", walk)])
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp = transit_expected(directed, tuple(int(v) for v in verts), 6)
    # conditions on the input (from the oracle's chains), not on the code under test
    assert exp.transit_destinations() >= 80, exp.transit_destinations()
    assert exp.branching() >= 100, exp.branching()
    check_load(top.link_load(sip, dip), exp)
    ls = top.link_load_stats()
    assert ls["hop_weight"] == int(exp.hops.sum())
    assert ls["tree_vertices"] == (0 if walk else exp.tree_vertices)
    assert ls["sources"] == 6 and ls["chunks"] == 1


@pytest.mark.parametrize("walk", [0, 1])
def test_all_pairs_loads_sum_to_the_table_hops(walk):
    top, g, ips, verts = pinned(transit_grid_graphml(False), TRANSIT_POI, [("load_walk", walk)])
    sip, dip, sv, dv = all_pairs(ips, verts, TRANSIT_POI)
    exp = transit_expected(False, tuple(int(v) for v in verts), TRANSIT_POI)
    out = top.link_load(sip, dip, np.ones(len(sip), np.uint64))
    check_load(out, exp)
    a, lat, rel, hops = top.table()
    assert int(out["edge_fwd"].sum() + out["edge_rev"].sum()) == int(hops.astype(np.int64).sum())
    assert top.link_load_stats()["hop_weight"] == int(hops.astype(np.int64).sum())


@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("directed", [False, True])
def test_multigraph_charges_the_lowest_edge_id(directed, walk):
    data = random_topology_graphml(n_routers=400, n_poi=40, extra=1600, seed=9, integer=True,
                                   directed=directed, parallel=400)
    top, g, av, aip = random_hosts(data, 120, [("load_walk", walk)])
    sip, dip, sv, dv = all_pairs(aip, av, 6)
    exp = ExpectedLoad(g, sv, dv, None, av)
    out = top.link_load(sip, dip)
    check_load(out, exp)
    key = (lambda a, b: (a, b)) if directed else (lambda a, b: (min(a, b), max(a, b)))
    lowest, mult = {}, {}
    for e, (a, b) in enumerate(zip(g.eu.tolist(), g.ev.tolist())):
        lowest.setdefault(key(a, b), e)
        mult[key(a, b)] = mult.get(key(a, b), 0) + 1
    charged = np.nonzero(out["edge_fwd"] + out["edge_rev"])[0]
    assert all(lowest[key(int(g.eu[e]), int(g.ev[e]))] == e for e in charged)
    on_group = sum(1 for c in exp.verts for a, b in zip(c[:-1], c[1:])
                   if a != b and mult[key(a, b)] > 1)
    assert on_group > 50, on_group


@pytest.mark.parametrize("walk", [0, 1])
def test_long_chain_loads(walk):
    top, g, ips, verts = pinned(long_chain_graphml(), 3, [("load_walk", walk)])
    sip, dip, sv, dv = all_pairs(ips, verts, 3)
    w = np.asarray([3, 5, 7, 11, 13, 17, 19, 23, 29], np.uint64) << np.uint64(33)
    exp = ExpectedLoad(g, sv, dv, w, verts)
    assert exp.hops.reshape(3, 3).tolist() == [[1, 201, 102], [201, 1, 101], [102, 101, 1]]
    check_load(top.link_load(sip, dip, w), exp)
    assert top.link_load_stats()["hop_weight"] == exp.hop_weight


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


@pytest.mark.parametrize("walk", [0, 1])
def test_duplicates_order_self_pairs_and_unattached_ends(walk):
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70, [("load_walk", walk)])
    v2, _ = top.attach_ip(host_ip(500), 99, typeHint="t7")  # a second host on poi 7
    assert v2 == verts[7]
    rng = np.random.default_rng(2)
    si = rng.integers(0, 5, 80)
    di = rng.integers(0, 70, 80)
    si[10:20], di[10:20] = si[:10], di[:10]  # duplicates
    di[20:26] = si[20:26]                    # self pairs
    sip, dip = ips[si], ips[di]
    sv, dv = verts[si], verts[di]
    # two hosts on one vertex, both ways
    sip = np.concatenate([sip, [ips[7], host_ip(500)]]).astype(np.uint32)
    dip = np.concatenate([dip, [host_ip(500), ips[7]]]).astype(np.uint32)
    sv = np.concatenate([sv, [v2, v2]])
    dv = np.concatenate([dv, [v2, v2]])
    w = rng.integers(1, 2**40, len(sip)).astype(np.uint64)
    order = rng.permutation(len(sip))
    sip, dip, sv, dv, w = sip[order], dip[order], sv[order], dv[order], w[order]
    exp = ExpectedLoad(g, sv, dv, w, verts)
    loop = g.get_eid(v2, v2)
    assert g.eu[loop] == v2 == g.ev[loop] and exp.edge_fwd[loop] > 0
    out = top.link_load(sip, dip, w)
    check_load(out, exp)
    ls = top.link_load_stats()
    assert ls["unattached"] == 0 and ls["broken"] == 0 and ls["routed"] == len(sip)
    # an unattached IP at either end is counted and changes nothing else
    stranger = sa.ip_to_network("10.9.8.7")
    sip2 = np.concatenate([[stranger], sip, [ips[3]]]).astype(np.uint32)
    dip2 = np.concatenate([[ips[4]], dip, [stranger]]).astype(np.uint32)
    w2 = np.concatenate([[1 << 50], w, [1 << 51]]).astype(np.uint64)
    out2 = top.link_load(sip2, dip2, w2)
    check_load(out2, exp)
    ls2 = top.link_load_stats()
    assert ls2["unattached"] == 2 and ls2["routed"] == len(sip) and ls2["requests"] == len(sip2)
    assert ls2["hop_weight"] == exp.hop_weight


@pytest.mark.parametrize("walk", [0, 1])
def test_chunked_load_is_byte_identical(grid, walk):
    top, g, ips, verts = grid
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    w = tie_grid_weights()
    top.set_option("load_walk", walk)
    try:
        a = top.link_load(sip, dip, w)
        assert top.link_load_stats()["chunks"] == 1
        top.set_option("trace_chunk", 2)
        b = top.link_load(sip, dip, w)
        ls = top.link_load_stats()
        assert ls["chunks"] == 3 and ls["sources"] == 6
    finally:
        top.set_option("trace_chunk", 0)
        top.set_option("load_walk", 1)
    for k in ("edge_fwd", "edge_rev", "vertex"):
        assert a[k].tobytes() == b[k].tobytes(), k
    check_load(b, tie_grid_expected(False, tuple(int(v) for v in verts))[0])


def test_multi_device_topology_loads_on_its_first_device():
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70, [("devices", 2)])
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    top.table()
    st0 = top.stats()
    assert st0["devices"] == 2
    out = top.link_load(sip, dip, tie_grid_weights())
    check_load(out, tie_grid_expected(False, tuple(int(v) for v in verts))[0])
    assert top.stats() == st0


def check_trace(tr, exp):
    """A trace's routes equal the oracle's chains (vertex by vertex, edge by edge)."""
    assert np.all(tr["status"] == 0) and np.array_equal(tr["hops"], exp.hops)
    for i in range(len(exp.verts)):
        o, h = int(tr["offset"][i]), int(tr["hops"][i])
        assert list(tr["vertices"][o:o + h + 1]) == exp.verts[i], i
        assert list(tr["edges"][o:o + h]) == exp.edges[i], i


@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("tie_free", [False, True])
def test_load_leaves_stats_table_lazy_rows_and_traces_alone(tie_free, walk):
    """After a link load the last build's statistics, the table and the materialised lazy rows are
    what they were -- also when the call is the first use of the replay (a tie-free build replays
    no row).  The vertex-record words the accumulation reuses are re-initialised by the next
    replay: a trace after a load, and a load after a trace, still equal the oracle."""
    if tie_free:
        top, g, av, ips = random_hosts(random_topology_graphml(600, 60, 2400, seed=3), 100)
        verts = av
    else:
        top, g, ips, verts = pinned(tie_grid_graphml(False), 70)
    top.set_option("load_walk", walk)
    assert top.latency_ip(ips[0], ips[1]) > 0  # builds the table, materialises a lazy row
    a0, lat0, rel0, hops0 = top.table()
    st0 = top.stats()
    lz0 = top.lazy_rows()
    lm0 = top.lazyMinimumLatency()
    if tie_free:
        assert st0["replay_rows"] == 0
    sip, dip, sv, dv = all_pairs(ips, verts, 4)
    exp = ExpectedLoad(g, sv, dv, None, verts)
    check_load(top.link_load(sip, dip), exp)
    assert top.stats() == st0
    assert all(np.array_equal(x, y) for x, y in zip(top.lazy_rows(), lz0))
    assert top.lazyMinimumLatency() == lm0
    a1, lat1, rel1, hops1 = top.table()
    assert top.stats() == st0  # no rebuild
    assert np.array_equal(a0, a1) and np.array_equal(hops0, hops1)
    assert lat0.tobytes() == lat1.tobytes() and rel0.tobytes() == rel1.tobytes()
    check_trace(top.trace_routes(sip, dip), exp)  # the same slots, replayed again
    check_load(top.link_load(sip, dip), exp)      # and a load after a trace
    assert top.stats() == st0


def test_output_buffers(grid):
    """NULL outputs are accepted; buffers are overwritten, not added to; nothing beyond 2E / V
    is written."""
    top, g, ips, verts = grid
    lib, _ = _lib.load()
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    sip, dip = np.ascontiguousarray(sip), np.ascontiguousarray(dip)
    w = tie_grid_weights()
    exp = tie_grid_expected(False, tuple(int(v) for v in verts))[0]
    n, E, V, G = len(sip), g.E, g.V, 16
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
    eb = np.full(2 * E + 2 * G, sentinel, np.uint64)
    vb = np.full(V + 2 * G, sentinel, np.uint64)
    pe = ctypes.c_void_p(eb.ctypes.data + 8 * G)
    pv = ctypes.c_void_p(vb.ctypes.data + 8 * G)

    def check_edges():
        assert np.array_equal(eb[G:G + E], exp.edge_fwd)
        assert np.array_equal(eb[G + E:G + 2 * E], exp.edge_rev)
        assert np.all(eb[:G] == sentinel) and np.all(eb[G + 2 * E:] == sentinel)

    def check_vertices():
        assert np.array_equal(vb[G:G + V], exp.vertex)
        assert np.all(vb[:G] == sentinel) and np.all(vb[G + V:] == sentinel)
    assert lib.shdtopo_link_load(top._h, p(sip), p(dip), p(w), n, pe, pv) == n
    check_edges()
    check_vertices()
    assert lib.shdtopo_link_load(top._h, p(sip), p(dip), p(w), n, pe, pv) == n  # not added to
    check_edges()
    check_vertices()
    eb[G:G + 2 * E] = sentinel
    vb[G:G + V] = sentinel
    assert lib.shdtopo_link_load(top._h, p(sip), p(dip), p(w), n, None, pv) == n
    check_vertices()
    assert np.all(eb == sentinel)
    vb[G:G + V] = sentinel
    assert lib.shdtopo_link_load(top._h, p(sip), p(dip), p(w), n, pe, None) == n
    check_edges()
    assert np.all(vb == sentinel)
    assert lib.shdtopo_link_load(top._h, p(sip), p(dip), p(w), n, None, None) == n
    # no request: the outputs are still overwritten
    assert lib.shdtopo_link_load(top._h, None, None, None, 0, pe, pv) == 0
    assert not eb[G:G + 2 * E].any() and not vb[G:G + V].any()
    assert np.all(eb[:G] == sentinel) and np.all(vb[G + V:] == sentinel)
