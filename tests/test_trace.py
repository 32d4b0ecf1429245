"""GPU tests of route tracing (shdtopo_trace_routes, topo_trace.hip): the vertex / edge path
behind a table entry, compared vertex by vertex and edge by edge against the oracle.

Expected routes are derived inside the tests from the CPU oracle: g.dijkstra(s, targets) gives the
parent vertices (the chain), g.get_eid(u, v) each hop's edge (never the relaxed edge pe: for a
parallel group the helper sums the lowest id), g.source_rows latency, reliability and hops.  On the
tie-free graph the vertex lists are also compared with chains walked over scipy's predecessor
trees.  Latency, reliability and hops must equal the table entry at [col(src)][col(dst)] bit for
bit.  Every graph has at most 700 vertices.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import attach_hosts, graphml_doc, host_ip, random_topology_graphml
from shadow_amd import _lib

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# fixtures' graphs
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_grid_graphml(directed=False):
    """16 x 16 router grid, integer latencies U{1, 2} (ties across most chains), 70 poi of a type
    of their own (a type hint pins a host to its poi) with an uplink of 5.0 and a self loop; edge
    order shuffled.  directed: two arcs per edge with independent latencies."""
    rng = np.random.default_rng(5)
    n, npoi = 16, 70
    rid = lambda i, j: "pop-%d" % (i * n + j)
    nodes = [(rid(i, j), "pop", 0.0) for i in range(n) for j in range(n)]
    nodes += [("poi-%d" % k, "t%d" % k, rng.uniform(0, 0.05)) for k in range(npoi)]
    edges = []

    def link(a, b):
        edges.append((a, b, int(rng.integers(1, 3)), rng.uniform(0, 0.01)))
        if directed:
            edges.append((b, a, int(rng.integers(1, 3)), rng.uniform(0, 0.01)))
    for i in range(n):
        for j in range(n):
            if j + 1 < n:
                link(rid(i, j), rid(i, j + 1))
            if i + 1 < n:
                link(rid(i, j), rid(i + 1, j))
    for k in range(npoi):
        r = "pop-%d" % int(rng.integers(0, n * n))
        edges.append(("poi-%d" % k, r, 5.0, 0.0))
        if directed:
            edges.append((r, "poi-%d" % k, 5.0, 0.0))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.001 * k))
    order = rng.permutation(len(edges))
    return graphml_doc(nodes, [edges[i] for i in order], directed)


@functools.lru_cache(maxsize=None)
def long_chain_graphml():
    """A path of 200 routers, poi at both ends and in the middle: routes of 201, 102 and 101
    hops, all beyond the table kernels' in-register path buffer (kMaxHops = 48)."""
    rng = np.random.default_rng(8)
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(200)]
    nodes += [("poi-%d" % k, "t%d" % k, 0.01 * (k + 1)) for k in range(3)]
    edges = [("pop-%d" % i, "pop-%d" % (i + 1), rng.uniform(1, 100), rng.uniform(0, 0.01))
             for i in range(199)]
    for k, r in enumerate((0, 199, 100)):
        edges.append(("poi-%d" % k, "pop-%d" % r, 5.0, 0.0))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.0))
    order = rng.permutation(len(edges))
    return graphml_doc(nodes, [edges[i] for i in order])


def pinned(data, npoi, options=()):
    """Product + oracle topology with host k pinned to poi k by its type hint.
    Returns (top, g, ips, verts)."""
    top = sa.Topology.from_buffer(data)
    g = oracle.OGraph.from_graphml(data)
    for k, v in options:
        top.set_option(k, v)
    otop, ips, verts = attach_hosts(top, g, npoi, type_hints=["t%d" % k for k in range(npoi)])
    assert len(set(verts)) == npoi
    return top, g, ips, verts


def random_hosts(data, n_hosts, options=()):
    top = sa.Topology.from_buffer(data)
    g = oracle.OGraph.from_graphml(data)
    for k, v in options:
        top.set_option(k, v)
    otop, ips, verts = attach_hosts(top, g, n_hosts, type_hints=["client", "relay", "server"])
    return top, g, ips, verts


# ------------------------------------------------------------------------------------------
# the oracle's routes
# ------------------------------------------------------------------------------------------
class Expected:
    """Routes of (sv[i], dv[i]) from the oracle: per request the vertex list, the get_eid edges,
    and {lat, rel, hops} of the helper; per source the dijkstra result (tie analysis)."""

    def __init__(self, g, sv, dv, targets):
        targets = np.asarray(sorted(set(int(t) for t in targets)), np.int32)
        self.verts, self.edges = [], []
        self.lat = np.empty(len(sv))
        self.rel = np.empty(len(sv))
        self.hops = np.empty(len(sv), np.int64)
        self.dij = {}
        for s in sorted(set(int(x) for x in sv)):
            self.dij[s] = g.dijkstra(s, targets)
            idx = [i for i in range(len(sv)) if sv[i] == s]
            lat, rel, hops = g.source_rows([s], [dv[i] for i in idx])
            self.lat[idx], self.rel[idx], self.hops[idx] = lat[0], rel[0], hops[0]
        for s, d in zip(sv, dv):
            s, d = int(s), int(d)
            if s == d:
                chain = [s, s]
            else:
                pv = self.dij[s][1]
                chain = [d]
                while chain[-1] != s:
                    assert pv[chain[-1]] >= 0 and len(chain) <= g.V
                    chain.append(int(pv[chain[-1]]))
                chain.reverse()
            self.verts.append(chain)
            self.edges.append([g.get_eid(a, b) for a, b in zip(chain[:-1], chain[1:])])

    def total(self):
        return sum(len(c) for c in self.verts)


def check_routes(tr, exp):
    """Every route of the trace equals the oracle's: vertices, edges, hops, latency and
    reliability bits, offsets = the running sum of hops + 1 in request order."""
    n = len(exp.verts)
    assert np.all(tr["status"] == 0), tr["status"]
    assert np.array_equal(tr["hops"], exp.hops)
    off = np.concatenate([[0], np.cumsum(exp.hops + 1)])
    assert np.array_equal(tr["offset"], off[:-1]) and tr["total"] == off[-1] == exp.total()
    assert np.array_equal(tr["latency"].view(np.uint64), exp.lat.view(np.uint64))
    assert np.array_equal(tr["reliability"].view(np.uint64), exp.rel.view(np.uint64))
    for i in range(n):
        o, h = int(tr["offset"][i]), int(tr["hops"][i])
        assert list(tr["vertices"][o:o + h + 1]) == exp.verts[i], i
        assert list(tr["edges"][o:o + h + 1]) == exp.edges[i] + [-1], i


def check_table(top, tr, sv, dv):
    a, lat, rel, hops = top.table()
    col = {int(v): k for k, v in enumerate(a)}
    cs = [col[int(v)] for v in sv]
    cd = [col[int(v)] for v in dv]
    assert np.array_equal(tr["latency"].view(np.uint64), lat[cs, cd].view(np.uint64))
    assert np.array_equal(tr["reliability"].view(np.uint64), rel[cs, cd].view(np.uint64))
    assert np.array_equal(tr["hops"], hops[cs, cd])


def tied_vertices(g, dist, src):
    """Vertices with >= 2 candidate parents at the minimal d[u] (igraph's pop order decides)."""
    if not g.directed:
        return g.parent_ties(dist, src) >= 2
    nl = g.eu != g.ev  # directed: the candidates of v are the tails of its in-arcs
    u, v, w = g.eu[nl], g.ev[nl], g.elat[nl]
    cand = (dist[u] >= 0) & (dist[v] >= 0) & (dist[u] + w == dist[v]) & (v != src)
    best = np.full(g.V, np.inf)
    np.minimum.at(best, v[cand], dist[u][cand])
    cnt = np.zeros(g.V, np.int64)
    np.add.at(cnt, v[cand], dist[u][cand] == best[v[cand]])
    return cnt >= 2


def pairs_crossing_ties(g, exp, sv, dv):
    tied = {s: tied_vertices(g, g.dijkstra(s)[0], s) for s in exp.dij}
    return sum(1 for i, c in enumerate(exp.verts)
               if sv[i] != dv[i] and tied[int(sv[i])][c[1:]].any())


def all_pairs(ips, verts, nsrc):
    """The first nsrc hosts as sources to every host: (sip, dip, sv, dv)."""
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    k = len(ips)
    si = np.repeat(np.arange(nsrc), k)
    di = np.tile(np.arange(k), nsrc)
    return ips[si], ips[di], verts[si], verts[di]


# ------------------------------------------------------------------------------------------
# routes against the oracle
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_grid_expected(directed, verts):
    """The oracle's routes of the first 6 poi to all 70, computed once for both key encodings."""
    g = oracle.OGraph.from_graphml(tie_grid_graphml(directed))
    sv = np.repeat(verts[:6], 70)
    dv = np.tile(verts, 6)
    exp = Expected(g, sv, dv, verts)
    return exp, pairs_crossing_ties(g, exp, sv, dv)


@pytest.mark.parametrize("directed,int_keys", [(False, 1), (False, 0), (True, 1), (True, 0)])
def test_tie_grid_routes(directed, int_keys):
    """Ties across most chains (integer latencies U{1, 2}): 6 sources x 70 targets -- more than one
    wavefront of requests per source -- on the u32-key and the f64-key replay, undirected and
    directed.  At least 100 traced pairs cross a vertex whose parent igraph's pop order decides."""
    top, g, ips, verts = pinned(tie_grid_graphml(directed), 70,
                                [("replay_int_keys", int_keys)])
    assert top.is_directed == directed
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    assert len(sip) == 420
    exp, crossing = tie_grid_expected(directed, tuple(int(v) for v in verts))
    assert crossing >= 100, crossing
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)
    ts = top.trace_stats()
    assert ts["sources"] == 6 and ts["requests"] == 420 and ts["entries"] == tr["total"]


def test_real_latencies_routes_match_oracle_and_scipy():
    """Continuous latencies: no chain crosses a tie, so scipy's predecessor trees pin the vertex
    lists independently of the oracle."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    data = random_topology_graphml(600, 60, 2400, seed=3)
    top, g, ips, verts = random_hosts(data, 300)
    first = {}
    for ip, v in zip(ips, verts):
        first.setdefault(v, ip)
    av = sorted(first)
    assert len(av) >= 50
    src = av[:5]
    sv = np.repeat(src, len(av)).astype(np.int32)
    dv = np.tile(av, len(src)).astype(np.int32)
    sip = np.asarray([first[int(v)] for v in sv], np.uint32)
    dip = np.asarray([first[int(v)] for v in dv], np.uint32)
    exp = Expected(g, sv, dv, av)
    assert pairs_crossing_ties(g, exp, sv, dv) == 0
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)
    nl = g.eu != g.ev
    r = np.concatenate([g.eu[nl], g.ev[nl]])
    c = np.concatenate([g.ev[nl], g.eu[nl]])
    W = sp.csr_matrix((np.concatenate([g.elat[nl], g.elat[nl]]), (r, c)), shape=(g.V, g.V))
    assert W.nnz == len(r)  # no parallel edges
    _, pred = dijkstra(W, directed=False, indices=np.asarray(src), return_predecessors=True)
    row = {s: k for k, s in enumerate(src)}
    for i in range(len(sv)):
        s, d = int(sv[i]), int(dv[i])
        if s == d:
            continue
        chain = [d]
        while chain[-1] != s:
            chain.append(int(pred[row[s], chain[-1]]))
        o, h = int(tr["offset"][i]), int(tr["hops"][i])
        assert list(tr["vertices"][o:o + h + 1]) == chain[::-1], i


@pytest.mark.parametrize("directed", [False, True])
def test_multigraph_routes_use_the_lowest_edge_id(directed):
    """Parallel edges: every hop reports igraph_get_eid's edge, the lowest id of its group."""
    data = random_topology_graphml(n_routers=400, n_poi=40, extra=1600, seed=9, integer=True,
                                   directed=directed, parallel=400)
    top, g, ips, verts = random_hosts(data, 120)
    first = {}
    for ip, v in zip(ips, verts):
        first.setdefault(v, ip)
    av = sorted(first)
    src = av[:6]
    sv = np.repeat(src, len(av)).astype(np.int32)
    dv = np.tile(av, len(src)).astype(np.int32)
    sip = np.asarray([first[int(v)] for v in sv], np.uint32)
    dip = np.asarray([first[int(v)] for v in dv], np.uint32)
    exp = Expected(g, sv, dv, av)
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)
    key = (lambda a, b: (a, b)) if directed else (lambda a, b: (min(a, b), max(a, b)))
    mult = {}
    for a, b in zip(g.eu.tolist(), g.ev.tolist()):
        mult[key(a, b)] = mult.get(key(a, b), 0) + 1
    on_group = sum(1 for c in exp.verts for a, b in zip(c[:-1], c[1:])
                   if a != b and mult[key(a, b)] > 1)
    assert on_group > 50, on_group


def test_long_chain_routes_beyond_the_path_buffer():
    top, g, ips, verts = pinned(long_chain_graphml(), 3)
    sip, dip, sv, dv = all_pairs(ips, verts, 3)
    exp = Expected(g, sv, dv, verts)
    assert exp.hops.reshape(3, 3).tolist() == [[1, 201, 102], [201, 1, 101], [102, 101, 1]]
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)


# ------------------------------------------------------------------------------------------
# the call's contract
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    """The undirected tie grid with its table built, shared by the contract tests (none of them
    changes the topology)."""
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70)
    top.table()
    return top, g, np.asarray(ips, np.uint32), np.asarray(verts, np.int32)


def test_self_pair_and_two_hosts_on_one_vertex():
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70)
    v2, _ = top.attach_ip(host_ip(500), 99, typeHint="t7")  # a second host on poi 7
    assert v2 == verts[7]
    sip = np.asarray([ips[7], ips[7], host_ip(500)], np.uint32)
    dip = np.asarray([ips[7], host_ip(500), ips[7]], np.uint32)
    tr = top.trace_routes(sip, dip)
    loop = g.get_eid(v2, v2)
    assert g.eu[loop] == v2 == g.ev[loop]
    assert list(tr["hops"]) == [1, 1, 1] and list(tr["status"]) == [0, 0, 0]
    assert list(tr["vertices"]) == [v2, v2] * 3 and list(tr["edges"]) == [loop, -1] * 3
    check_table(top, tr, [v2] * 3, [v2] * 3)
    lat, rel, _ = g.source_rows([v2], [v2])
    assert tr["latency"][0] == lat[0, 0] and tr["reliability"][0] == rel[0, 0]


def test_multi_device_topology_traces_on_its_first_device():
    """Option "devices": the table is built by several engines; the trace runs on the first one
    and still reports the table's routes."""
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70, [("devices", 2)])
    sip, dip, sv, dv = all_pairs(ips, verts, 2)
    top.table()
    st0 = top.stats()
    assert st0["devices"] == 2
    tr = top.trace_routes(sip, dip)
    check_routes(tr, Expected(g, sv, dv, verts))
    check_table(top, tr, sv, dv)
    assert top.stats() == st0


def test_chunked_trace_is_byte_identical(grid):
    top, g, ips, verts = grid
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    a = top.trace_routes(sip, dip)
    assert top.trace_stats()["chunks"] == 1
    top.set_option("trace_chunk", 2)
    try:
        b = top.trace_routes(sip, dip)
        assert top.trace_stats()["chunks"] == 3 and top.trace_stats()["sources"] == 6
    finally:
        top.set_option("trace_chunk", 0)
    for k in ("offset", "hops", "status", "latency", "reliability", "vertices", "edges"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["total"] == b["total"]


def test_request_order_shuffled_and_duplicated(grid):
    top, g, ips, verts = grid
    rng = np.random.default_rng(1)
    si = rng.integers(0, 5, 60)
    di = rng.integers(0, 70, 60)
    si[10:20], di[10:20] = si[:10], di[:10]  # duplicates
    exp = Expected(g, verts[si], verts[di], verts)
    tr = top.trace_routes(ips[si], ips[di])
    check_routes(tr, exp)  # request order, running-sum offsets
    for k in range(10):
        a, b = int(tr["offset"][k]), int(tr["offset"][10 + k])
        h = int(tr["hops"][k])
        assert np.array_equal(tr["vertices"][a:a + h + 1], tr["vertices"][b:b + h + 1])


def test_buffer_sizing_and_cap(grid):
    top, g, ips, verts = grid
    lib, _ = _lib.load()
    si, di = np.asarray([0, 1, 2, 3, 0]), np.asarray([9, 8, 7, 6, 0])
    sip, dip = np.ascontiguousarray(ips[si]), np.ascontiguousarray(ips[di])
    n = len(si)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    routes = (_lib.ShdRoute * n)()
    total = lib.shdtopo_trace_routes(top._h, p(sip), p(dip), n, routes, None, None, 0)
    exp = Expected(g, verts[si], verts[di], verts)
    assert total == exp.total()
    assert [r.status for r in routes] == [3] * n and [r.offset for r in routes] == [-1] * n
    assert [r.hops for r in routes] == exp.hops.tolist()
    full = top.trace_routes(sip, dip)
    check_routes(full, exp)
    # a cap that cuts the third route short
    cap = int(full["offset"][2]) + 2
    assert cap < full["offset"][3]
    V = np.full(total + 16, -7, np.int32)
    E = np.full(total + 16, -7, np.int32)
    r = lib.shdtopo_trace_routes(top._h, p(sip), p(dip), n, routes, p(V), p(E), cap)
    assert r == total
    fit = int(full["offset"][2])
    assert [x.status for x in routes] == [0, 0, 3, 3, 3]
    assert [x.offset for x in routes] == [0, int(full["offset"][1]), -1, -1, -1]
    assert [x.hops for x in routes] == exp.hops.tolist()
    assert [x.latency for x in routes] == exp.lat.tolist()
    assert [x.reliability for x in routes] == exp.rel.tolist()
    assert np.array_equal(V[:fit], full["vertices"][:fit])
    assert np.array_equal(E[:fit], full["edges"][:fit])
    assert np.all(V[fit:] == -7) and np.all(E[fit:] == -7)  # nothing past the routes that fit


def test_unattached_ip_gets_status_1(grid):
    top, g, ips, verts = grid
    stranger = sa.ip_to_network("10.9.8.7")
    sip = np.asarray([ips[0], stranger, ips[1], ips[2]], np.uint32)
    dip = np.asarray([ips[5], ips[5], stranger, ips[6]], np.uint32)
    tr = top.trace_routes(sip, dip)
    assert list(tr["status"]) == [0, 1, 1, 0]
    assert list(tr["hops"][1:3]) == [-1, -1] and list(tr["offset"][1:3]) == [-1, -1]
    exp = Expected(g, verts[[0, 2]], verts[[5, 6]], verts)
    assert tr["offset"][0] == 0 and tr["offset"][3] == exp.hops[0] + 1
    assert tr["total"] == exp.total()
    for k, i in enumerate((0, 3)):
        o, h = int(tr["offset"][i]), int(tr["hops"][i])
        assert list(tr["vertices"][o:o + h + 1]) == exp.verts[k]
        assert list(tr["edges"][o:o + h]) == exp.edges[k]
        assert tr["latency"][i] == exp.lat[k] and tr["reliability"][i] == exp.rel[k]


@pytest.mark.parametrize("tie_free", [False, True])
def test_trace_leaves_stats_table_and_lazy_rows_alone(tie_free):
    """After a trace the last build's statistics, the table and the materialised lazy rows are
    what they were, and no rebuild happened -- also when the trace is the first use of the replay
    (a tie-free build replays no row, so the trace uploads the replay's CSR itself)."""
    if tie_free:
        top, g, ips, verts = random_hosts(random_topology_graphml(600, 60, 2400, seed=3), 100)
    else:
        top, g, ips, verts = pinned(tie_grid_graphml(False), 70)
    ips = np.asarray(ips, np.uint32)
    assert top.latency_ip(ips[0], ips[1]) > 0  # builds the table, materialises a lazy row
    a0, lat0, rel0, hops0 = top.table()
    st0 = top.stats()
    lz0 = top.lazy_rows()
    lm0 = top.lazyMinimumLatency()
    if tie_free:
        assert st0["replay_rows"] == 0
    tr = top.trace_routes(ips[[2, 3, 4]], ips[[5, 6, 2]])
    assert np.all(tr["status"] == 0)
    assert top.stats() == st0
    assert all(np.array_equal(x, y) for x, y in zip(top.lazy_rows(), lz0))
    assert top.lazyMinimumLatency() == lm0
    a1, lat1, rel1, hops1 = top.table()
    assert top.stats() == st0  # no rebuild
    assert np.array_equal(a0, a1) and np.array_equal(hops0, hops1)
    assert lat0.tobytes() == lat1.tobytes() and rel0.tobytes() == rel1.tobytes()


def test_format_route_is_the_reference_debug_line(grid):
    top, g, ips, verts = grid
    si, di = np.asarray([0, 3, 4]), np.asarray([41, 3, 69])
    exp = Expected(g, verts[si], verts[di], verts)
    tr = top.trace_routes(ips[si], ips[di])
    ids = g.vattrs["id"]
    for i in range(3):
        c, e = exp.verts[i], exp.edges[i]
        path = ids[c[0]] + "".join("--[%f,%f]-->%s" % (g.elat[x], 1.0 - g.eloss[x], ids[v])
                                   for x, v in zip(e, c[1:]))
        want = "shortest path %s-->%s (%i-->%i) is %f ms with %f loss, path: %s" % (
            ids[c[0]], ids[c[-1]], c[0], c[-1], exp.lat[i], 1 - exp.rel[i], path)
        assert top.format_route(tr, i) == want
