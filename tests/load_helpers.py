"""Shared fixtures and the expected values of the link-load tests (test_link_load.py,
test_link_load_cpu.py).

Expected loads come from the CPU oracle alone: g.dijkstra(s, targets) gives the parent vertices
(the chain of every destination), g.get_eid(a, b) each hop's edge (the lowest id of a parallel
group), and the sums are numpy uint64.  Nothing here calls trace_routes or link_load.
"""
import functools

import numpy as np

import oracle
import shadow_amd as sa
from helpers import attach_hosts, graphml_doc


# ------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_grid_graphml(directed=False):
    """The tie grid of test_trace.py (same recipe, seed 5): 16 x 16 routers, latencies U{1, 2},
    70 poi of a type of their own with an uplink of 5.0 and a self loop, edge order shuffled."""
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


TRANSIT_POI = 48


@functools.lru_cache(maxsize=None)
def transit_grid_graphml(directed=False):
    """12 x 12 grid whose routers (i, j) with (i + j) % 3 == 0 are the poi themselves (type t<k>,
    a self loop each): destinations lie on other destinations' routes.  Latencies U{1, 2, 3}."""
    rng = np.random.default_rng(11)
    n = 12
    # (attach only considers vertices whose id contains "poi")
    nid = lambda i, j: ("poi-%d" if (i + j) % 3 == 0 else "pop-%d") % (i * n + j)
    nodes, poi = [], []
    for i in range(n):
        for j in range(n):
            if (i + j) % 3 == 0:
                nodes.append((nid(i, j), "t%d" % len(poi), rng.uniform(0, 0.05)))
                poi.append(nid(i, j))
            else:
                nodes.append((nid(i, j), "pop", 0.0))
    assert len(poi) == TRANSIT_POI
    edges = []

    def link(a, b):
        edges.append((a, b, int(rng.integers(1, 4)), rng.uniform(0, 0.01)))
        if directed:
            edges.append((b, a, int(rng.integers(1, 4)), rng.uniform(0, 0.01)))
    for i in range(n):
        for j in range(n):
            if j + 1 < n:
                link(nid(i, j), nid(i, j + 1))
            if i + 1 < n:
                link(nid(i, j), nid(i + 1, j))
    for p in poi:
        edges.append((p, p, 1.0, 0.001))
    order = rng.permutation(len(edges))
    return graphml_doc(nodes, [edges[i] for i in order], directed)


@functools.lru_cache(maxsize=None)
def long_chain_graphml():
    """The 200-router path of test_trace.py (seed 8): routes of 201, 102 and 101 hops."""
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
    Returns (top, g, ips, verts) with ips / verts as numpy arrays."""
    top = sa.Topology.from_buffer(data)
    g = oracle.OGraph.from_graphml(data)
    for k, v in options:
        top.set_option(k, v)
    otop, ips, verts = attach_hosts(top, g, npoi, type_hints=["t%d" % k for k in range(npoi)])
    assert len(set(verts)) == npoi
    return top, g, np.asarray(ips, np.uint32), np.asarray(verts, np.int32)


def random_hosts(data, n_hosts, options=()):
    """Hosts attached by the client / relay / server hints; the first host of every attached
    vertex.  Returns (top, g, av, aip): attached vertices ascending and one IP each."""
    top = sa.Topology.from_buffer(data)
    g = oracle.OGraph.from_graphml(data)
    for k, v in options:
        top.set_option(k, v)
    otop, ips, verts = attach_hosts(top, g, n_hosts, type_hints=["client", "relay", "server"])
    first = {}
    for ip, v in zip(ips, verts):
        first.setdefault(v, ip)
    av = np.asarray(sorted(first), np.int32)
    return top, g, av, np.asarray([first[int(v)] for v in av], np.uint32)


def all_pairs(ips, verts, nsrc):
    """The first nsrc hosts as sources to every host: (sip, dip, sv, dv)."""
    k = len(ips)
    si = np.repeat(np.arange(nsrc), k)
    di = np.tile(np.arange(k), nsrc)
    return ips[si], ips[di], verts[si], verts[di]


# ------------------------------------------------------------------------------------------
# the oracle's loads
# ------------------------------------------------------------------------------------------
class ExpectedLoad:
    """Loads of the flows (sv[i], dv[i], w[i]) from the oracle: per request the vertex chain and
    its get_eid edges; edge_fwd / edge_rev u64[E], vertex u64[V]; hops, hop_weight, and per source
    the union tree of the requested chains (tree_vertices = its vertices, the source aside)."""

    def __init__(self, g, sv, dv, w, targets):
        targets = np.asarray(sorted(set(int(t) for t in targets)), np.int32)
        n = len(sv)
        w = np.ones(n, np.uint64) if w is None else np.asarray(w, np.uint64)
        self.g = g
        self.dij = {s: g.dijkstra(s, targets) for s in sorted(set(int(x) for x in sv))}
        self.verts, self.edges = [], []
        eid = {}
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
            es = []
            for a, b in zip(chain[:-1], chain[1:]):
                if (a, b) not in eid:
                    eid[(a, b)] = g.get_eid(a, b)
                    assert eid[(a, b)] >= 0
                es.append(eid[(a, b)])
            self.verts.append(chain)
            self.edges.append(es)
        self.hops = np.asarray([len(e) for e in self.edges], np.int64)
        self.edge_fwd = np.zeros(g.E, np.uint64)
        self.edge_rev = np.zeros(g.E, np.uint64)
        self.vertex = np.zeros(g.V, np.uint64)
        for c, es, wi in zip(self.verts, self.edges, w):
            a = np.asarray(c[:-1])
            e = np.asarray(es)
            fwd = g.eu[e] == a
            np.add.at(self.edge_fwd, e[fwd], wi)
            np.add.at(self.edge_rev, e[~fwd], wi)
            np.add.at(self.vertex, np.asarray(c[1:]), wi)
        self.routed = n
        self.hop_weight = int((w * self.hops.astype(np.uint64)).sum())
        # union tree per source: vertex -> parent
        self.tree = {}
        for c in self.verts:
            if c[0] == c[-1]:
                continue
            t = self.tree.setdefault(c[0], {})
            for a, b in zip(c[:-1], c[1:]):
                assert t.setdefault(b, a) == a
        self.tree_vertices = sum(len(t) for t in self.tree.values())

    def transit_destinations(self):
        """Requested (source, destination) pairs whose destination is an interior vertex of
        another requested route from the same source."""
        interior = {}
        for c in self.verts:
            interior.setdefault(c[0], set()).update(c[1:-1])
        return len({(c[0], c[-1]) for c in self.verts
                    if c[0] != c[-1] and c[-1] in interior[c[0]]})

    def branching(self):
        """(source, vertex) combinations with >= 2 children in the source's union tree."""
        n = 0
        for t in self.tree.values():
            kids = {}
            for v, p in t.items():
                kids[p] = kids.get(p, 0) + 1
            n += sum(1 for k in kids.values() if k >= 2)
        return n


def check_load(out, exp):
    assert out["routed"] == exp.routed
    assert np.array_equal(out["edge_fwd"], exp.edge_fwd)
    assert np.array_equal(out["edge_rev"], exp.edge_rev)
    assert np.array_equal(out["vertex"], exp.vertex)


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


def pairs_crossing_ties(g, exp):
    tied = {s: tied_vertices(g, g.dijkstra(s)[0], s) for s in exp.dij}
    return sum(1 for c in exp.verts if c[0] != c[-1] and tied[c[0]][c[1:]].any())
