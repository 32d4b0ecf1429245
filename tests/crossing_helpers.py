"""Expected values and shared inputs of the link-crossing tests (test_link_crossings.py,
test_link_crossings_cpu.py).

Expected records come from the CPU oracle alone: load_helpers.ExpectedLoad gives every flow's
vertex chain and get_eid edges (g.dijkstra for the parents, g.get_eid for each hop's edge); the
records, offsets, counts and weights are derived from those chains here.  Nothing in this file
calls trace_routes, link_load or link_crossings.
"""
import functools

import numpy as np

import oracle
from helpers import graphml_doc
from load_helpers import ExpectedLoad, tied_vertices

# one record of the call (ShdCrossing), restated: the product's dtype is not the reference
RECORD = np.dtype([("flow", np.int32), ("watch", np.int32), ("hop", np.int32),
                   ("reverse", np.int32)])
STAT_KEYS = ("requests", "routed", "unattached", "broken", "sources", "crossings", "flows_hit")


class ExpectedCrossings:
    """Crossings of the flows of `exp` (an ExpectedLoad built with the same weights `w`) over the
    watched `edges` (edge ids) and `vertices` (original ids).  `flows[i]` is the request index of
    exp's flow i within a call of `n` requests (default: the flows are the call's requests); the
    other requests of the call (unattached ends) have no record.

    records  RECORD array ordered by flow, hop, edge before vertex
    offsets  int64[n + 1], the running sum of the flows' record counts
    count    uint64[ne + nv] records per watch;  weight: their flows' weights, wrapping
    """

    def __init__(self, g, exp, w, edges, vertices, flows=None, n=None):
        m = len(exp.verts)
        w = np.ones(m, np.uint64) if w is None else np.asarray(w, np.uint64)
        flows = np.arange(m) if flows is None else np.asarray(flows)
        assert len(flows) == m == len(w) and np.all(np.diff(flows) > 0)
        n = m if n is None else n
        edges = [int(e) for e in edges]
        vertices = [int(v) for v in vertices]
        ne = len(edges)
        ewatch = {e: k for k, e in enumerate(edges)}
        vwatch = {v: ne + k for k, v in enumerate(vertices)}
        assert len(ewatch) == ne and len(vwatch) == len(vertices)
        recs = []
        per_flow = np.zeros(n, np.int64)
        self.both = 0  # hops with an edge and a vertex record
        for i, (chain, es) in enumerate(zip(exp.verts, exp.edges)):
            for hop, (a, b, e) in enumerate(zip(chain[:-1], chain[1:], es)):
                k0 = len(recs)
                if e in ewatch:
                    recs.append((flows[i], ewatch[e], hop, int(a != b and g.eu[e] != a)))
                if b in vwatch:
                    recs.append((flows[i], vwatch[b], hop, 0))
                per_flow[flows[i]] += len(recs) - k0
                self.both += len(recs) - k0 == 2
        self.records = np.array(recs, RECORD) if recs else np.zeros(0, RECORD)
        self.offsets = np.concatenate([[0], np.cumsum(per_flow)]).astype(np.int64)
        self.total = int(self.offsets[-1])
        self.count = np.zeros(ne + len(vertices), np.uint64)
        self.weight = np.zeros(ne + len(vertices), np.uint64)
        wf = np.zeros(n, np.uint64)
        wf[flows] = w
        np.add.at(self.count, self.records["watch"], np.uint64(1))
        np.add.at(self.weight, self.records["watch"], wf[self.records["flow"]])
        self.flows_hit = int((per_flow > 0).sum())
        self.per_flow = per_flow
        self.flows = flows
        self.routed = m
        self.n = n
        self.ne = ne

    # what the input exercises (asserted by the tests with margin, from these records alone)
    def flows_with_several(self):
        return int((self.per_flow >= 2).sum())

    def reverse_crossings(self):
        return int(self.records["reverse"].sum())

    def flows_without_any(self):
        return int((self.per_flow[self.flows] == 0).sum())

    def fitting(self, cap):
        """The records a call with this cap writes: flow i's iff offsets[i + 1] <= cap."""
        fit = int(self.offsets[np.searchsorted(self.offsets, cap, side="right") - 1])
        return self.records[:fit]


def check_crossings(out, xc):
    """A link_crossings result equals the oracle's: the records byte for byte."""
    assert out["total"] == xc.total
    assert np.array_equal(out["offsets"], xc.offsets)
    assert out["records"].dtype.itemsize == 16
    assert out["records"].tobytes() == xc.records.tobytes()
    assert np.array_equal(out["count"], xc.count)
    assert np.array_equal(out["weight"], xc.weight)


def check_stats(cs, xc, sources, unattached=0):
    want = dict(requests=xc.n, routed=xc.routed, unattached=unattached, broken=0, sources=sources,
                crossings=xc.total, flows_hit=xc.flows_hit)
    assert {k: cs[k] for k in STAT_KEYS} == want


def watch_recipe(exp, sv, dv):
    """The deterministic watch set of the tests, from the oracle's loads: the 8 heaviest edges
    (stable descending), the first 4 edge ids without load and the loop of the first self pair;
    the 4 heaviest vertices, the first flow's source and the lowest vertex id without load.  Both
    lists without repeats, first occurrences kept.  Returns (edges, vertices)."""
    top_of = lambda x, k: np.argsort(np.iinfo(np.uint64).max - x, kind="stable")[:k].tolist()
    eload = exp.edge_fwd + exp.edge_rev
    edges = top_of(eload, 8) + np.nonzero(eload == 0)[0][:4].tolist()
    selfp = np.nonzero(np.asarray(sv) == np.asarray(dv))[0]
    if len(selfp):
        edges.append(exp.edges[int(selfp[0])][0])
    vertices = top_of(exp.vertex, 4) + [int(sv[0])]
    unloaded = np.nonzero(exp.vertex == 0)[0]
    if len(unloaded):
        vertices.append(int(unloaded[0]))
    dedup = lambda xs: list(dict.fromkeys(int(x) for x in xs))
    return dedup(edges), dedup(vertices)


def parallel_groups_on_chains(g, exp):
    """[(lowest id, a higher id)] of the parallel groups the oracle's chains use."""
    key = (lambda a, b: (a, b)) if g.directed else (lambda a, b: (min(a, b), max(a, b)))
    members = {}
    for e, (a, b) in enumerate(zip(g.eu.tolist(), g.ev.tolist())):
        members.setdefault(key(a, b), []).append(e)
    used = sorted({e for es in exp.edges for e in es})
    out = []
    for e in used:
        grp = members[key(int(g.eu[e]), int(g.ev[e]))]
        if len(grp) > 1:
            assert grp[0] == e  # the chains' edges are get_eid's: the lowest id
            out.append((e, grp[1]))
    return out


# ------------------------------------------------------------------------------------------
# the diamond graph of test_trace_batch.py (same recipe, seed 17), restated
# ------------------------------------------------------------------------------------------
DIAMOND_POI = 40


@functools.lru_cache(maxsize=None)
def diamond_graphml():
    """300 routers with continuous latencies (a ring plus 900 random edges) and one planted
    diamond a - {b1, b2} - c of four equal latencies: a chain through it has two candidate parents
    at the same distance.  40 poi of a type of their own (host k pinned to poi k), a self loop
    each."""
    rng = np.random.default_rng(17)
    n = 300
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(n)]
    nodes += [("pop-b1", "pop", 0.0), ("pop-b2", "pop", 0.0)]
    nodes += [("poi-%d" % k, "t%d" % k, rng.uniform(0, 0.05)) for k in range(DIAMOND_POI)]
    edges = [("pop-%d" % i, "pop-%d" % ((i + 1) % n), rng.uniform(1, 100), rng.uniform(0, 0.01))
             for i in range(n)]
    seen = set()
    while len(seen) < 900:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        key = (min(a, b), max(a, b))
        if a == b or abs(a - b) in (1, n - 1) or key in seen:
            continue
        seen.add(key)
        edges.append(("pop-%d" % a, "pop-%d" % b, rng.uniform(1, 100), rng.uniform(0, 0.01)))
    a, c = 10, 160
    for b in ("pop-b1", "pop-b2"):
        edges.append(("pop-%d" % a, b, 4.0, 0.001))
        edges.append((b, "pop-%d" % c, 4.0, 0.002))
    for k in range(DIAMOND_POI):
        edges.append(("poi-%d" % k, "pop-%d" % int(rng.integers(0, n)), 5.0, 0.0))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.0))
    order = rng.permutation(len(edges))
    return graphml_doc(nodes, [edges[i] for i in order])


@functools.lru_cache(maxsize=None)
def diamond_case(verts):
    """The oracle's view of the diamond graph: (g, free, tied) -- the poi whose rows to every poi
    cross no tied parent and those whose rows cross the planted tie."""
    g = oracle.OGraph.from_graphml(diamond_graphml())
    v = np.asarray(verts, np.int32)
    full = ExpectedLoad(g, np.repeat(v, len(v)), np.tile(v, len(v)), None, v)
    crossing = set()
    for s in full.dij:
        tied = tied_vertices(g, g.dijkstra(s)[0], s)
        if any(c[0] == s and c[0] != c[-1] and tied[c[1:]].any() for c in full.verts):
            crossing.add(s)
    free = [int(x) for x in v if int(x) not in crossing]
    tied = [int(x) for x in v if int(x) in crossing]
    return g, free, tied
