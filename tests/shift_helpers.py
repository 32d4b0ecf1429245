"""Expected values and shared inputs of the load shift tests (test_load_shift.py,
test_load_shift_cpu.py).

Every expected value comes from the CPU oracle alone: load_helpers.ExpectedLoad on the parent
graph and on whatif_helpers.filtered(g, fail), np.flatnonzero(keep) as the child's origin map, and
numpy uint64 arithmetic (which wraps, as the product's does) for the comparison.  Nothing in this
file calls ``load_shift``, ``link_load``, ``without`` or ``edge_origin``.
"""
import functools

import numpy as np

import oracle
from helpers import graphml_doc, host_ip
from impact_helpers import impact_flows
from load_helpers import ExpectedLoad
from whatif_helpers import case, filtered

# one record of the shift (ShdLoadChange), restated: the product's dtype is not the reference
LOAD_CHANGE = np.dtype([("kind", np.int32), ("id", np.int32), ("idA", np.int32),
                        ("idB", np.int32), ("before", np.uint64), ("after", np.uint64)])
BY_KIND = ("changed", "gained", "lost", "newlyUsed", "abandoned", "gainedWeight", "lostWeight")
SCALARS = ("flows", "unattached", "routedA", "routedB", "brokenA", "brokenB", "hopWeightA",
           "hopWeightB", "displaced", "appeared", "worstGain", "worstLoss", "worstGainIndex",
           "worstLossIndex", "peakBefore", "peakAfter", "peakBeforeIndex", "peakAfterIndex")
U64 = np.uint64
M64 = (1 << 64) - 1
CASES = ("real", "int", "directed", "parallel", "one_router", "two", "one")
# changed entries of every case (from the oracle; the tests assert them as preconditions)
CHANGED = {"real": 819, "int": 817, "directed": 983, "parallel": 964, "one_router": 181, "two": 34,
           "one": 0}


def usum(x):
    return int(np.asarray(x, U64).sum(dtype=U64))


def identity(n):
    return np.arange(n, dtype=np.int64)


def side_loads(ex, origin, R, V):
    """The loads of one side (an ExpectedLoad whose graph has the root edge ids `origin`) in the
    root's index space [0, 2 R + V), and per root edge the side's own id (-1: it lacks it)."""
    origin = np.asarray(origin, np.int64)
    assert len(origin) == ex.g.E and ex.g.V == V
    load = np.zeros(2 * R + V, U64)
    load[origin] = ex.edge_fwd
    load[R + origin] = ex.edge_rev
    load[2 * R:] = ex.vertex
    own = np.full(R, -1, np.int32)
    own[origin] = np.arange(len(origin), dtype=np.int32)
    return load, own


def expected_shift(ea, eb, origin_a, origin_b, R, V, flows, unattached):
    """The shift between two oracle loads, in numpy: a dict with the keys of Topology.load_shift."""
    before, own_a = side_loads(ea, origin_a, R, V)
    after, own_b = side_loads(eb, origin_b, R, V)
    X = 2 * R + V
    x = np.flatnonzero(before != after)
    kind = (x >= R).astype(np.int32) + (x >= 2 * R)
    rid = (x - np.where(kind == 2, 2 * R, kind * R)).astype(np.int32)
    edge = kind < 2
    rec = np.zeros(len(x), LOAD_CHANGE)
    rec["kind"], rec["id"] = kind, rid
    rec["idA"] = np.where(edge, own_a[np.where(edge, rid, 0)], rid)
    rec["idB"] = np.where(edge, own_b[np.where(edge, rid, 0)], rid)
    rec["before"], rec["after"] = before[x], after[x]
    b, a = rec["before"], rec["after"]
    up, down = a > b, a < b
    out = {"total": len(x), "records": rec, "flows": flows, "unattached": unattached,
           "routedA": ea.routed, "routedB": eb.routed, "brokenA": 0, "brokenB": 0,
           "hopWeightA": ea.hop_weight & M64, "hopWeightB": eb.hop_weight & M64}
    by = lambda m, dt: np.array([int(m[kind == k].sum(dtype=dt)) for k in range(3)], dt)
    out["changed"] = by(np.ones(len(x), np.int64), np.int64)
    out["gained"], out["lost"] = by(up.astype(np.int64), np.int64), by(down.astype(np.int64), np.int64)
    out["newlyUsed"] = by((up & (b == 0)).astype(np.int64), np.int64)
    out["abandoned"] = by((down & (a == 0)).astype(np.int64), np.int64)
    out["gainedWeight"] = by(np.where(up, a - b, U64(0)), U64)
    out["lostWeight"] = by(np.where(down, b - a, U64(0)), U64)
    out["displaced"] = usum(b[edge & (rec["idB"] < 0)])
    out["appeared"] = usum(a[edge & (rec["idA"] < 0)])

    def worst(m, v):  # the largest v over m and the lowest x reaching it
        if not m.any():
            return 0, -1
        top = v[m].max()
        return int(top), int(x[m & (v == top)][0])
    out["worstGain"], out["worstGainIndex"] = worst(up, a - b)
    out["worstLoss"], out["worstLossIndex"] = worst(down, b - a)
    for key, load in (("peakBefore", before), ("peakAfter", after)):
        half = load[:2 * R]
        top = half.max() if len(half) else 0
        out[key] = int(top)
        out[key + "Index"] = int(np.flatnonzero(half == top)[0]) if top else -1
    out["before"], out["after"], out["entries"] = before, after, X
    return out


def swapped(exp):
    """exp in the other direction: what b.load_shift(a) must report."""
    rec = exp["records"].copy()
    rec["before"], rec["after"] = exp["records"]["after"], exp["records"]["before"]
    rec["idA"], rec["idB"] = exp["records"]["idB"], exp["records"]["idA"]
    out = dict(exp, records=rec)
    for x, y in (("routedA", "routedB"), ("brokenA", "brokenB"), ("hopWeightA", "hopWeightB"),
                 ("gained", "lost"), ("newlyUsed", "abandoned"), ("gainedWeight", "lostWeight"),
                 ("displaced", "appeared"), ("worstGain", "worstLoss"),
                 ("worstGainIndex", "worstLossIndex"), ("peakBefore", "peakAfter"),
                 ("peakBeforeIndex", "peakAfterIndex"), ("before", "after")):
        out[x], out[y] = exp[y], exp[x]
    return out


def assert_totals_equal(got, exp, what=""):
    """Everything but the records."""
    assert got["total"] == exp["total"], (what, got["total"], exp["total"])
    for k in SCALARS:
        assert int(got[k]) == int(exp[k]), (what, k, got[k], exp[k])
    for k in BY_KIND:
        assert len(got[k]) == 3 and [int(v) for v in got[k]] == [int(v) for v in exp[k]], \
            (what, k, got[k], exp[k])


def assert_shift_equal(got, exp, cap=None, what=""):
    """Every output of load_shift against expected_shift; records are the first `cap`."""
    assert_totals_equal(got, exp, what)
    n = exp["total"] if cap is None else min(cap, exp["total"])
    assert len(got["records"]) == n, what
    assert got["records"].dtype.itemsize == LOAD_CHANGE.itemsize == 32
    assert got["records"].tobytes() == exp["records"][:n].tobytes(), what


def words_of(exp):
    """(full, empty, partial) 64-entry ballot words of the changed entries."""
    X = exp["entries"]
    flag = np.zeros((X + 63) // 64 * 64, bool)
    flag[:X] = exp["before"] != exp["after"]
    valid = np.zeros(len(flag), bool)
    valid[:X] = True
    w, v = flag.reshape(-1, 64), valid.reshape(-1, 64)
    full = (w | ~v).all(axis=1) & w.any(axis=1)
    empty = ~w.any(axis=1)
    return int(full.sum()), int(empty.sum()), int((~full & ~empty).sum())


def reduced(w):
    """Weights 1..1448: gains and losses that mean something."""
    return (np.asarray(w, U64) % U64(1448) + U64(1)).astype(U64)


def vertices_of(c, ips):
    """The vertices of the hosts' IPs in case c (-1: not attached)."""
    vert = dict(zip(c["ips"], c["verts"]))
    return np.array([vert.get(int(ip), -1) for ip in ips], np.int64)


def oracle_loads(c, graphs, src_ip, dst_ip, w):
    """ExpectedLoad of the flows on each of `graphs` (flows with an unattached end are left out),
    and how many were."""
    sv, dv = vertices_of(c, src_ip), vertices_of(c, dst_ip)
    ok = (sv >= 0) & (dv >= 0)
    w = None if w is None else np.asarray(w, U64)[ok]
    return [ExpectedLoad(g, sv[ok], dv[ok], w, c["verts"]) for g in graphs], int((~ok).sum())


@functools.lru_cache(maxsize=None)
def shift_flows(name, small=False):
    """The flows of impact_helpers.impact_flows on whatif_helpers.case(name) -- full-range weights,
    or (small) those reduced to 1..1448 -- with exp, the expected shift parent -> child (computed
    once, shared, never modified), and the two oracle loads."""
    c, fl = case(name), impact_flows(name)
    w = reduced(fl["weight"]) if small else fl["weight"]
    (ea, eb), un = oracle_loads(c, (c["g"], c["g2"]), fl["src_ip"], fl["dst_ip"], w)
    g = c["g"]
    exp = expected_shift(ea, eb, identity(g.E), np.flatnonzero(c["keep"]), g.E, g.V, len(w), un)
    return dict(src_ip=fl["src_ip"], dst_ip=fl["dst_ip"], weight=w, exp=exp, ea=ea, eb=eb)


# ---- the ring: the compaction's edge cases (full and empty words, an empty aligned 256 run) ----
RING_N, RING_FAIL, RING_POPS = 512, 70, (0, 200)


@functools.lru_cache(maxsize=None)
def ring_graphml():
    """512 routers pop-i, edge i = (pop-i, pop-(i + 1) mod 512) with latency 1.0 in id order; two
    poi with a 5.0 uplink to pop-0 and pop-200 and a self loop each."""
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(RING_N)]
    nodes += [("poi-%d" % k, "t%d" % k, 0.0) for k in range(2)]
    edges = [("pop-%d" % i, "pop-%d" % ((i + 1) % RING_N), 1.0, 0.0) for i in range(RING_N)]
    for k, r in enumerate(RING_POPS):
        edges.append(("poi-%d" % k, "pop-%d" % r, 5.0, 0.0))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.0))
    return graphml_doc(nodes, edges)


@functools.lru_cache(maxsize=None)
def ring(both_ways=False):
    """dict: data, g / g2 / keep / fail, ips / verts (host k on poi k), the flows (poi-0 -> poi-1
    twice and poi-0's self pair; both_ways: the return flow too), weights 1..1448, and exp."""
    data = ring_graphml()
    g = oracle.OGraph.from_graphml(data)
    assert (g.E, g.V) == (516, 514)
    fail = np.array([RING_FAIL], np.int32)
    g2, keep = filtered(g, fail)
    ips = (host_ip(1), host_ip(2))
    verts = (RING_N, RING_N + 1)
    s, d = [ips[0], ips[0], ips[0]], [ips[1], ips[1], ips[0]]
    if both_ways:
        s.append(ips[1])
        d.append(ips[0])
    s, d = np.array(s, np.uint32), np.array(d, np.uint32)
    w = np.array([700, 41, 1448, 5][:len(s)], U64)
    c = dict(ips=ips, verts=verts)
    (ea, eb), un = oracle_loads(c, (g, g2), s, d, w)
    exp = expected_shift(ea, eb, identity(g.E), np.flatnonzero(keep), g.E, g.V, len(w), un)
    return dict(data=data, g=g, g2=g2, keep=keep, fail=fail, ips=ips, verts=verts, src_ip=s,
                dst_ip=d, weight=w, exp=exp, ea=ea, eb=eb)


# ---- a tiny complete graph: every pair of its poi directly linked, a self loop each ----
COMPLETE_N = 6


@functools.lru_cache(maxsize=None)
def complete_graphml(seed=17):
    """Latencies in [10, 15): the direct edge is the only shortest route of every pair, so the
    oracle's Dijkstra takes the route a complete topology takes by rule.  Another seed: the same
    vertices, other latencies and another edge order."""
    rng = np.random.default_rng(seed)
    nodes = [("poi-%d" % k, "t%d" % k, 0.0) for k in range(COMPLETE_N)]
    edges = [("poi-%d" % a, "poi-%d" % b, rng.uniform(10, 15), 0.0)
             for a in range(COMPLETE_N) for b in range(a + 1, COMPLETE_N)]
    edges += [("poi-%d" % k, "poi-%d" % k, 1.0, 0.0) for k in range(COMPLETE_N)]
    order = rng.permutation(len(edges))
    return graphml_doc(nodes, [edges[i] for i in order])


@functools.lru_cache(maxsize=None)
def complete_flows():
    """Every ordered pair of the hosts (host k on poi k) twice, self pairs included, and one flow
    with an unattached end; weights 1..1448."""
    ips = np.array([host_ip(k + 1) for k in range(COMPLETE_N)], np.uint32)
    si, di = np.divmod(np.arange(COMPLETE_N * COMPLETE_N), COMPLETE_N)
    s, d = np.tile(ips[si], 2), np.tile(ips[di], 2)
    s, d = np.append(s, host_ip(1000)).astype(np.uint32), np.append(d, ips[0]).astype(np.uint32)
    w = reduced(np.random.default_rng(19).integers(0, 2**64, len(s), dtype=U64))
    return dict(ips=tuple(int(x) for x in ips), verts=tuple(range(COMPLETE_N)), src_ip=s,
                dst_ip=d, weight=w)
