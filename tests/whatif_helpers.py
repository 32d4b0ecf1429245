"""Expected values and shared inputs of the link-failure what-if tests (test_whatif.py,
test_whatif_cpu.py).

Every expected value comes from the CPU oracle or from numpy on the oracle's tables: the filtered
edge arrays of the oracle's graph are the reference for a derived topology (deleting edges in
igraph keeps the order and so the "lowest edge id" rule), and the diff of two oracle tables,
computed here in numpy, is the reference for the device diff.  Nothing in this file calls
``without``, ``edge_origin`` or ``table_diff``.
"""
import functools
import os

import numpy as np

import oracle
import shadow_amd as sa
from helpers import (DOMAIN_HOSTS, domain_graphml, domain_oracle, host_ip,
                     random_topology_graphml)

# one record of the diff (ShdTableChange), restated: the product's dtype is not the reference
CHANGE = np.dtype([("srcCol", np.int32), ("dstCol", np.int32), ("lat0", np.float64),
                   ("lat1", np.float64), ("rel0", np.float64), ("rel1", np.float64),
                   ("hops0", np.uint16), ("hops1", np.uint16), ("kind", np.uint32)])
ROSE, FELL, REL, HOPS = 1, 2, 4, 8
N_ROUTERS = 600
NTHREADS = min(8, os.cpu_count() or 1)


def router_count(g):
    """Routers come first in the documents of random_topology_graphml ("pop-i" is vertex i)."""
    ids = g.vattrs["id"]
    n = sum(1 for x in ids if x.startswith("pop-"))
    assert all(ids[i] == "pop-%d" % i for i in range(n))
    return n


def extra_edges(g):
    """Edge ids of the "extra" router edges: both ends routers, neither a cycle edge (routers i
    and i + 1 mod n, identified by their endpoints) nor a self loop."""
    n = router_count(g)
    a, b = g.eu.astype(np.int64), g.ev.astype(np.int64)
    gap = np.abs(a - b)
    m = (a < n) & (b < n) & (a != b) & (gap != 1) & (gap != n - 1)
    return np.flatnonzero(m)


def failing_set(g, k, among=None):
    """The recipe: the k lowest-latency extra router edges (ties by edge id)."""
    ex = extra_edges(g) if among is None else np.asarray(among)
    order = np.argsort(g.elat[ex], kind="stable")
    return np.sort(ex[order[:k]]).astype(np.int32)


def filtered(g, fail_edges=(), fail_vertices=()):
    """(the oracle's graph without the edges and vertices, the keep mask over g's edge ids)."""
    keep = np.ones(g.E, bool)
    keep[np.asarray(fail_edges, np.int64)] = False
    for v in fail_vertices:
        keep &= (g.eu != v) & (g.ev != v)
    g2 = oracle.OGraph(g.V, g.eu[keep], g.ev[keep], g.elat[keep], g.eloss[keep], g.vloss,
                       g.directed, g.vattrs)
    return g2, keep


def oracle_attach(g, n_hosts, hints=None, seed=1, only=None):
    """attach_hosts' stream, the oracle's half: (ips, verts, states); `only`: the hosts of the
    stream to attach (indices; every host has its own random stream, so the others do not
    matter)."""
    otop = oracle.OracleTopology(g)
    ips, verts, states = [], [], []
    st = seed
    for k in range(n_hosts):
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        if only is not None and k not in only:
            continue
        v, s = otop.attach(host_ip(k + 1), st, type_hint=hints[k % len(hints)] if hints else None)
        ips.append(host_ip(k + 1))
        verts.append(v)
        states.append(s)
    return ips, verts, states


def product_attach(top, n_hosts, hints=None, seed=1, only=None):
    """The same stream on the product: (ips, verts, states)."""
    ips, verts, states = [], [], []
    st = seed
    for k in range(n_hosts):
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        if only is not None and k not in only:
            continue
        v, s = top.attach_ip(host_ip(k + 1), st, typeHint=hints[k % len(hints)] if hints else None)
        ips.append(host_ip(k + 1))
        verts.append(v)
        states.append(s)
    return ips, verts, states


def expected_diff(t0, t1):
    """The diff of two oracle tables (attached, lat, rel, hops) in numpy: a dict with the keys of
    Topology.table_diff."""
    a0, lat0, rel0, hops0 = t0
    a1, lat1, rel1, hops1 = t1
    assert np.array_equal(a0, a1)
    A = len(a0)
    hops0, hops1 = hops0.astype(np.uint16), hops1.astype(np.uint16)
    dl = lat0.view(np.uint64) != lat1.view(np.uint64)
    dr = rel0.view(np.uint64) != rel1.view(np.uint64)
    dh = hops0 != hops1
    rose, fell = dl & (lat1 > lat0), dl & (lat1 < lat0)
    kind = (rose * ROSE + fell * FELL + dr * REL + dh * HOPS).astype(np.uint32)
    changed = dl | dr | dh
    s, d = np.nonzero(changed)  # row-major: srcCol, then dstCol
    rec = np.zeros(len(s), CHANGE)
    rec["srcCol"], rec["dstCol"] = s, d
    rec["lat0"], rec["lat1"] = lat0[s, d], lat1[s, d]
    rec["rel0"], rec["rel1"] = rel0[s, d], rel1[s, d]
    rec["hops0"], rec["hops1"] = hops0[s, d], hops1[s, d]
    rec["kind"] = kind[s, d]
    rise = np.where(rose, lat1 - lat0, -np.inf)
    col = np.where(rose.any(axis=1), rise.argmax(axis=1), -1).astype(np.int32)  # the lowest column
    worst = np.where(col >= 0, rise.max(axis=1) if A else 0.0, 0.0)
    return {"total": len(s), "records": rec,
            "kind_count": np.array([(kind & b != 0).sum() for b in (ROSE, FELL, REL, HOPS)],
                                   np.uint64),
            "row_changed": changed.sum(axis=1).astype(np.uint32),
            "row_worst_rise": worst.astype(np.float64), "row_worst_col": col}


def swapped(exp):
    """The records of exp with the two sides exchanged: lat0 <-> lat1, rel0 <-> rel1, hops0 <->
    hops1, kind bit 1 <-> bit 2 -- what the diff in the other direction must report."""
    rec = exp["records"].copy()
    for x, y in (("lat0", "lat1"), ("rel0", "rel1"), ("hops0", "hops1")):
        rec[x], rec[y] = exp["records"][y], exp["records"][x]
    k = exp["records"]["kind"]
    rec["kind"] = (k & ~np.uint32(3)) | ((k & 1) << 1) | ((k & 2) >> 1)
    return rec


def assert_diff_equal(got, exp, cap=None):
    """Every output of table_diff against expected_diff; records are the first `cap` (None: all)."""
    assert got["total"] == exp["total"]
    n = exp["total"] if cap is None else min(cap, exp["total"])
    assert len(got["records"]) == n
    for f in CHANGE.names:
        x, y = got["records"][f], exp["records"][f][:n]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), np.ascontiguousarray(y).view(np.uint64)
        assert np.array_equal(x, y), f
    assert np.array_equal(got["kind_count"], exp["kind_count"])
    assert np.array_equal(got["row_changed"], exp["row_changed"])
    assert np.array_equal(got["row_worst_rise"].view(np.uint64),
                          exp["row_worst_rise"].view(np.uint64))
    assert np.array_equal(got["row_worst_col"], exp["row_worst_col"])


# ---- the recipe's four cases, their oracle tables computed once and shared (never modified) ----
CASES = {
    "real": dict(doc=dict(), k=8, hosts=60),
    "int": dict(doc=dict(integer=True), k=8, hosts=60),
    "directed": dict(doc=dict(directed=True), k=8, hosts=60),
    "parallel": dict(doc=dict(parallel=50), k=8, hosts=60),
    # the 3,000-router tie-free domain graph: 120 hosts without hints (72 columns), and with the
    # hints and the shared parent table of domain_oracle (69 columns)
    "logu": dict(doc=None, k=16, hosts=DOMAIN_HOSTS),
    "logu_hints": dict(doc=None, k=16, hosts=DOMAIN_HOSTS),
    # shapes: one host (the self pair alone), two columns, about 300 columns (a row spans several
    # wavefronts and more than one 256-thread workgroup step), and a failing set that touches one
    # router only (most rows have no change)
    "one": dict(doc=dict(), k=8, hosts=1),
    "two": dict(doc=dict(), k=8, hosts=60, pick=True),
    "wide": dict(doc=dict(n_poi=400), k=8, hosts=600),
    "one_router": dict(doc=dict(), k=None, hosts=60),
}


def one_router_edges(g, verts, t0):
    """All extra edges of one router: the first router, by descending number of extra edges,
    whose failure changes some rows of the oracle's table but at most a third of them."""
    ex = extra_edges(g)
    deg = np.bincount(np.concatenate([g.eu[ex], g.ev[ex]]), minlength=g.V)
    for r in np.argsort(-deg, kind="stable")[:40]:
        fail = ex[(g.eu[ex] == r) | (g.ev[ex] == r)].astype(np.int32)
        rows = expected_diff(t0, filtered(g, fail)[0].table(verts))["row_changed"]
        if 0 < (rows > 0).sum() <= len(rows) // 3:
            return fail
    raise AssertionError("no router with a small blast radius among the candidates")


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: data (GraphML bytes), g (parent oracle graph), fail (edge ids), g2 / keep (the
    filtered graph and mask), ips / verts / hints, t0 / t1 (parent and child oracle tables)."""
    c = CASES[name]
    only = None
    if name == "logu_hints":
        data = domain_graphml("logu")
        g, ips, verts, t0 = domain_oracle("logu")
        hints = ("client", "relay", "server")
    else:
        data = domain_graphml("logu") if name == "logu" else random_topology_graphml(**c["doc"])
        g = oracle.OGraph.from_graphml(data)
        hints = None
        if c.get("pick"):
            # the two hosts of the first changed pair of the 60-host case on the same graph
            base = case("real")
            r = base["exp"]["records"][0]
            ends = [int(base["t0"][0][r["srcCol"]]), int(base["t0"][0][r["dstCol"]])]
            only = tuple(base["verts"].index(v) for v in ends)
        ips, verts, _ = oracle_attach(g, c["hosts"], only=only)
        t0 = g.table(verts, nthreads=NTHREADS)
    fail = one_router_edges(g, verts, t0) if c["k"] is None else failing_set(g, c["k"])
    g2, keep = filtered(g, fail)
    assert g2.is_strongly_connected()
    t1 = g2.table(verts, nthreads=NTHREADS)
    return dict(data=data, g=g, fail=fail, g2=g2, keep=keep, ips=tuple(ips), verts=tuple(verts),
                hints=hints, hosts=c["hosts"], only=only, t0=t0, t1=t1,
                exp=expected_diff(t0, t1))


def product(name):
    """The product's parent topology of a case with its hosts attached (a fresh one each call)."""
    c = case(name)
    top = sa.Topology.from_buffer(c["data"])
    assert top is not None
    _, verts, _ = product_attach(top, c["hosts"], c["hints"], only=c["only"])
    assert tuple(verts) == c["verts"]
    return top


def assert_table_equal(top, t):
    a, lat, rel, hops = top.table()
    oa, olat, orel, ohops = t
    assert np.array_equal(a, oa)
    assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64))
    assert np.array_equal(rel.view(np.uint64), orel.view(np.uint64))
    assert np.array_equal(hops, ohops.astype(np.uint16))


def attach_off_column(c, parent, child, ip=host_ip(5000), state=12345):
    """One more host on parent and child, on the same vertex, one that is no column of case c yet;
    returns the vertex.  The bundled graphs give their vertices no ip, so no ipHint can pin it:
    the host's random stream does (the same state draws the same candidate on both), and the state
    is the first one of the stream that lands off the columns."""
    while True:
        v, nxt = parent.attach_ip(ip, state)
        if v not in c["verts"]:
            break
        parent.detach_ip(ip)
        state = nxt
    assert child.attach_ip(ip, state)[0] == v
    assert np.array_equal(parent.attached_vertices(), child.attached_vertices())
    return v


BUILD_COUNTERS = ("paths_computed", "sources", "targets", "build_ms")


def build_counters(top):
    """The fields of stats() a table build moves."""
    st = top.stats()
    return {k: st[k] for k in BUILD_COUNTERS}
