"""Route tracing from the batch kernel's parent records (option "trace_batch").

A chunk of traced sources runs the batch kernel's keep launch; a source whose row the launch
leaves unflagged is walked from the slots' pair records, a flagged one goes through the exact heap
replay as before.  The tests compare the routes with the CPU oracle (test_trace.Expected) and, byte
for byte, with the replay path (trace_batch = 0), and check which path served which source through
the trace's own counters.  Conditions on the inputs (which rows cross a tied parent) come from the
oracle alone.  Every graph has at most 700 vertices.
"""
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import (attach_hosts, bundled_pair, graphml_doc, host_ip, oracle_table,
                     random_topology_graphml)
from test_trace import (Expected, all_pairs, check_routes, check_table, long_chain_graphml, pinned,
                        random_hosts, tie_grid_graphml, tied_vertices)

gpu = pytest.mark.gpu
ROUTE_KEYS = ("offset", "hops", "status", "latency", "reliability", "vertices", "edges")


# ------------------------------------------------------------------------------------------
# inputs and their oracle analysis (CPU only, computed once, never modified)
# ------------------------------------------------------------------------------------------
def first_hosts(ips, verts):
    """One IP per attached vertex: (attached vertices ascending, {vertex: ip})."""
    first = {}
    for ip, v in zip(ips, verts):
        first.setdefault(int(v), ip)
    return sorted(first), first


def requests(av, first, src):
    """Every source of src to every attached vertex: (sip, dip, sv, dv)."""
    sv = np.repeat(src, len(av)).astype(np.int32)
    dv = np.tile(av, len(src)).astype(np.int32)
    sip = np.asarray([first[int(v)] for v in sv], np.uint32)
    dip = np.asarray([first[int(v)] for v in dv], np.uint32)
    return sip, dip, sv, dv


def sources_crossing_ties(g, exp):
    """Sources of exp with a requested chain over a vertex whose parent igraph's pop order
    decides (exp must request every attached vertex from each source)."""
    out = set()
    for s in exp.dij:
        tied = tied_vertices(g, g.dijkstra(s)[0], s)
        if any(c[0] == s and c[0] != c[-1] and tied[c[1:]].any() for c in exp.verts):
            out.add(s)
    return out


def real_graphml(directed=False):
    return random_topology_graphml(600, 60, 2400, seed=3, directed=directed)


def real_topology(directed=False, options=(), first_src=0, nsrc=5):
    """The real-latency graph with 300 hosts; nsrc sources x every attached vertex.
    Returns (top, g, av, first, (sip, dip, sv, dv))."""
    top, g, ips, verts = random_hosts(real_graphml(directed), 300, options)
    av, first = first_hosts(ips, verts)
    assert len(av) >= 50
    return top, g, av, first, requests(av, first, av[first_src:first_src + nsrc])


@functools.lru_cache(maxsize=None)
def real_expected(directed, av, src):
    """(Expected, sources crossing a tie) of src x av on the real-latency graph."""
    g = oracle.OGraph.from_graphml(real_graphml(directed))
    sv = np.repeat(src, len(av)).astype(np.int32)
    dv = np.tile(av, len(src)).astype(np.int32)
    exp = Expected(g, sv, dv, av)
    return exp, sources_crossing_ties(g, exp)


def expected_of(directed, av, sv):
    src = tuple(sorted(set(int(v) for v in sv)))
    return real_expected(directed, tuple(int(v) for v in av), src)


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
    """The oracle's view of the diamond graph: the poi whose rows cross the planted tie and those
    whose rows cross none; the test's sources are 3 of each."""
    g = oracle.OGraph.from_graphml(diamond_graphml())
    v = np.asarray(verts, np.int32)
    full = Expected(g, np.repeat(v, len(v)), np.tile(v, len(v)), v)
    crossing = sources_crossing_ties(g, full)
    free = [int(x) for x in v if int(x) not in crossing]
    tied = [int(x) for x in v if int(x) in crossing]
    return g, free, tied


def bytes_equal(a, b):
    for k in ROUTE_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["total"] == b["total"]


def trace_both(top, sip, dip):
    """The same requests on the replay path and on the batch path: (replay, batch, batch stats)."""
    top.set_option("trace_batch", 0)
    try:
        a = top.trace_routes(sip, dip)
        ts = top.trace_stats()
        assert ts["batch_sources"] == 0 and ts["batch_fallback"] == 0 and ts["batch_ms"] == 0
    finally:
        top.set_option("trace_batch", 1)
    b = top.trace_routes(sip, dip)
    return a, b, top.trace_stats()


# ------------------------------------------------------------------------------------------
# 1. real latencies: served from pair records
# ------------------------------------------------------------------------------------------
@gpu
def test_real_latencies_are_served_from_pair_records():
    top, g, av, first, (sip, dip, sv, dv) = real_topology()
    exp, crossing = expected_of(False, av, sv)
    assert not crossing  # input condition: no requested row crosses a tie
    top.table()
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)
    ts = top.trace_stats()
    assert ts["sources"] == 5 and ts["chunks"] == 1 and ts["requests"] == len(sip)
    assert ts["batch_sources"] == 5 and ts["batch_fallback"] == 0
    assert ts["replay_ms"] == 0 and ts["batch_ms"] > 0


# ------------------------------------------------------------------------------------------
# 2. byte-identical to the replay path
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("directed", [False, True])
def test_real_latencies_equal_the_replay_path(directed):
    top, g, av, first, (sip, dip, sv, dv) = real_topology(directed)
    exp, crossing = expected_of(directed, av, sv)
    assert top.is_directed == directed and not crossing
    top.table()
    a, b, ts = trace_both(top, sip, dip)
    bytes_equal(a, b)
    check_routes(b, exp)
    assert ts["batch_sources"] + ts["batch_fallback"] == ts["sources"] == 5
    assert ts["batch_sources"] > 0  # the (directed) keep instantiation ran and served routes


@gpu
@pytest.mark.parametrize("directed", [False, True])
def test_tie_grids_equal_the_replay_path(directed):
    top, g, ips, verts = pinned(tie_grid_graphml(directed), 70)
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    top.table()
    a, b, ts = trace_both(top, sip, dip)
    bytes_equal(a, b)
    check_table(top, b, sv, dv)
    assert ts["sources"] == 6


@gpu
def test_long_chain_equals_the_replay_path():
    """Routes of 201 hops, beyond kMaxHops: the pair walk stages in HBM like the replay's."""
    top, g, ips, verts = pinned(long_chain_graphml(), 3)
    sip, dip, sv, dv = all_pairs(ips, verts, 3)
    exp = Expected(g, sv, dv, verts)
    assert exp.hops.max() == 201 and not sources_crossing_ties(g, exp)
    top.table()
    a, b, ts = trace_both(top, sip, dip)
    bytes_equal(a, b)
    check_routes(b, exp)
    assert ts["batch_sources"] == 3 and ts["batch_fallback"] == 0


# ------------------------------------------------------------------------------------------
# 3. a chunk with both kinds of sources
# ------------------------------------------------------------------------------------------
@gpu
def test_mixed_chunk_replays_only_the_tied_sources():
    top, g0, ips, verts = pinned(diamond_graphml(), DIAMOND_POI)
    g, free, tied = diamond_case(tuple(int(v) for v in verts))
    assert len(free) >= 2 and len(tied) >= 2, (len(free), len(tied))  # input condition
    src = sorted(free[:3] + tied[:3])
    nfree = len(free[:3])
    ipof = {int(v): ip for ip, v in zip(ips, verts)}
    vs = sorted(ipof)
    sip, dip, sv, dv = requests(vs, ipof, src)
    exp = Expected(g, sv, dv, verts)
    top.table()
    a, b, ts = trace_both(top, sip, dip)
    check_routes(b, exp)
    check_table(top, b, sv, dv)
    bytes_equal(a, b)
    assert ts["chunks"] == 1 and ts["sources"] == len(src)
    assert ts["batch_sources"] >= 1 and ts["batch_fallback"] >= 1
    assert ts["batch_sources"] + ts["batch_fallback"] == ts["sources"]
    assert ts["batch_sources"] <= nfree
    assert ts["replay_ms"] > 0 and ts["batch_ms"] > 0


# ------------------------------------------------------------------------------------------
# 4. chunks and slot reuse
# ------------------------------------------------------------------------------------------
@gpu
def test_chunks_and_slot_reuse():
    top, g, av, first, (sip, dip, sv, dv) = real_topology()
    exp, _ = expected_of(False, av, sv)
    top.table()
    a = top.trace_routes(sip, dip)
    assert top.trace_stats()["chunks"] == 1
    top.set_option("trace_chunk", 2)
    try:
        b = top.trace_routes(sip, dip)
        ts = top.trace_stats()
        assert ts["chunks"] == 3 and ts["sources"] == 5 and ts["batch_sources"] == 5
    finally:
        top.set_option("trace_chunk", 0)
    bytes_equal(a, b)
    check_routes(b, exp)
    # other sources in the same slots: the earlier batches' records carry another tag
    sip2, dip2, sv2, dv2 = requests(av, first, av[7:11])
    exp2, _ = expected_of(False, av, sv2)
    c = top.trace_routes(sip2, dip2)
    check_routes(c, exp2)
    assert top.trace_stats()["batch_sources"] == 4


# ------------------------------------------------------------------------------------------
# 5. every batch width, with and without LDS hubs
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hubs", [0, None])
@pytest.mark.parametrize("batch", [2, 4, 16])
def test_every_batch_width_and_the_hubs(batch, hubs):
    opts = [("batch", batch)] + ([("lds_hubs", hubs)] if hubs is not None else [])
    top, g, av, first, (sip, dip, sv, dv) = real_topology(options=opts)
    exp, _ = expected_of(False, av, sv)
    top.table()
    assert top.stats()["batch"] == batch
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)
    assert top.trace_stats()["batch_sources"] > 0


# ------------------------------------------------------------------------------------------
# 6. a target set the relaxation copy was not prepared for
# ------------------------------------------------------------------------------------------
@gpu
def test_stale_target_set_takes_the_replay():
    data = real_graphml()
    top, g, ips, verts = random_hosts(data, 100)
    top.table()
    # a host on a vertex no host was on: the attached set changes, the table is stale
    otop = oracle.OracleTopology(g)
    have = set(int(v) for v in verts)
    ips, verts = list(ips), list(verts)
    st, k = 12345, 0
    while True:
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        ip = host_ip(1000 + k)
        v, _ = top.attach_ip(ip, st, typeHint=("client", "relay", "server")[k % 3])
        ips.append(ip)
        verts.append(v)
        k += 1
        if int(v) not in have:
            break
        assert k < 200
    av, first = first_hosts(ips, verts)
    assert len(av) == len(have) + 1
    src = [av[0], av[1], int(v)]
    sip, dip, sv, dv = requests(av, first, src)
    exp = Expected(g, sv, dv, av)
    tr = top.trace_routes(sip, dip)  # before any rebuild
    check_routes(tr, exp)
    ts = top.trace_stats()
    assert ts["batch_sources"] == 0 and ts["batch_fallback"] == 0 and ts["sources"] == 3
    top.table()
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)
    assert top.trace_stats()["batch_sources"] > 0


# ------------------------------------------------------------------------------------------
# 7. a batch-path trace and load leave everything alone
# ------------------------------------------------------------------------------------------
@gpu
def test_batch_path_leaves_stats_table_and_workspace_alone():
    top, g, av, first, (sip, dip, sv, dv) = real_topology()
    ip0, ip1 = first[av[0]], first[av[1]]
    assert top.latency_ip(ip0, ip1) > 0  # builds the table, materialises a lazy row
    a0, lat0, rel0, hops0 = top.table()
    st0 = top.stats()
    lz0 = top.lazy_rows()
    lm0 = top.lazyMinimumLatency()
    tr = top.trace_routes(sip, dip)
    assert np.all(tr["status"] == 0) and top.trace_stats()["batch_sources"] == 5
    out = top.link_load(sip, dip)
    assert out["routed"] == len(sip) and top.link_load_stats()["batch_sources"] == 5
    assert top.stats() == st0
    assert all(np.array_equal(x, y) for x, y in zip(top.lazy_rows(), lz0))
    assert top.lazyMinimumLatency() == lm0
    a1, lat1, rel1, hops1 = top.table()
    assert top.stats() == st0  # no rebuild
    assert np.array_equal(a0, a1) and np.array_equal(hops0, hops1)
    assert lat0.tobytes() == lat1.tobytes() and rel0.tobytes() == rel1.tobytes()
    # the workspace was left clean: the next build is the oracle's table bit for bit
    top.rebuild()
    a2, lat2, rel2, hops2 = top.table()
    oa, olat, orel, ohops = oracle_table(g, a2)
    assert np.array_equal(a2, oa) and np.array_equal(hops2, ohops.astype(np.uint16))
    assert lat2.tobytes() == olat.tobytes() and rel2.tobytes() == orel.tobytes()


# ------------------------------------------------------------------------------------------
# 9. multi-device
# ------------------------------------------------------------------------------------------
@gpu
def test_multi_device_topology_traces_either_way():
    top, g, av, first, (sip, dip, sv, dv) = real_topology(options=[("devices", 2)])
    exp, _ = expected_of(False, av, sv)
    top.table()
    st0 = top.stats()
    assert st0["devices"] == 2
    tr = top.trace_routes(sip, dip)
    check_routes(tr, exp)
    check_table(top, tr, sv, dv)
    ts = top.trace_stats()
    assert ts["batch_sources"] + ts["batch_fallback"] in (0, ts["sources"])
    assert top.stats() == st0


# ------------------------------------------------------------------------------------------
# 10. the option and the counters without a device
# ------------------------------------------------------------------------------------------
def test_trace_batch_option_and_counters_on_a_complete_topology():
    top, g = bundled_pair("topology.simple")
    assert top.is_complete
    for v in (0, 1):
        top.set_option("trace_batch", v)
    for bad in (2, -1):
        with pytest.raises(KeyError):
            top.set_option("trace_batch", bad)
    otop, ips, verts = attach_hosts(top, g, 4)
    ips = np.asarray(ips, np.uint32)
    tr = top.trace_routes(ips[[0, 1]], ips[[2, 3]])
    assert np.all(tr["status"] == 0)
    ts = top.trace_stats()
    assert ts["batch_ms"] == 0 and ts["batch_sources"] == 0 and ts["batch_fallback"] == 0
    out = top.link_load(ips[[0, 1]], ips[[2, 3]])
    assert out["routed"] == 2
    ls = top.link_load_stats()
    assert ls["batch_ms"] == 0 and ls["batch_sources"] == 0 and ls["batch_fallback"] == 0
