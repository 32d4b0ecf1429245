"""GPU tests of the link timeline (shdtopo_link_timeline, topo_timeline.hip): the weight of a set of
flows per time bin on watched edges and vertices, compared exactly with bins derived from the CPU
oracle's chains (timeline_helpers.ExpectedTimeline over load_helpers.ExpectedLoad: g.dijkstra for
the parents, g.get_eid for each hop's edge, Python floats for the prefix latencies).  The watch
sets follow the crossings' recipe over the oracle's loads (crossing_helpers.watch_recipe);
conditions on the inputs are asserted from the oracle's expectation.  Every graph has at most 700
vertices.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from crossing_helpers import (DIAMOND_POI, ExpectedCrossings, diamond_case, diamond_graphml,
                              watch_recipe)
from helpers import graphml_doc, random_topology_graphml
from load_helpers import (TRANSIT_POI, ExpectedLoad, all_pairs, check_load, long_chain_graphml,
                          pairs_crossing_ties, pinned, random_hosts, tie_grid_graphml,
                          transit_grid_graphml)
from shadow_amd import _lib
from timeline_helpers import ExpectedTimeline, bytes_equal, check_stats, check_timeline, flat

pytestmark = pytest.mark.gpu
NSRC = 5
BASE = 1_000_000_000  # ns: the start of the tests' windows
MS = 1_000_000
# the bins of the real-latency cases (hops of 1 .. 100 ms): 12 bins of 4 ms after a lead of 6 ms
RT0, RBIN, RNB = BASE + 6 * MS, 4 * MS, 12


# ------------------------------------------------------------------------------------------
# expected values, computed once per graph and shared (never modified)
# ------------------------------------------------------------------------------------------
def tie_grid_weights():
    return np.random.default_rng(21).integers(1, 2**40, 420, endpoint=True).astype(np.uint64)


def window_now(n, span_ns):
    return (BASE + np.random.default_rng(77).integers(0, span_ns, n)).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def tie_grid_expected(directed, verts):
    """6 sources x 70 destinations on the tie grid, random weights in [1, 2^40], emission times
    over a 10 ms window, 24 bins of 1 ms from its middle: (ExpectedTimeline, edges, vertices)."""
    g = oracle.OGraph.from_graphml(tie_grid_graphml(directed))
    v = np.asarray(verts, np.int32)
    sv, dv = np.repeat(v[:6], 70), np.tile(v, 6)
    exp = ExpectedLoad(g, sv, dv, tie_grid_weights(), v)
    edges, vertices = watch_recipe(exp, sv, dv)
    xt = ExpectedTimeline(g, exp, tie_grid_weights(), window_now(420, 10 * MS), edges, vertices,
                          BASE + 5 * MS, MS, 24)
    return xt, edges, vertices


@functools.lru_cache(maxsize=None)
def transit_expected(directed, verts):
    """6 x 48 unit flows on the transit grid, emission times over 6 ms, 16 bins of 1 ms after a
    lead of 2 ms."""
    g = oracle.OGraph.from_graphml(transit_grid_graphml(directed))
    v = np.asarray(verts, np.int32)
    sv, dv = np.repeat(v[:6], len(v)), np.tile(v, 6)
    exp = ExpectedLoad(g, sv, dv, None, v)
    edges, vertices = watch_recipe(exp, sv, dv)
    xt = ExpectedTimeline(g, exp, None, window_now(len(sv), 6 * MS), edges, vertices,
                          BASE + 2 * MS, MS, 16)
    return exp, xt, edges, vertices


def real_graphml():
    return random_topology_graphml(600, 60, 2400, seed=3)


def real_flows(av, aip):
    """The flow recipe of test_link_crossings.py, restated: NSRC sources x every attached vertex,
    then duplicates and self pairs, weights up to 2^40.  Returns (sip, dip, sv, dv, w)."""
    k = len(av)
    si = np.concatenate([np.repeat(np.arange(NSRC), k), [0, 0, 1, 3, 3, 2], [0, 1, 2]])
    di = np.concatenate([np.tile(np.arange(k), NSRC), [9, 9, 8, 7, 7, 11], [0, 1, 2]])
    w = np.random.default_rng(33).integers(1, 2**40, len(si), endpoint=True).astype(np.uint64)
    w[:3] = [2**40, 1, 2**40 - 1]
    return aip[si], aip[di], av[si], av[di], w


@functools.lru_cache(maxsize=None)
def real_expected(av):
    """(g, ExpectedLoad, ExpectedCrossings of the n + 1 requests, edges, vertices, chains over
    ties) of the real-latency flows plus one unattached source as the call's last request."""
    g = oracle.OGraph.from_graphml(real_graphml())
    v = np.asarray(av, np.int32)
    sip, dip, sv, dv, w = real_flows(v, np.zeros(len(v), np.uint32))
    exp = ExpectedLoad(g, sv, dv, w, v)
    edges, vertices = watch_recipe(exp, sv, dv)
    xc = ExpectedCrossings(g, exp, w, edges, vertices, flows=np.arange(len(sv)), n=len(sv) + 1)
    return g, exp, xc, edges, vertices, pairs_crossing_ties(g, exp)


def real_case(options=()):
    """Case A: (top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices); the last request has
    an unattached source, w and now cover it, sv / dv / exp / xc's flows do not."""
    top, g0, av, aip = random_hosts(real_graphml(), 300, options)
    sip, dip, sv, dv, w = real_flows(av, aip)
    g, exp, xc, edges, vertices, crossing = real_expected(tuple(int(v) for v in av))
    assert crossing == 0  # input condition: no requested chain crosses a tie
    stranger = sa.ip_to_network("10.9.8.7")
    sip = np.concatenate([sip, [stranger]]).astype(np.uint32)
    dip = np.concatenate([dip, [aip[0]]]).astype(np.uint32)
    w = np.concatenate([w, [2**39]]).astype(np.uint64)
    now = window_now(len(sip), 10 * MS)
    return top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices


def diamond_flows(ips, verts):
    """Case B: 3 free and 3 tied sources of the diamond graph to every poi, in one call."""
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
    return g, src, sip, dip, sv, dv, w


def rows_total(out):
    bins, outside = flat(out)
    return bins.sum(1, dtype=np.uint64) + outside.sum(1, dtype=np.uint64)


def crossing_rows(xc):
    """ExpectedCrossings.weight per timeline row group: fwd + rev of an edge watch, a vertex."""
    return xc.weight[:xc.ne], xc.weight[xc.ne:]


def check_against_crossings(out, xc):
    tot = rows_total(out)
    ne = xc.ne
    we, wv = crossing_rows(xc)
    assert np.array_equal(tot[:ne] + tot[ne:2 * ne], we)
    assert np.array_equal(tot[2 * ne:], wv)
    assert out["hits"] == xc.total


# ------------------------------------------------------------------------------------------
# 1, 2. the timeline against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int_keys", [0, 1])
@pytest.mark.parametrize("directed", [False, True])
def test_tie_grid_timeline(directed, int_keys):
    top, g, ips, verts = pinned(tie_grid_graphml(directed), 70, [("replay_int_keys", int_keys)])
    assert top.is_directed == directed
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    xt, edges, vertices = tie_grid_expected(directed, tuple(int(v) for v in verts))
    # conditions on the input (from the oracle's expectation), not on the code under test
    c = xt.conditions()
    print(c)
    assert c["hits"] >= 800 and c["in_range"] >= 500 and c["before"] >= 30 and c["after"] >= 3, c
    assert c["cells"] >= 60 and c["flows2"] >= 100, c
    if directed:
        assert c["rev_rows"] == 0
    else:
        assert c["rev_rows"] >= 4, c
    out = top.link_timeline(sip, dip, window_now(420, 10 * MS), edges, vertices,
                            tie_grid_weights(), t0=BASE + 5 * MS, bin_ns=MS, nbins=24)
    check_timeline(out, xt)
    if directed:
        assert not out["edge_rev"].any() and not out["outside"]["edge_rev"].any()
    ts = top.link_timeline_stats()
    check_stats(ts, xt, requests=420, sources=6)
    assert ts["chunks"] == 1 and ts["kernel_ms"] > 0
    assert ts["staged_hops"] >= ts["flows_hit"] - 6  # (the 6 self pairs are not staged)


@pytest.mark.parametrize("directed", [False, True])
def test_transit_grid_timeline(directed):
    """Destinations on other destinations' chains."""
    top, g, ips, verts = pinned(transit_grid_graphml(directed), TRANSIT_POI)
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    exp, xt, edges, vertices = transit_expected(directed, tuple(int(v) for v in verts))
    assert exp.transit_destinations() >= 80
    c = xt.conditions()
    print(c)
    assert c["hits"] >= 800 and c["in_range"] >= 500 and c["before"] >= 30 and c["after"] >= 3, c
    assert c["cells"] >= 60, c
    if directed:
        assert c["rev_rows"] == 0
    out = top.link_timeline(sip, dip, window_now(len(sip), 6 * MS), edges, vertices,
                            t0=BASE + 2 * MS, bin_ns=MS, nbins=16)
    check_timeline(out, xt)
    check_stats(top.link_timeline_stats(), xt, requests=len(sip), sources=6)


# ------------------------------------------------------------------------------------------
# 3. the prefix is summed from the source
# ------------------------------------------------------------------------------------------
def order_path_graphml():
    """poi-0 - pop-1 - pop-2 - poi-1 with latencies 0.1, 0.2, 0.3 and a self loop of 1.0 on each
    poi: (0.0 + 0.1 + 0.2) + 0.3 = 0.6000000000000001 but (0.3 + 0.2) + 0.1 = 0.6."""
    nodes = [("poi-0", "t0", 0.0), ("pop-1", "pop", 0.0), ("pop-2", "pop", 0.0),
             ("poi-1", "t1", 0.0)]
    edges = [("poi-0", "pop-1", 0.1, 0.0), ("pop-1", "pop-2", 0.2, 0.0),
             ("pop-2", "poi-1", 0.3, 0.0), ("poi-0", "poi-0", 1.0, 0.0),
             ("poi-1", "poi-1", 1.0, 0.0)]
    return graphml_doc(nodes, edges)


def test_prefix_latency_is_accumulated_from_the_source():
    top, g, ips, verts = pinned(order_path_graphml(), 2)
    assert verts.tolist() == [0, 3]
    edges, vertices = [0, 1, 2], [0, 3]
    now = 5 * BASE
    nb = 700_000
    last = {}
    for s, d in ((0, 1), (1, 0)):
        sv, dv = verts[[s]], verts[[d]]
        exp = ExpectedLoad(g, sv, dv, None, verts)
        assert exp.hops.tolist() == [3]
        xt = ExpectedTimeline(g, exp, None, [now], edges, vertices, now, 1, nb)
        out = top.link_timeline(ips[[s]], ips[[d]], [now], edges, vertices, t0=now, bin_ns=1,
                                nbins=nb)
        check_timeline(out, xt)
        assert out["hits"] == 4 and not flat(out)[1].any()
        arrive = np.nonzero(out["vertex"][d])[0]
        last[(s, d)] = arrive.tolist()
        if (s, d) == (0, 1):  # the last edge is entered after (0.0 + 0.1) + 0.2
            e2 = out["edge_fwd"][2] + out["edge_rev"][2]
            assert np.nonzero(e2)[0].tolist() == [300001]
    assert last[(0, 1)] == [600001] and last[(1, 0)] == [600000]
    # self pairs: the loop entered at `now`, the arrival one loop latency later
    for k, loop in ((0, 3), (1, 4)):
        v = int(verts[k])
        out = top.link_timeline(ips[[k]], ips[[k]], [now], [loop], [v], t0=now + MS - 1,
                                bin_ns=1, nbins=3)
        assert out["hits"] == 2
        assert out["outside"]["edge_fwd"].tolist() == [[1, 0]] and not out["edge_fwd"].any()
        assert out["vertex"].tolist() == [[0, 1, 0]] and not out["outside"]["vertex"].any()
        assert not out["edge_rev"].any() and not out["outside"]["edge_rev"].any()
        out = top.link_timeline(ips[[k]], ips[[k]], [now], [loop], [v], t0=now, bin_ns=MS,
                                nbins=2)
        assert out["edge_fwd"].tolist() == [[1, 0]] and out["vertex"].tolist() == [[0, 1]]


# ------------------------------------------------------------------------------------------
# 4. routes beyond any on-chip hop buffer
# ------------------------------------------------------------------------------------------
def test_long_chain_timeline():
    top, g, ips, verts = pinned(long_chain_graphml(), 3)
    sip, dip, sv, dv = all_pairs(ips, verts, 3)
    w = np.asarray([3, 5, 7, 11, 13, 17, 19, 23, 29], np.uint64) << np.uint64(33)
    exp = ExpectedLoad(g, sv, dv, w, verts)
    assert exp.hops.reshape(3, 3).tolist() == [[1, 201, 102], [201, 1, 101], [102, 101, 1]]
    vid = {name: k for k, name in enumerate(g.vattrs["id"])}
    uplink = g.get_eid(vid["poi-2"], vid["pop-100"])   # the middle router's poi uplink
    tail = g.get_eid(vid["pop-198"], vid["pop-199"])   # the last path edge
    assert uplink >= 0 and tail >= 0
    edges, vertices = [uplink, tail], [int(v) for v in verts]
    now = (BASE + 50 * MS * np.arange(9)).astype(np.uint64)
    bin_ns, nbins = 100 * MS, 96
    xt = ExpectedTimeline(g, exp, w, now, edges, vertices, BASE, bin_ns, nbins)
    # input conditions: the 201-hop routes arrive ~10.3 s after their emission, past the bins
    assert max(xt.hit_time) - BASE > 10_000 * MS and xt.after >= 2 and xt.in_range >= 12
    assert xt.flows_hit == 9 and xt.reverse_rows_nonzero() >= 1
    out = top.link_timeline(sip, dip, now, edges, vertices, w, t0=BASE, bin_ns=bin_ns,
                            nbins=nbins)
    check_timeline(out, xt)
    ts = top.link_timeline_stats()
    check_stats(ts, xt, requests=9, sources=3)
    assert ts["staged_hops"] == int(exp.hops[sv != dv].sum()) == 2 * (201 + 102 + 101)


# ------------------------------------------------------------------------------------------
# 5. consistency with what is already pinned
# ------------------------------------------------------------------------------------------
def check_last_arrivals(top, g, sip, dip, sv, dv, w, verts, exp):
    """Every destination vertex watched at 1 ns: emitted at T - (the packet kernel's delay of the
    table latency), every flow's last arrival lands in the one bin at T."""
    a, lat, rel, hops = g.table(verts)
    col = {int(v): k for k, v in enumerate(a)}
    i, j = [col[int(v)] for v in sv], [col[int(v)] for v in dv]
    T = 3 * BASE
    zero = np.zeros(len(sv), np.uint64)
    delay, dl, _ = oracle.route_packets(lat[i, j], rel[i, j], zero.astype(np.uint32),
                                        zero.astype(np.uint32), zero, 0, False)
    assert dl.all() and delay.min() >= MS and delay.max() < T
    now = (T - delay).astype(np.uint64)
    vertices = sorted(set(int(v) for v in dv))
    xt = ExpectedTimeline(g, exp, w, now, [], vertices, T, 1, 1)
    out = top.link_timeline(sip, dip, now, [], vertices, w, t0=T, bin_ns=1, nbins=1)
    check_timeline(out, xt)
    want = np.zeros(len(vertices), np.uint64)
    np.add.at(want, [vertices.index(int(v)) for v in dv], w)
    got = out["vertex"][:, 0]
    # (an earlier arrival of another flow in the same nanosecond could only add to a row)
    assert np.all(got >= want) and (got == want).sum() >= len(vertices) - 2
    assert not out["outside"]["vertex"][:, 1].any()  # nothing arrives after a flow's last arrival


def test_real_graph_rows_sum_to_the_crossings_and_end_at_the_packet_time():
    top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices = real_case()
    top.table()
    out = top.link_timeline(sip, dip, now, edges, vertices, w, t0=RT0, bin_ns=RBIN, nbins=RNB)
    check_against_crossings(out, xc)
    xt = ExpectedTimeline(g, exp, w[:-1], now[:-1], edges, vertices, RT0, RBIN, RNB)
    assert xt.in_range >= 100 and xt.before >= 10 and xt.after >= 10  # input conditions
    check_timeline(out, xt)
    ts = top.link_timeline_stats()
    check_stats(ts, xt, requests=len(sip), sources=NSRC, unattached=1)
    assert ts["batch_sources"] == NSRC and ts["batch_fallback"] == 0 and ts["replay_ms"] == 0
    check_last_arrivals(top, g, sip[:-1], dip[:-1], sv, dv, w[:-1], np.unique(dv), exp)


def test_diamond_graph_mixed_chunk_rows_sum_to_the_crossings():
    top, g0, ips, verts = pinned(diamond_graphml(), DIAMOND_POI)
    g, src, sip, dip, sv, dv, w = diamond_flows(ips, verts)
    exp = ExpectedLoad(g, sv, dv, w, verts)
    edges, vertices = watch_recipe(exp, sv, dv)
    xc = ExpectedCrossings(g, exp, w, edges, vertices)
    now = window_now(len(sv), 10 * MS)
    top.table()
    out = top.link_timeline(sip, dip, now, edges, vertices, w, t0=RT0, bin_ns=RBIN, nbins=RNB)
    check_against_crossings(out, xc)
    check_timeline(out, ExpectedTimeline(g, exp, w, now, edges, vertices, RT0, RBIN, RNB))
    ts = top.link_timeline_stats()
    assert ts["chunks"] == 1 and ts["sources"] == len(src) and ts["unattached"] == 0
    assert ts["batch_sources"] >= 1 and ts["batch_fallback"] >= 1
    assert ts["batch_sources"] + ts["batch_fallback"] == len(src)
    assert ts["replay_ms"] > 0 and ts["batch_ms"] > 0
    check_last_arrivals(top, g, sip, dip, sv, dv, w, verts, exp)


# ------------------------------------------------------------------------------------------
# 6. invariance
# ------------------------------------------------------------------------------------------
def test_bytes_do_not_depend_on_chain_source_chunking_or_an_explicit_zero_now():
    top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices = real_case()
    top.table()
    kw = dict(edges=edges, vertices=vertices, weight=w, t0=RT0, bin_ns=RBIN, nbins=RNB)
    a = top.link_timeline(sip, dip, now, **kw)
    assert top.link_timeline_stats()["chunks"] == 1
    top.set_option("trace_batch", 0)
    try:
        b = top.link_timeline(sip, dip, now, **kw)
        tb = top.link_timeline_stats()
    finally:
        top.set_option("trace_batch", 1)
    assert tb["batch_sources"] == 0 and tb["batch_ms"] == 0 and tb["replay_ms"] > 0
    bytes_equal(a, b)
    top.set_option("trace_chunk", 1)
    try:
        c = top.link_timeline(sip, dip, now, **kw)
        tc = top.link_timeline_stats()
    finally:
        top.set_option("trace_chunk", 0)
    assert tc["chunks"] == NSRC and tc["sources"] == NSRC and tc["batch_sources"] == NSRC
    bytes_equal(a, c)
    # "load_walk" has no meaning here: the tree accumulation's option forces no replay
    top.set_option("load_walk", 0)
    try:
        bytes_equal(a, top.link_timeline(sip, dip, now, **kw))
        assert top.link_timeline_stats()["batch_sources"] == NSRC
    finally:
        top.set_option("load_walk", 1)
    # time since emission: now = None is an explicit array of zeros
    kz = dict(edges=edges, vertices=vertices, weight=w, t0=0, bin_ns=10 * MS, nbins=32)
    z0 = top.link_timeline(sip, dip, None, **kz)
    z1 = top.link_timeline(sip, dip, np.zeros(len(sip), np.uint64), **kz)
    bytes_equal(z0, z1)
    check_timeline(z0, ExpectedTimeline(g, exp, w[:-1], None, edges, vertices, 0, 10 * MS, 32))
    assert z0["hits"] == a["hits"] == xc.total


def test_no_bins_and_no_outside():
    top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices = real_case()
    lib, _ = _lib.load()
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    we, wv = np.asarray(edges, np.int32), np.asarray(vertices, np.int32)
    rows = 2 * len(we) + len(wv)
    t0 = RT0

    def call(nbins, bins, outside, bin_ns=RBIN):
        return lib.shdtopo_link_timeline(top._h, p(sip), p(dip), p(w), p(now), len(sip), p(we),
                                         len(we), p(wv), len(wv), t0, bin_ns, nbins, p(bins),
                                         p(outside))
    # nbins = 0, bins = NULL: every hit at or after t0 is "after"
    xt = ExpectedTimeline(g, exp, w[:-1], now[:-1], edges, vertices, t0, RBIN, 0)
    assert xt.before >= 10 and xt.after >= 100 and xt.in_range == 0
    outside = np.full((rows, 2), 7, np.uint64)
    assert call(0, None, outside, bin_ns=0) == xt.hits == xc.total
    assert np.array_equal(outside, xt.outside)
    ts = top.link_timeline_stats()
    assert (ts["before"], ts["after"], ts["in_range"]) == (xt.before, xt.after, 0)
    # outside = NULL: the bins alone
    xb = ExpectedTimeline(g, exp, w[:-1], now[:-1], edges, vertices, t0, RBIN, RNB)
    bins = np.full((rows, RNB), 7, np.uint64)
    assert call(RNB, bins, None) == xb.hits
    assert np.array_equal(bins, xb.bins)
    assert call(0, None, None, bin_ns=0) == xb.hits


# ------------------------------------------------------------------------------------------
# 7. nothing else moves
# ------------------------------------------------------------------------------------------
def check_trace(tr, exp):
    """A trace's routes equal the oracle's chains (vertex by vertex, edge by edge)."""
    assert np.all(tr["status"] == 0) and np.array_equal(tr["hops"], exp.hops)
    for i in range(len(exp.verts)):
        o, h = int(tr["offset"][i]), int(tr["hops"][i])
        assert list(tr["vertices"][o:o + h + 1]) == exp.verts[i], i
        assert list(tr["edges"][o:o + h]) == exp.edges[i], i


@pytest.mark.parametrize("tie_free", [False, True])
def test_timeline_leaves_stats_table_lazy_rows_traces_loads_and_crossings_alone(tie_free):
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
    now = window_now(len(sip), 10 * MS)
    xt = ExpectedTimeline(g, exp, None, now, edges, vertices, BASE + 5 * MS, MS, 24)
    kw = dict(edges=edges, vertices=vertices, t0=BASE + 5 * MS, bin_ns=MS, nbins=24)
    check_trace(top.trace_routes(sip, dip), exp)
    check_load(top.link_load(sip, dip), exp)
    assert top.link_crossings(sip, dip, edges, vertices)["total"] == xc.total
    st0, ts0, ls0 = top.stats(), top.trace_stats(), top.link_load_stats()
    cs0 = top.link_crossings_stats()
    lz0 = top.lazy_rows()
    lm0 = top.lazyMinimumLatency()
    check_timeline(top.link_timeline(sip, dip, now, **kw), xt)
    assert top.stats() == st0 and top.trace_stats() == ts0 and top.link_load_stats() == ls0
    assert top.link_crossings_stats() == cs0
    assert all(np.array_equal(x, y) for x, y in zip(top.lazy_rows(), lz0))
    assert top.lazyMinimumLatency() == lm0
    a1, lat1, rel1, hops1 = top.table()
    assert top.stats() == st0  # no rebuild
    assert np.array_equal(a0, a1) and np.array_equal(hops0, hops1)
    assert lat0.tobytes() == lat1.tobytes() and rel0.tobytes() == rel1.tobytes()
    check_trace(top.trace_routes(sip, dip), exp)  # the same slots, used again
    check_load(top.link_load(sip, dip), exp)
    out = top.link_timeline(sip, dip, now, **kw)
    check_timeline(out, xt)
    assert out["hits"] == xc.total
    assert top.stats() == st0


def test_multi_device_topology_answers_on_its_first_device():
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70, [("devices", 2)])
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    xt, edges, vertices = tie_grid_expected(False, tuple(int(v) for v in verts))
    top.table()
    st0 = top.stats()
    assert st0["devices"] == 2
    out = top.link_timeline(sip, dip, window_now(420, 10 * MS), edges, vertices,
                            tie_grid_weights(), t0=BASE + 5 * MS, bin_ns=MS, nbins=24)
    check_timeline(out, xt)
    assert top.stats() == st0
