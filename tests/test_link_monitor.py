"""GPU tests of the link monitor (shdtopo_monitor_*, topo_monitor.hip): a persistent set of watched
edges and vertices whose per-time-bin traffic is fed by packet windows from a hit index over the
table's column pairs, instead of walking every packet's route.  Expected values come from the CPU
oracle alone (monitor_helpers: timeline_helpers.ExpectedTimeline over load_helpers.ExpectedLoad);
the comparison with one link_timeline call on all fed packets is a second, separate assertion.
Watch sets follow the crossings' recipe over the oracle's loads; conditions on the inputs are
asserted from the oracle's expectation.  Every graph has at most 700 vertices.
"""
import ctypes
import functools
import types
import zlib

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from crossing_helpers import DIAMOND_POI, diamond_graphml, watch_recipe
from helpers import attach_hosts, host_ip
from load_helpers import (TRANSIT_POI, ExpectedLoad, all_pairs, long_chain_graphml, pinned,
                          random_hosts, tie_grid_graphml, transit_grid_graphml)
from monitor_helpers import check_counters, check_index, check_last, pair_grid, zero_bins
from shadow_amd import _lib
from test_link_timeline import (BASE, MS, NSRC, RBIN, RNB, RT0, diamond_flows, order_path_graphml,
                                real_case, real_graphml, tie_grid_expected, tie_grid_weights,
                                transit_expected, window_now)
from timeline_helpers import ExpectedTimeline, bytes_equal, check_timeline, flat

pytestmark = pytest.mark.gpu
KW = dict(t0=RT0, bin_ns=RBIN, nbins=RNB)


# ------------------------------------------------------------------------------------------
# expected values, computed once per graph and shared (never modified)
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_chains(data, av):
    """(g, the oracle's chains of every ordered pair of the attached vertices av)."""
    g = oracle.OGraph.from_graphml(data)
    v = np.asarray(av, np.int32)
    sv, dv = pair_grid(v)
    return g, ExpectedLoad(g, sv, dv, None, v)


def cut(chains, idx):
    return types.SimpleNamespace(verts=[chains.verts[i] for i in idx],
                                 edges=[chains.edges[i] for i in idx])


def windows(n, k=3):
    """k index ranges over n packets and emission times in k different ranges: window j is emitted
    over [BASE + 20 j ms, BASE + 20 j ms + 10 ms)."""
    idx = np.array_split(np.arange(n), k)
    now = window_now(n, 10 * MS)
    for j, i in enumerate(idx):
        now[i] += np.uint64(20 * MS * j)
    return idx, now


def columns(av, v):
    return np.searchsorted(np.asarray(av), v).astype(np.int32)


def cu(x):
    import torch
    x = np.ascontiguousarray(x)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(x.dtype)
    return torch.from_numpy(x.view(view) if view else x).cuda()


def index_bytes(mon):
    return tuple(x.tobytes() for x in mon.export_index())


# ------------------------------------------------------------------------------------------
# 1. the index equals the oracle
# ------------------------------------------------------------------------------------------
def test_real_graph_index_equals_the_oracle_whatever_the_chain_source_and_the_chunk():
    top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices = real_case()
    av = top.attached_vertices()
    g2, chains = all_chains(real_graphml(), tuple(int(v) for v in av))
    top.table()
    mon = top.link_monitor(edges, vertices, **KW)
    xt = check_index(mon, g, chains, edges, vertices, min_hits=300)
    st = mon.stats()
    A = len(av)
    assert st["prepares"] == 1 and st["sources"] == A and st["chunks"] >= 1
    assert st["batch_sources"] >= NSRC and st["batch_sources"] + st["batch_fallback"] == A
    assert st["kernel_ms"] > 0 and st["prepare_ms"] > 0
    a = index_bytes(mon)
    top.set_option("trace_batch", 0)
    try:
        assert mon.prepare() == xt.hits
        sb = mon.stats()
        b = index_bytes(mon)
    finally:
        top.set_option("trace_batch", 1)
    assert sb["batch_sources"] == 0 and sb["batch_ms"] == 0 and sb["replay_ms"] > 0
    top.set_option("trace_chunk", 2)
    try:
        assert mon.prepare() == xt.hits
        sc = mon.stats()
        c = index_bytes(mon)
    finally:
        top.set_option("trace_chunk", 0)
    assert sc["chunks"] == (A + 1) // 2 and sc["sources"] == A and sc["prepares"] == 3
    assert a == b == c


@pytest.mark.parametrize("directed", [False, True])
def test_tie_grid_index_equals_the_oracle(directed):
    """Every source of the tie grid goes through the heap replay."""
    top, g, ips, verts = pinned(tie_grid_graphml(directed), 70)
    xt0, edges, vertices = tie_grid_expected(directed, tuple(int(v) for v in verts))
    g2, chains = all_chains(tie_grid_graphml(directed), tuple(int(v) for v in verts))
    mon = top.link_monitor(edges, vertices, t0=BASE + 5 * MS, bin_ns=MS, nbins=24)
    xt = check_index(mon, g, chains, edges, vertices, min_hits=2000)
    if directed:
        assert xt.reverse_rows_nonzero() == 0
    else:
        assert xt.reverse_rows_nonzero() >= 4
    st = mon.stats()
    assert st["sources"] == 70 and st["replay_ms"] > 0
    assert st["batch_sources"] + st["batch_fallback"] in (0, 70)


def test_transit_grid_directed_index_equals_the_oracle():
    """Destinations on other destinations' chains, arcs of a directed topology."""
    top, g, ips, verts = pinned(transit_grid_graphml(True), TRANSIT_POI)
    exp, xt0, edges, vertices = transit_expected(True, tuple(int(v) for v in verts))
    g2, chains = all_chains(transit_grid_graphml(True), tuple(int(v) for v in verts))
    mon = top.link_monitor(edges, vertices, t0=0, bin_ns=MS, nbins=4)
    xt = check_index(mon, g, chains, edges, vertices, min_hits=2000)
    assert chains.transit_destinations() >= 500 and xt.reverse_rows_nonzero() == 0


def test_diamond_graph_index_mixes_both_chain_sources_in_one_prepare():
    top, g0, ips, verts = pinned(diamond_graphml(), DIAMOND_POI)
    g, src, sip, dip, sv, dv, w = diamond_flows(ips, verts)
    exp = ExpectedLoad(g, sv, dv, w, verts)
    edges, vertices = watch_recipe(exp, sv, dv)
    g2, chains = all_chains(diamond_graphml(), tuple(int(v) for v in verts))
    top.table()
    mon = top.link_monitor(edges, vertices, **KW)
    check_index(mon, g, chains, edges, vertices, min_hits=500)
    st = mon.stats()
    assert st["chunks"] == 1 and st["sources"] == DIAMOND_POI
    assert st["batch_sources"] >= 2 and st["batch_fallback"] >= 2
    assert st["batch_sources"] + st["batch_fallback"] == DIAMOND_POI
    assert st["replay_ms"] > 0 and st["batch_ms"] > 0


# ------------------------------------------------------------------------------------------
# 2. feeds accumulate
# ------------------------------------------------------------------------------------------
def test_host_feeds_accumulate_and_reset():
    top, g, sip, dip, sv, dv, w, now0, exp, xc, edges, vertices = real_case()
    n = len(sip)  # the last request has an unattached source
    idx, now = windows(n)
    xt = ExpectedTimeline(g, exp, w[:-1], now[:-1], edges, vertices, **KW)
    c = xt.conditions()
    print(c)
    assert c["hits"] >= 200 and c["in_range"] >= 100 and c["before"] >= 10 and c["after"] >= 10, c
    assert c["rev_rows"] >= 1 and c["flows2"] >= 20, c
    xw = [ExpectedTimeline(g, cut(exp, i[i < n - 1]), w[i[i < n - 1]], now[i[i < n - 1]], edges,
                           vertices, **KW) for i in idx]
    assert all(x.hits >= 30 for x in xw)
    top.table()
    mon = top.link_monitor(edges, vertices, **KW)
    for j, i in enumerate(idx):
        assert mon.feed(sip[i], dip[i], now[i], w[i]) == xw[j].hits
        st = mon.stats()
        check_last(st, xw[j], fed=len(i) - (j == 2), unattached=int(j == 2))
        assert st["feed_kernel_ms"] > 0
    out = mon.read()
    check_timeline(out, xt)
    st = mon.stats()
    check_counters(st, xw, fed=n - 1, unattached=1)
    assert st["prepares"] == 1 and st["feeds"] == 3
    # the second, separate assertion: one link_timeline call on the concatenation
    bytes_equal(out, top.link_timeline(sip, dip, now, edges, vertices, w, **KW))
    mon.reset()
    assert zero_bins(mon.read()) and mon.stats()["hits"] == 0
    assert mon.feed(sip[idx[1]], dip[idx[1]], now[idx[1]], w[idx[1]]) == xw[1].hits
    check_timeline(mon.read(), xw[1])
    check_counters(mon.stats(), [xw[1]], fed=len(idx[1]))
    assert mon.stats()["prepares"] == 1


# ------------------------------------------------------------------------------------------
# 3. the device feed
# ------------------------------------------------------------------------------------------
def test_device_feeds_filter_skip_bad_columns_and_order_across_streams():
    import torch
    top, g, sip, dip, sv, dv, w, now0, exp, xc, edges, vertices = real_case()
    av = top.attached_vertices()
    A, n = len(av), len(sv)  # (the attached flows only)
    idx, now = windows(n, 2)
    sc, dc = columns(av, sv), columns(av, dv)
    pay = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    pay[:3] = [0xFFFFFFFF, 1, 0]
    keep = np.random.default_rng(9).integers(0, 2, n).astype(np.uint8)
    keep[:4] = [1, 0, 1, 1]
    k = np.nonzero(keep)[0]
    xk = ExpectedTimeline(g, cut(exp, k), pay[k], now[k], edges, vertices, **KW)
    c = xk.conditions()
    assert c["hits"] >= 100 and c["in_range"] >= 50 and c["before"] >= 5 and c["after"] >= 5, c
    top.table()
    mon = top.link_monitor(edges, vertices, **KW)
    # two columns of -1 and two of A among the packets: counted, nothing read through them
    ins = np.asarray([5, 5, 40, 90])
    bs = np.insert(sc, ins, [-1, 3, A, 2]).astype(np.int32)
    bd = np.insert(dc, ins, [0, -1, 1, A]).astype(np.int32)
    grow = lambda x, fill: np.insert(x, ins, fill).astype(x.dtype)
    mon.feed_device(cu(bs), cu(bd), cu(grow(now, BASE)), cu(grow(pay, 7)), cu(grow(keep, 1)))
    check_timeline(mon.read(), xk)
    st = mon.stats()
    check_counters(st, [xk], fed=len(k), skipped=n - len(k), bad=4)
    check_last(st, xk, fed=len(k), skipped=n - len(k), bad=4)
    assert st["feed_kernel_ms"] > 0
    # payload = None counts packets; two feeds on two streams in sequence, then one read
    mon.reset()
    x1 = ExpectedTimeline(g, exp, None, now, edges, vertices, **KW)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    parts = []
    for s, i in zip((s1, s2), idx):
        t = [cu(sc[i]), cu(dc[i]), cu(now[i])]
        parts.append(t)  # (alive until the read below has waited for the feeds)
        mon.feed_device(t[0], t[1], t[2], stream=s.cuda_stream)
    out = mon.read()
    check_timeline(out, x1)
    check_counters(mon.stats(), [x1], fed=n)
    bytes_equal(out, top.link_timeline(sip[:-1], dip[:-1], now, edges, vertices, **KW))


def test_device_feed_composes_with_the_packet_batch():
    import torch
    top, g, sip, dip, sv, dv, w, now0, exp, xc, edges, vertices = real_case()
    av = top.attached_vertices()
    n = len(sv)
    now = window_now(n, 10 * MS)
    sc, dc = columns(av, sv), columns(av, dv)
    rng = np.random.default_rng(12)
    pay = rng.integers(1, 1500, n).astype(np.uint32)
    state = rng.integers(1, 2**31, n).astype(np.uint32)
    a, lat, rel, hops = g.table(av)
    ot, od, os_ = oracle.route_packets(lat[sc, dc], rel[sc, dc], pay, state, now, 0, 0)
    k = np.nonzero(od)[0]
    assert 10 <= n - len(k) and len(k) >= n // 2  # input condition: drops, and deliveries
    xk = ExpectedTimeline(g, cut(exp, k), pay[k], now[k], edges, vertices, **KW)
    assert xk.hits >= 100
    top.table()
    mon = top.link_monitor(edges, vertices, **KW)
    mon.prepare()
    d = [cu(sc), cu(dc), cu(pay), cu(state), cu(now)]
    t_out = torch.empty(n, dtype=torch.int64, device="cuda")
    s_out = torch.empty(n, dtype=torch.int32, device="cuda")
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    top.route_batch_device(d[0], d[1], d[2], d[3], d[4], 0, 0, t_out, s_out, d_out,
                           stream=s.cuda_stream)
    mon.feed_device(d[0], d[1], d[4], payload=d[2], delivered=d_out, stream=s.cuda_stream)
    out = mon.read()
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), od)
    check_timeline(out, xk)
    bins, outside = flat(out)
    tot = bins.sum(1, dtype=np.uint64) + outside.sum(1, dtype=np.uint64)
    assert np.array_equal(tot, xk.bins.sum(1, dtype=np.uint64) + xk.outside.sum(1, dtype=np.uint64))
    check_counters(mon.stats(), [xk], fed=len(k), skipped=n - len(k))


# ------------------------------------------------------------------------------------------
# 4. shapes that break arithmetic
# ------------------------------------------------------------------------------------------
def test_no_bins_self_pairs_and_single_kind_watch_sets():
    top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices = real_case()
    top.table()
    # nbins = 0: everything goes to outside
    x0 = ExpectedTimeline(g, exp, w[:-1], now[:-1], edges, vertices, RT0, RBIN, 0)
    assert x0.before >= 10 and x0.after >= 100 and x0.in_range == 0
    mon = top.link_monitor(edges, vertices, t0=RT0, bin_ns=0, nbins=0)
    assert mon.feed(sip, dip, now, w) == x0.hits
    check_timeline(mon.read(), x0)
    # two hosts on one vertex are a self pair, as src == dst is: the loop, then the arrival
    hosts = np.asarray([host_ip(k + 1) for k in range(300)], np.uint32)
    hv = np.asarray([top.vertex_of_ip(int(ip)) for ip in hosts])
    v0 = int(sv[0])
    twins = hosts[hv == v0][:2]
    assert len(twins) == 2 and twins[0] != twins[1]
    loop = g.get_eid(v0, v0)
    assert loop >= 0
    t = 5 * BASE
    dl = int(np.ceil((0.0 + float(g.elat[loop])) * 1000000.0))
    ms = top.link_monitor([loop], [v0], t0=t, bin_ns=dl, nbins=2)
    assert ms.feed(twins[[0, 0, 1]], twins[[1, 0, 1]], [t, t, t], [1, 10, 100]) == 6
    one = ms.read()
    assert one["edge_fwd"].tolist() == [[111, 0]] and one["vertex"].tolist() == [[0, 111]]
    assert not one["edge_rev"].any() and not flat(one)[1].any()
    # vertices only (no hop's edge is looked up on the pair records' walks) and edges only
    for e, v in ((), vertices), (edges, ()):
        xt = ExpectedTimeline(g, exp, w[:-1], now[:-1], e, v, **KW)
        assert xt.hits >= 50
        m = top.link_monitor(e, v, **KW)
        assert m.feed(sip, dip, now, w) == xt.hits
        out = m.read()
        check_timeline(out, xt)
        bytes_equal(out, top.link_timeline(sip, dip, now, e, v, w, **KW))
    # no watches: no index, nothing launched
    me = top.link_monitor((), (), **KW)
    assert me.prepare() == 0 and me.feed(sip, dip, now, w) == 0
    z = np.zeros(4, np.int32)
    me.feed_device(cu(z), cu(z), cu(z.astype(np.uint64)))
    st = me.stats()
    assert st["index_records"] == 0 and st["index_pairs"] == 0 and st["prepares"] == 0
    assert st["fed"] == 0 and st["feed_kernel_ms"] == 0 and me.read()["hits"] == 0


def test_long_chain_and_the_accumulation_order():
    # the 201-hop chain, vertex watches at both ends (and the middle poi)
    top, g, ips, verts = pinned(long_chain_graphml(), 3)
    sip, dip, sv, dv = all_pairs(ips, verts, 3)
    w = np.asarray([3, 5, 7, 11, 13, 17, 19, 23, 29], np.uint64) << np.uint64(33)
    exp = ExpectedLoad(g, sv, dv, w, verts)
    assert exp.hops.reshape(3, 3).tolist() == [[1, 201, 102], [201, 1, 101], [102, 101, 1]]
    vid = {name: k for k, name in enumerate(g.vattrs["id"])}
    tail = g.get_eid(vid["pop-198"], vid["pop-199"])
    edges, vertices = [tail], [int(v) for v in verts]
    now = (BASE + 50 * MS * np.arange(9)).astype(np.uint64)
    xt = ExpectedTimeline(g, exp, w, now, edges, vertices, BASE, 100 * MS, 96)
    assert max(xt.hit_time) - BASE > 10_000 * MS and xt.after >= 2 and xt.in_range >= 8
    mon = top.link_monitor(edges, vertices, t0=BASE, bin_ns=100 * MS, nbins=96)
    g2, chains = all_chains(long_chain_graphml(), tuple(int(v) for v in verts))
    check_index(mon, g, chains, edges, vertices, min_hits=12, min_empty=0)
    assert mon.feed(sip, dip, now, w) == xt.hits
    check_timeline(mon.read(), xt)
    # 0.1 + 0.2 + 0.3 ms hops, 1-ns bins: the prefix is summed from the source
    top, g, ips, verts = pinned(order_path_graphml(), 2)
    edges, vertices = [0, 1, 2], [0, 3]
    t, nb = 5 * BASE, 700_000
    mon = top.link_monitor(edges, vertices, t0=t, bin_ns=1, nbins=nb)
    g2, chains = all_chains(order_path_graphml(), tuple(int(v) for v in verts))
    check_index(mon, g, chains, edges, vertices, min_hits=10, min_empty=0)
    off, row, ns = mon.export_index()
    assert ns[off[1]:off[2]].tolist() == [0, 100000, 300001, 600001]  # (0.0 + 0.1) + 0.2, + 0.3
    assert ns[off[2]:off[3]].tolist() == [0, 300000, 500000, 600000]  # (0.0 + 0.3) + 0.2, + 0.1
    exp = ExpectedLoad(g, verts[[0, 1]], verts[[1, 0]], None, verts)
    xt = ExpectedTimeline(g, exp, None, [t, t], edges, vertices, t, 1, nb)
    assert mon.feed(ips[[0, 1]], ips[[1, 0]], [t, t]) == 8 == xt.hits
    out = mon.read()
    check_timeline(out, xt)
    assert np.nonzero(out["vertex"][1])[0].tolist() == [600001]
    assert np.nonzero(out["vertex"][0])[0].tolist() == [600000]


# ------------------------------------------------------------------------------------------
# 5. staleness
# ------------------------------------------------------------------------------------------
def test_a_new_column_rebuilds_the_index_and_keeps_the_bins():
    data = tie_grid_graphml(False)
    top = sa.Topology.from_buffer(data)
    g = oracle.OGraph.from_graphml(data)
    otop, ips, verts = attach_hosts(top, g, 40, type_hints=["t%d" % (k + 10) for k in range(40)])
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    assert len(set(verts.tolist())) == 40
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    n = len(sv)
    e1 = ExpectedLoad(g, sv, dv, None, verts)
    edges, vertices = watch_recipe(e1, sv, dv)
    now1, now2 = window_now(n, 10 * MS), window_now(n + 2, 10 * MS) + np.uint64(4 * MS)
    kw = dict(t0=BASE + 5 * MS, bin_ns=MS, nbins=24)
    x1 = ExpectedTimeline(g, e1, None, now1, edges, vertices, **kw)
    mon = top.link_monitor(edges, vertices, **kw)
    assert mon.prepare() >= 1 and mon.feed(sip, dip, now1) == x1.hits
    # a host on poi-3: a vertex below every column, so every column moves up by one
    new_ip = host_ip(4000)
    nv, _ = top.attach_ip(new_ip, 12345, typeHint="t3")
    assert 0 <= nv < verts.min()
    verts2 = np.concatenate([[nv], verts]).astype(np.int32)
    sv2, dv2 = np.concatenate([sv, [nv, sv[0]]]), np.concatenate([dv, [dv[1], nv]])
    sip2 = np.concatenate([sip, [new_ip, sip[0]]]).astype(np.uint32)
    dip2 = np.concatenate([dip, [dip[1], new_ip]]).astype(np.uint32)
    e2 = ExpectedLoad(g, sv2, dv2, None, verts2)
    x2 = ExpectedTimeline(g, e2, None, now2, edges, vertices, **kw)
    assert x1.hits >= 100 and x2.hits >= 100
    assert mon.feed(sip2, dip2, now2) == x2.hits  # by IP: prepares again by itself
    assert mon.stats()["prepares"] == 2
    av2 = top.attached_vertices()
    assert av2.tolist() == sorted(verts2.tolist())
    mon.feed_device(cu(columns(av2, sv2)), cu(columns(av2, dv2)), cu(now2))  # by fresh columns
    bins, outside = flat(mon.read())
    with np.errstate(over="ignore"):
        assert np.array_equal(bins, x1.bins + x2.bins + x2.bins)
        assert np.array_equal(outside, x1.outside + x2.outside + x2.outside)
    st = mon.stats()
    assert st["prepares"] == 2 and st["index_pairs"] == 41 * 41
    check_counters(st, [x1, x2, x2], fed=n + 2 * (n + 2))


# ------------------------------------------------------------------------------------------
# 6. the cap
# ------------------------------------------------------------------------------------------
def test_an_index_over_the_cap_is_refused_and_leaves_the_bins_alone():
    top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices = real_case()
    lib, _ = _lib.load()
    av = top.attached_vertices()
    top.table()
    mon = top.link_monitor(edges, vertices, **KW)
    top.set_option("monitor_index_mb", 1e-6)
    h, m, n = top._h, mon.id, len(sv)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    sc, dc = cu(columns(av, sv)), cu(columns(av, dv))
    assert lib.shdtopo_monitor_prepare(h, m) == -5
    assert lib.shdtopo_monitor_feed(h, m, p(sip), p(dip), None, None, None, len(sip)) == -5
    assert lib.shdtopo_monitor_feed_vertices(h, m, p(sv), p(dv), None, None, None, n) == -5
    assert lib.shdtopo_monitor_feed_device(h, m, sc.data_ptr(), dc.data_ptr(), None, None, None,
                                           n, None) == -5
    st = mon.stats()
    assert zero_bins(mon.read()) and st["index_pairs"] == 0 and st["prepares"] == 0
    # between the offsets alone and the whole index: refused by the count pass
    g2, chains = all_chains(real_graphml(), tuple(int(v) for v in av))
    xi = ExpectedTimeline(g, chains, None, None, edges, vertices, 0, 1, 0)
    off_bytes = 8 * (len(av) ** 2 + 1)
    top.set_option("monitor_index_mb", (off_bytes + 16 * xi.hits - 16) / 1048576.0)
    assert lib.shdtopo_monitor_prepare(h, m) == -5 and zero_bins(mon.read())
    top.set_option("monitor_index_mb", (off_bytes + 16 * xi.hits) / 1048576.0)
    assert mon.prepare() == xi.hits
    xt = ExpectedTimeline(g, exp, w[:-1], now[:-1], edges, vertices, **KW)
    assert mon.feed(sip, dip, now, w) == xt.hits
    check_timeline(mon.read(), xt)


# ------------------------------------------------------------------------------------------
# 7. nothing else moves
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie_free", [False, True])
def test_monitor_leaves_stats_table_lazy_rows_and_the_family_statistics_alone(tie_free):
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
    now = window_now(len(sip), 10 * MS)
    kw = dict(t0=BASE + 5 * MS, bin_ns=MS, nbins=24)
    xt = ExpectedTimeline(g, exp, None, now, edges, vertices, **kw)
    top.trace_routes(sip, dip)
    top.link_load(sip, dip)
    top.link_crossings(sip, dip, edges, vertices)
    top.link_timeline(sip, dip, now, edges, vertices, **kw)
    family = lambda: (top.stats(), top.trace_stats(), top.link_load_stats(),
                      top.link_crossings_stats(), top.link_timeline_stats())
    f0 = family()
    lz0, lm0 = top.lazy_rows(), top.lazyMinimumLatency()
    table_hash = lambda: zlib.crc32(b"".join(x.tobytes() for x in top.table()))
    h0 = table_hash()
    assert family() == f0
    mon = top.link_monitor(edges, vertices, **kw)
    assert mon.prepare() >= xt.hits
    assert mon.feed(sip, dip, now) == xt.hits
    mon.feed_device(cu(columns(top.attached_vertices(), sv)),
                    cu(columns(top.attached_vertices(), dv)), cu(now))
    out = mon.read()
    mon.stats()
    mon.export_index()
    assert family() == f0
    assert all(np.array_equal(x, y) for x, y in zip(top.lazy_rows(), lz0))
    assert top.lazyMinimumLatency() == lm0
    assert table_hash() == h0 and family() == f0  # no rebuild
    bins, outside = flat(out)
    assert np.array_equal(bins, 2 * xt.bins) and np.array_equal(outside, 2 * xt.outside)
    mon.free()
    assert family() == f0


def test_multi_device_topology_monitors_on_its_first_device():
    top, g, ips, verts = pinned(tie_grid_graphml(False), 70, [("devices", 2)])
    sip, dip, sv, dv = all_pairs(ips, verts, 6)
    xt, edges, vertices = tie_grid_expected(False, tuple(int(v) for v in verts))
    top.table()
    st0 = top.stats()
    assert st0["devices"] == 2
    mon = top.link_monitor(edges, vertices, t0=BASE + 5 * MS, bin_ns=MS, nbins=24)
    assert mon.feed(sip, dip, window_now(420, 10 * MS), tie_grid_weights()) == xt.hits
    check_timeline(mon.read(), xt)
    assert top.stats() == st0
