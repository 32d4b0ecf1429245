"""The traffic matrix on the device (topo_matrix.hip): the feed, re-layout, add, count and fill
kernels against numpy (matrix_helpers.ExpectedMatrix) over the oracle's attach.

The graph (helpers.graphml_doc) has 300 poi vertices, ids 0..299, each with an ip attribute of its
own so that an exact ipHint pins a host to it, and 300 routers behind them: 600 vertices, not
complete.  296 poi are attached at first: M = 296 is above 256 (a thread of the count and fill
kernels takes two column steps) and no multiple of 64; poi 3 and 100 are attached late, below old
vertex ids, so old columns shift and old cells move.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import attach_hosts, bundled_pair, graphml_doc, host_ip
from matrix_helpers import (FLOW, SUMS, ExpectedMatrix, bytes_equal, check_counters, check_read,
                            reads_equal)
from shadow_amd import _lib

pytestmark = pytest.mark.gpu

NPOI, NROUTER, NEXTRA = 300, 300, 900
LATE = (3, 100)       # attached late
NEVER = (10, 299)     # never attached
QUIET = range(200, 260)  # attached, never a source: rows with no reported cell


def poi_ip(k):
    return "10.%d.%d.1" % (k >> 8, k & 255)


@functools.lru_cache(maxsize=None)
def graph_doc():
    """(GraphML bytes, ids of edges whose removal keeps the graph connected)."""
    rng = np.random.default_rng(17)
    nodes = [("poi-%d" % k, ("client", "relay", "server")[k % 3], 0.0, poi_ip(k))
             for k in range(NPOI)]
    nodes += [("pop-%d" % i, "pop", 0.0) for i in range(NROUTER)]
    edges = [("pop-%d" % i, "pop-%d" % ((i + 1) % NROUTER), rng.uniform(1, 100), 0.0)
             for i in range(NROUTER)]
    seen = set()
    while len(seen) < NEXTRA:
        a, b = (int(x) for x in rng.integers(0, NROUTER, 2))
        key = (min(a, b), max(a, b))
        if a == b or abs(a - b) in (1, NROUTER - 1) or key in seen:
            continue
        seen.add(key)
        edges.append(("pop-%d" % a, "pop-%d" % b, rng.uniform(1, 100), 0.0))
    extra = list(range(NROUTER, NROUTER + NEXTRA))  # beside the ring: the ring keeps it connected
    for k in range(NPOI):
        edges.append(("poi-%d" % k, "pop-%d" % int(rng.integers(0, NROUTER)), 5.0, 0.0))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.0))
    return graphml_doc(nodes, edges), tuple(extra)


class World:
    """A product topology and the oracle's attach map: hosts pinned to poi vertices by an exact
    ipHint, every 7th vertex with a second host."""

    def __init__(self, options=()):
        data, self.extra = graph_doc()
        self.top = sa.Topology.from_buffer(data)
        self.g = oracle.OGraph.from_graphml(data)
        for k, v in options:
            self.top.set_option(k, v)
        assert not self.top.is_complete and self.g.V == NPOI + NROUTER <= 700
        self.ips, self.verts, self.n = [], [], 0
        for k in range(NPOI):
            if k not in LATE and k not in NEVER:
                self.attach(k)
                if k % 7 == 0:
                    self.attach(k)

    def attach(self, poi):
        self.n += 1
        ip, st = host_ip(self.n), (self.n * 2654435761) & 0x7FFFFFFF
        v1, _ = self.top.attach_ip(ip, st, ipHint=poi_ip(poi))
        v2, _, _ = oracle.attach_vertex(self.g.vattrs, st, ip_hint=poi_ip(poi))
        assert v1 == v2 == poi  # (poi k is vertex k)
        self.ips.append(ip)
        self.verts.append(v1)

    @property
    def av(self):
        return np.asarray(sorted(set(self.verts)), np.int32)

    def packets(self, n, seed):
        """n packets: sources among the hosts off the QUIET vertices, destinations anywhere; host
        0 sends to every host (a dense row); self pairs and duplicates; a third of the payloads
        0; a delivered mask.  Returns a dict of arrays (host indices si / di among them)."""
        rng = np.random.default_rng(seed)
        verts = np.asarray(self.verts, np.int32)
        loud = np.nonzero(~np.isin(verts, list(QUIET)))[0]
        k = len(verts)
        si = np.concatenate([loud[rng.integers(0, len(loud), n - k - 6)], np.zeros(k, np.int64),
                             [5, 5, 5, 9, 9, 11]])
        di = np.concatenate([rng.integers(0, k, n - k - 6), np.arange(k), [5, 5, 5, 9, 8, 11]])
        pay = np.where(rng.random(n) < 1 / 3, 0, rng.integers(1, 1449, n)).astype(np.uint32)
        dl = (rng.random(n) < 0.8).astype(np.uint8)
        dl[n - k - 6:n - 6] = 1  # the dense row is delivered
        ips = np.asarray(self.ips, np.uint32)
        return dict(si=si, di=di, sip=ips[si], dip=ips[di], sv=verts[si], dv=verts[di], pay=pay,
                    dl=dl, w=pay.astype(np.uint64))

    def cols(self, v):
        return np.searchsorted(self.av, v).astype(np.int32)


def dev(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def feed_dev(m, sc, dc, pay, dl, stream=0):
    import torch
    t = [dev(sc), dev(dc), dev(pay) if pay is not None else None,
         dev(dl) if dl is not None else None]
    torch.cuda.synchronize()
    m.feed_device(t[0], t[1], t[2], t[3], stream=stream)
    return t  # (kept alive by the caller until the matrix is read)


def other_stats(top):
    return (top.stats(), top.trace_stats(), top.link_load_stats(), top.link_crossings_stats(),
            top.link_timeline_stats(), top.table_diff_stats(), top.flow_impact_stats(),
            top.load_shift_stats())


def shape_conditions(rec, M):
    """The shapes at which the kernels can go wrong, asserted on the expected records."""
    assert M >= 257 and M % 64 != 0
    rows = np.bincount(rec["srcIndex"], minlength=M)
    assert (rows == 0).sum() >= 20 and (rows > 0).sum() >= 100  # rows with no reported cell
    # a row whose reported cells straddle a wave boundary (two adjacent columns around a multiple
    # of 64) and one with cells in both 256-column steps
    j, i = rec["dstIndex"], rec["srcIndex"]
    adj = (i[1:] == i[:-1]) & (j[1:] == j[:-1] + 1) & (j[1:] % 64 == 0)
    assert adj.any()
    assert len(set(i[j >= 256]) & set(i[j < 256])) >= 1
    assert ((rec["packets"] != 0) & (rec["weight"] == 0)).any()  # payload 0 only: still reported


def test_feed_forms_give_identical_reads():
    w = World()
    top, av = w.top, w.av
    A = len(av)
    p = w.packets(6000, 1)
    exp = ExpectedMatrix(w.g.V)
    # the same packets in the three forms; where the device form has a column outside [0, A) the
    # host forms have a stranger's IP / vertex -1
    badc = np.asarray([-1, A, 2**31 - 1, -2**31, A + 5], np.int32)
    nb = len(badc)
    stranger = np.full(nb, 0x01020304, np.uint32)
    one = np.ones(nb, np.uint8)
    sip = np.concatenate([stranger, p["sip"]])
    dip = np.concatenate([p["dip"][:nb], p["dip"]])
    sv = np.concatenate([np.full(nb, -1, np.int32), p["sv"]])
    dv = np.concatenate([p["dv"][:nb], p["dv"]])
    sc = np.concatenate([badc, w.cols(p["sv"])])
    dc = np.concatenate([w.cols(p["dv"][:nb]), w.cols(p["dv"])])
    sc[nb - 1], dc[nb - 1] = dc[nb - 1], sc[nb - 1]  # a bad destination column too
    pay = np.concatenate([p["pay"][:nb], p["pay"]])
    dl = np.concatenate([one, p["dl"]])
    want = exp.add(sv, dv, pay, dl)
    assert exp.unattached == nb and exp.skipped >= 500 and want >= 3000
    mh, mvx, md = top.traffic_matrix(), top.traffic_matrix(), top.traffic_matrix()
    assert mh.feed(sip, dip, pay.astype(np.uint64), dl) == want
    assert mvx.feed_vertices(sv, dv, pay.astype(np.uint64), dl) == want
    keep = feed_dev(md, sc, dc, pay, dl)
    rec, sums, tot = exp.view(av)
    shape_conditions(rec, A)
    rh, rv, rd = check_read(mh, exp, av), check_read(mvx, exp, av), check_read(md, exp, av)
    reads_equal(rh, rv)
    reads_equal(rh, rd)
    del keep
    check_counters(mh.stats(), exp, feeds=1)
    check_counters(mvx.stats(), exp, feeds=1)
    st = md.stats()
    assert (st["fed"], st["skipped_undelivered"], st["unattached"], st["bad_columns"]) == \
        (exp.fed, exp.skipped, 0, nb)
    assert (st["last_fed"], st["last_bad_columns"], st["last_unattached"]) == (exp.fed, nb, 0)
    assert mh.stats()["last_unattached"] == nb and mh.stats()["last_bad_columns"] == 0
    assert st["feed_kernel_ms"] > 0 and st["read_kernel_ms"] > 0 and st["relayouts"] == 0
    assert st["bytes"] == 16 * A * A
    assert st["bytes_model"] == 16 * A * A + 16 * A * int(len(set(rec["srcIndex"]))) + 32 * len(rec)
    for m in (mh, mvx, md):
        m.free()


def test_matrix_leaves_stats_the_table_and_the_family_statistics_alone():
    w = World()
    top, av = w.top, w.av
    ips = np.asarray(w.ips, np.uint32)
    assert top.latency_ip(int(ips[0]), int(ips[1])) > 0  # builds the table
    top.link_load(ips[:40], ips[40:80])
    before = other_stats(top)
    assert before[0]["paths_computed"] > 0
    lz0, lm0 = top.lazy_rows(), top.lazyMinimumLatency()
    p = w.packets(2000, 9)
    exp = ExpectedMatrix(w.g.V)
    m = top.traffic_matrix()
    assert m.feed(p["sip"], p["dip"], p["w"], p["dl"]) == exp.add(p["sv"], p["dv"], p["pay"],
                                                                 p["dl"])
    m.feed_vertices(p["sv"], p["dv"], p["w"], p["dl"])
    exp.add(p["sv"], p["dv"], p["pay"], p["dl"])
    keep = feed_dev(m, w.cols(p["sv"]), w.cols(p["dv"]), p["pay"], p["dl"])
    exp.add(p["sv"], p["dv"], p["pay"], p["dl"])
    check_read(m, exp, av)
    m.flows()
    m.reset()
    del keep
    # ShdStats (no build: paths_computed unchanged), the lazy rows and the family's statistics
    assert other_stats(top) == before
    assert all(np.array_equal(x, y) for x, y in zip(top.lazy_rows(), lz0))
    assert top.lazyMinimumLatency() == lm0
    m.free()
    assert other_stats(top) == before


def test_order_and_split_of_the_feeds_do_not_matter():
    import torch
    w = World()
    top, av = w.top, w.av
    p = w.packets(5000, 2)
    n = len(p["sv"])
    sc, dc = w.cols(p["sv"]), w.cols(p["dv"])
    exp = ExpectedMatrix(w.g.V)
    exp.add(p["sv"], p["dv"], p["pay"], p["dl"])
    m1, m3, mr, ms = (top.traffic_matrix() for _ in range(4))
    keep = [feed_dev(m1, sc, dc, p["pay"], p["dl"])]
    for a, b in ((0, 1700), (1700, 1701), (1701, n)):
        keep.append(feed_dev(m3, sc[a:b], dc[a:b], p["pay"][a:b], p["dl"][a:b]))
    keep.append(feed_dev(mr, sc[::-1], dc[::-1], p["pay"][::-1], p["dl"][::-1]))
    # two streams: the library's, then one of the caller's; the read sees all of it
    s2 = torch.cuda.Stream()
    h = n // 2
    keep.append(feed_dev(ms, sc[:h], dc[:h], p["pay"][:h], p["dl"][:h]))
    keep.append(feed_dev(ms, sc[h:], dc[h:], p["pay"][h:], p["dl"][h:], stream=s2.cuda_stream))
    r1 = check_read(m1, exp, av)
    for m in (m3, mr, ms):
        reads_equal(check_read(m, exp, av), r1)
    assert m3.stats()["feeds"] == 3 and m3.stats()["last_fed"] == int(p["dl"][1701:].sum())
    # weight = NULL counts packets; delivered = NULL takes all
    mp = top.traffic_matrix()
    keep.append(feed_dev(mp, sc, dc, None, None))
    e2 = ExpectedMatrix(w.g.V)
    assert e2.add(p["sv"], p["dv"]) == n
    rec, _, tot = check_read(mp, e2, av)
    assert np.array_equal(rec["weight"], rec["packets"]) and tot["packets"] == n
    # reset keeps mv and zeroes the rest
    mp.reset()
    e2.reset()
    check_read(mp, e2, av)
    assert mp.stats()["fed"] == 0
    del keep


def test_records_in_order_and_a_cap_inside_a_row():
    w = World()
    top, av = w.top, w.av
    p = w.packets(5000, 3)
    exp = ExpectedMatrix(w.g.V)
    exp.add(p["sv"], p["dv"], p["pay"], p["dl"])
    m = top.traffic_matrix()
    keep = feed_dev(m, w.cols(p["sv"]), w.cols(p["dv"]), p["pay"], p["dl"])
    rec, sums, tot = check_read(m, exp, av)
    key = rec["srcVertex"].astype(np.int64) * w.g.V + rec["dstVertex"]
    assert (np.diff(key) > 0).all()
    # caps: inside the dense first rows, inside a later row with several cells, one past a row's
    # end, the total, beyond the total; the sentinel behind the cap stays
    rows = np.bincount(rec["srcIndex"], minlength=len(av))
    off = np.concatenate([[0], np.cumsum(rows)])
    later = int(np.nonzero((rows >= 3) & (off[:-1] > 300))[0][0])
    total = len(rec)
    lib, h = m._lib, top._h
    assert lib.shdtopo_matrix_read(h, m.id, None, 0, None, None, None, None, None) == total
    for cap in (1, 70, int(off[later]) + 2, int(off[later + 1]), total, total + 9):
        buf = np.zeros(total + 16, FLOW)
        buf[:] = 0x5A
        sentinel = buf.copy()
        tt = _lib.ShdMatrixTotals()
        got = {k: np.zeros(len(av), np.uint64) for k in SUMS}
        assert lib.shdtopo_matrix_read(h, m.id, buf.ctypes.data, cap,
                                       *[got[k].ctypes.data for k in SUMS],
                                       ctypes.byref(tt)) == total
        k = min(cap, total)
        bytes_equal(buf[:k], rec[:k])
        bytes_equal(buf[k:], sentinel[k:])
        assert {f: getattr(tt, f) for f, _ in _lib.ShdMatrixTotals._fields_} == tot
        for f in SUMS:
            bytes_equal(got[f], sums[f])
    del keep


def test_growth_on_the_device_and_the_cap():
    w = World()
    top = w.top
    av0 = w.av
    p = w.packets(4000, 4)
    exp = ExpectedMatrix(w.g.V)
    exp.add(p["sv"], p["dv"], p["pay"], p["dl"])
    m = top.traffic_matrix()
    keep = [feed_dev(m, w.cols(p["sv"]), w.cols(p["dv"]), p["pay"], p["dl"])]
    check_read(m, exp, av0)
    for k in LATE:  # below old vertex ids: old columns shift, old cells move
        w.attach(k)
    av1 = w.av
    assert len(av1) == len(av0) + 2 and av1[3] == 3 and LATE[1] < av0[-1]
    assert not np.array_equal(w.cols(av0), np.arange(len(av0)))
    p2 = w.packets(3000, 5)
    assert np.isin(p2["sv"], LATE).any() and np.isin(p2["dv"], LATE).any()
    sc, dc = w.cols(p2["sv"]), w.cols(p2["dv"])
    # the growth does not fit: -5, nothing counted, contents and mv as they were
    top.set_option("matrix_mb", (16 * len(av1) ** 2 - 1) / 1048576.0)
    with pytest.raises(RuntimeError) as e:
        feed_dev(m, sc, dc, p2["pay"], p2["dl"])
    assert e.value.args[1] == -5
    with pytest.raises(RuntimeError) as e:
        m.feed_vertices(p2["sv"], p2["dv"], p2["w"], p2["dl"])
    assert e.value.args[1] == -5
    check_read(m, exp, av0)
    assert m.stats()["fed"] == exp.fed and m.stats()["relayouts"] == 0
    top.set_option("matrix_mb", 16 * len(av1) ** 2 / 1048576.0)  # exactly enough
    keep.append(feed_dev(m, sc, dc, p2["pay"], p2["dl"]))
    exp.add(p2["sv"], p2["dv"], p2["pay"], p2["dl"])
    rec, _, _ = check_read(m, exp, av1)
    assert m.stats()["relayouts"] == 1 and m.stats()["bytes"] == 16 * len(av1) ** 2
    assert np.isin(rec["srcVertex"], LATE).any()
    # a vertex that loses its column keeps its row; the columns behind it shift back
    gone = w.verts[20]
    for ip, v in zip(w.ips, w.verts):
        if v == gone:
            top.detach_ip(ip)
    left = np.asarray([v for v in av1 if v != gone], np.int32)
    assert np.array_equal(top.attached_vertices(), left)
    ok = (p2["sv"] != gone) & (p2["dv"] != gone)
    cols = lambda v: np.searchsorted(left, v).astype(np.int32)
    keep.append(feed_dev(m, cols(p2["sv"][ok]), cols(p2["dv"][ok]), p2["pay"][ok], p2["dl"][ok]))
    exp.add(p2["sv"][ok], p2["dv"][ok], p2["pay"][ok], p2["dl"][ok])
    rec, _, _ = check_read(m, exp, av1)
    assert gone in rec["srcVertex"] and m.stats()["relayouts"] == 1
    del keep


def test_complete_topology_device_feeds_merge_with_host_feeds():
    top, g = bundled_pair("topology")
    assert top.is_complete
    otop, ips, verts = attach_hosts(top, g, 120)
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    av = np.asarray(sorted(set(verts.tolist())), np.int32)
    rng = np.random.default_rng(8)
    n = 3000
    si, di = rng.integers(0, len(ips), n), rng.integers(0, len(ips), n)
    pay = np.where(rng.random(n) < 1 / 3, 0, 1448).astype(np.uint32)
    dl = (rng.random(n) < 0.8).astype(np.uint8)
    exp = ExpectedMatrix(g.V)
    m = top.traffic_matrix()
    h = n // 3
    assert m.feed(ips[si[:h]], ips[di[:h]], pay[:h].astype(np.uint64), dl[:h]) == \
        exp.add(verts[si[:h]], verts[di[:h]], pay[:h], dl[:h])
    assert m.stats()["feed_kernel_ms"] == 0
    cols = lambda v: np.searchsorted(av, v).astype(np.int32)
    keep = feed_dev(m, cols(verts[si[h:2 * h]]), cols(verts[di[h:2 * h]]), pay[h:2 * h],
                    dl[h:2 * h])
    exp.add(verts[si[h:2 * h]], verts[di[h:2 * h]], pay[h:2 * h], dl[h:2 * h])
    check_read(m, exp, av)  # host cells added into the device cells
    assert m.stats()["read_kernel_ms"] > 0
    check_read(m, exp, av)  # ... once
    assert m.feed_vertices(verts[si[2 * h:]], verts[di[2 * h:]], pay[2 * h:].astype(np.uint64),
                           dl[2 * h:]) == exp.add(verts[si[2 * h:]], verts[di[2 * h:]],
                                                  pay[2 * h:], dl[2 * h:])
    check_read(m, exp, av)
    st = m.stats()
    check_counters(st, exp, feeds=3)
    del keep


def test_closing_the_loop_with_link_load_and_flow_impact():
    w = World()
    top, av = w.top, w.av
    p = w.packets(4000, 6)
    m = top.traffic_matrix()
    keep = feed_dev(m, w.cols(p["sv"]), w.cols(p["dv"]), p["pay"], p["dl"])
    fs, fd, fw, fp = m.flows()
    del keep
    ok = p["dl"] != 0
    assert m.dropped == 0 and int(fp.sum()) == int(ok.sum()) and len(fs) < int(ok.sum())
    raw = top.link_load(p["sip"][ok], p["dip"][ok], p["w"][ok])
    agg = top.link_load(fs, fd, fw)
    assert raw["vertex"].any() and raw["edge_fwd"].any()
    for k in ("edge_fwd", "edge_rev", "vertex"):
        bytes_equal(agg[k], raw[k])
    # what a link failure does to the aggregated flows is what it does to the raw packets
    cut = top.without(edges=list(w.extra[:40]))
    ti_raw = top.flow_impact(cut, p["sip"][ok], p["dip"][ok], p["w"][ok], cap=0)["totals"]
    ti_agg = top.flow_impact(cut, fs, fd, fw, cap=0)["totals"]
    assert ti_raw["changedWeight"] > 0 and ti_raw["weight"] == int(p["w"][ok].sum())
    assert ti_agg["weight"] == ti_raw["weight"]
    assert ti_agg["changedWeight"] == ti_raw["changedWeight"]
    assert np.array_equal(ti_agg["kindWeight"], ti_raw["kindWeight"])
