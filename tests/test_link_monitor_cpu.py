"""The link monitor on complete topologies and its argument checks (no GPU): the hit index of a
complete topology is built on the host from the parsed graph -- one hop over the igraph_get_eid
edge of the pair, entered at offset 0, the arrival ns(0.0 + latency) later, the self loop for a
self pair -- and the host feeds walk it on the host, so no device is initialised.  Expected values
are derived (monitor_helpers, timeline_helpers) from one-hop chains over the oracle's get_eid;
nothing expected comes from the product.
"""
import ctypes
import types

import numpy as np
import pytest

from crossing_helpers import watch_recipe
from helpers import attach_hosts, bundled_pair
from monitor_helpers import check_counters, check_index, check_last, pair_grid, zero_bins
from shadow_amd import _lib
from test_link_timeline_cpu import BASE, MS, _pairs, direct_chains
from timeline_helpers import ExpectedTimeline, bytes_equal, check_timeline, ns


def check_no_device_used(top):
    """No call initialised a device: dev_inits is 0 -- except where a device is visible, where
    creating a topology initialises it in the background, once, whatever is called later."""
    n = top.stats()["dev_inits"]
    if n:
        import torch
        assert n == 1 and torch.cuda.is_available()


@pytest.mark.parametrize("name", ["topology.simple", "topology", "topology.plab"])
def test_complete_topology_index_and_host_feeds(name):
    top, g = bundled_pair(name)
    assert top.is_complete and g.is_complete()
    otop, ips, verts = attach_hosts(top, g, 120)
    s, d, w = _pairs(ips, verts)
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    sip, dip, sv, dv = ips[s], ips[d], verts[s], verts[d]
    chains, e = direct_chains(g, sv, dv, w)
    edges, vertices = watch_recipe(chains, sv, dv)
    n = len(s)
    now = (BASE + np.random.default_rng(77).integers(0, 10 * MS, n)).astype(np.uint64)
    lat = np.asarray([ns(float(g.elat[k])) for k in e])
    bin_ns, nbins, t0 = max(1, int(lat.max()) // 10), 8, BASE + 5 * MS
    mon = top.link_monitor(edges, vertices, t0=t0, bin_ns=bin_ns, nbins=nbins)
    # the index: every ordered pair of attached vertices, one hop over the direct edge
    av = top.attached_vertices()
    asv, adv = pair_grid(av)
    allc, _ = direct_chains(g, asv, adv, np.ones(len(asv), np.uint64))
    # (topology.simple has two vertices, both watched with all three edges: 4 pairs, 2 hits each)
    few = name == "topology.simple"
    assert mon.prepare() == check_index(mon, g, allc, edges, vertices, min_hits=8 if few else 40,
                                        min_empty=0 if few else 1).hits
    # two windows by IP, one unattached request in the second; then the rest by vertex
    h = n // 2
    x1 = ExpectedTimeline(g, _cut(chains, 0, h), w[:h], now[:h], edges, vertices, t0, bin_ns, nbins)
    x2 = ExpectedTimeline(g, _cut(chains, h, n), w[h:], now[h:], edges, vertices, t0, bin_ns, nbins)
    xt = ExpectedTimeline(g, chains, w, now, edges, vertices, t0, bin_ns, nbins)
    assert xt.hits >= 20 and xt.in_range >= 5 and xt.before >= 5 and xt.flows_with_several() >= 1
    assert x1.hits >= 5 and x2.hits >= 5
    assert mon.feed(sip[:h], dip[:h], now[:h], w[:h]) == x1.hits
    check_timeline(mon.read(), x1)
    stranger = np.asarray([0x01020304], np.uint32)
    assert mon.feed(np.concatenate([stranger, sip[h:]]), np.concatenate([dip[:1], dip[h:]]),
                    np.concatenate([now[:1], now[h:]]), np.concatenate([w[:1], w[h:]])) == x2.hits
    out = mon.read()
    check_timeline(out, xt)
    st = mon.stats()
    check_counters(st, [x1, x2], fed=n, unattached=1)
    check_last(st, x2, fed=n - h, unattached=1)
    assert st["prepares"] == 1 and st["feed_kernel_ms"] == 0 and st["feeds"] == 2
    # the second, separate assertion: one link_timeline call on the concatenation
    bytes_equal(out, top.link_timeline(sip, dip, now, edges, vertices, w, t0=t0, bin_ns=bin_ns,
                                       nbins=nbins))
    if g.directed:
        assert not out["edge_rev"].any() and not out["outside"]["edge_rev"].any()
    # delivered filters; vertices instead of IPs; weight = None counts packets, now = None is 0
    mon.reset()
    assert zero_bins(mon.read()) and mon.stats()["hits"] == 0
    keep = np.random.default_rng(5).integers(0, 2, n).astype(np.uint8)
    keep[:4] = [1, 0, 1, 0]
    k = np.nonzero(keep)[0]
    xk = ExpectedTimeline(g, _pick(chains, k), None, None, edges, vertices, t0, bin_ns, nbins)
    assert mon.feed_vertices(sv, dv, delivered=keep) == xk.hits
    check_timeline(mon.read(), xk)
    check_counters(mon.stats(), [xk], fed=len(k), skipped=n - len(k))
    assert mon.stats()["prepares"] == 1
    mon.free()
    check_no_device_used(top)


def _cut(chains, a, b):
    return types.SimpleNamespace(verts=chains.verts[a:b], edges=chains.edges[a:b])


def _pick(chains, idx):
    return types.SimpleNamespace(verts=[chains.verts[i] for i in idx],
                                 edges=[chains.edges[i] for i in idx])


def test_empty_watch_set_builds_no_index():
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 8)
    ips = np.asarray(ips, np.uint32)
    mon = top.link_monitor((), (), t0=0, bin_ns=MS, nbins=4)
    assert mon.prepare() == 0
    assert mon.feed(ips, ips[::-1]) == 0 and mon.feed_vertices(verts, verts) == 0
    st = mon.stats()
    assert st["index_records"] == 0 and st["index_pairs"] == 0 and st["prepares"] == 0
    out = mon.read()
    assert out["hits"] == 0 and out["vertex"].shape == (0, 4)
    check_no_device_used(top)


def test_bad_arguments_and_stale_ids_return_minus_one():
    lib, _ = _lib.load()
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 4)
    other, g2 = bundled_pair("topology.simple")
    attach_hosts(other, g2, 4)
    a = np.asarray(ips[:2], np.uint32)
    v = np.asarray(verts[:2], np.int32)
    we, wv = np.asarray([0, 1], np.int32), np.asarray([0], np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)

    def new(top_h=top._h, e=we, ne=2, vs=wv, nv=1, t0=0, bin_ns=MS, nbins=4):
        return lib.shdtopo_monitor_new(top_h, p(e), ne, p(vs), nv, t0, bin_ns, nbins)
    ok = new()
    assert ok >= 0
    assert new(top_h=None) == -1
    assert new(ne=-1) == -1 and new(nv=-1) == -1 and new(nbins=-1) == -1
    assert new(bin_ns=0) == -1
    assert new(e=None) == -1 and new(vs=None) == -1
    for bad in (-1, g.E):
        assert new(e=np.asarray([0, bad], np.int32)) == -1
    for bad in (-1, g.V):
        assert new(vs=np.asarray([bad], np.int32)) == -1
    assert new(e=np.asarray([1, 1], np.int32)) == -1
    assert new(vs=np.asarray([0, 0], np.int32), nv=2) == -1
    # what is optional: bins without bins; the arrays of empty lists; the empty watch set
    for m in (new(nbins=0, bin_ns=0), new(e=None, ne=0), new(vs=None, nv=0),
              new(e=None, ne=0, vs=None, nv=0)):
        assert m >= 0 and m != ok
        assert lib.shdtopo_monitor_free(top._h, m) == 0

    st = _lib.ShdMonitorStats()
    bins, outside = np.zeros((5, 4), np.uint64), np.zeros((5, 2), np.uint64)

    def every_call(top_h, m):
        return [lib.shdtopo_monitor_prepare(top_h, m),
                lib.shdtopo_monitor_feed(top_h, m, p(a), p(a), None, None, None, 2),
                lib.shdtopo_monitor_feed_vertices(top_h, m, p(v), p(v), None, None, None, 2),
                lib.shdtopo_monitor_feed_device(top_h, m, None, None, None, None, None, 0, None),
                lib.shdtopo_monitor_read(top_h, m, p(bins), p(outside)),
                lib.shdtopo_monitor_reset(top_h, m),
                lib.shdtopo_monitor_stats(top_h, m, ctypes.byref(st)),
                lib.shdtopo_monitor_export_index(top_h, m, None, None, None, 0)]
    assert all(r >= 0 for r in every_call(top._h, ok))
    # a NULL IP / vertex array with n > 0, a negative n, a NULL stats pointer
    assert lib.shdtopo_monitor_feed(top._h, ok, None, p(a), None, None, None, 2) == -1
    assert lib.shdtopo_monitor_feed(top._h, ok, p(a), None, None, None, None, 2) == -1
    assert lib.shdtopo_monitor_feed(top._h, ok, p(a), p(a), None, None, None, -1) == -1
    assert lib.shdtopo_monitor_feed_vertices(top._h, ok, None, p(v), None, None, None, 2) == -1
    assert lib.shdtopo_monitor_feed_device(top._h, ok, None, None, None, None, None, 2, None) == -1
    assert lib.shdtopo_monitor_stats(top._h, ok, None) == -1
    assert lib.shdtopo_monitor_feed(top._h, ok, None, None, None, None, None, 0) == 0
    # an id of another topology, an id never handed out, a NULL topology, a freed id
    theirs = lib.shdtopo_monitor_new(other._h, p(we), 2, p(wv), 1, 0, MS, 4)
    assert theirs >= 0 and theirs != ok
    assert every_call(top._h, theirs) == [-1] * 8 and lib.shdtopo_monitor_free(top._h, theirs) == -1
    assert every_call(other._h, ok) == [-1] * 8
    assert every_call(top._h, 1 << 20) == [-1] * 8 and every_call(top._h, -1) == [-1] * 8
    assert every_call(None, ok) == [-1] * 8 and lib.shdtopo_monitor_free(None, ok) == -1
    assert all(r >= 0 for r in every_call(other._h, theirs))
    assert lib.shdtopo_monitor_free(top._h, ok) == 0
    assert every_call(top._h, ok) == [-1] * 8 and lib.shdtopo_monitor_free(top._h, ok) == -1
    # topology_free releases what is left (theirs); the option takes non-negative values only
    assert lib.shdtopo_set_option(top._h, b"monitor_index_mb", -1.0) == -1
    assert lib.shdtopo_set_option(top._h, b"monitor_index_mb", 64.0) == 0
    other.free()
    check_no_device_used(top)


def test_index_cap_on_the_host_builder():
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 8)
    ips = np.asarray(ips, np.uint32)
    lib, _ = _lib.load()
    mon = top.link_monitor([0], [int(verts[0])], t0=0, bin_ns=MS, nbins=4)
    top.set_option("monitor_index_mb", 1e-6)
    h = top._h
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    v = np.asarray(verts, np.int32)
    assert lib.shdtopo_monitor_prepare(h, mon.id) == -5
    assert lib.shdtopo_monitor_feed(h, mon.id, p(ips), p(ips), None, None, None, len(ips)) == -5
    assert lib.shdtopo_monitor_feed_vertices(h, mon.id, p(v), p(v), None, None, None, len(v)) == -5
    assert zero_bins(mon.read()) and mon.stats()["index_pairs"] == 0
    top.set_option("monitor_index_mb", 0)
    assert mon.feed(ips, ips) >= 1 and mon.stats()["prepares"] == 1
