"""The link timeline on complete topologies and the call's argument checks (no GPU):
shdtopo_link_timeline answers complete topologies on the host from the parsed graph, as the trace,
the load and the crossings do -- one hop over the igraph_get_eid edge of the pair, entered at the
emission time, the self loop for a self pair -- and initialises no device.  Expected bins are
derived (timeline_helpers) from one-hop chains over the oracle's get_eid; nothing expected comes
from the product.
"""
import ctypes
import types

import numpy as np
import pytest

from crossing_helpers import watch_recipe
from helpers import attach_hosts, bundled_pair
from shadow_amd import _lib
from timeline_helpers import ExpectedTimeline, check_stats, check_timeline, ns

BASE = 1_000_000_000
MS = 1_000_000


def _pairs(ips, verts, n_pairs=400, seed=4):
    """The pair recipe of test_link_crossings_cpu.py, restated: random pairs, 20 self pairs, two
    hosts on one vertex, weights up to 2^40."""
    rng = np.random.default_rng(seed)
    k = len(ips)
    s = np.concatenate([rng.integers(0, k, n_pairs), np.arange(min(k, 20))])
    d = np.concatenate([rng.integers(0, k, n_pairs), np.arange(min(k, 20))])
    by_vertex = {}
    for i, v in enumerate(verts):
        by_vertex.setdefault(v, []).append(i)
    shared = [(h[0], h[1]) for h in by_vertex.values() if len(h) > 1][:20]
    if shared:
        s = np.concatenate([s, [a for a, _ in shared]])
        d = np.concatenate([d, [b for _, b in shared]])
    w = rng.integers(1, 2**40, len(s)).astype(np.uint64)
    return s, d, w


def direct_chains(g, sv, dv, w):
    """What ExpectedTimeline and watch_recipe read of an ExpectedLoad, for one-hop routes over the
    direct edge."""
    e = np.asarray([g.get_eid(int(a), int(b)) for a, b in zip(sv, dv)])
    assert np.all(e >= 0)
    x = types.SimpleNamespace(verts=[[int(a), int(b)] for a, b in zip(sv, dv)],
                              edges=[[int(k)] for k in e])
    fwd = g.eu[e] == sv
    x.edge_fwd, x.edge_rev = np.zeros(g.E, np.uint64), np.zeros(g.E, np.uint64)
    x.vertex = np.zeros(g.V, np.uint64)
    np.add.at(x.edge_fwd, e[fwd], w[fwd])
    np.add.at(x.edge_rev, e[~fwd], w[~fwd])
    np.add.at(x.vertex, dv, w)
    return x, e


@pytest.mark.parametrize("name", ["topology.simple", "topology", "topology.plab"])
def test_complete_topology_timeline_is_one_hop_over_the_direct_edge(name):
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
    # bins of a tenth of the largest direct latency, from the middle of the emission window
    lat = np.asarray([ns(float(g.elat[k])) for k in e])
    bin_ns, nbins, t0 = max(1, int(lat.max()) // 10), 8, BASE + 5 * MS
    xt = ExpectedTimeline(g, chains, w, now, edges, vertices, t0, bin_ns, nbins)
    # conditions on the input
    selfp = sv == dv
    assert selfp.sum() >= 20
    loop = int(e[np.nonzero(selfp)[0][0]])
    assert loop in edges and g.eu[loop] == g.ev[loop]
    assert xt.hits >= 20 and xt.in_range >= 5 and xt.before >= 5 and xt.flows_with_several() >= 1
    out = top.link_timeline(sip, dip, now, edges, vertices, w, t0=t0, bin_ns=bin_ns, nbins=nbins)
    check_timeline(out, xt)
    ts = top.link_timeline_stats()
    check_stats(ts, xt, requests=n, sources=0)
    assert ts["chunks"] == 0 and ts["replay_ms"] == 0 and ts["kernel_ms"] == 0
    assert ts["batch_ms"] == 0 and ts["staged_hops"] == 0
    if g.directed:
        assert not out["edge_rev"].any() and not out["outside"]["edge_rev"].any()
    # a self pair alone: its loop entered at `now`, the arrival one loop latency later
    i = int(np.nonzero(selfp)[0][0])
    t = int(now[i])
    dl = ns(0.0 + float(g.elat[loop]))
    one = top.link_timeline(sip[[i]], dip[[i]], now[[i]], [loop], [int(sv[i])], t0=t, bin_ns=dl,
                            nbins=2)
    assert one["hits"] == 2 and one["edge_fwd"].tolist() == [[1, 0]]
    assert one["vertex"].tolist() == [[0, 1]] and not one["edge_rev"].any()
    # weight = NULL counts 1 per flow, now = NULL is time since emission; an unattached end is
    # counted and skipped
    sip3 = np.concatenate([[0x01020304], sip[:50]]).astype(np.uint32)
    dip3 = np.concatenate([[dip[0]], dip[:50]]).astype(np.uint32)
    c3, _ = direct_chains(g, sv[:50], dv[:50], np.ones(50, np.uint64))
    x3 = ExpectedTimeline(g, c3, None, None, edges, vertices, 0, bin_ns, 16)
    out3 = top.link_timeline(sip3, dip3, None, edges, vertices, t0=0, bin_ns=bin_ns, nbins=16)
    check_timeline(out3, x3)
    check_stats(top.link_timeline_stats(), x3, requests=51, sources=0, unattached=1)
    assert top.stats()["dev_inits"] == 0  # no device was initialised


def test_bad_arguments_return_minus_one():
    lib, _ = _lib.load()
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 4)
    a = np.asarray(ips[:2], np.uint32)
    w = np.ones(2, np.uint64)
    t = np.zeros(2, np.uint64)
    we, wv = np.asarray([0, 1], np.int32), np.asarray([0], np.int32)
    bins = np.zeros((5, 4), np.uint64)
    outside = np.zeros((5, 2), np.uint64)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)

    def call(top_h=top._h, s=a, d=a, wgt=w, now=t, n=2, e=we, ne=2, v=wv, nv=1, t0=0, bin_ns=MS,
             nbins=4, b=bins, o=outside):
        return lib.shdtopo_link_timeline(top_h, p(s), p(d), p(wgt), p(now), n, p(e), ne, p(v), nv,
                                         t0, bin_ns, nbins, p(b), p(o))
    assert call() >= 0
    assert call(top_h=None) == -1
    assert call(n=-1) == -1 and call(ne=-1) == -1 and call(nv=-1) == -1 and call(nbins=-1) == -1
    assert call(bin_ns=0) == -1
    assert call(s=None) == -1 and call(d=None) == -1
    assert call(e=None) == -1 and call(v=None) == -1
    assert call(b=None) == -1
    for bad in (-1, g.E):
        assert call(e=np.asarray([0, bad], np.int32)) == -1
    for bad in (-1, g.V):
        assert call(v=np.asarray([bad], np.int32)) == -1
    assert call(e=np.asarray([1, 1], np.int32)) == -1
    assert call(v=np.asarray([0, 0], np.int32), nv=2) == -1
    # what is optional: weight, now, outside; bins without bins; the arrays of empty lists
    assert call(wgt=None, now=None, o=None) >= 0
    assert call(nbins=0, b=None) >= 0 and call(nbins=0, b=None, bin_ns=0) >= 0
    assert call(e=None, ne=0) >= 0 and call(v=None, nv=0) >= 0
    # the empty watch set: 0 hits, nothing is walked, no row to write
    assert call(e=None, ne=0, v=None, nv=0, b=None, o=None) == 0
    s = _lib.ShdTimelineStats()
    assert lib.shdtopo_link_timeline_stats(top._h, ctypes.byref(s)) == 0
    assert (s.requests, s.routed, s.hits, s.flows_hit) == (2, 0, 0, 0)
    assert call(s=None, d=None, wgt=None, now=None, n=0) == 0
    assert lib.shdtopo_link_timeline_stats(None, None) == -1
    assert lib.shdtopo_link_timeline_stats(top._h, None) == -1
    # the same id in both lists is no duplicate: edge 0 and vertex 0 are different watches
    assert call(e=np.asarray([0, 1], np.int32), v=np.asarray([0], np.int32)) >= 0
    # the outputs are overwritten, not accumulated into
    bins[:] = 9
    outside[:] = 9
    r = call()
    assert r >= 0 and int(bins.sum() + outside.sum()) == r  # (unit weights)
