"""Route tracing on complete topologies (no GPU): shdtopo_trace_routes answers them on the host
from the parsed graph, as the reference's _topology_lookupPath (shd-topology.c:835-873) -- one
hop over the igraph_get_eid edge of the pair, the self loop for a self pair -- with no device and
no table.  Expected routes come from the oracle: get_eid and complete_pairs.
"""
import ctypes

import numpy as np
import pytest

from helpers import attach_hosts, bundled_pair
from shadow_amd import _lib


def _pairs(ips, verts, n_pairs=400, seed=3):
    rng = np.random.default_rng(seed)
    k = len(ips)
    s = rng.integers(0, k, n_pairs)
    d = rng.integers(0, k, n_pairs)
    # every host with itself, and pairs of distinct hosts that share a vertex
    s = np.concatenate([s, np.arange(min(k, 20))])
    d = np.concatenate([d, np.arange(min(k, 20))])
    by_vertex = {}
    for i, v in enumerate(verts):
        by_vertex.setdefault(v, []).append(i)
    shared = [(h[0], h[1]) for h in by_vertex.values() if len(h) > 1][:20]
    if shared:
        s = np.concatenate([s, [a for a, _ in shared]])
        d = np.concatenate([d, [b for _, b in shared]])
    return s, d, len(shared)


@pytest.mark.parametrize("name", ["topology.simple", "topology", "topology.plab"])
def test_complete_topology_routes_are_the_direct_edge(name):
    top, g = bundled_pair(name)
    assert top.is_complete and g.is_complete()
    otop, ips, verts = attach_hosts(top, g, 120)
    s, d, nshared = _pairs(ips, verts)
    sip = np.asarray(ips, np.uint32)[s]
    dip = np.asarray(ips, np.uint32)[d]
    sv = np.asarray(verts, np.int32)[s]
    dv = np.asarray(verts, np.int32)[d]
    tr = top.trace_routes(sip, dip)
    n = len(s)
    assert tr["total"] == 2 * n and np.all(tr["status"] == 0) and np.all(tr["hops"] == 1)
    assert np.array_equal(tr["offset"], 2 * np.arange(n))
    olat, orel = g.complete_pairs(sv, dv)
    assert np.array_equal(tr["latency"].view(np.uint64), olat.view(np.uint64))
    assert np.array_equal(tr["reliability"].view(np.uint64), orel.view(np.uint64))
    V = tr["vertices"].reshape(n, 2)
    E = tr["edges"].reshape(n, 2)
    assert np.array_equal(V[:, 0], sv) and np.array_equal(V[:, 1], dv)
    assert np.array_equal(E[:, 0], [g.get_eid(a, b) for a, b in zip(sv, dv)])
    assert np.all(E[:, 1] == -1)
    # self pairs (one host, or two hosts on one vertex) go over the vertex's self loop
    selfp = sv == dv
    assert selfp.sum() >= 20 + nshared
    assert np.array_equal(g.eu[E[selfp, 0]], sv[selfp]) and np.array_equal(g.ev[E[selfp, 0]], sv[selfp])
    # the debug line of one route
    i = int(np.nonzero(~selfp)[0][0])
    ids = g.vattrs["id"]
    e = int(E[i, 0])
    want = "shortest path %s-->%s (%i-->%i) is %f ms with %f loss, path: %s" % (
        ids[sv[i]], ids[dv[i]], sv[i], dv[i], olat[i], 1 - orel[i],
        "%s--[%f,%f]-->%s" % (ids[sv[i]], g.elat[e], 1.0 - g.eloss[e], ids[dv[i]]))
    assert top.format_route(tr, i) == want
    # a host that is not attached: status 1, the other request unaffected
    tr2 = top.trace_routes(np.asarray([sip[0], 0x01020304], np.uint32),
                           np.asarray([dip[0], dip[0]], np.uint32))
    assert list(tr2["status"]) == [0, 1] and list(tr2["hops"]) == [1, -1]
    assert list(tr2["offset"]) == [0, -1] and tr2["total"] == 2
    assert list(tr2["vertices"]) == [sv[0], dv[0]]


def test_complete_topology_cap_and_request_order():
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 12)
    sip = np.asarray(ips, np.uint32)[[5, 0, 5, 3]]
    dip = np.asarray(ips, np.uint32)[[1, 2, 1, 3]]
    full = top.trace_routes(sip, dip)
    assert list(full["offset"]) == [0, 2, 4, 6] and full["total"] == 8
    assert np.array_equal(full["vertices"][0:2], full["vertices"][4:6])  # the duplicate request
    cut = top.trace_routes(sip, dip, cap=5)  # the third route does not fit
    assert cut["total"] == 8
    assert list(cut["status"]) == [0, 0, 3, 3] and list(cut["offset"]) == [0, 2, -1, -1]
    assert list(cut["hops"]) == [1, 1, 1, 1]
    assert np.array_equal(cut["latency"].view(np.uint64), full["latency"].view(np.uint64))
    assert np.array_equal(cut["vertices"][:4], full["vertices"][:4])
    assert cut["vertices"][4] == -2 and cut["edges"][4] == -2  # the buffers' fill: untouched


def test_trace_bad_arguments():
    lib, _ = _lib.load()
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 4)
    a = np.asarray(ips[:2], np.uint32)
    routes = (_lib.ShdRoute * 2)()
    buf = np.zeros(8, np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert lib.shdtopo_trace_routes(None, p(a), p(a), 2, routes, p(buf), p(buf), 8) < 0
    assert lib.shdtopo_trace_routes(top._h, p(a), p(a), -1, routes, p(buf), p(buf), 8) < 0
    assert lib.shdtopo_trace_routes(top._h, p(a), p(a), 2, routes, None, None, 8) < 0
    assert lib.shdtopo_trace_routes(top._h, p(a), p(a), 2, None, p(buf), p(buf), 8) < 0
    assert lib.shdtopo_trace_routes(top._h, p(a), p(a), 2, routes, p(buf), p(buf), -1) < 0
    assert lib.shdtopo_trace_routes(top._h, p(a), p(a), 2, routes, p(buf), p(buf), 8) == 4
    assert lib.shdtopo_format_route(None, routes, p(buf), p(buf), None, 0) < 0
    assert lib.shdtopo_trace_routes(top._h, None, None, 0, None, None, None, 0) == 0
