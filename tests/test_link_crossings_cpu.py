"""Link crossings on complete topologies and the call's argument checks (no GPU):
shdtopo_link_crossings answers complete topologies on the host from the parsed graph, as the trace
and the load do -- one hop (hop 0) over the igraph_get_eid edge of the pair, the self loop for a
self pair -- and initialises no device.  Expected records are derived (crossing_helpers) from
one-hop chains over the oracle's get_eid; nothing expected comes from the product.
"""
import ctypes
import types

import numpy as np
import pytest

import shadow_amd as sa
from crossing_helpers import RECORD, ExpectedCrossings, check_crossings, check_stats, watch_recipe
from helpers import attach_hosts, bundled_pair
from shadow_amd import _lib


def _pairs(ips, verts, n_pairs=400, seed=4):
    """The pair recipe of test_link_load_cpu.py: random pairs, 20 self pairs, two hosts on one
    vertex, weights up to 2^40."""
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
    """What ExpectedCrossings and watch_recipe read of an ExpectedLoad, for one-hop routes over
    the direct edge."""
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


def complete_case(name):
    top, g = bundled_pair(name)
    assert top.is_complete and g.is_complete()
    otop, ips, verts = attach_hosts(top, g, 120)
    s, d, w = _pairs(ips, verts)
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    sv, dv = verts[s], verts[d]
    chains, e = direct_chains(g, sv, dv, w)
    edges, vertices = watch_recipe(chains, sv, dv)
    return top, g, ips[s], ips[d], sv, dv, w, chains, e, edges, vertices


@pytest.mark.parametrize("name", ["topology.simple", "topology", "topology.plab"])
def test_complete_topology_crossings_are_one_hop_over_the_direct_edge(name):
    top, g, sip, dip, sv, dv, w, chains, e, edges, vertices = complete_case(name)
    xc = ExpectedCrossings(g, chains, w, edges, vertices)
    # conditions on the input
    assert xc.total >= 20 and xc.both >= 1
    # (topology.simple has two vertices and the recipe watches both)
    assert xc.flows_without_any() >= 1 or len(vertices) == g.V
    selfp = sv == dv
    assert selfp.sum() >= 20
    loop = int(e[np.nonzero(selfp)[0][0]])
    assert loop in edges and g.eu[loop] == g.ev[loop]
    out = top.link_crossings(sip, dip, edges, vertices, w)
    check_crossings(out, xc)
    check_stats(top.link_crossings_stats(), xc, sources=0)
    rec = out["records"]
    assert not rec["hop"].any()
    # reverse follows eu[e] != source, on edge records alone
    isedge = rec["watch"] < len(edges)
    we = np.asarray(edges)[rec["watch"][isedge]]
    assert np.array_equal(we, e[rec["flow"][isedge]])
    assert np.array_equal(rec["reverse"][isedge], (g.eu[we] != sv[rec["flow"][isedge]]).astype(np.int32))
    assert not rec["reverse"][~isedge].any()
    if g.directed:
        assert not rec["reverse"].any()
    # self pairs (one host, or two hosts on one vertex) cross the loop and arrive at the vertex
    k = edges.index(loop)
    on_loop = rec[rec["watch"] == k]
    assert np.array_equal(on_loop["flow"], np.nonzero(e == loop)[0]) and not on_loop["reverse"].any()
    out2 = top.link_crossings(sip, dip, [loop], [int(g.eu[loop])], w)
    f = np.nonzero(e == loop)[0]
    both = out2["records"][np.isin(out2["records"]["flow"], f)]
    assert both["watch"].tolist() == [0, 1] * len(f) and both["flow"].tolist() == np.repeat(f, 2).tolist()
    cs = top.link_crossings_stats()
    assert cs["chunks"] == 0 and cs["replay_ms"] == 0 and cs["kernel_ms"] == 0 and cs["batch_ms"] == 0
    # weight = NULL counts 1 per flow; an unattached end is counted and skipped
    sip3 = np.concatenate([[0x01020304], sip[:50]]).astype(np.uint32)
    dip3 = np.concatenate([[dip[0]], dip[:50]]).astype(np.uint32)
    c3, _ = direct_chains(g, sv[:50], dv[:50], np.ones(50, np.uint64))
    x3 = ExpectedCrossings(g, c3, None, edges, vertices, flows=np.arange(1, 51), n=51)
    out3 = top.link_crossings(sip3, dip3, edges, vertices)
    check_crossings(out3, x3)
    assert np.array_equal(out3["weight"], out3["count"])
    check_stats(top.link_crossings_stats(), x3, sources=0, unattached=1)
    assert top.stats()["dev_inits"] == 0  # no device was initialised


def test_cap_rule_on_the_host_path():
    top, g, sip, dip, sv, dv, w, chains, e, edges, vertices = complete_case("topology")
    lib, _ = _lib.load()
    xc = ExpectedCrossings(g, chains, w, edges, vertices)
    two = np.nonzero(xc.per_flow == 2)[0]
    assert len(two) >= 1 and xc.offsets[two[0]] > 0  # a cap in the middle of a flow
    cap = int(xc.offsets[two[0]]) + 1
    out = top.link_crossings(sip, dip, edges, vertices, w, cap=cap)
    want = xc.fitting(cap)
    assert len(want) == cap - 1
    assert out["records"].tobytes() == want.tobytes()
    assert out["total"] == xc.total and np.array_equal(out["offsets"], xc.offsets)
    assert np.array_equal(out["count"], xc.count) and np.array_equal(out["weight"], xc.weight)
    # nothing at or beyond cap -- nor the slot the cut flow would have started in -- is touched
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    buf = np.full(4 * (xc.total + 8), -7, np.int32)
    we, wv = np.asarray(edges, np.int32), np.asarray(vertices, np.int32)
    sip, dip = np.ascontiguousarray(sip), np.ascontiguousarray(dip)
    r = lib.shdtopo_link_crossings(top._h, p(sip), p(dip), p(w), len(sip), p(we), len(we), p(wv),
                                   len(wv), None, p(buf), cap, None, None)
    assert r == xc.total
    assert buf[:4 * (cap - 1)].tobytes() == want.tobytes() and np.all(buf[4 * (cap - 1):] == -7)
    # cap = 0 sizes: out may be NULL
    r = lib.shdtopo_link_crossings(top._h, p(sip), p(dip), p(w), len(sip), p(we), len(we), p(wv),
                                   len(wv), None, None, 0, None, None)
    assert r == xc.total


def test_bad_arguments_return_minus_one():
    lib, _ = _lib.load()
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 4)
    a = np.asarray(ips[:2], np.uint32)
    w = np.ones(2, np.uint64)
    we, wv = np.asarray([0, 1], np.int32), np.asarray([0], np.int32)
    off = np.zeros(3, np.int64)
    out = np.zeros(16, RECORD)
    cnt, wt = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)

    def call(top_h=top._h, s=a, d=a, wgt=w, n=2, e=we, ne=2, v=wv, nv=1, o=off, rec=out, cap=16,
             c=cnt, ww=wt):
        return lib.shdtopo_link_crossings(top_h, p(s), p(d), p(wgt), n, p(e), ne, p(v), nv, p(o),
                                          p(rec), cap, p(c), p(ww))
    assert call() >= 0
    assert call(top_h=None) == -1
    assert call(n=-1) == -1 and call(ne=-1) == -1 and call(nv=-1) == -1 and call(cap=-1) == -1
    assert call(s=None) == -1 and call(d=None) == -1
    assert call(e=None) == -1 and call(v=None) == -1
    assert call(rec=None) == -1
    for bad in (-1, g.E):
        assert call(e=np.asarray([0, bad], np.int32)) == -1
    for bad in (-1, g.V):
        assert call(v=np.asarray([bad], np.int32)) == -1
    assert call(e=np.asarray([1, 1], np.int32)) == -1
    assert call(v=np.asarray([0, 0], np.int32), nv=2) == -1
    # what is optional: weight, offsets, totals; out with cap = 0; the arrays of empty lists
    assert call(wgt=None, o=None, c=None, ww=None) >= 0
    assert call(rec=None, cap=0) >= 0
    assert call(e=None, ne=0) >= 0 and call(v=None, nv=0) >= 0
    off[:] = 5
    assert call(e=None, ne=0, v=None, nv=0) == 0 and not off.any()  # the empty watch set
    assert call(s=None, d=None, wgt=None, n=0) == 0
    assert lib.shdtopo_link_crossings_stats(None, None) == -1
    assert lib.shdtopo_link_crossings_stats(top._h, None) == -1
    # the same edge id in both lists is no duplicate: edge 0 and vertex 0 are different watches
    assert call(e=np.asarray([0, 1], np.int32), v=np.asarray([0], np.int32)) >= 0


def test_crossings_by_watch_inverts_the_records():
    top, g, sip, dip, sv, dv, w, chains, e, edges, vertices = complete_case("topology.plab")
    xc = ExpectedCrossings(g, chains, w, edges, vertices)
    out = top.link_crossings(sip, dip, edges, vertices, w)
    by = sa.crossings_by_watch(out)
    assert sorted(by) == list(range(len(edges) + len(vertices)))
    for k in by:
        want = xc.records["flow"][xc.records["watch"] == k]
        assert by[k].tolist() == want.tolist() and len(want) == xc.count[k]
    assert sum(len(v) for v in by.values()) == xc.total and xc.total > 0
    # an empty result inverts to empty lists
    none = top.link_crossings(sip[:0], dip[:0], edges, vertices)
    assert none["total"] == 0 and len(none["records"]) == 0
    assert all(len(v) == 0 for v in sa.crossings_by_watch(none).values())
