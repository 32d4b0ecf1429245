"""Link load on complete topologies (no GPU): shdtopo_link_load answers them on the host from the
parsed graph, as the trace does -- one hop over the igraph_get_eid edge of the pair, the self loop
for a self pair -- and initialises no device.  Expected loads are direct-edge sums over
shdtopo_export_graph's edge ends and the oracle's get_eid.
"""
import ctypes

import numpy as np
import pytest

from helpers import attach_hosts, bundled_pair
from shadow_amd import _lib


def _pairs(ips, verts, n_pairs=400, seed=4):
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


@pytest.mark.parametrize("name", ["topology.simple", "topology", "topology.plab"])
def test_complete_topology_loads_are_direct_edge_sums(name):
    top, g = bundled_pair(name)
    assert top.is_complete and g.is_complete()
    otop, ips, verts = attach_hosts(top, g, 120)
    s, d, w = _pairs(ips, verts)
    sip, dip = np.asarray(ips, np.uint32)[s], np.asarray(ips, np.uint32)[d]
    sv, dv = np.asarray(verts, np.int32)[s], np.asarray(verts, np.int32)[d]
    V, eu, ev, _, _, _ = top.export_graph()
    E = len(eu)
    e = np.asarray([g.get_eid(a, b) for a, b in zip(sv, dv)])
    assert np.all(e >= 0)
    fwd = eu[e] == sv
    assert np.all(ev[e][~fwd] == sv[~fwd])
    efwd, erev, vert = np.zeros(E, np.uint64), np.zeros(E, np.uint64), np.zeros(V, np.uint64)
    np.add.at(efwd, e[fwd], w[fwd])
    np.add.at(erev, e[~fwd], w[~fwd])
    np.add.at(vert, dv, w)
    out = top.link_load(sip, dip, w)
    assert out["routed"] == len(s)
    assert np.array_equal(out["edge_fwd"], efwd) and np.array_equal(out["edge_rev"], erev)
    assert np.array_equal(out["vertex"], vert)
    if top.is_directed:
        assert not erev.any()
    # self pairs (one host, or two hosts on one vertex) take the vertex's self loop, forward half
    selfp = sv == dv
    assert selfp.sum() >= 20
    assert np.array_equal(eu[e[selfp]], sv[selfp]) and np.array_equal(ev[e[selfp]], sv[selfp])
    assert np.all(out["edge_fwd"][e[selfp]] > 0)
    ls = top.link_load_stats()
    assert ls["requests"] == len(s) and ls["routed"] == len(s)
    assert ls["unattached"] == 0 and ls["broken"] == 0
    assert ls["sources"] == 0 and ls["chunks"] == 0 and ls["tree_vertices"] == 0
    assert ls["hop_weight"] == int(w.sum())  # one hop each
    assert ls["replay_ms"] == 0 and ls["load_kernel_ms"] == 0
    # weight = NULL counts 1 per flow; an unattached end is counted and skipped
    sip2 = np.concatenate([sip[:50], [0x01020304]]).astype(np.uint32)
    dip2 = np.concatenate([dip[:50], [dip[0]]]).astype(np.uint32)
    out = top.link_load(sip2, dip2)
    assert out["routed"] == 50 and int(out["vertex"].sum()) == 50
    assert int(out["edge_fwd"].sum() + out["edge_rev"].sum()) == 50
    assert top.link_load_stats()["unattached"] == 1
    assert top.stats()["dev_inits"] == 0  # no device was initialised


def test_link_load_bad_arguments_and_option():
    lib, _ = _lib.load()
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 4)
    a = np.asarray(ips[:2], np.uint32)
    w = np.ones(2, np.uint64)
    eb = np.zeros(2 * g.E, np.uint64)
    vb = np.zeros(g.V, np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert lib.shdtopo_link_load(None, p(a), p(a), p(w), 2, p(eb), p(vb)) == -1
    assert lib.shdtopo_link_load(top._h, p(a), p(a), p(w), -1, p(eb), p(vb)) == -1
    assert lib.shdtopo_link_load(top._h, None, p(a), p(w), 2, p(eb), p(vb)) == -1
    assert lib.shdtopo_link_load(top._h, p(a), None, p(w), 2, p(eb), p(vb)) == -1
    assert lib.shdtopo_link_load(top._h, p(a), p(a), None, 2, p(eb), p(vb)) == 2
    assert lib.shdtopo_link_load(top._h, p(a), p(a), p(w), 2, None, None) == 2
    assert lib.shdtopo_link_load(top._h, None, None, None, 0, None, None) == 0
    assert lib.shdtopo_link_load_stats(None, None) == -1
    assert lib.shdtopo_link_load_stats(top._h, None) == -1
    top.set_option("load_walk", 1)
    top.set_option("load_walk", 0)
    for bad in (2, -1, 0.5):
        with pytest.raises(KeyError):
            top.set_option("load_walk", bad)
