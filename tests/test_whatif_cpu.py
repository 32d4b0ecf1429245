"""Link-failure what-if, host side (no device): shdtopo_derive_without / shdtopo_edge_origin.

The derived graph must be the parent's with the failed edges squeezed out (what deleting them in
igraph gives); expected arrays are the oracle's filtered edge arrays (whatif_helpers.filtered).
"""
import copy
import ctypes
import os
import tempfile

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from conftest import bundled_topology
from helpers import graphml_doc, host_ip, random_topology_graphml
from shadow_amd import _lib
from whatif_helpers import failing_set, filtered, oracle_attach, product_attach


def load(data):
    top = sa.Topology.from_buffer(data)
    assert top is not None
    return top, oracle.OGraph.from_graphml(data)


def assert_graph_equal(top, g2):
    V, eu, ev, el, lo, vl = top.export_graph()
    assert V == g2.V and top.num_edges == g2.E
    assert np.array_equal(eu, g2.eu) and np.array_equal(ev, g2.ev)
    assert np.array_equal(el.view(np.uint64), g2.elat.view(np.uint64))
    assert np.array_equal(lo.view(np.uint64), g2.eloss.view(np.uint64))
    assert np.array_equal(vl.view(np.uint64), g2.vloss.view(np.uint64))


def written_graph(top):
    fd, path = tempfile.mkstemp(suffix=".graphml.xml")
    os.close(fd)
    try:
        top.write_graphml(path)
        return oracle.OGraph.from_graphml(path)
    finally:
        os.unlink(path)


def parallel_pair(g):
    """(lower id, higher id) of two edges with the same ends."""
    key = np.minimum(g.eu, g.ev).astype(np.int64) * g.V + np.maximum(g.eu, g.ev)
    order = np.argsort(key, kind="stable")
    dup = np.flatnonzero(key[order][1:] == key[order][:-1])
    assert len(dup) > 0
    return int(order[dup[0]]), int(order[dup[0] + 1])


@pytest.mark.parametrize("kind", ["undirected", "directed", "parallel"])
def test_derived_graph_arrays(kind):
    doc = {"undirected": {}, "directed": {"directed": True}, "parallel": {"parallel": 50}}[kind]
    top, g = load(random_topology_graphml(**doc))
    if kind == "parallel":
        fail = np.array([parallel_pair(g)[0]], np.int32)  # the other edge of the pair stays
    else:
        fail = failing_set(g, 8)
    g2, keep = filtered(g, fail)
    assert g2.is_strongly_connected()
    child = top.without(edges=fail)
    assert child.num_vertices == top.num_vertices == g.V
    assert child.is_directed == top.is_directed
    assert_graph_equal(child, g2)
    assert np.array_equal(child.edge_origin(), np.flatnonzero(keep))
    assert np.array_equal(top.edge_origin(), np.arange(g.E))
    w = written_graph(child)
    assert w.V == g2.V and w.directed == g2.directed
    assert np.array_equal(w.eu, g2.eu) and np.array_equal(w.ev, g2.ev)
    assert np.array_equal(w.elat.view(np.uint64), g2.elat.view(np.uint64))
    assert np.array_equal(w.eloss.view(np.uint64), g2.eloss.view(np.uint64))
    assert w.vattrs["id"] == g.vattrs["id"]
    assert_graph_equal(top, g)  # the parent is as it was
    # duplicates in the failing list change nothing; the child outlives its parent
    again = top.without(edges=np.concatenate([fail, fail]))
    top.free()
    assert_graph_equal(again, g2)
    assert again.num_edges == g2.E


def a_poi(g, k=7):
    v = g.vattrs["id"].index("poi-%d" % k)
    return v


def test_vertex_failure_and_composed_origin():
    top, g = load(random_topology_graphml())
    poi = a_poi(g)
    g2, keep = filtered(g, fail_vertices=[poi])
    assert int((~keep).sum()) == 2  # its uplink and its loop
    child = top.without(vertices=[poi])
    assert_graph_equal(child, g2)
    assert np.array_equal(child.edge_origin(), np.flatnonzero(keep))
    # a derive of the derived topology: edge ids of the child in, root ids out
    fail2 = failing_set(g2, 5)
    g3, keep2 = filtered(g2, fail2)
    grand = child.without(edges=fail2)
    assert_graph_equal(grand, g3)
    root_ids = np.flatnonzero(keep)[np.flatnonzero(keep2)]
    assert np.array_equal(grand.edge_origin(), root_ids)
    assert not np.isin(grand.edge_origin(), np.flatnonzero(~keep)).any()
    # the failed vertex stays failed down the chain: failing it again is a no-op
    same = grand.without(vertices=[poi])
    assert_graph_equal(same, g3)


def test_attached_set_is_carried_over():
    top, g = load(random_topology_graphml())
    ips, verts, _ = product_attach(top, 60)
    _, overts, _ = oracle_attach(g, 60)
    assert verts == overts
    assert len(set(verts)) < len(verts)  # at least two hosts share a vertex
    child = top.without(edges=failing_set(g, 8))
    assert np.array_equal(child.attached_vertices(), top.attached_vertices())
    assert np.array_equal(child.attached_vertices(), np.unique(verts))
    for ip, v in zip(ips, verts):
        assert child.vertex_of_ip(ip) == top.vertex_of_ip(ip) == v
        assert child.column_of_ip(ip) == top.column_of_ip(ip)
    assert child.vertex_of_ip(host_ip(1000)) == -1


def test_attach_after_deriving_skips_the_failed_vertex():
    hints = ("client", "relay", "server")
    data = random_topology_graphml()
    top, g = load(data)
    poi = a_poi(g)
    child = top.without(vertices=[poi])
    vattrs = copy.deepcopy(g.vattrs)
    vattrs["id"][poi] = vattrs["id"][poi].replace("poi", "gone")
    _, verts, states = product_attach(child, 200, hints, seed=5)
    st = 5
    for k in range(200):
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        v, s, _ = oracle.attach_vertex(vattrs, st, type_hint=hints[k % 3])
        assert (verts[k], states[k]) == (v, s), k
    assert poi not in verts
    # a condition on the input: the same streams on the parent do choose that vertex
    _, pverts, _ = product_attach(top, 200, hints, seed=5)
    assert poi in pverts


def two_triangles():
    nodes = [("poi-%d" % i, "client", 0.0) for i in range(6)]
    tri = lambda a: [("poi-%d" % (a + i), "poi-%d" % (a + (i + 1) % 3), 1.0 + i, 0.0)
                     for i in range(3)]
    edges = tri(0) + tri(3) + [("poi-0", "poi-3", 5.0, 0.0), ("poi-1", "poi-4", 7.0, 0.0)]
    edges += [("poi-%d" % i, "poi-%d" % i, 1.0, 0.0) for i in range(6)]
    return graphml_doc(nodes, edges)


def derive_error(top, edges=(), vertices=()):
    with pytest.raises(ValueError) as e:
        top.without(edges=edges, vertices=vertices)
    return e.value.args[1]


def test_errors_leave_the_parent_alone():
    top, g = load(random_topology_graphml())
    E = g.E
    # a poi's uplink: that poi is cut off
    poi = a_poi(g)
    uplink = int(np.flatnonzero(((g.eu == poi) | (g.ev == poi)) & (g.eu != g.ev))[0])
    assert derive_error(top, edges=[uplink]) == -3
    assert derive_error(top, edges=[E]) == -1
    assert derive_error(top, edges=[-1]) == -1
    assert derive_error(top, vertices=[g.V]) == -1
    assert derive_error(top, vertices=[-1]) == -1
    _, verts, _ = product_attach(top, 5)
    assert derive_error(top, vertices=[verts[0]]) == -2
    assert top.num_edges == E
    lib, _ = _lib.load()
    err = ctypes.c_int32(7)
    assert not lib.shdtopo_derive_without(None, None, 0, None, 0, ctypes.byref(err))
    assert err.value == -1
    assert not lib.shdtopo_derive_without(top._h, None, 1, None, 0, ctypes.byref(err))
    assert err.value == -1
    assert not lib.shdtopo_derive_without(top._h, None, -1, None, 0, None)  # err may be NULL
    assert lib.shdtopo_edge_origin(None, None, 0) == -1
    assert top.num_edges == E
    # the two links of a cut: a cycle edge of the joined triangles is not enough, both joints are
    tri, tg = load(two_triangles())
    assert tri.without(edges=[0]).num_edges == tg.E - 1
    assert tri.without(edges=[6]).num_edges == tg.E - 1
    assert derive_error(tri, edges=[6, 7]) == -3
    assert tri.num_edges == tg.E


@pytest.mark.parametrize("name", ["topology.simple", "topology"])
def test_complete_topology(name):
    """topology.simple has two vertices and one non-loop edge, a bridge: failing it must be
    refused (-3).  The 183-vertex bundled topology is complete as well and loses completeness,
    not connectivity, with one edge."""
    data = bundled_topology(name)
    top, g = load(data)
    assert top.is_complete and g.is_complete()
    same = top.without()
    assert same.is_complete
    assert_graph_equal(same, g)
    assert np.array_equal(same.edge_origin(), np.arange(g.E))
    e = int(np.flatnonzero(g.eu != g.ev)[0])
    if g.V == 2:
        assert derive_error(top, edges=[e]) == -3
        return
    g2, keep = filtered(g, [e])
    assert g2.is_strongly_connected() and not g2.is_complete()
    child = top.without(edges=[e])
    assert not child.is_complete
    assert_graph_equal(child, g2)
