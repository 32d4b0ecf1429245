"""Route schedule, host side (no device): the argument checks of shdtopo_route_schedule*, the -4
for unequal attached sets, the empty window, and topowindow_set_schedule's validation -- all
answered before any device is used.
"""
import ctypes

import numpy as np

import shadow_amd as sa
from helpers import random_topology_graphml
from impact_helpers import check_no_device_used
from shadow_amd import _lib
from whatif_helpers import product_attach


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pair(hosts_b=None):
    data = random_topology_graphml()
    a, b = sa.Topology.from_buffer(data), sa.Topology.from_buffer(data)
    ips, verts, _ = product_attach(a, 20)
    product_attach(b, 20, only=hosts_b)
    return a, b, np.array(ips, np.uint32), np.array(verts, np.int32)


def _handles(*tops):
    return (ctypes.c_void_p * len(tops))(*[t._h if t is not None else None for t in tops])


def _calls(lib, ips, verts, n=8):
    """The three variants as call(tops, from_ns, k, n=n, **nulls): nulls names the arrays to pass
    as NULL.  The device variant's pointers are never read: every call here ends in the checks."""
    s, d = verts[:n].copy(), verts[n:2 * n].copy()
    pay, st = np.full(n, 1448, np.uint32), np.arange(n, dtype=np.uint32)
    now = np.arange(n, dtype=np.uint64)
    ins = np.zeros(n, sa.topology.PACKET_IN)
    ins["srcIP"], ins["dstIP"] = ips[:n], ips[n:2 * n]
    out = np.zeros(n, sa.topology.PACKET_OUT)
    tim, so, dl = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    arrays = dict(src=s, dst=d, pay=pay, state=st, now=now, ins=ins, out=out, time=tim, sout=so,
                  dl=dl)

    def ptr(name, nulls):
        return None if name in nulls else _p(arrays[name])

    def device(tops, f, k, n=n, nulls=()):
        return lib.shdtopo_route_schedule_device(
            tops, f, k, ptr("src", nulls), ptr("dst", nulls), ptr("pay", nulls),
            ptr("state", nulls), ptr("now", nulls), n, 1000, 1, ptr("time", nulls),
            ptr("sout", nulls), ptr("dl", nulls), None, None, None)

    def vertices(tops, f, k, n=n, nulls=()):
        return lib.shdtopo_route_schedule_vertices(
            tops, f, k, ptr("src", nulls), ptr("dst", nulls), ptr("pay", nulls),
            ptr("state", nulls), ptr("now", nulls), n, 1000, 1, ptr("out", nulls), None, None)

    def hosts(tops, f, k, n=n, nulls=()):
        return lib.shdtopo_route_schedule(tops, f, k, ptr("ins", nulls), ptr("out", nulls), n,
                                          1000, 1, None, None)

    return {"device": (device, ("src", "dst", "pay", "state", "now", "time", "sout", "dl")),
            "vertices": (vertices, ("src", "dst", "pay", "state", "now", "out")),
            "hosts": (hosts, ("ins", "out"))}


def test_bad_arguments_are_refused_before_any_device_is_used():
    lib, _ = _lib.load()
    a, b, ips, verts = _pair()
    f3 = np.array([0, 10, 20], np.uint64)
    ok3 = _handles(a, b, a)
    for name, (call, arrays) in _calls(lib, ips, verts).items():
        assert call(None, _p(f3), 3) == -1, name
        assert call(ok3, None, 3) == -1, name
        assert call(_handles(a, None, b), _p(f3), 3) == -1, name
        assert call(_handles(None, a, b), _p(f3), 3) == -1, name
        assert call(ok3, _p(f3), 0) == -1 and call(ok3, _p(f3), -1) == -1, name
        many = _handles(*([a, b] * 9))
        f18 = np.arange(18, dtype=np.uint64)
        assert call(many, _p(f18), 17) == -1 and call(many, _p(f18), 18) == -1, name
        for bad in ([1, 10, 20], [0, 10, 10], [0, 20, 10], [0, 0, 5]):
            assert call(ok3, _p(np.array(bad, np.uint64)), 3) == -1, (name, bad)
        assert call(ok3, _p(f3), 3, n=-1) == -1, name
        for x in arrays:
            assert call(ok3, _p(f3), 3, nulls=(x,)) == -1, (name, x)
    assert lib.shdtopo_route_schedule_stats(None, None) == -1
    assert lib.shdtopo_route_schedule_stats(a._h, None) == -1
    for t in (a, b):
        check_no_device_used(t)
        assert t.stats()["sources"] == 0 and t.stats()["build_ms"] == 0


def test_unequal_attached_sets_are_refused_before_any_device_is_used():
    """Two topologies of one document, the second with the first 10 hosts only."""
    lib, _ = _lib.load()
    a, b, ips, verts = _pair(hosts_b=tuple(range(10)))
    assert len(a.attached_vertices()) != len(b.attached_vertices())
    f = np.array([0, 10, 20], np.uint64)
    for name, (call, _) in _calls(lib, ips, verts).items():
        for tops in (_handles(a, b, a), _handles(b, a, a), _handles(a, a, b)):
            assert call(tops, _p(f), 3) == -4, name
            assert call(tops, _p(f), 3, n=0) == -4, name
    for t in (a, b):
        check_no_device_used(t)
        assert t.stats()["sources"] == 0 and t.stats()["build_ms"] == 0


def test_an_empty_window_is_answered_without_a_table():
    lib, _ = _lib.load()
    a, b, ips, verts = _pair()
    f = np.array([0, 10, 20], np.uint64)
    for name, (call, arrays) in _calls(lib, ips, verts).items():
        assert call(_handles(a, b, a), _p(f), 3, n=0) == 0, name
        assert call(_handles(a, b, a), _p(f), 3, n=0, nulls=arrays) == 0, name
        assert call(_handles(a), _p(f), 1, n=0) == 0, name
    sched = sa.RouteSchedule([a, b, a], f)
    t, dl, st, ep, count, bad = sched.route_vertices([], [], [], [], [], 1000)
    assert len(t) == len(dl) == len(st) == len(ep) == 0 and bad == 0
    assert count.shape == (3, 3) and not count.any()
    s = sched.stats()
    assert (s["packets"], s["epochs"], s["not_routed"], s["kernel_ms"]) == (0, 3, 0, 0)
    for t in (a, b):
        check_no_device_used(t)
        assert t.stats()["sources"] == 0 and t.stats()["build_ms"] == 0


def test_window_schedule_is_validated():
    lib, _ = _lib.load()
    a, b, _, _ = _pair()
    w = lib.topowindow_new(a._h)
    f = np.array([0, 10, 20], np.uint64)
    assert lib.topowindow_set_schedule(None, _handles(a, b, a), _p(f), 3) == -1
    # tops[0] must be the window's topology
    assert lib.topowindow_set_schedule(w, _handles(b, a, a), _p(f), 3) == -1
    assert lib.topowindow_set_schedule(w, _handles(b), _p(f), 1) == -1
    assert lib.topowindow_set_schedule(w, None, _p(f), 3) == -1
    assert lib.topowindow_set_schedule(w, _handles(a, b, a), None, 3) == -1
    assert lib.topowindow_set_schedule(w, _handles(a, None, a), _p(f), 3) == -1
    assert lib.topowindow_set_schedule(w, _handles(a, b, a), _p(f), -1) == -1
    assert lib.topowindow_set_schedule(w, _handles(*([a, b] * 9)),
                                       _p(np.arange(18, dtype=np.uint64)), 17) == -1
    for bad in ([1, 10, 20], [0, 10, 10], [0, 20, 10]):
        assert lib.topowindow_set_schedule(w, _handles(a, b, a), _p(np.array(bad, np.uint64)),
                                           3) == -1, bad
    # a valid one, replaced, cleared (k = 0 takes no arrays), set again and freed with the window
    assert lib.topowindow_set_schedule(w, _handles(a, b, a), _p(f), 3) == 0
    assert lib.topowindow_set_schedule(w, _handles(a, b), _p(f), 2) == 0
    assert lib.topowindow_set_schedule(w, None, None, 0) == 0
    assert lib.topowindow_set_schedule(w, _handles(a, b, a), _p(f), 3) == 0
    assert lib.topowindow_pending(w) == 0
    lib.topowindow_free(w)
    for t in (a, b):
        check_no_device_used(t)
