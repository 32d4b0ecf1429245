"""The window adapter feeding a link monitor (topowindow_set_monitor, include/
shd_topology_window.h): every flushed window goes to shdtopo_monitor_feed_vertices with the batch's
`delivered` outputs, weighted by the payload length, before the window's deferred columns are
released.  The expected bins are the oracle's timeline (timeline_helpers.ExpectedTimeline over
load_helpers.ExpectedLoad) of the packets the deliver callback reported as delivered.
"""
import types

import numpy as np
import pytest

from crossing_helpers import watch_recipe
from load_helpers import ExpectedLoad, random_hosts
from monitor_helpers import check_counters
from shadow_amd import _lib
from test_link_timeline import BASE, MS, RBIN, RNB, RT0, real_graphml
from timeline_helpers import ExpectedTimeline, bytes_equal, check_timeline

pytestmark = pytest.mark.gpu


def test_flushed_windows_feed_the_monitor_with_the_delivered_packets():
    top, g, av, aip = random_hosts(real_graphml(), 300)
    lib, shim = _lib.load()
    rng = np.random.default_rng(41)
    nwin, per = 3, 400
    k = len(av)
    si, di = rng.integers(0, k, nwin * per), rng.integers(0, k, nwin * per)
    si[:4], di[:4] = [0, 1, 2, 2], [0, 1, 2, 3]  # self pairs among them
    pay = np.where(rng.random(nwin * per) < 0.8, 1448, 0).astype(np.uint32)
    state = rng.integers(1, 2**31, nwin * per).astype(np.uint32)
    now = (BASE + rng.integers(0, 10 * MS, nwin * per)).astype(np.uint64)
    now += np.repeat(np.arange(nwin), per).astype(np.uint64) * np.uint64(10 * MS)
    sv, dv = av[si], av[di]
    exp = ExpectedLoad(g, sv, dv, None, av)
    edges, vertices = watch_recipe(exp, sv, dv)
    kw = dict(t0=RT0, bin_ns=RBIN, nbins=RNB)
    mon = top.link_monitor(edges, vertices, **kw)
    w = lib.topowindow_new(top._h)
    assert lib.topowindow_set_monitor(None, mon.id, 1) == -1
    assert lib.topowindow_set_monitor(w, mon.id, 1) == 0
    jump = lib.topowindow_jump_ns(top._h, 0)
    got = {}

    @_lib.WINDOW_DELIVER
    def deliver(ctx, packet, delivered, time):
        got[int(packet) - 1] = int(delivered)

    def flush(win):
        for i in range(win * per, (win + 1) * per):
            assert lib.topowindow_emit_state(w, int(aip[si[i]]), int(aip[di[i]]), int(pay[i]),
                                             int(state[i]), int(now[i]), i + 1) == i - win * per
        assert lib.topowindow_flush(w, jump, 1, deliver, None) == 0

    def expected(upto):
        kept = np.asarray([i for i in range(upto) if got[i]], np.int64)
        assert 20 <= upto - len(kept) and len(kept) >= upto // 2  # drops, and deliveries
        cut = types.SimpleNamespace(verts=[exp.verts[i] for i in kept],
                                    edges=[exp.edges[i] for i in kept])
        return kept, ExpectedTimeline(g, cut, pay[kept], now[kept], edges, vertices, **kw)

    flush(0)
    flush(1)
    kept, xt = expected(2 * per)
    c = xt.conditions()
    assert c["hits"] >= 100 and c["in_range"] >= 30 and c["before"] >= 5 and c["after"] >= 5, c
    out = mon.read()
    check_timeline(out, xt)
    st = mon.stats()
    assert st["feeds"] == 2 and st["fed"] == len(kept) and st["unattached"] == 0
    assert st["skipped_undelivered"] == 2 * per - len(kept) and st["prepares"] == 1
    bytes_equal(out, top.link_timeline(aip[si[kept]], aip[di[kept]], now[kept], edges, vertices,
                                       pay[kept].astype(np.uint64), **kw))
    # monitor -1: the third window is routed and delivered, and nothing is fed
    assert lib.topowindow_set_monitor(w, -1, 1) == 0
    flush(2)
    assert len(got) == 3 * per
    check_timeline(mon.read(), xt)
    assert mon.stats()["feeds"] == 2
    # bytes = 0 counts packets
    mon.reset()
    assert lib.topowindow_set_monitor(w, mon.id, 0) == 0
    got.clear()
    flush(0)
    kept = np.asarray([i for i in range(per) if got[i]], np.int64)
    cut = types.SimpleNamespace(verts=[exp.verts[i] for i in kept],
                                edges=[exp.edges[i] for i in kept])
    x1 = ExpectedTimeline(g, cut, None, now[kept], edges, vertices, **kw)
    check_timeline(mon.read(), x1)
    check_counters(mon.stats(), [x1], fed=len(kept), skipped=per - len(kept))
    lib.topowindow_free(w)
    mon.free()
