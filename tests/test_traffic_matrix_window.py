"""The window adapter feeding a traffic matrix (topowindow_set_matrix, include/
shd_topology_window.h): every flushed window goes to shdtopo_matrix_feed_vertices with the batch's
`delivered` outputs, weighted by the payload length or 1 per packet, before the window's deferred
columns are released -- independently of, and next to, a link monitor.  The expected cells are
numpy's (matrix_helpers.ExpectedMatrix) of the packets the deliver callback reported as delivered.
"""
import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import attach_hosts
from matrix_helpers import ExpectedMatrix, check_counters, check_read
from shadow_amd import _lib
from test_link_timeline import BASE, MS, real_graphml

pytestmark = pytest.mark.gpu


class Windows:
    """A window adapter over a topology with hosts attached by the client / relay / server hints
    (av: the attached vertices ascending, aip: the first host of each) and nwin x per packets to
    emit between those first hosts."""

    def __init__(self, nwin=3, per=400, seed=41, hosts=300):
        data = real_graphml()
        self.top, self.g = sa.Topology.from_buffer(data), oracle.OGraph.from_graphml(data)
        _, self.ips, self.verts = attach_hosts(self.top, self.g, hosts,
                                               type_hints=["client", "relay", "server"])
        first = {}
        for ip, v in zip(self.ips, self.verts):
            first.setdefault(v, ip)
        self.av = np.asarray(sorted(first), np.int32)
        self.aip = np.asarray([first[int(v)] for v in self.av], np.uint32)
        self.lib, _ = _lib.load()
        rng = np.random.default_rng(seed)
        n, k = nwin * per, len(self.av)
        self.per = per
        self.si, self.di = rng.integers(0, k, n), rng.integers(0, k, n)
        self.si[:4], self.di[:4] = [0, 1, 2, 2], [0, 1, 2, 3]  # self pairs among them
        self.pay = np.where(rng.random(n) < 0.8, 1448, 0).astype(np.uint32)
        self.state = rng.integers(1, 2**31, n).astype(np.uint32)
        self.now = (BASE + rng.integers(0, 10 * MS, n)).astype(np.uint64)
        self.sv, self.dv = self.av[self.si], self.av[self.di]
        self.w = self.lib.topowindow_new(self.top._h)
        self.jump = self.lib.topowindow_jump_ns(self.top._h, 0)
        self.got = {}

        @_lib.WINDOW_DELIVER
        def deliver(ctx, packet, delivered, time):
            self.got[int(packet) - 1] = int(delivered)
        self.deliver = deliver

    def emit(self, win):
        lib, per = self.lib, self.per
        for i in range(win * per, (win + 1) * per):
            assert lib.topowindow_emit_state(self.w, int(self.aip[self.si[i]]),
                                             int(self.aip[self.di[i]]), int(self.pay[i]),
                                             int(self.state[i]), int(self.now[i]),
                                             i + 1) == i - win * per

    def flush(self, win=None):
        if win is not None:
            self.emit(win)
        assert self.lib.topowindow_flush(self.w, self.jump, 1, self.deliver, None) == 0

    def delivered(self, a, b):
        """(indices in [a, b), delivered u8) as the deliver callback reported them."""
        idx = np.arange(a, b)
        dl = np.asarray([self.got[i] for i in idx], np.uint8)
        assert 5 <= (dl == 0).sum() and dl.sum() >= (b - a) // 2  # drops, and deliveries
        return idx, dl


@pytest.mark.parametrize("bytes_", [1, 0])
def test_flushed_windows_feed_the_matrix_with_the_delivered_packets(bytes_):
    x = Windows()
    top, lib, per = x.top, x.lib, x.per
    m = top.traffic_matrix()
    assert lib.topowindow_set_matrix(None, m.id, 1) == -1
    assert lib.topowindow_set_matrix(x.w, m.id, bytes_) == 0
    exp = ExpectedMatrix(x.g.V)
    for win in (0, 1):
        x.flush(win)
        idx, dl = x.delivered(win * per, (win + 1) * per)
        exp.add(x.sv[idx], x.dv[idx], x.pay[idx] if bytes_ else None, dl)
    rec, _, tot = check_read(m, exp, x.av)
    assert tot["selfCells"] >= 1 and tot["cells"] >= 300
    assert (tot["weight"] == tot["packets"]) == (not bytes_)
    st = m.stats()
    check_counters(st, exp, feeds=2)
    assert exp.skipped >= 20 and exp.unattached == 0
    # matrix -1: the third window is routed and delivered, and nothing is fed
    assert lib.topowindow_set_matrix(x.w, -1, 1) == 0
    x.flush(2)
    assert len(x.got) == 3 * per
    check_read(m, exp, x.av)
    assert m.stats()["feeds"] == 2
    lib.topowindow_free(x.w)
    m.free()


def test_a_monitor_and_a_matrix_on_one_window_both_get_it():
    x = Windows(nwin=1)
    top, lib, per = x.top, x.lib, x.per
    m = top.traffic_matrix()
    mon = top.link_monitor((), [int(v) for v in x.av[:8]], t0=0, bin_ns=MS, nbins=0)
    assert lib.topowindow_set_monitor(x.w, mon.id, 1) == 0
    assert lib.topowindow_set_matrix(x.w, m.id, 0) == 0
    x.flush(0)
    idx, dl = x.delivered(0, per)
    exp = ExpectedMatrix(x.g.V)
    exp.add(x.sv[idx], x.dv[idx], None, dl)
    check_read(m, exp, x.av)
    ms, st = mon.stats(), m.stats()
    assert ms["feeds"] == 1 and st["feeds"] == 1
    assert ms["fed"] == st["fed"] == int(dl.sum())
    assert ms["skipped_undelivered"] == st["skipped_undelivered"] == int((dl == 0).sum())
    # the monitor alone again: the matrix stays as it is
    assert lib.topowindow_set_matrix(x.w, -1, 0) == 0
    x.got.clear()
    x.flush(0)
    check_read(m, exp, x.av)
    assert mon.stats()["feeds"] == 2 and m.stats()["feeds"] == 1
    lib.topowindow_free(x.w)
    mon.free()
    m.free()


def test_a_host_detached_inside_a_held_window_is_counted_on_its_deferred_column():
    x = Windows(nwin=1, hosts=40)
    top, lib, per = x.top, x.lib, x.per
    m = top.traffic_matrix()
    assert lib.topowindow_set_matrix(x.w, m.id, 1) == 0
    x.emit(0)
    # a vertex with one host loses it before the flush: the column is deferred
    lone = next(int(v) for v in x.av if x.verts.count(int(v)) == 1 and int(v) > x.av[0])
    assert (x.sv[:per] == lone).sum() >= 1 and (x.dv[:per] == lone).sum() >= 1
    top.detach_ip(int(x.aip[list(x.av).index(lone)]))
    x.flush()
    idx, dl = x.delivered(0, per)
    exp = ExpectedMatrix(x.g.V)
    exp.add(x.sv[idx], x.dv[idx], x.pay[idx], dl)
    rec, _, _ = check_read(m, exp, x.av)  # mv has the vertex: it was still a column
    assert lone in rec["srcVertex"] and m.stats()["unattached"] == 0
    # after the flush the column is gone; the vertex keeps its row
    assert lone not in top.attached_vertices()
    check_read(m, exp, x.av)
    lib.topowindow_free(x.w)
    m.free()
