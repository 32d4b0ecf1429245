"""The window adapter under a route schedule (topowindow_set_schedule): windows emitted with
topowindow_emit_state and flushed through three hand-made 8 x 8 tables, against
schedule_helpers.expected_schedule in emission order.
"""
import ctypes

import numpy as np
import pytest

from schedule_helpers import FROM_NS, expected_schedule, rolled_tables
from shadow_amd import _lib
from table_helpers import bound_topologies, install

pytestmark = pytest.mark.gpu

P = 8
JUMP = 3_000_000


def small_tables():
    return [(t[0][:P], t[1][:P, :P], t[2][:P, :P], t[3][:P, :P]) for t in rolled_tables()]


def scheduled_window(lib):
    tops, ips = bound_topologies(P, k=3)
    tabs = small_tables()
    for top, t in zip(tops, tabs):
        top.set_option("lazy", 0)  # (the one-table flush then reads the forward row too)
        install(top, t)
    w = lib.topowindow_new(tops[0]._h)
    return tops, ips, tabs, w


def set_schedule(lib, w, tops, from_ns=FROM_NS):
    h = (ctypes.c_void_p * len(tops))(*[t._h for t in tops])
    f = np.array(from_ns[:len(tops)], np.uint64)
    return lib.topowindow_set_schedule(w, h, f.ctypes.data_as(ctypes.c_void_p), len(tops))


def packets(seed, n=200, hosts=P):
    rng = np.random.default_rng(seed)
    return dict(src_col=rng.integers(0, hosts, n).astype(np.int32),
                dst_col=rng.integers(0, hosts, n).astype(np.int32),
                payload=np.where(rng.random(n) < 0.8, 1448, 0).astype(np.uint32),
                state=rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32),
                now=rng.integers(10**9, 2 * 10**9, n).astype(np.uint64))


def emit(lib, w, ips, pk):
    for i in range(len(pk["now"])):
        assert lib.topowindow_emit_state(w, int(ips[pk["src_col"][i]]), int(ips[pk["dst_col"][i]]),
                                         int(pk["payload"][i]), int(pk["state"][i]),
                                         int(pk["now"][i]), i + 1) == i


def flush(lib, w, n):
    got = []

    @_lib.WINDOW_DELIVER
    def deliver(ctx, packet, delivered, time):
        got.append((int(packet), int(delivered), int(time)))

    assert lib.topowindow_flush(w, JUMP, 1, deliver, None) == 0
    assert lib.topowindow_pending(w) == 0
    assert [g[0] for g in got] == list(range(1, n + 1))  # emission order
    return [g[1:] for g in got]


def want(tabs, from_ns, pk):
    exp = expected_schedule(tabs, from_ns, pk["src_col"], pk["dst_col"], pk["payload"],
                            pk["state"], pk["now"], JUMP, 1)
    assert 0 < exp["delivered"].sum() < len(exp["delivered"])
    assert (np.bincount(exp["epoch"], minlength=len(tabs)) > 0).all()
    return list(zip(exp["delivered"].tolist(), exp["time"].tolist()))


def test_windows_follow_the_schedule_and_a_detached_host_keeps_its_column():
    lib, _ = _lib.load()
    tops, ips, tabs, w = scheduled_window(lib)
    assert set_schedule(lib, w, tops) == 0
    # the first window
    pk = packets(1)
    emit(lib, w, ips, pk)
    got = flush(lib, w, len(pk["now"]))
    assert got == want(tabs, FROM_NS, pk)
    assert got != want(tabs[:1], FROM_NS[:1], pk)  # (one table alone gives another window)
    # the second window: host 7 leaves every member before the flush and is still routed
    pk = packets(2)
    assert (pk["src_col"] == P - 1).any() and (pk["dst_col"] == P - 1).any()
    emit(lib, w, ips, pk)
    for top in tops:
        top.detach_ip(int(ips[P - 1]))
        assert len(top.attached_vertices()) == P  # the column is kept for the window
    assert flush(lib, w, len(pk["now"])) == want(tabs, FROM_NS, pk)
    # ... and is gone once the window is flushed, on every member
    for top in tops:
        assert len(top.attached_vertices()) == P - 1
    assert lib.topowindow_emit_state(w, int(ips[0]), int(ips[P - 1]), 1448, 1, 10**9, 1) == -1
    assert flush(lib, w, 0) == []
    lib.topowindow_free(w)


def test_clearing_the_schedule_restores_the_one_table_route():
    lib, _ = _lib.load()
    tops, ips, tabs, w = scheduled_window(lib)
    pk = packets(3)
    n = len(pk["now"])
    emit(lib, w, ips, pk)
    plain = flush(lib, w, n)  # no schedule yet
    assert plain == want(tabs[:1], FROM_NS[:1], pk)
    assert set_schedule(lib, w, [tops[0], tops[1], tops[0]]) == 0
    emit(lib, w, ips, pk)
    assert flush(lib, w, n) == want([tabs[0], tabs[1], tabs[0]], FROM_NS, pk)
    assert lib.topowindow_set_schedule(w, None, None, 0) == 0
    emit(lib, w, ips, pk)
    assert flush(lib, w, n) == plain
    # the members' holds went with the schedule: a detach on one takes its column at once
    tops[1].detach_ip(int(ips[P - 1]))
    assert len(tops[1].attached_vertices()) == P - 1
    lib.topowindow_free(w)
