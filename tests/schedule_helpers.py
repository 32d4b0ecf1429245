"""Expected values of the route schedule tests (test_route_schedule*.py).

Every expected value comes from oracle.route_packets on the latency and reliability that each
packet's epoch selects, e = np.searchsorted(from_ns, now, side="right") - 1, with numpy for the
counts.  Nothing in this file calls the schedule (RouteSchedule, shdtopo_route_schedule*,
topowindow_set_schedule).
"""
import functools

import numpy as np

import oracle
from table_helpers import ROUTE_JUMP, route_inputs

U64 = np.uint64
# the hand-made schedule: three epochs over route_inputs()' emission times in [1e9, 2e9)
FROM_NS = (0, 1_300_000_000, 1_700_000_000)


def epoch_of(from_ns, now):
    """The epoch of every emission time: the largest e with from_ns[e] <= now."""
    f = np.ascontiguousarray(from_ns, U64)
    assert f[0] == 0 and (np.diff(f.astype(object)) > 0).all()
    return (np.searchsorted(f, np.ascontiguousarray(now, U64), side="right") - 1).astype(np.uint8)


def expected_schedule(tables, from_ns, src_col, dst_col, payload, state, now, jump, clamp,
                      unrouted="unchanged"):
    """The schedule of a window in numpy and the oracle: tables[e] = (attached, lat, rel, hops) of
    epoch e.  A packet with a column outside [0, A) is not routed: delivered 0, time 0 and its state
    unchanged (the device variant) or after one draw (unrouted="drawn": the host variants).  dict:
    time, delivered, state, epoch, epoch_count (u64 [k, 3]: packets, delivered, not routed),
    not_routed."""
    s, d = np.asarray(src_col, np.int64), np.asarray(dst_col, np.int64)
    payload, state = np.asarray(payload, np.uint32), np.asarray(state, np.uint32)
    now = np.asarray(now, U64)
    n, k = len(s), len(tables)
    A = len(tables[0][0])
    ok = (s >= 0) & (s < A) & (d >= 0) & (d < A)
    ep = epoch_of(from_ns, now)
    lat, rel = np.zeros(n), np.zeros(n)
    for e in range(k):
        m = ok & (ep == e)
        lat[m], rel[m] = tables[e][1][s[m], d[m]], tables[e][2][s[m], d[m]]
    time, dl, st = np.zeros(n, U64), np.zeros(n, np.uint8), state.copy()
    if ok.any():
        time[ok], dl[ok], st[ok] = oracle.route_packets(lat[ok], rel[ok], payload[ok], state[ok],
                                                        now[ok], jump, clamp)
    if unrouted == "drawn":
        for i in np.flatnonzero(~ok):
            st[i] = oracle.rand_r(int(state[i]))[1]
    count = np.array([[(ep == e).sum(), dl[ep == e].sum(), (~ok & (ep == e)).sum()]
                      for e in range(k)], U64).reshape(k, 3)
    return dict(time=time, delivered=dl, state=st, epoch=ep, epoch_count=count,
                not_routed=int((~ok).sum()))


def assert_schedule_equal(got, exp, what=""):
    """got: dict with any of expected_schedule's keys."""
    for key in ("delivered", "time", "state", "epoch", "epoch_count", "not_routed"):
        if key in got and got[key] is not None:
            assert np.array_equal(got[key], exp[key]), (what, key)


@functools.lru_cache(maxsize=None)
def rolled_tables():
    """Three 64 x 64 tables: route_inputs()' and its copies with lat and rel rolled by 1 and 2
    rows.  Shared, never modified."""
    a, lat, rel, hops = route_inputs()["t"]
    out = []
    for r in range(3):
        t = (a, np.roll(lat, r, axis=0), np.roll(rel, r, axis=0), hops)
        for x in t[1:3]:
            x.setflags(write=False)
        out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_times():
    """route_inputs()' emission times with the epochs' edges planted at packets 100 .. 106: 0 and
    from[e] - 1, from[e], from[e] + 1 for e = 1, 2.  Shared, never modified."""
    now = route_inputs()["now"].copy()
    edges = [0] + [FROM_NS[e] + x for e in (1, 2) for x in (-1, 0, 1)]
    now[100:100 + len(edges)] = edges
    now.setflags(write=False)
    return now


def check_inputs(clamp):
    """The conditions on the hand-made inputs, from numpy and the oracle alone."""
    ri = route_inputs()
    tabs = rolled_tables()
    s, d, now = ri["src_col"], ri["dst_col"], edge_times()
    n = len(s)
    ep = epoch_of(FROM_NS, now)
    for e in range(3):
        assert (ep == e).mean() >= 0.2, e
    alone = [oracle.route_packets(t[1][s, d], t[2][s, d], ri["payload"], ri["state"], now,
                                  ROUTE_JUMP, clamp) for t in tabs]
    for i in range(3):
        for j in range(i + 1, 3):
            differ = (alone[i][0] != alone[j][0]) | (alone[i][1] != alone[j][1])
            assert differ.mean() >= 0.4, (i, j, differ.mean())
    exp = expected_schedule(tabs, FROM_NS, s, d, ri["payload"], ri["state"], now, ROUTE_JUMP, clamp)
    for e in range(3):
        dl = exp["delivered"][ep == e]
        assert 0 < dl.sum() < len(dl), e
    assert int(exp["epoch_count"][:, 0].sum()) == n
