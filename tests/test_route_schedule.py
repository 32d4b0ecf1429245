"""Route schedule (shdtopo_route_schedule*, topo_schedule.hip): a packet window routed through k
resident tables, each packet by the table live at its emission time.

Hand-made tables (table_helpers.bound_topologies / install): route_inputs()' 64 x 64 table and its
copies with lat and rel rolled by 1 and 2 rows, three epochs over its 4096 packets.  A searched
graph: the `real` what-if case, schedule [parent, child, parent].  Every expected value is
schedule_helpers.expected_schedule's: oracle.route_packets on the lat / rel each packet's epoch
selects.  Everything is compared exactly.
"""
import functools

import numpy as np
import pytest

import shadow_amd as sa
from helpers import host_ip
from schedule_helpers import (FROM_NS, assert_schedule_equal, check_inputs, edge_times,
                              expected_schedule, rolled_tables)
from table_helpers import ROUTE_A, ROUTE_JUMP, bound_topologies, install, route_inputs
from whatif_helpers import assert_table_equal, case, product

pytestmark = pytest.mark.gpu

# tile edges of the 256-thread workgroup and its 64-lane waves.  (The default build routes one
# packet per thread, so 257 is already past a 256 x kRouteU tile and 4096 spans 16 workgroups.)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4096)


def cu(x):
    import torch
    x = np.array(x)  # (a copy: the shared inputs are read-only)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(x.dtype)
    return torch.from_numpy(x.view(view) if view else x).cuda()


@functools.lru_cache(maxsize=None)
def members():
    """Three topologies of 64 pinned columns with rolled_tables() installed (only read)."""
    tops, ips = bound_topologies(ROUTE_A, k=3)
    for top, t in zip(tops, rolled_tables()):
        install(top, t)
    return tops, ips


def window(n=None, now=None):
    ri = route_inputs()
    n = len(ri["src_col"]) if n is None else n
    now = edge_times() if now is None else now
    return dict(src_col=ri["src_col"][:n], dst_col=ri["dst_col"][:n], payload=ri["payload"][:n],
                state=ri["state"][:n], now=now[:n])


def run_device(sched, w, clamp, want_epoch=True, jump=ROUTE_JUMP):
    """route_device on a window dict: the outputs as numpy, with the device variant's return."""
    import torch
    n = len(w["src_col"])
    t_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    s_out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_out = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    ep = torch.full((n,), 99, dtype=torch.uint8, device="cuda") if want_epoch else None
    count = sched.route_device(cu(w["src_col"]), cu(w["dst_col"]), cu(w["payload"]),
                               cu(w["state"]), cu(w["now"]), jump, clamp, t_out, s_out, d_out,
                               epoch=ep)
    torch.cuda.synchronize()
    return dict(time=t_out.cpu().numpy().view(np.uint64), delivered=d_out.cpu().numpy(),
                state=s_out.cpu().numpy().view(np.uint32),
                epoch=ep.cpu().numpy() if want_epoch else None, epoch_count=count)


def expected(tables, from_ns, w, clamp, jump=ROUTE_JUMP, unrouted="unchanged"):
    return expected_schedule(tables, from_ns, w["src_col"], w["dst_col"], w["payload"], w["state"],
                             w["now"], jump, clamp, unrouted)


@pytest.mark.parametrize("clamp", (0, 1))
def test_inputs_tell_the_epochs_apart(clamp):
    check_inputs(clamp)


@pytest.mark.parametrize("clamp", (0, 1))
def test_three_epochs_match_the_oracle(clamp):
    tops, _ = members()
    sched = sa.RouteSchedule(tops, FROM_NS)
    w = window()
    exp = expected(rolled_tables(), FROM_NS, w, clamp)
    # the planted times fall where the rule says
    assert exp["epoch"][100:107].tolist() == [0, 0, 1, 1, 1, 2, 2]
    got = run_device(sched, w, clamp)
    assert_schedule_equal(got, exp)
    st = sched.stats()
    n = len(w["now"])
    assert (st["packets"], st["epochs"], st["not_routed"]) == (n, 3, 0)
    assert np.array_equal(st["epoch_packets"][:3], exp["epoch_count"][:, 0].astype(np.int64))
    assert np.array_equal(st["epoch_delivered"][:3], exp["epoch_count"][:, 1].astype(np.int64))
    assert not st["epoch_packets"][3:].any() and not st["epoch_delivered"][3:].any()
    assert st["bytes_model"] == 54 * n and st["kernel_ms"] > 0 and st["total_ms"] > 0


@pytest.mark.parametrize("n", SIZES)
def test_tile_edges(n):
    tops, _ = members()
    sched = sa.RouteSchedule(tops, FROM_NS)
    w = window(n)
    got = run_device(sched, w, 1)
    assert_schedule_equal(got, expected(rolled_tables(), FROM_NS, w, 1), n)
    assert int(got["epoch_count"][:, 0].sum()) == n


def test_a_window_of_more_tiles_than_workgroups():
    """A launch has at most 4,096 workgroups (kGrid, topo_schedule.hip), each striding over the
    tiles: 4,096 x 256 + 257 packets give the first workgroups a second tile, the last of them a
    partial one."""
    tops, _ = members()
    rng = np.random.default_rng(77)
    n = 4096 * 256 + 257
    w = dict(src_col=rng.integers(0, ROUTE_A, n).astype(np.int32),
             dst_col=rng.integers(0, ROUTE_A, n).astype(np.int32),
             payload=np.where(rng.random(n) < 0.8, 1448, 0).astype(np.uint32),
             state=rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32),
             now=rng.integers(10**9, 2 * 10**9, n).astype(np.uint64))
    w["src_col"][[5, n - 1]] = -1  # one not routed in a first tile, one in the last
    exp = expected(rolled_tables(), FROM_NS, w, 1)
    got = run_device(sa.RouteSchedule(tops, FROM_NS), w, 1)
    assert_schedule_equal(got, exp)
    assert int(got["epoch_count"][:, 0].sum()) == n and int(got["epoch_count"][:, 2].sum()) == 2


def test_one_epoch_is_the_one_table_route():
    import torch
    tops, _ = members()
    w = window()
    n = len(w["now"])
    for top, tab in zip(tops[:2], rolled_tables()[:2]):
        got = run_device(sa.RouteSchedule([top], [0]), w, 1)
        t_out = torch.empty(n, dtype=torch.int64, device="cuda")
        s_out = torch.empty(n, dtype=torch.int32, device="cuda")
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        top.route_batch_device(cu(w["src_col"]), cu(w["dst_col"]), cu(w["payload"]),
                               cu(w["state"]), cu(w["now"]), ROUTE_JUMP, 1, t_out, s_out, d_out)
        torch.cuda.synchronize()
        assert got["time"].tobytes() == t_out.cpu().numpy().tobytes()
        assert got["state"].tobytes() == s_out.cpu().numpy().tobytes()
        assert got["delivered"].tobytes() == d_out.cpu().numpy().tobytes()
        assert not got["epoch"].any()
        assert_schedule_equal(got, expected([tab], [0], w, 1))


def test_sixteen_epochs_over_two_topologies_and_a_link_that_comes_back():
    tops, _ = members()
    tabs = rolled_tables()
    w = window()
    # 16 epochs: 0, then 15 starts across the window's [1e9, 2e9)
    from16 = [0] + [1_000_000_000 + 62_500_000 * e for e in range(1, 16)]
    exp = expected([tabs[0], tabs[1]] * 8, from16, w, 1)
    assert (np.bincount(exp["epoch"], minlength=16) > 0).all()
    got = run_device(sa.RouteSchedule([tops[0], tops[1]] * 8, from16), w, 1)
    assert_schedule_equal(got, exp, "k = 16")
    exp = expected([tabs[0], tabs[1], tabs[0]], FROM_NS, w, 0)
    got = run_device(sa.RouteSchedule([tops[0], tops[1], tops[0]], FROM_NS), w, 0)
    assert_schedule_equal(got, exp, "parent, child, parent")


def test_no_epoch_output_leaves_the_others_unchanged():
    tops, _ = members()
    sched = sa.RouteSchedule(tops, FROM_NS)
    w = window(1000)
    exp = expected(rolled_tables(), FROM_NS, w, 1)
    got = run_device(sched, w, 1, want_epoch=False)
    assert got["epoch"] is None
    assert_schedule_equal(got, exp)
    assert sched.stats()["bytes_model"] == 53 * 1000


def test_columns_outside_the_table_are_not_routed():
    tops, _ = members()
    sched = sa.RouteSchedule(tops, FROM_NS)
    w = window()
    n = len(w["now"])
    s, d = w["src_col"].copy(), w["dst_col"].copy()
    s[[0, 64]] = -1
    d[[63, n - 1]] = ROUTE_A
    w.update(src_col=s, dst_col=d)
    exp = expected(rolled_tables(), FROM_NS, w, 1)
    at = [0, 63, 64, n - 1]
    assert exp["not_routed"] == 4 and int(exp["epoch_count"][:, 2].sum()) == 4
    assert not exp["delivered"][at].any() and not exp["time"][at].any()
    assert np.array_equal(exp["state"][at], w["state"][at])
    bad0 = [t.stats()["route_bad_packets"] for t in tops]
    got = run_device(sched, w, 1)  # (the device variant returns 0: route_device did not raise)
    assert_schedule_equal(got, exp)
    assert sched.stats()["not_routed"] == 4
    assert [t.stats()["route_bad_packets"] for t in tops] == bad0


def test_members_statistics_and_tables_stay_as_they_were():
    tops, _ = members()
    before = [t.stats() for t in tops]
    run_device(sa.RouteSchedule(tops, FROM_NS), window(), 1)
    for top, st, tab in zip(tops, before, rolled_tables()):
        assert top.stats() == st
        assert_table_equal(top, tab)


# ---- a searched graph: [parent, child, parent] ----
@functools.lru_cache(maxsize=None)
def real_pair():
    c = case("real")
    parent = product("real")
    child = parent.without(edges=c["fail"])
    return c, parent, child


@functools.lru_cache(maxsize=None)
def real_window():
    c = case("real")
    rng = np.random.default_rng(41)
    n, nh = 2000, len(c["ips"])
    hs = rng.integers(0, nh, n)
    hd = (hs + rng.integers(1, nh, n)) % nh  # another host
    ips, verts = np.array(c["ips"], np.uint32), np.array(c["verts"], np.int32)
    col = {int(v): k for k, v in enumerate(c["t0"][0])}
    cols = np.array([col[int(v)] for v in verts], np.int32)
    w = dict(src_ip=ips[hs], dst_ip=ips[hd], src_v=verts[hs], dst_v=verts[hd],
             src_col=cols[hs], dst_col=cols[hd],
             payload=np.where(rng.random(n) < 0.8, 1448, 0).astype(np.uint32),
             state=rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32),
             now=rng.integers(10**9, 2 * 10**9, n).astype(np.uint64))
    # five packets with an address that is not attached
    for i, end in ((0, "src"), (63, "dst"), (64, "src"), (1000, "dst"), (n - 1, "src")):
        w[end + "_ip"][i] = host_ip(7000 + i)
        w[end + "_v"][i] = -1
        w[end + "_col"][i] = -1
    return w


def test_real_graph_parent_child_parent():
    c, parent, child = real_pair()
    w = real_window()
    sched = sa.RouteSchedule([parent, child, parent], FROM_NS)
    jump = 5_000_000
    exp = expected([c["t0"], c["t1"], c["t0"]], FROM_NS, w, 1, jump, unrouted="drawn")
    assert exp["not_routed"] == 5
    alone = expected([c["t0"]], [0], w, 1, jump, unrouted="drawn")
    assert (exp["time"] != alone["time"]).any()  # the failure shows in the middle epoch
    keys = ("time", "delivered", "state", "epoch", "epoch_count", "not_routed")
    got = dict(zip(keys, sched.route(w["src_ip"], w["dst_ip"], w["payload"], w["state"], w["now"],
                                     jump)))
    assert_schedule_equal(got, exp, "route")
    got = dict(zip(keys, sched.route_vertices(w["src_v"], w["dst_v"], w["payload"], w["state"],
                                              w["now"], jump)))
    assert_schedule_equal(got, exp, "route_vertices")
    assert sched.stats()["not_routed"] == 5
    assert_table_equal(parent, c["t0"])
    assert_table_equal(child, c["t1"])


# ---- errors ----
def test_a_member_with_another_attached_set_is_refused():
    """b is a without its last host (each host of bound_topologies has a vertex of its own), so a
    has one more host attached and one more column."""
    (a, b), ips = bound_topologies(8, k=2)
    b.detach_ip(int(ips[7]))
    assert len(b.attached_vertices()) == 7 and len(a.attached_vertices()) == 8
    w = window(16)
    w.update(src_col=w["src_col"] % 8, dst_col=w["dst_col"] % 8)
    t = rolled_tables()[0]
    small = (t[0][:8], t[1][:8, :8], t[2][:8, :8], t[3][:8, :8])
    install(a, small)
    for tops in ([b, a], [a, b], [a, a, b]):
        with pytest.raises(RuntimeError) as e:
            run_device(sa.RouteSchedule(tops, FROM_NS[:len(tops)]), w, 1)
        assert e.value.args[1] == -4
    # the same handle throughout is a valid schedule
    got = run_device(sa.RouteSchedule([a, a, a], FROM_NS), w, 1)
    assert_schedule_equal(got, expected([small] * 3, FROM_NS, w, 1))
