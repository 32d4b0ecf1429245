"""Every consumer of the finished A x A table on hand-made tables installed with
shdtopo_bind_table / shdtopo_bind_table_ref (table_helpers): the diff (topo_diff.hip), the flow
impact (topo_impact.hip), the packet route and the row minima (topo_kernels.hip), the getters' row
copy, and the installer itself.  No graph search runs except in the by-reference lifecycle test.

References: whatif_helpers.expected_diff, impact_helpers.expected_impact, oracle.route_packets and
numpy.min on the same tables.  Everything is exact: bit patterns for doubles, array_equal for the
rest.  The conditions on the inputs are in test_bound_tables_cpu.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from helpers import attach_hosts, host_ip, oracle_table, synthetic_pair
from impact_helpers import FLOW_CHANGE, assert_impact_equal, assert_sums_equal, expected_impact
from shadow_amd import _lib
from table_helpers import (IMPACT_SIZES, ROUTE_JUMP, SIZES, U64, bound_flows, bound_topologies,
                           flow_ips, install, make_tables, pack, rowmin_table, route_inputs)
from whatif_helpers import CHANGE, assert_diff_equal, assert_table_equal, expected_diff, swapped

pytestmark = pytest.mark.gpu

HOWS = ("copy", "ref")
BUILD_COUNTERS = ("paths_computed", "path_seconds_total", "sources", "batches", "relaxations",
                  "sssp_kernel_ms", "build_wall_ms", "replay_rows")


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(U64)


def cu(x):
    import torch
    x = np.array(x)  # (a copy: the shared inputs are read-only)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(x.dtype)
    return torch.from_numpy(x.view(view) if view else x).cuda()


def one_topology(A, lazy=0):
    (top,), ips = bound_topologies(A, 1)
    top.set_option("lazy", lazy)
    return top, ips


def make_pair(A, how0="copy", how1="copy"):
    """Two topologies with make_tables(A)'s t0 and t1 installed: (a, b, ips)."""
    (a, b), ips = bound_topologies(A, 2)
    t0, t1, _ = make_tables(A)
    install(a, t0, how0)
    install(b, t1, how1)
    return a, b, ips


@functools.lru_cache(maxsize=None)
def pair(A):
    """make_pair(A) with both tables copied in, made once (the tests only read them)."""
    return make_pair(A)


def sample_pairs(A, m=24, seed=1):
    """Ordered column pairs, each with its reverse, the corners among them."""
    rng = np.random.default_rng([seed, A])
    p = [(0, 0), (0, A - 1), (A - 1, A - 1)] + [tuple(int(x) for x in rng.integers(0, A, 2))
                                                for _ in range(m)]
    return p + [(j, i) for i, j in p]


def assert_getters(top, ips, t, pairs):
    _, lat, rel, _ = t
    for i, j in pairs:
        got = (top.latency_ip(int(ips[i]), int(ips[j])), top.reliability_ip(int(ips[i]), int(ips[j])))
        assert bits(got[0]) == bits(lat[i, j]) and bits(got[1]) == bits(rel[i, j]), (i, j)


def route(top, s, d, pay, state, now, jump, clamp):
    import torch
    n = len(s)
    t_out = torch.empty(n, dtype=torch.int64, device="cuda")
    s_out = torch.empty(n, dtype=torch.int32, device="cuda")
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    top.route_batch_device(cu(s), cu(d), cu(pay), cu(state), cu(now), jump, clamp, t_out, s_out,
                           d_out)
    torch.cuda.synchronize()
    return (t_out.cpu().numpy().view(np.uint64), d_out.cpu().numpy(),
            s_out.cpu().numpy().view(np.uint32))


def assert_routes(top, t, seed=2, n=600):
    """A window of packets over random pairs of table t against the oracle's schedule."""
    _, lat, rel, _ = t
    A = len(lat)
    rng = np.random.default_rng([seed, A])
    s, d = rng.integers(0, A, n).astype(np.int32), rng.integers(0, A, n).astype(np.int32)
    pay = np.where(rng.random(n) < 0.8, 1448, 0).astype(np.uint32)
    state = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    now = rng.integers(10**9, 2 * 10**9, n).astype(np.uint64)
    got = route(top, s, d, pay, state, now, 5_000_000, 1)
    want = oracle.route_packets(lat[s, d], rel[s, d], pay, state, now, 5_000_000, 1)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    assert 0 < want[1].mean() < 1  # some dropped, some delivered


# ---- install and read back ----
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("A", SIZES)
def test_install_and_read_back(A, how):
    t0 = make_tables(A).t0
    top, ips = one_topology(A)
    before = top.stats()
    kept = install(top, t0, how)
    assert_table_equal(top, t0)
    assert top.getMinimumLatency() == t0[1].min()
    assert_getters(top, ips, t0, sample_pairs(A))
    assert_table_equal(top, t0)
    after = top.stats()
    for k in BUILD_COUNTERS:  # the graph is never searched
        assert after[k] == before[k] == 0, k
    assert after["errors"] == 0
    del kept


# ---- row_min_kernel ----
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("A", SIZES)
def test_row_minima_of_an_installed_table(A, how):
    t, pos, mins = rowmin_table(A)
    lat = t[1]
    top, ips = one_topology(A, lazy=1)
    kept = install(top, t, how)
    assert top.lazyMinimumLatency() == 0.0
    # each row once as a source (its self pair), the rows in descending order of their minimum:
    # every query lowers the running minimum to its row's
    for r in np.argsort(-mins):
        got = top.latency_ip(int(ips[r]), int(ips[r]))
        assert bits(got) == bits(lat[r, r]), r
        assert top.lazyMinimumLatency() == mins[r], r
    v, _, m = top.lazy_rows()
    assert np.array_equal(v, t[0])
    want = np.where(lat >= 0, lat, np.inf).min(axis=1)
    assert np.array_equal(bits(m), bits(want))
    assert top.stats()["paths_computed"] == 0
    del kept


# ---- re-binding ----
def test_rebinding_a_copied_table():
    import torch
    A = 65
    t0, t1, _ = make_tables(A)
    top, ips = one_topology(A)
    install(top, t0, "copy")
    assert_getters(top, ips, t0, [(3, c) for c in range(A)])  # row 3 is on the host now
    assert top.stats()["rows_to_host"] == 1
    lr, hops = install(top, t1, "copy")
    assert_getters(top, ips, t1, [(3, c) for c in range(A)] + sample_pairs(A))
    assert_table_equal(top, t1)
    assert_routes(top, t1)
    # the caller's tensors are the caller's again
    lr.fill_(7.0)
    hops.zero_()
    torch.cuda.synchronize()
    assert_table_equal(top, t1)
    assert_getters(top, ips, t1, [(5, c) for c in range(A)])  # (a row not yet on the host)
    assert_routes(top, t1, seed=3)
    assert top.stats()["paths_computed"] == 0


def test_rebinding_by_reference_after_a_change_in_place():
    import torch
    A = 65
    t0, t1, _ = make_tables(A)
    top, ips = one_topology(A)
    lr, hops = install(top, t0, "ref")
    assert_getters(top, ips, t0, [(3, c) for c in range(A)])
    assert_table_equal(top, t0)
    new_lr, new_hops = pack(t1)
    lr.copy_(torch.from_numpy(new_lr))
    hops.copy_(torch.from_numpy(new_hops))
    torch.cuda.synchronize()
    top.bind_table_ref(lr, hops, float(t1[1].min()))
    assert top.getMinimumLatency() == t1[1].min()
    assert_getters(top, ips, t1, [(3, c) for c in range(A)] + sample_pairs(A))
    assert_table_equal(top, t1)
    assert_routes(top, t1)
    assert top.stats()["paths_computed"] == 0


# ---- table_diff ----
@pytest.mark.parametrize("hows", (("copy", "copy"), ("ref", "copy"), ("copy", "ref")))
@pytest.mark.parametrize("A", SIZES)
def test_table_diff(A, hows):
    t0, t1, _ = make_tables(A)
    a, b, _ = pair(A) if hows == ("copy", "copy") else make_pair(A, *hows)
    exp = expected_diff(t0, t1)
    got = a.table_diff(b)
    assert_diff_equal(got, exp)
    st = a.table_diff_stats()
    assert st["pairs"] == A * A and st["changed"] == exp["total"]
    assert st["bytes_read"] == 36 * (A * A + int((exp["row_changed"] > 0).sum()) * A)
    back = b.table_diff(a)
    assert_diff_equal(back, expected_diff(t1, t0))
    assert back["records"].tobytes() == swapped(exp).tobytes()
    for x in (a, b):
        same = x.table_diff(x)
        assert same["total"] == 0 and len(same["records"]) == 0 and not same["kind_count"].any()
        assert not same["row_changed"].any() and (same["row_worst_col"] == -1).all()
        assert not same["row_worst_rise"].any()
    assert_table_equal(a, t0)
    assert_table_equal(b, t1)
    if hows != ("copy", "copy"):
        a.free()
        b.free()


def sweep_caps(first, total):
    """0, 1, every first-record offset - 1 / + 0 / + 1, total - 1, total, total + 7."""
    caps = {0, 1, total - 1, total, total + 7}
    for o in first:
        caps |= {int(o) - 1, int(o), int(o) + 1}
    return sorted(c for c in caps if c >= 0)


@pytest.mark.parametrize("A", (65, 257))
def test_table_diff_cap_sweep(A):
    t0, t1, _ = make_tables(A)
    a, b, _ = pair(A)
    exp = expected_diff(t0, t1)
    total = exp["total"]
    rc = exp["row_changed"].astype(np.int64)
    first = (np.cumsum(rc) - rc)[rc > 0]  # every changed row's first record
    assert len(first) > A // 2
    caps = sweep_caps(first, total)
    for cap in caps:
        assert_diff_equal(a.table_diff(b, cap=cap), exp, cap=cap)
    # through the C ABI into a prefilled buffer: nothing past min(cap, total) is written
    lib, _ = _lib.load()
    for cap in (1, int(first[len(first) // 2]) + 1, total - 1, total):
        buf = np.full(total + 7, 0xFF, np.uint8).repeat(CHANGE.itemsize).view(CHANGE)
        r = lib.shdtopo_table_diff(a._h, b._h, buf.ctypes.data_as(ctypes.c_void_p), cap, None,
                                   None, None, None)
        assert r == total
        assert buf[:cap].tobytes() == exp["records"][:cap].tobytes()
        assert (buf[cap:].view(np.uint8) == 0xFF).all()


# ---- flow_impact / flow_impact_device ----
def tile_of(top):
    T = top.flow_impact_stats()["tile_flows"]
    assert T >= 256 and T % 256 == 0
    return T


@functools.lru_cache(maxsize=None)
def impact_expected(A, T, edges, weights, n=None):
    t0, t1, _ = make_tables(A)
    fl = bound_flows(A, T)
    w = fl[weights] if weights else None
    return expected_impact(t0, t1, fl["src_col"][:n], fl["dst_col"][:n],
                           None if w is None else w[:n], fl["edge_sets"][edges])


def run_host(a, b, ips, fl, edges, n=None, **kw):
    return a.flow_impact(b, flow_ips(ips, fl["src_col"][:n]), flow_ips(ips, fl["dst_col"][:n]),
                         weight=fl["weight"][:n], rise_edges_ns=fl["edge_sets"][edges], **kw)


@pytest.mark.parametrize("edges", ("none", "zero", "exact", "max"))
@pytest.mark.parametrize("A", IMPACT_SIZES)
def test_flow_impact(A, edges):
    a, b, ips = pair(A)
    T = tile_of(a)
    fl = bound_flows(A, T)
    exp = impact_expected(A, T, edges, "weight")
    got = run_host(a, b, ips, fl, edges)
    assert_impact_equal(got, exp, what="host")
    assert got["totals"]["worstFlow"] == fl["worst"][0]
    assert got["records"].dtype.itemsize == FLOW_CHANGE.itemsize == 48
    # the device variant: columns as they are (-1 and A: unattached), u32 payloads as weights
    d_sc, d_dc, d_pay = cu(fl["src_col"]), cu(fl["dst_col"]), cu(fl["payload"])
    dev = a.flow_impact_device(b, d_sc, d_dc, payload=d_pay, rise_edges_ns=fl["edge_sets"][edges])
    assert_impact_equal(dev, impact_expected(A, T, edges, "payload"), what="device")
    assert dev["records"].tobytes() == got["records"].tobytes()
    # the other direction
    t0, t1, _ = make_tables(A)
    back = run_host(b, a, ips, fl, edges)
    assert_impact_equal(back, expected_impact(t1, t0, fl["src_col"], fl["dst_col"], fl["weight"],
                                              fl["edge_sets"][edges]), what="back")


@pytest.mark.parametrize("A", IMPACT_SIZES)
def test_flow_impact_prefixes(A):
    a, b, ips = pair(A)
    T = tile_of(a)
    fl = bound_flows(A, T)
    d_sc, d_dc, d_pay = cu(fl["src_col"]), cu(fl["dst_col"]), cu(fl["payload"])
    for n in (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1):
        assert_impact_equal(run_host(a, b, ips, fl, "exact", n),
                            impact_expected(A, T, "exact", "weight", n), what=n)
        assert a.flow_impact_stats()["flows"] == n
        dev = a.flow_impact_device(b, d_sc[:n], d_dc[:n], payload=d_pay[:n],
                                   rise_edges_ns=fl["edge_sets"]["exact"])
        assert_impact_equal(dev, impact_expected(A, T, "exact", "payload", n), what=n)


def test_flow_impact_cap_sweep():
    A = 65
    a, b, ips = pair(A)
    T = tile_of(a)
    fl = bound_flows(A, T)
    exp = impact_expected(A, T, "exact", "weight")
    total = exp["total"]
    flows = exp["records"]["flow"]
    n = len(fl["weight"])
    per_tile = np.bincount(flows // T, minlength=(n + T - 1) // T)
    first = (np.cumsum(per_tile) - per_tile)[per_tile > 0]  # every tile's first record
    assert len(first) >= 4
    # and every 64-flow word's, the unit the fill kernel ranks by
    per_word = np.bincount(flows // 64, minlength=(n + 63) // 64)
    first = np.concatenate([first, (np.cumsum(per_word) - per_word)[per_word > 0][::7]])
    for cap in sweep_caps(first, total):
        got = run_host(a, b, ips, fl, "exact", cap=cap)
        assert_impact_equal(got, exp, cap=cap, what=cap)
    zero = run_host(a, b, ips, fl, "exact", cap=0)
    assert len(zero["records"]) == 0
    assert_sums_equal(zero, exp)
    lib, _ = _lib.load()
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(ctypes.c_void_p)
    s, d = flow_ips(ips, fl["src_col"]), flow_ips(ips, fl["dst_col"])
    e = fl["edge_sets"]["exact"]
    for cap in (1, int(first[1]) + 1, total - 1):
        buf = np.full(total + 7, 0xFF, np.uint8).repeat(FLOW_CHANGE.itemsize).view(FLOW_CHANGE)
        r = lib.shdtopo_flow_impact(a._h, b._h, p(s), p(d), p(fl["weight"]), n, p(e), len(e),
                                    p(buf), cap, None, None, None, None, None)
        assert r == total
        assert buf[:cap].tobytes() == exp["records"][:cap].tobytes()
        assert (buf[cap:].view(np.uint8) == 0xFF).all()


# ---- packet route ----
@functools.lru_cache(maxsize=None)
def route_topology():
    ri = route_inputs()
    top, _ = one_topology(len(ri["t"][0]))
    install(top, ri["t"], "copy")
    return top


@pytest.mark.parametrize("clamp", (0, 1))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 4096))
def test_packet_route_on_the_drop_rule(n, clamp):
    ri = route_inputs()
    top = route_topology()
    _, lat, rel, _ = ri["t"]
    s, d = ri["src_col"][:n], ri["dst_col"][:n]
    args = (ri["payload"][:n], ri["state"][:n], ri["now"][:n], ROUTE_JUMP, clamp)
    t, dl, st = route(top, s, d, *args)
    ot, odl, ost = oracle.route_packets(lat[s, d], rel[s, d], *args)
    assert np.array_equal(dl, odl)
    assert np.array_equal(t, ot)
    assert np.array_equal(st, ost)
    assert top.stats()["route_bad_packets"] == 0


# ---- the by-reference lifecycle on a searched graph ----
def test_by_reference_lifecycle():
    import torch
    from shadow_amd import sharding
    top, g = synthetic_pair(n_routers=800, n_poi=40, n_edges=8000)
    _, ips, verts = attach_hosts(top, g, 60)
    top.set_option("lazy", 0)
    to = oracle_table(g, verts)
    a, lat, rel, _ = to
    A = len(a)
    col = {int(v): k for k, v in enumerate(a)}
    host_col = [col[v] for v in verts]

    def check_getters(t, hosts, cols):
        rng = np.random.default_rng(4)
        for x, y in rng.integers(0, len(hosts), (30, 2)):
            want = (t[1][cols[x], cols[y]], t[2][cols[x], cols[y]])
            got = (top.latency_ip(hosts[x], hosts[y]), top.reliability_ip(hosts[x], hosts[y]))
            assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]), (x, y)

    built = lambda: top.stats()["paths_computed"]
    st = sharding.build_distributed(top, 0, 1, "cuda")  # world 1: no process group
    assert built() == A
    assert_table_equal(top, to)
    check_getters(to, ips, host_col)
    assert top.getMinimumLatency() == lat.min()
    assert built() == A  # the bound table answered: no build
    # rows written into the bound buffers: the binding is void, the next getter builds the table
    lr, hops = st.table()
    top.build_rows_into(0, A, lr, hops)
    torch.cuda.synchronize()
    assert built() == 2 * A
    check_getters(to, ips, host_col)
    assert built() == 3 * A  # one whole-table build, then no more
    assert_table_equal(top, to)
    assert top.getMinimumLatency() == lat.min()
    assert built() == 3 * A
    # bound again; rows written elsewhere leave the binding alone
    st = sharding.build_distributed(top, 0, 1, "cuda")
    assert built() == 4 * A
    lr, hops = st.table()
    other = torch.empty_like(lr), torch.empty_like(hops)
    top.build_rows_into(0, A, *other)
    torch.cuda.synchronize()
    assert built() == 5 * A
    assert np.array_equal(other[0].cpu().numpy()[..., 0].view(np.uint64), lat.view(np.uint64))
    check_getters(to, ips, host_col)
    assert_table_equal(top, to)
    assert built() == 5 * A
    lr[0, 0, 0] = 123.0  # (still read in place)
    torch.cuda.synchronize()
    assert top.table()[1][0, 0] == 123.0
    # one more host on a new vertex: the next query builds, it does not read the stale table
    seed = 12345
    while True:
        v, seed = top.attach_ip(host_ip(5000), seed)
        if v not in verts:
            break
        top.detach_ip(host_ip(5000))
    t2 = oracle_table(g, list(verts) + [v])
    col2 = {int(x): k for k, x in enumerate(t2[0])}
    hosts2 = list(ips) + [host_ip(5000)]
    cols2 = [col2[x] for x in list(verts) + [v]]
    got = top.latency_ip(hosts2[0], hosts2[-1])
    assert bits(got) == bits(t2[1][cols2[0], cols2[-1]])
    assert built() == 5 * A + (A + 1)
    check_getters(t2, hosts2, cols2)
    assert_table_equal(top, t2)
    assert top.getMinimumLatency() == t2[1].min()
    assert built() == 5 * A + (A + 1)
