"""GPU parity across latency domains (helpers.LATENCY_DOMAINS): the reader, the table (batch kernel
and heap replay), route traces, link loads, link crossings, the packet kernel and the lazy getters
on graphs whose latencies are decimal (k/10: bitwise ties next to near misses), dyadic (k/4,
integers x 2^-30: exact ties that are no integers), spread over eight decades (logu), bimodal
around the f16 range of the kappa fields, or today's distributions moved by 2^-30, 2^30 and 1e-3.

Every graph is helpers.domain_graphml: 3,000 routers, 15,000 extra edges, 100 poi, 120 hosts --
the smallest on which the batch kernel's tail paths still run once lds_hubs is 0.  Expected values
come from the CPU oracle alone (helpers.domain_oracle, computed once per graph and shared, never
modified; test_latency_domains_cpu.py shows what each domain holds); the power-of-two metamorphism
needs no oracle at all.  No assertion counts ties the oracle cannot derive.
"""
import functools

import numpy as np
import pytest

import shadow_amd as sa
from crossing_helpers import ExpectedCrossings, check_crossings, check_stats, watch_recipe
from helpers import (DOMAIN_HOSTS, TIE_FREE_DOMAINS, attach_hosts, domain_graphml, domain_oracle)
from load_helpers import ExpectedLoad, all_pairs, check_load
from test_trace import Expected, check_routes, check_table

pytestmark = pytest.mark.gpu

DOMAINS = ("dec", "quarter", "logu", "bimodal", "real_dn30", "real_up30", "int_dn30", "real_milli")
NON_INTEGER_TIES = ("dec", "quarter", "int_dn30")
HINTS = ("client", "relay", "server")
NSRC = 5


def product(domain, directed, options=()):
    """The product's topology of a domain graph with the oracle's hosts attached (the stream of
    helpers.attach_hosts; every host must land on the oracle's vertex).
    Returns (top, g, ips, verts, oracle table)."""
    top = sa.Topology.from_buffer(domain_graphml(domain, directed))
    assert top is not None and top.is_directed == directed and not top.is_complete
    for k, v in options:
        top.set_option(k, v)
    g, ips, verts, tab = domain_oracle(domain, directed)
    st = 1
    for k in range(DOMAIN_HOSTS):
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        v, _ = top.attach_ip(ips[k], st, typeHint=HINTS[k % 3])
        assert v == verts[k], (k, v, verts[k])
    return top, g, np.asarray(ips, np.uint32), np.asarray(verts, np.int32), tab


def bits_equal(got, want):
    (a, lat, rel, hops), (oa, olat, orel, ohops) = got, want
    assert np.array_equal(a, oa)
    assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64))
    assert np.array_equal(rel.view(np.uint64), orel.view(np.uint64))
    assert np.array_equal(hops, ohops.astype(np.uint16))


# ------------------------------------------------------------------------------------------
# 1. the reader
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("domain", DOMAINS)
def test_reader_parses_every_domain_bit_for_bit(domain, directed):
    """repr strings with exponents (4.6566128730773926e-09), twelve-digit values (x 2^30) and plain
    decimals: the product's arrays equal the oracle's ElementTree + float() parse bit for bit."""
    data = domain_graphml(domain, directed)
    if domain in ("real_dn30", "int_dn30"):
        assert b"e-0" in data  # exponents in the document
    top = sa.Topology.from_buffer(data)
    g = domain_oracle(domain, directed)[0]
    V, eu, ev, elat, eloss, vloss = top.export_graph()
    assert V == g.V and np.array_equal(eu, g.eu) and np.array_equal(ev, g.ev)
    assert np.array_equal(elat.view(np.uint64), g.elat.view(np.uint64))
    assert np.array_equal(eloss.view(np.uint64), g.eloss.view(np.uint64))
    assert np.array_equal(vloss.view(np.uint64), g.vloss.view(np.uint64))


# ------------------------------------------------------------------------------------------
# 2. the table through the batch kernel (flagged rows through the replay)
# ------------------------------------------------------------------------------------------
BATCH_CASES = [(d, dr, None) for d in DOMAINS for dr in (False, True)]
BATCH_CASES += [(d, dr, 0) for d in ("dec", "logu", "bimodal") for dr in (False, True)]


@pytest.mark.parametrize("domain,directed,hubs", BATCH_CASES)
def test_table_batch_path(domain, directed, hubs):
    """Latency, reliability and hops of every pair bit for bit the oracle's, with the default
    number of LDS-resident distance rows or none (lds_hubs = 0: every vertex on the tail paths)."""
    opts = [("tie_dense", 0)] + ([("lds_hubs", hubs)] if hubs is not None else [])
    top, g, ips, verts, tab = product(domain, directed, opts)
    got = top.table()
    st = top.stats()
    assert st["errors"] == 0
    assert st["sssp_kernel_ms"] > 0  # the batch kernel ran
    bits_equal(got, tab)
    assert top.getMinimumLatency() == tab[1].min()
    if domain in TIE_FREE_DOMAINS:
        assert st["ambiguous_pairs"] == 0 and st["replay_rows"] == 0
    if domain in NON_INTEGER_TIES:
        assert st["replay_int_keys"] == 0


# ------------------------------------------------------------------------------------------
# 3. the table through the replay alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("domain", ["dec", "quarter", "bimodal", "int_dn30"])
def test_table_replay_alone(domain, directed):
    """replay_all = 1 (f64 heap keys: no domain here is integer): bit-exact against the oracle and
    equal to the batch path's table of the same topology."""
    top, g, ips, verts, tab = product(domain, directed, [("tie_dense", 0)])
    batch = top.table()
    assert top.stats()["errors"] == 0
    top.set_option("replay_all", 1)
    top.rebuild()
    got = top.table()
    st = top.stats()
    assert st["errors"] == 0 and st["replay_rows"] == len(got[0])
    assert st["replay_int_keys"] == 0
    bits_equal(got, tab)
    for x, y in zip(got, batch):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------
# 4. power-of-two metamorphism (no oracle)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("base", ["real", "int"])
def test_power_of_two_metamorphism(base, directed):
    """Every latency times 2^k scales every f64 sum exactly (no overflow, no subnormal at k = -30,
    +30): the same parents, so hops and reliability are bit-identical and latency is the base
    latency times 2^k exactly.  And the bucket width (option delta, at mean / 64 and mean x 8)
    changes only the order of the work, never the table."""
    top, g, ips, verts, tab = product(base, directed, [("tie_dense", 0)])
    a0, lat0, rel0, hops0 = top.table()
    assert top.stats()["errors"] == 0
    for tag, k in (("_dn30", -30), ("_up30", 30)):
        t2 = product(base + tag, directed, [("tie_dense", 0)])[0]
        a, lat, rel, hops = t2.table()
        assert t2.stats()["errors"] == 0
        assert np.array_equal(a, a0)
        assert np.array_equal(lat.view(np.uint64), (lat0 * 2.0 ** k).view(np.uint64)), k
        assert np.array_equal(rel.view(np.uint64), rel0.view(np.uint64)), k
        assert np.array_equal(hops, hops0), k
    nl = g.eu != g.ev
    mean = float(g.elat[nl].mean())
    for delta in (mean / 64, mean * 8):
        top.set_option("delta", delta)
        top.rebuild()
        a, lat, rel, hops = top.table()
        assert top.stats()["errors"] == 0
        assert lat.tobytes() == lat0.tobytes() and rel.tobytes() == rel0.tobytes(), delta
        assert np.array_equal(hops, hops0), delta


# ------------------------------------------------------------------------------------------
# 5. routes, loads and crossings
# ------------------------------------------------------------------------------------------
FLOW_CASES = [(d, dr) for d in ("dec", "quarter", "bimodal") for dr in (False, True)]


def flow_weights(n):
    return np.random.default_rng(33).integers(1, 2**40, n, endpoint=True).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def flows_expected(domain, directed):
    """The first NSRC hosts as sources to every host, from the oracle: (Expected routes,
    ExpectedLoad, ExpectedCrossings, watched edges, watched vertices, distinct source vertices)."""
    g, ips, verts, tab = domain_oracle(domain, directed)
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    sip, dip, sv, dv = all_pairs(ips, verts, NSRC)
    w = flow_weights(len(sv))
    routes = Expected(g, sv, dv, verts)
    load = ExpectedLoad(g, sv, dv, w, verts)
    edges, vertices = watch_recipe(load, sv, dv)
    xc = ExpectedCrossings(g, load, w, edges, vertices)
    return routes, load, xc, edges, vertices, len(set(int(v) for v in verts[:NSRC]))


@pytest.fixture(scope="module")
def flows_topology():
    """One built topology per graph, shared by the three tests below (each restores the options
    it changes) and freed with the module."""
    built = {}

    def get(domain, directed):
        if (domain, directed) not in built:
            top, g, ips, verts, tab = product(domain, directed, [("tie_dense", 0)])
            bits_equal(top.table(), tab)
            built[domain, directed] = top, ips, verts
        return built[domain, directed]
    yield get
    for top, _, _ in built.values():
        top.free()


@pytest.mark.parametrize("domain,directed", FLOW_CASES)
def test_routes(flows_topology, domain, directed):
    """shdtopo_trace_routes, NSRC x 120 requests: vertices, edges, hops, latency and reliability
    equal the oracle's chains, from the batch kernel's pair records (trace_batch = 1) and from
    the replay (0)."""
    top, ips, verts = flows_topology(domain, directed)
    sip, dip, sv, dv = all_pairs(ips, verts, NSRC)
    routes, _, _, _, _, nsrc = flows_expected(domain, directed)
    for tb in (1, 0):
        top.set_option("trace_batch", tb)
        try:
            tr = top.trace_routes(sip, dip)
            ts = top.trace_stats()
        finally:
            top.set_option("trace_batch", 1)
        check_routes(tr, routes)
        check_table(top, tr, sv, dv)
        assert ts["sources"] == nsrc and ts["requests"] == len(sip)
        if tb == 0:
            assert ts["batch_sources"] == 0 and ts["batch_fallback"] == 0
        else:
            assert ts["batch_sources"] + ts["batch_fallback"] == nsrc
            if domain in TIE_FREE_DOMAINS:  # no row crosses a tie: every source from the records
                assert ts["batch_sources"] == nsrc


@pytest.mark.parametrize("walk", [1, 0])
@pytest.mark.parametrize("domain,directed", FLOW_CASES)
def test_link_load(flows_topology, domain, directed, walk):
    top, ips, verts = flows_topology(domain, directed)
    sip, dip, sv, dv = all_pairs(ips, verts, NSRC)
    _, load, _, _, _, nsrc = flows_expected(domain, directed)
    top.set_option("load_walk", walk)
    try:
        out = top.link_load(sip, dip, flow_weights(len(sip)))
        ls = top.link_load_stats()
    finally:
        top.set_option("load_walk", 1)
    check_load(out, load)
    assert ls["routed"] == len(sip) and ls["broken"] == 0 and ls["unattached"] == 0
    assert ls["sources"] == nsrc and ls["hop_weight"] == load.hop_weight


@pytest.mark.parametrize("domain,directed", FLOW_CASES)
def test_link_crossings(flows_topology, domain, directed):
    top, ips, verts = flows_topology(domain, directed)
    sip, dip, sv, dv = all_pairs(ips, verts, NSRC)
    _, load, xc, edges, vertices, nsrc = flows_expected(domain, directed)
    assert xc.total > 0 and xc.flows_with_several() > 0  # the watches are crossed
    out = top.link_crossings(sip, dip, edges, vertices, flow_weights(len(sip)))
    check_crossings(out, xc)
    check_stats(top.link_crossings_stats(), xc, sources=nsrc)


# ------------------------------------------------------------------------------------------
# 6. packets
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", ["bimodal", "real_dn30", "real_up30"])
def test_packets(domain):
    """20,000 seeded packets through packet_route_kernel on the built table against the oracle's
    worker_schedulePacket: delivery time, drop flag and next RNG state, clamp on, jump 1 ms.
    Delays below 1 ns (x 2^-30: ceil gives 1 ns, every delivery clamps to now + jump) and near
    4e17 ns (x 2^30: no delivery clamps)."""
    import torch

    import oracle
    top, g, ips, verts, tab = product(domain, False, [("tie_dense", 0)])
    a, lat, rel, hops = got = top.table()
    bits_equal(got, tab)
    A = len(a)
    rng = np.random.default_rng(5)
    n = 20_000
    jump = 1_000_000
    src = rng.integers(0, A, n).astype(np.int32)
    dst = rng.integers(0, A, n).astype(np.int32)
    pay = np.where(rng.random(n) < 0.8, 1448, 0).astype(np.uint32)
    sin = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    now = rng.integers(10**9, 2 * 10**9, n).astype(np.uint64)
    dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                                     (x.view(np.int32) if x.dtype == np.uint32 else x)).cuda()
    t_out = torch.empty(n, dtype=torch.int64, device="cuda")
    s_out = torch.empty(n, dtype=torch.int32, device="cuda")
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    top.route_batch_device(dev(src), dev(dst), dev(pay), dev(sin), dev(now), jump, 1, t_out,
                           s_out, d_out)
    torch.cuda.synchronize()
    t = t_out.cpu().numpy().view(np.uint64)
    ot, od, os_ = oracle.route_packets(lat[src, dst], rel[src, dst], pay, sin, now, jump, 1)
    assert np.array_equal(d_out.cpu().numpy(), od)
    assert np.array_equal(t, ot)
    assert np.array_equal(s_out.cpu().numpy().view(np.uint32), os_)
    sent = od == 1
    assert 0 < sent.mean() < 1
    ut, _, _ = oracle.route_packets(lat[src, dst], rel[src, dst], pay, sin, now, jump, 0)
    clamped = sent & (ut != ot)
    if domain == "real_dn30":
        assert lat.max() * 1e6 < 1.0  # every delay is ceil(< 1 ns) = 1 ns
        assert np.array_equal(t[sent], now[sent] + np.uint64(jump)) and clamped[sent].all()
    elif domain == "real_up30":
        assert not clamped.any()
        assert (t[sent] - now[sent]).min() > jump and (t[sent] - now[sent]).max() > 10**17
    else:
        assert clamped.any() and (sent & ~clamped).any()


# ------------------------------------------------------------------------------------------
# 7. lazy getters
# ------------------------------------------------------------------------------------------
def test_lazy_getters_decimal_domain():
    """topology_getLatency / getReliability against the reference's lazy two-level cache on one
    query sequence over the decimal graph, with the running minimum's trajectory."""
    top = sa.Topology.from_buffer(domain_graphml("dec", False))
    g = domain_oracle("dec", False)[0]
    otop, ips, verts = attach_hosts(top, g, DOMAIN_HOSTS, type_hints=list(HINTS))  # its own cache
    assert tuple(verts) == domain_oracle("dec", False)[2]
    shim = sa.topology.shim()
    shim.shim_reset()
    rng = np.random.default_rng(21)
    addrs = {ip: sa.Address(ip) for ip in ips}
    for q in range(300):
        x, y = (int(v) for v in rng.choice(ips, 2))
        assert top.getLatency(addrs[x], addrs[y]) == otop.get_latency(x, y), q
        assert top.getReliability(addrs[x], addrs[y]) == otop.get_reliability(x, y), q
        assert top.lazyMinimumLatency() == otop.minimum_path_latency, q
    assert shim.shim_last_min_latency() == otop.minimum_path_latency
    assert len(otop.min_updates) >= 1
