"""Load shift on the GPU (shdtopo_load_shift, topo_shift.hip): where a link failure moves the
traffic of a set of flows -- two link loads left on the device and compared there, entry by entry,
in the root topology's numbering.

Reference: the CPU oracle alone (shift_helpers.expected_shift: load_helpers.ExpectedLoad on the
parent graph and on the filtered graph, np.flatnonzero(keep) as the origin map), computed once per
case and shared.  Every sum is a u64 that wraps, so every comparison is exact.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import host_ip
from impact_helpers import impact_flows
from shadow_amd import _lib
from shift_helpers import (CASES, COMPLETE_N, LOAD_CHANGE, M64, assert_shift_equal,
                           assert_totals_equal, complete_flows, complete_graphml, expected_shift,
                           identity, oracle_loads, ring, shift_flows, swapped)
from whatif_helpers import build_counters, case, failing_set, filtered, product

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def pair(name):
    """The product's parent and child of a case, made once (the shift leaves both as they were)."""
    top = product(name)
    return top, top.without(edges=case(name)["fail"])


@functools.lru_cache(maxsize=None)
def ring_pair():
    r = ring()
    top = sa.Topology.from_buffer(r["data"])
    for k, ip in enumerate(r["ips"]):
        assert top.attach_ip(ip, 100 + k, typeHint="t%d" % k)[0] == r["verts"][k]
    return top, top.without(edges=r["fail"])


def run(a, b, fl, **kw):
    return a.load_shift(b, fl["src_ip"], fl["dst_ip"], weight=fl["weight"], **kw)


def same_bytes(x, y):
    assert x["records"].tobytes() == y["records"].tobytes()
    assert_totals_equal(x, y)


def check_identity(got):
    """What the edge halves gain less what they lose is what the routes grew by."""
    net = sum(int(v) for v in got["gainedWeight"][:2]) - sum(int(v) for v in got["lostWeight"][:2])
    assert net & M64 == (int(got["hopWeightB"]) - int(got["hopWeightA"])) & M64


@pytest.mark.parametrize("small", (False, True), ids=("full", "small"))
@pytest.mark.parametrize("name", CASES)
def test_shift_matches_the_oracle(name, small):
    c, fl = case(name), shift_flows(name, small)
    exp = fl["exp"]
    top, child = pair(name)
    got = run(top, child, fl)
    assert_shift_equal(got, exp, what=name)
    check_identity(got)
    rec, R = got["records"], c["g"].E
    x = np.where(rec["kind"] == 2, 2 * R, rec["kind"].astype(np.int64) * R) + rec["id"]
    assert (np.diff(x) > 0).all()  # ascending x
    # ids in the root's numbering: the child's own id leads back to it through edge_origin
    kept = rec[(rec["kind"] < 2) & (rec["idB"] >= 0)]
    assert np.array_equal(child.edge_origin()[kept["idB"]], kept["id"])
    st = top.load_shift_stats()
    assert st["entries"] == 2 * c["g"].E + c["g"].V and st["changed"] == exp["total"]
    assert st["kernel_ms"] > 0 and st["total_ms"] >= st["load_a_ms"] + st["load_b_ms"]
    assert st["loadA"]["routed"] == exp["routedA"] and st["loadB"]["routed"] == exp["routedB"]
    assert st["loadA"]["hop_weight"] == exp["hopWeightA"]
    assert st["loadB"]["hop_weight"] == exp["hopWeightB"]
    assert st["bytes_model"] > 0 and 0 <= st["words_skipped"] <= (st["entries"] + 63) // 64


@pytest.mark.parametrize("both_ways", (False, True), ids=("one_way", "both_ways"))
def test_ring(both_ways):
    r = ring(both_ways)
    top, child = ring_pair()
    got = run(top, child, r)
    assert_shift_equal(got, r["exp"])
    check_identity(got)
    assert_shift_equal(run(child, top, r), swapped(r["exp"]))
    # the fill pass loads for the words that have a change, and for no other
    st = top.load_shift_stats()
    flag = r["exp"]["before"] != r["exp"]["after"]
    flag = np.append(flag, np.zeros(-len(flag) % 64, bool)).reshape(-1, 64)
    assert st["words_skipped"] == int((~flag.any(axis=1)).sum())


def caps_of(exp, T):
    """0, 1, a word boundary and a tile boundary -- as numbers, and as the ranks at which a word
    and a tile begin -- the total and one more."""
    flag = exp["before"] != exp["after"]
    total = exp["total"]
    below = lambda x: int(flag[:x].sum())
    caps = {0, 1, 64, T, total, total + 1}
    # the rank at which a word in the middle begins (one with records before it and in it), and
    # the ranks at which the tiles begin
    words = [below(64 * k) for k in range(1, len(flag) // 64)
             if flag[64 * k:64 * k + 64].any() and 0 < below(64 * k)]
    caps.add(words[len(words) // 2])
    tiles = [below(T * k) for k in range(1, (len(flag) + T - 1) // T)]
    caps |= {tiles[0], tiles[len(tiles) // 2]}
    return sorted(caps)


@pytest.mark.parametrize("which", ("real", "ring"))
def test_cap(which):
    if which == "real":
        fl, (top, child) = shift_flows("real", small=True), pair("real")
    else:
        fl, (top, child) = ring(), ring_pair()
    exp = fl["exp"]
    total = exp["total"]
    run(top, child, fl, cap=0)
    T = top.load_shift_stats()["tile_entries"]
    assert T >= 256 and T % 256 == 0 and exp["entries"] > T + 1
    lib, _ = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    caps = caps_of(exp, T)
    assert {0, 1, total, total + 1} <= set(caps) and len(caps) >= 7
    for cap in caps:
        # through the C ABI: exactly that prefix, the sentinel behind it untouched
        buf = np.full(total + 2, 0xFF, np.uint8).repeat(LOAD_CHANGE.itemsize).view(LOAD_CHANGE)
        tt = _lib.ShdShiftTotals()
        r = lib.shdtopo_load_shift(top._h, child._h, p(fl["src_ip"]), p(fl["dst_ip"]),
                                   p(fl["weight"]), len(fl["weight"]), p(buf) if cap else None,
                                   cap, ctypes.byref(tt))
        assert r == total, cap
        n = min(cap, total)
        assert buf[:n].tobytes() == exp["records"][:n].tobytes(), cap
        assert (buf[n:].view(np.uint8) == 0xFF).all(), cap
        assert list(tt.changed) == [int(v) for v in exp["changed"]], cap
        assert tt.worstGain == exp["worstGain"] and tt.peakAfterIndex == exp["peakAfterIndex"]
        # ... and through the binding: the totals are complete whatever cap is
        assert_shift_equal(run(top, child, fl, cap=cap), exp, cap=cap, what=cap)
        if cap == 0:
            assert top.load_shift_stats()["words_skipped"] == (exp["entries"] + 63) // 64


def test_direction():
    fl = shift_flows("real", small=True)
    top, child = pair("real")
    back = run(child, top, fl)
    assert_shift_equal(back, swapped(fl["exp"]))
    check_identity(back)
    fwd = fl["exp"]["records"]
    assert np.array_equal(back["records"]["before"], fwd["after"])
    assert np.array_equal(back["records"]["idA"], fwd["idB"])
    assert back["appeared"] == fl["exp"]["displaced"] > 0 and back["displaced"] == 0
    assert child.load_shift_stats()["changed"] == fl["exp"]["total"]  # kept by the first argument


def test_order_independence_and_repeatability():
    fl = shift_flows("real")
    top, child = pair("real")
    first = run(top, child, fl)
    assert_shift_equal(first, fl["exp"])
    same_bytes(run(top, child, fl), first)
    perm = np.random.default_rng(31).permutation(len(fl["weight"]))
    shuffled = {k: fl[k][perm] for k in ("src_ip", "dst_ip", "weight")}
    same_bytes(run(top, child, shuffled), first)


OPTIONS = (("a", "load_walk", 0), ("b", "load_walk", 0), ("ab", "trace_chunk", 3),
           ("a", "trace_batch", 0), ("b", "trace_batch", 0))


@pytest.mark.parametrize("side,option,value", OPTIONS, ids=["%s-%s" % o[:2] for o in OPTIONS])
def test_each_side_uses_its_own_options(side, option, value):
    c, fl = case("real"), shift_flows("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    for s, t in (("a", top), ("b", child)):
        if option == "trace_batch":
            t.table()  # the batch kernel's records serve a load only once a table was built
        if s in side:
            t.set_option(option, value)
    got = run(top, child, fl)
    assert_shift_equal(got, fl["exp"])
    same_bytes(got, run(*pair("real"), fl))
    st = top.load_shift_stats()
    if option == "load_walk":
        assert (st["loadA"]["tree_vertices"] > 0) == ("a" in side)
        assert (st["loadB"]["tree_vertices"] > 0) == ("b" in side)
    if option == "trace_chunk":
        assert st["loadA"]["chunks"] > 1 and st["loadB"]["chunks"] > 1
    if option == "trace_batch":
        ran = lambda ls: ls["batch_sources"] + ls["batch_fallback"] > 0  # a keep launch
        assert ran(st["loadA"]) == ("a" not in side)
        assert ran(st["loadB"]) == ("b" not in side)


@pytest.mark.parametrize("walk", (1, 0))
def test_tie_dense_graph_both_load_paths(walk):
    c, fl = case("int"), shift_flows("int", small=True)
    top = product("int")
    child = top.without(edges=c["fail"])
    for t in (top, child):
        t.set_option("load_walk", walk)
    assert_shift_equal(run(top, child, fl), fl["exp"])


def test_failed_vertex():
    """A router that carries traffic fails: its vertex entry drops to 0 and every incident half
    that carried something is an edge the child lacks."""
    c, fl = case("real"), shift_flows("real", small=True)
    g = c["g"]
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    routers = [int(v) for v in np.argsort(-fl["ea"].vertex.astype(np.float64), kind="stable")
               if g.vattrs["id"][v].startswith("pop-")]
    for v in routers:  # the busiest router whose failure leaves the other vertices connected
        g2, keep = filtered(g, fail_vertices=[v])
        adj = coo_matrix((np.ones(g2.E), (g2.eu, g2.ev)), shape=(g.V, g.V))
        if connected_components(adj, directed=False)[0] == 2:  # the rest, and v alone
            break
    touched = np.flatnonzero((g.eu == v) | (g.ev == v))
    assert fl["ea"].vertex[v] > 0 and len(touched) >= 3
    (eb,), un = oracle_loads(c, (g2,), fl["src_ip"], fl["dst_ip"], fl["weight"])
    exp = expected_shift(fl["ea"], eb, identity(g.E), np.flatnonzero(keep), g.E, g.V,
                         len(fl["weight"]), un)
    top, _ = pair("real")
    child = top.without(vertices=[int(v)])
    got = run(top, child, fl)
    assert_shift_equal(got, exp)
    rec = got["records"]
    at = rec[(rec["kind"] == 2) & (rec["id"] == v)]
    assert len(at) == 1 and at["after"][0] == 0 and at["before"][0] == fl["ea"].vertex[v]
    lacking = rec[(rec["kind"] < 2) & (rec["idB"] < 0)]
    assert len(lacking) >= 2 and np.isin(lacking["id"], touched).all()
    assert (lacking["after"] == 0).all() and got["displaced"] == exp["displaced"] > 0


def test_a_derivation_of_a_derivation_and_siblings():
    """Ids are the root's whatever the two sides are: child against grandchild, root against
    grandchild, two siblings."""
    c, fl = case("real"), shift_flows("real", small=True)
    g, ea = c["g"], fl["ea"]
    f1 = c["fail"]
    f2 = np.setdiff1d(failing_set(g, 12), f1)  # the next four of the recipe (root ids)
    assert len(f1) == 8 and len(f2) == 4
    g1, keep1 = filtered(g, f1)
    o1 = np.flatnonzero(keep1)
    f2_in_1 = np.searchsorted(o1, f2)  # the child's ids of f2
    assert np.array_equal(o1[f2_in_1], f2)
    g12, keep12 = filtered(g1, f2_in_1)
    o12 = o1[np.flatnonzero(keep12)]
    gs, keeps = filtered(g, f2)
    os_ = np.flatnonzero(keeps)
    assert g12.is_strongly_connected() and gs.is_strongly_connected()
    (e1, e12, es), un = oracle_loads(c, (g1, g12, gs), fl["src_ip"], fl["dst_ip"], fl["weight"])
    n = len(fl["weight"])
    top, child = pair("real")
    grand = child.without(edges=f2_in_1)
    sib = top.without(edges=f2)
    assert np.array_equal(grand.edge_origin(), o12) and np.array_equal(sib.edge_origin(), os_)
    o0 = identity(g.E)
    sides = {"child-grandchild": (child, grand, e1, e12, o1, o12),
             "root-grandchild": (top, grand, ea, e12, o0, o12),
             "siblings": (child, sib, e1, es, o1, os_),
             "grandchild-root": (grand, top, e12, ea, o12, o0)}
    for what, (a, b, xa, xb, oa, ob) in sides.items():
        exp = expected_shift(xa, xb, oa, ob, g.E, g.V, n, un)
        assert exp["total"] >= 30, what
        if what == "siblings":  # they lack different edges: halves appear, halves are displaced
            assert exp["displaced"] > 0 and exp["appeared"] > 0
            assert (exp["records"]["idA"] < 0).any() and (exp["records"]["idB"] < 0).any()
        got = run(a, b, fl)
        assert_shift_equal(got, exp, what=what)
        check_identity(got)


def test_identical_child_and_the_same_topology():
    fl = shift_flows("real", small=True)
    exp = fl["exp"]
    top, _ = pair("real")
    same = top.without()
    for other in (same, top):
        got = run(top, other, fl)
        assert got["total"] == 0 and len(got["records"]) == 0
        assert (got["flows"], got["unattached"]) == (exp["flows"], 5)
        assert got["routedA"] == got["routedB"] == exp["routedA"]
        assert got["hopWeightA"] == got["hopWeightB"] == exp["hopWeightA"]
        assert got["peakBefore"] == got["peakAfter"] == exp["peakBefore"] > 0
        assert got["peakBeforeIndex"] == got["peakAfterIndex"] == exp["peakBeforeIndex"]
        for k in ("changed", "gained", "lost", "newlyUsed", "abandoned", "gainedWeight",
                  "lostWeight"):
            assert not got[k].any(), k
        assert got["displaced"] == got["appeared"] == got["worstGain"] == got["worstLoss"] == 0
        assert got["worstGainIndex"] == got["worstLossIndex"] == -1
        st = top.load_shift_stats()
        assert st["words_skipped"] == (st["entries"] + 63) // 64 and st["kernel_ms"] > 0
        assert (st["load_b_ms"] == 0) == (other is top)
        assert st["loadA"]["routed"] == st["loadB"]["routed"] == exp["routedA"]


def test_a_complete_parent_and_its_sssp_child():
    """One edge of a complete topology fails: the child is no longer complete, and the direct
    edge's load moves to a two-hop route.  The parent is accumulated on the host and uploaded."""
    fl = complete_flows()
    g = oracle.OGraph.from_graphml(complete_graphml())
    e = int(np.flatnonzero(g.eu != g.ev)[0])
    g2, keep = filtered(g, [e])
    top = sa.Topology.from_buffer(complete_graphml())
    for k in range(COMPLETE_N):
        assert top.attach_ip(host_ip(k + 1), 100 + k, typeHint="t%d" % k)[0] == k
    child = top.without(edges=[e])
    assert top.is_complete and not child.is_complete
    (ea, eb), un = oracle_loads(fl, (g, g2), fl["src_ip"], fl["dst_ip"], fl["weight"])
    exp = expected_shift(ea, eb, identity(g.E), np.flatnonzero(keep), g.E, g.V,
                         len(fl["weight"]), un)
    assert set(ea.hops.tolist()) == {1} and set(eb.hops.tolist()) == {1, 2}
    assert exp["displaced"] > 0 and exp["newlyUsed"][2] == 0 and exp["gained"][2] == 1
    got = run(top, child, fl)
    assert_shift_equal(got, exp)
    check_identity(got)
    assert_shift_equal(run(child, top, fl), swapped(exp))
    assert top.load_shift_stats()["loadA"]["sources"] == 0  # (the host path groups nothing)


def test_errors_and_side_effects():
    c, fl = case("real"), shift_flows("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    ips = np.array(c["ips"], np.uint32)
    # a first build, one call of every kind and a lazy row on both
    small = impact_flows("real")
    for t in (top, child):
        assert t.latency_ip(int(ips[0]), int(ips[1])) > 0
        t.trace_routes(ips[:8], ips[8:16])
        t.link_load(ips[:8], ips[8:16])
        t.link_crossings(ips[:8], ips[8:16], edges=[0, 1])
        t.link_timeline(ips[:8], ips[8:16], edges=[0, 1], nbins=4)
    top.table_diff(child)
    child.table_diff(top)
    top.flow_impact(child, small["src_ip"][:64], small["dst_ip"][:64])
    child.flow_impact(top, small["src_ip"][:64], small["dst_ip"][:64])
    state = lambda t: (t.stats(), t.trace_stats(), t.link_load_stats(), t.link_crossings_stats(),
                       t.link_timeline_stats(), t.table_diff_stats(), t.flow_impact_stats(),
                       [x.tolist() for x in t.lazy_rows()], t.lazyMinimumLatency())
    snaps = [state(top), state(child)]
    assert_shift_equal(run(top, child, fl), fl["exp"])
    assert_shift_equal(run(child, top, fl), swapped(fl["exp"]))
    assert run(top, top, fl)["total"] == 0
    assert [state(top), state(child)] == snaps
    # one more host on a vertex that was no column: the attached lists differ
    st = 12345
    while True:
        v, st = child.attach_ip(host_ip(5000), st)
        if v not in c["verts"]:
            break
    with pytest.raises(RuntimeError) as e:
        run(top, child, fl)
    assert e.value.args[1] == -4


def test_no_table_is_built():
    fl = shift_flows("real")
    c = case("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    assert_shift_equal(run(top, child, fl), fl["exp"])
    for t in (top, child):
        built = build_counters(t)
        assert built["build_ms"] == 0 and built["paths_computed"] == 0


def test_link_load_is_what_it_was():
    """link_load on parent and child gives the same bytes before and after a shift: the two share
    the accumulation and the replay's slots."""
    c, fl = case("real"), shift_flows("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    load = lambda t: t.link_load(fl["src_ip"], fl["dst_ip"], weight=fl["weight"])
    key = lambda out: (out["edge_fwd"].tobytes(), out["edge_rev"].tobytes(),
                       out["vertex"].tobytes(), out["routed"])
    counters = ("requests", "routed", "unattached", "broken", "sources", "chunks",
                "tree_vertices", "hop_weight", "batch_sources", "batch_fallback")
    before = [(key(load(t)), {k: t.link_load_stats()[k] for k in counters}) for t in (top, child)]
    assert_shift_equal(run(top, child, fl), fl["exp"])
    after = [(key(load(t)), {k: t.link_load_stats()[k] for k in counters}) for t in (top, child)]
    assert before == after
    # ... and they are the oracle's
    for (k, st), ex in zip(after, (fl["ea"], fl["eb"])):
        assert k == (ex.edge_fwd.tobytes(), ex.edge_rev.tobytes(), ex.vertex.tobytes(), ex.routed)
        assert st["hop_weight"] == ex.hop_weight & M64
