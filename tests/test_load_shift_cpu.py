"""Load shift, host side (no device): shdtopo_load_shift's argument checks, the -4 and -7 that come
before any device is used, the answer for two complete topologies (computed on the host), the
numpy reference of shift_helpers against a plain Python loop, and the properties of the fixtures
the GPU tests (test_load_shift.py) rely on.
"""
import ctypes

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import host_ip, random_topology_graphml
from impact_helpers import check_no_device_used
from load_helpers import ExpectedLoad
from shadow_amd import _lib
from shift_helpers import (CASES, CHANGED, COMPLETE_N, LOAD_CHANGE, M64, assert_shift_equal,
                           complete_flows, complete_graphml, expected_shift, identity, oracle_loads,
                           ring, shift_flows, swapped, words_of)
from whatif_helpers import case, product_attach


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


SMALL = dict(n_routers=100, n_poi=10, extra=200)


def _pair(hosts_b=None, doc_b=None):
    a = sa.Topology.from_buffer(random_topology_graphml(**SMALL))
    b = sa.Topology.from_buffer(random_topology_graphml(**dict(SMALL, **(doc_b or {}))))
    ips, _, _ = product_attach(a, 20)
    product_attach(b, 20, only=hosts_b)
    return a, b, np.array(ips, np.uint32)


def _untouched(*tops):
    for t in tops:
        check_no_device_used(t)
        assert t.stats()["sources"] == 0 and t.stats()["build_ms"] == 0


def _complete(seed=17):
    top = sa.Topology.from_buffer(complete_graphml(seed))
    assert top.is_complete
    for k in range(COMPLETE_N):
        v, _ = top.attach_ip(host_ip(k + 1), 100 + k, typeHint="t%d" % k)
        assert v == k
    return top


def test_bad_arguments_are_refused_before_any_device_is_used():
    lib, _ = _lib.load()
    a, b, ips = _pair()
    s, d = ips[:8].copy(), ips[8:16].copy()
    rec = np.zeros(4, sa.topology.LOAD_CHANGE_DTYPE)
    assert rec.dtype == LOAD_CHANGE and rec.dtype.itemsize == 32
    assert ctypes.sizeof(_lib.ShdLoadChange) == 32

    def call(ta=a._h, tb=b._h, src=_p(s), dst=_p(d), n=len(s), out=None, cap=0):
        return lib.shdtopo_load_shift(ta, tb, src, dst, None, n, out, cap, None)

    assert call(ta=None) == -1 and call(tb=None) == -1
    assert call(n=-1) == -1 and call(n=2**31 - 1) == -1
    assert call(src=None) == -1 and call(dst=None) == -1
    assert call(cap=-1) == -1
    assert call(out=None, cap=4) == -1
    assert lib.shdtopo_load_shift_stats(None, None) == -1
    assert lib.shdtopo_load_shift_stats(a._h, None) == -1
    _untouched(a, b)


def test_unequal_attached_sets_are_refused_before_any_device_is_used():
    """Two topologies of one document, the second with the first 10 hosts only."""
    a, b, ips = _pair(hosts_b=tuple(range(10)))
    assert len(a.attached_vertices()) != len(b.attached_vertices())
    for x, y in ((a, b), (b, a)):
        with pytest.raises(RuntimeError) as e:
            x.load_shift(y, ips[:8], ips[8:16])
        assert e.value.args[1] == -4
    _untouched(a, b)


@pytest.mark.parametrize("doc_b", (dict(n_routers=90), dict(extra=190)), ids=("V", "E"))
def test_other_graphs_are_refused_before_any_device_is_used(doc_b):
    """-7: the vertex counts or the root edge counts differ -- whatever is attached, and for a
    derived topology by its root's count."""
    a, b, ips = _pair(doc_b=doc_b)
    assert (a.num_vertices != b.num_vertices) == ("n_routers" in doc_b)
    assert a.num_edges != b.num_edges
    child = b.without(edges=[3, 5])
    for x, y in ((a, b), (b, a), (a, child), (child, a)):
        with pytest.raises(RuntimeError) as e:
            x.load_shift(y, ips[:8], ips[8:16])
        assert e.value.args[1] == -7
    _untouched(a, b, child)


def test_two_loads_of_one_file_and_a_family_are_accepted():
    """No flow with both ends attached: every load is 0 and no device is needed to say so."""
    a, b, ips = _pair()
    child = a.without(edges=[3, 5])
    grand = child.without(edges=[0])
    assert grand.num_edges == a.num_edges - 3
    none = np.array([host_ip(1000)], np.uint32)
    for x, y in ((a, b), (a, child), (child, a), (a, grand), (grand, child), (child, child)):
        for s, d in ((ips[:0], ips[:0]), (none, ips[:1]), (ips[:1], none)):
            got = x.load_shift(y, s, d)
            assert got["total"] == 0 and len(got["records"]) == 0
            assert (got["flows"], got["unattached"]) == (len(s), len(s))
            assert got["routedA"] == got["routedB"] == 0
            assert got["peakBeforeIndex"] == got["worstGainIndex"] == -1
        st = x.load_shift_stats()
        assert st["entries"] == 2 * a.num_edges + a.num_vertices and st["kernel_ms"] == 0
        assert st["tile_entries"] >= 256 and st["tile_entries"] % 256 == 0
    _untouched(a, b, child, grand)


def test_complete_topologies_are_answered_on_the_host():
    """A complete topology against its empty-set child, and against itself: 0 records, the totals
    of the host's link_load, no device."""
    fl = complete_flows()
    top = _complete()
    child = top.without()
    assert child.is_complete
    load = top.link_load(fl["src_ip"], fl["dst_ip"], weight=fl["weight"])
    lst = top.link_load_stats()
    halves = np.concatenate([load["edge_fwd"], load["edge_rev"]])
    assert lst["routed"] == len(fl["weight"]) - 1 and halves.max() > 0
    for other in (child, top):
        got = top.load_shift(other, fl["src_ip"], fl["dst_ip"], weight=fl["weight"])
        assert got["total"] == 0 and len(got["records"]) == 0
        assert (got["flows"], got["unattached"]) == (len(fl["weight"]), 1)
        assert got["routedA"] == got["routedB"] == lst["routed"]
        assert got["brokenA"] == got["brokenB"] == 0
        assert got["hopWeightA"] == got["hopWeightB"] == lst["hop_weight"]
        assert got["peakBefore"] == got["peakAfter"] == int(halves.max())
        assert got["peakBeforeIndex"] == got["peakAfterIndex"] == int(np.argmax(halves))
        for k in ("changed", "gained", "lost", "newlyUsed", "abandoned", "gainedWeight",
                  "lostWeight"):
            assert not got[k].any(), k
        assert got["displaced"] == got["appeared"] == got["worstGain"] == got["worstLoss"] == 0
        assert got["worstGainIndex"] == got["worstLossIndex"] == -1
        st = top.load_shift_stats()
        assert st["changed"] == 0 and st["kernel_ms"] == 0 and st["bytes_model"] == 0
        assert st["loadA"]["routed"] == st["loadB"]["routed"] == lst["routed"]
        assert st["loadA"]["hop_weight"] == lst["hop_weight"]
    assert top.link_load_stats() == lst  # the shift keeps its own statistics
    _untouched(top, child)


def test_two_complete_topologies_against_the_oracle():
    """The host answer in full: two loads of two complete documents with the same vertices whose
    edges come in another order -- edge identity is the caller's word, so the loads differ."""
    fl = complete_flows()
    tops = [_complete(17), _complete(23)]
    gs = [oracle.OGraph.from_graphml(complete_graphml(seed)) for seed in (17, 23)]
    assert gs[0].E == gs[1].E and not np.array_equal(gs[0].eu, gs[1].eu)
    (ea, eb), un = oracle_loads(fl, gs, fl["src_ip"], fl["dst_ip"], fl["weight"])
    E, V = gs[0].E, gs[0].V
    exp = expected_shift(ea, eb, identity(E), identity(E), E, V, len(fl["weight"]), un)
    assert exp["total"] >= 20 and un == 1
    got = tops[0].load_shift(tops[1], fl["src_ip"], fl["dst_ip"], weight=fl["weight"])
    assert_shift_equal(got, exp)
    assert_shift_equal(tops[1].load_shift(tops[0], fl["src_ip"], fl["dst_ip"], weight=fl["weight"]),
                       swapped(exp))
    for cap in (0, 1, exp["total"], exp["total"] + 1):
        got = tops[0].load_shift(tops[1], fl["src_ip"], fl["dst_ip"], weight=fl["weight"], cap=cap)
        assert_shift_equal(got, exp, cap=cap)
    _untouched(*tops)


def test_numpy_reference_agrees_with_a_plain_loop():
    """The ring, entry by entry in Python integers (sums modulo 2^64)."""
    r = ring()
    exp, ea, eb = r["exp"], r["ea"], r["eb"]
    R, V = r["g"].E, r["g"].V
    origin_b = [e for e in range(R) if r["keep"][e]]
    own_b = {root: e for e, root in enumerate(origin_b)}
    tot = {k: [0, 0, 0] for k in ("changed", "gained", "lost", "newlyUsed", "abandoned",
                                  "gainedWeight", "lostWeight")}
    one = dict(displaced=0, appeared=0, worstGain=0, worstGainIndex=-1, worstLoss=0,
               worstLossIndex=-1, peakBefore=0, peakBeforeIndex=-1, peakAfter=0, peakAfterIndex=-1)
    recs = []
    for x in range(2 * R + V):
        if x >= 2 * R:
            kind, rid = 2, x - 2 * R
            ida = idb = rid
            before, after = int(ea.vertex[rid]), int(eb.vertex[rid])
        else:
            kind, rid = (1, x - R) if x >= R else (0, x)
            ida, idb = rid, own_b.get(rid, -1)
            before = int((ea.edge_rev if kind else ea.edge_fwd)[ida])
            after = int((eb.edge_rev if kind else eb.edge_fwd)[idb]) if idb >= 0 else 0
            if before > one["peakBefore"]:
                one["peakBefore"], one["peakBeforeIndex"] = before, x
            if after > one["peakAfter"]:
                one["peakAfter"], one["peakAfterIndex"] = after, x
        if before == after:
            continue
        recs.append((kind, rid, ida, idb, before, after))
        tot["changed"][kind] += 1
        if after > before:
            tot["gained"][kind] += 1
            tot["gainedWeight"][kind] = (tot["gainedWeight"][kind] + after - before) & M64
            tot["newlyUsed"][kind] += before == 0
            if after - before > one["worstGain"]:
                one["worstGain"], one["worstGainIndex"] = after - before, x
        else:
            tot["lost"][kind] += 1
            tot["lostWeight"][kind] = (tot["lostWeight"][kind] + before - after) & M64
            tot["abandoned"][kind] += after == 0
            if before - after > one["worstLoss"]:
                one["worstLoss"], one["worstLossIndex"] = before - after, x
        if kind < 2 and idb < 0:
            one["displaced"] = (one["displaced"] + before) & M64
        if kind < 2 and ida < 0:
            one["appeared"] = (one["appeared"] + after) & M64
    assert exp["total"] == len(recs) == 1022
    assert [tuple(int(v) for v in rec) for rec in exp["records"]] == recs
    for k, v in tot.items():
        assert [int(y) for y in exp[k]] == v, k
    for k, v in one.items():
        assert int(exp[k]) == v, k
    assert one["displaced"] == 741 and one["worstGainIndex"] >= R  # edge 70 carried both flows
    # the other direction through the helper: the child lacks nothing the parent has
    back = swapped(exp)
    assert back["appeared"] == 741 and back["displaced"] == 0
    assert (back["records"]["idA"] == exp["records"]["idB"]).all()


@pytest.mark.parametrize("name", CASES)
def test_the_cases_exercise_the_shift(name):
    """Conditions on the what-if cases, from the oracle alone, so that no test passes on an empty
    shift; full-range weights, and those reduced to 1..1448."""
    c = case(name)
    full, small = shift_flows(name)["exp"], shift_flows(name, small=True)["exp"]
    X = 2 * c["g"].E + c["g"].V
    assert full["entries"] == small["entries"] == X
    assert full["total"] == CHANGED[name]
    assert full["unattached"] == 5 and full["routedA"] == full["routedB"] == full["flows"] - 5
    if name != "one":
        # the sums wrap with the full range, and do not with the reduced weights
        assert sum(int(w) for w in shift_flows(name)["weight"]) >= 2**64
        assert small["hopWeightA"] < 2**40 and small["hopWeightB"] < 2**40
        assert small["gained"].sum() > 0 and small["lost"].sum() > 0
    rec = full["records"]
    failed = rec[(rec["kind"] < 2) & (rec["idB"] < 0)]
    assert np.isin(failed["id"], c["fail"]).all() and (failed["after"] == 0).all()
    assert (rec["idA"] >= 0).all()
    full_w, empty_w, partial_w = words_of(full)
    if name == "real":
        assert X == 6900
        assert (full["gained"].sum(), full["lost"].sum()) == (401, 418)
        assert (full["newlyUsed"].sum(), full["abandoned"].sum()) == (77, 98)
        assert len(failed) == 16 == 2 * len(c["fail"])  # every failed half carried load
        assert full["changed"].tolist() == [308, 308, 203]
        assert (empty_w, full_w + partial_w) == (1, 107)
    if name == "directed":
        assert full["changed"][1] == 0 and not rec["kind"].tolist().count(1)
        assert (full_w + partial_w, empty_w) == (70, 59)
    if name == "one_router":
        assert 2 * len(c["fail"]) - len(failed) == 18 and empty_w == 25  # idle failed halves
    if name == "int":
        assert small["total"] == 817


def test_the_ring_exercises_the_compaction():
    one, both = ring(), ring(both_ways=True)
    for r in (one, both):
        assert (r["g"].E, r["g"].V, r["exp"]["entries"]) == (516, 514, 1546)
        assert r["g2"].is_strongly_connected()
        assert set(r["ea"].hops.tolist()) == {202, 1} and set(r["eb"].hops.tolist()) == {314, 1}
    exp = one["exp"]
    assert exp["total"] == 1022 and words_of(exp) == (13, 7, 5)
    flag = exp["before"] != exp["after"]
    assert not flag[256:512].any() and flag[:192].all()  # an aligned 256-entry run, full words
    assert both["exp"]["total"] == 1534 and words_of(both["exp"])[0] == 21


def test_the_complete_graph_is_complete():
    g = oracle.OGraph.from_graphml(complete_graphml())
    assert g.is_complete() and g.V == COMPLETE_N and g.E == COMPLETE_N * (COMPLETE_N + 1) // 2
    # the direct edge is the only shortest route: Dijkstra's route is the complete branch's
    fl = complete_flows()
    (ex,), un = oracle_loads(fl, (g,), fl["src_ip"], fl["dst_ip"], fl["weight"])
    assert un == 1 and set(ex.hops.tolist()) == {1}
    assert isinstance(ex, ExpectedLoad)
