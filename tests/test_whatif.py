"""Link-failure what-if on the GPU: the table of a derived topology (shdtopo_derive_without) and
the device-side table diff (shdtopo_table_diff, topo_diff.hip).

References: the oracle's table of the filtered edge arrays for the derived table, numpy on the two
oracle tables for the diff (whatif_helpers.expected_diff).  The oracle tables of every case are
computed once (whatif_helpers.case) and shared.
"""
import ctypes

import numpy as np
import pytest

import shadow_amd as sa
from helpers import host_ip
from shadow_amd import _lib
from whatif_helpers import (CHANGE, FELL, ROSE, assert_diff_equal, assert_table_equal,
                            attach_off_column, build_counters, case, expected_diff, filtered,
                            product, swapped)

pytestmark = pytest.mark.gpu

RECIPE = ("real", "int", "directed", "logu")   # the four graphs of the recipe
PARITY = ("real", "int", "directed", "parallel")


@pytest.mark.parametrize("name", RECIPE)
def test_inputs_exercise_the_diff(name):
    """Conditions on the input, from the oracle alone."""
    exp = case(name)["exp"]
    assert exp["total"] >= 100
    assert exp["kind_count"][1] == 0  # no latency falls
    if name == "int":
        r = exp["records"]
        assert (r["lat0"].view(np.uint64) == r["lat1"].view(np.uint64)).sum() >= 1


@pytest.mark.parametrize("name,replay_all", [(n, 0) for n in PARITY] + [("int", 1)])
def test_derived_table_matches_the_oracle_of_the_filtered_graph(name, replay_all):
    c = case(name)
    top = product(name)
    assert_table_equal(top, c["t0"])
    child = top.without(edges=c["fail"])
    if replay_all:
        child.set_option("replay_all", 1)
    assert_table_equal(child, c["t1"])
    if replay_all:
        assert child.stats()["replay_rows"] == len(c["t1"][0])
    assert_table_equal(top, c["t0"])  # the parent's table is what it was


def test_failed_vertex_table_matches_the_oracle():
    """A failed poi stays behind isolated: the preparation and the build go over a graph with a
    vertex of degree 0."""
    c = case("real")
    g = c["g"]
    poi = next(v for v in range(g.V) if "poi" in g.vattrs["id"][v] and v not in c["verts"])
    g2, _ = filtered(g, fail_vertices=[poi])
    top = product("real")
    child = top.without(vertices=[poi])
    assert_table_equal(child, g2.table(c["verts"]))
    assert_table_equal(child, c["t0"])  # nothing routes through a leaf


@pytest.mark.parametrize("name", ("real", "directed"))
def test_routes_avoid_what_failed(name):
    c = case(name)
    top = product(name)
    child = top.without(edges=c["fail"])
    rng = np.random.default_rng(11)
    n = 400
    si, di = rng.integers(0, len(c["ips"]), n), rng.integers(0, len(c["ips"]), n)
    ips = np.array(c["ips"], np.uint32)
    tr = child.trace_routes(ips[si], ips[di])
    assert (tr["status"] == 0).all()
    origin = child.edge_origin()
    a, lat1, _, _ = c["t1"]
    col = {int(v): k for k, v in enumerate(a)}
    for i in range(n):
        o, h = int(tr["offset"][i]), int(tr["hops"][i])
        used = origin[tr["edges"][o:o + h]]
        assert not np.isin(used, c["fail"]).any(), i
        want = lat1[col[c["verts"][si[i]]], col[c["verts"][di[i]]]]
        assert np.float64(tr["latency"][i]).view(np.uint64) == np.float64(want).view(np.uint64), i


@pytest.mark.parametrize("name", RECIPE + ("parallel", "one", "two", "wide", "one_router"))
def test_diff_matches_numpy_on_the_oracle_tables(name):
    c = case(name)
    exp = c["exp"]
    A = len(c["t0"][0])
    assert A == {"one": 1, "two": 2, "real": 41, "logu": 72}.get(name, A)
    if name == "wide":
        assert A > 256 + 32  # a row is more than one 256-thread step
    if name == "one_router":
        assert 0 < (exp["row_changed"] > 0).sum() <= A // 3
    top = product(name)
    child = top.without(edges=c["fail"])
    got = top.table_diff(child)
    assert_diff_equal(got, exp)
    st = top.table_diff_stats()
    assert st["pairs"] == A * A and st["changed"] == exp["total"]
    walked = int(((exp["row_changed"] > 0)).sum())
    assert st["bytes_read"] == 36 * (A * A + walked * A)
    # the tables themselves are the oracle's
    assert_table_equal(top, c["t0"])
    assert_table_equal(child, c["t1"])


@pytest.mark.parametrize("name", ("real", "logu"))
def test_diff_cap_and_direction(name):
    c = case(name)
    exp = c["exp"]
    total = exp["total"]
    top = product(name)
    child = top.without(edges=c["fail"])
    # cap = 0 sizes: the total, nothing written
    zero = top.table_diff(child, cap=0)
    assert zero["total"] == total and len(zero["records"]) == 0
    assert np.array_equal(zero["row_changed"], exp["row_changed"])
    # cap = total // 2: exactly that prefix, the rest of the buffer untouched
    lib, _ = _lib.load()
    half = total // 2
    buf = np.full(total, 0xFF, np.uint8).repeat(CHANGE.itemsize).view(CHANGE)
    r = lib.shdtopo_table_diff(top._h, child._h, buf.ctypes.data_as(ctypes.c_void_p), half,
                               None, None, None, None)
    assert r == total
    assert buf[:half].tobytes() == exp["records"][:half].tobytes()
    assert (buf[half:].view(np.uint8) == 0xFF).all()
    assert_diff_equal(top.table_diff(child, cap=half), exp, cap=half)
    # the other direction: the sides exchanged, "fell" where this one reports "rose"
    back = child.table_diff(top)
    assert_diff_equal(back, expected_diff(c["t1"], c["t0"]))
    assert back["records"].tobytes() == swapped(exp).tobytes()
    assert ((back["records"]["kind"] & FELL != 0) == (exp["records"]["kind"] & ROSE != 0)).all()
    assert back["kind_count"][1] == exp["kind_count"][0] and back["kind_count"][0] == 0
    assert (back["row_worst_col"] == -1).all() and (back["row_worst_rise"] == 0.0).all()


def test_nothing_changed():
    c = case("real")
    top = product("real")
    A = len(c["t0"][0])
    for other in (top, top.without()):
        got = top.table_diff(other)
        assert got["total"] == 0 and len(got["records"]) == 0
        assert not got["kind_count"].any()
        assert len(got["row_changed"]) == A and not got["row_changed"].any()
        assert (got["row_worst_col"] == -1).all() and not got["row_worst_rise"].any()
        assert_table_equal(other, c["t0"])  # bit-identical to the parent's


def test_changed_pairs_cross_what_failed():
    """Tie-free domain: a pair can change only if its parent route crosses a failed edge."""
    c = case("logu_hints")
    exp = c["exp"]
    assert exp["total"] >= 100
    top = product("logu_hints")
    child = top.without(edges=c["fail"])
    got = top.table_diff(child)
    assert_diff_equal(got, exp)
    a = c["t0"][0]
    A = len(a)
    ip_of = {}
    for ip, v in zip(c["ips"], c["verts"]):
        ip_of.setdefault(v, ip)
    colip = np.array([ip_of[int(v)] for v in a], np.uint32)
    s, d = np.divmod(np.arange(A * A), A)
    cr = top.link_crossings(colip[s], colip[d], edges=c["fail"])
    crossing = np.zeros(A * A, bool)
    crossing[cr["records"]["flow"]] = True
    changed = np.zeros(A * A, bool)
    changed[got["records"]["srcCol"].astype(np.int64) * A + got["records"]["dstCol"]] = True
    assert changed.sum() == exp["total"]
    assert not (changed & ~crossing).any()
    lat0, lat1 = c["t0"][1].ravel(), c["t1"][1].ravel()
    assert (lat1[crossing] >= lat0[crossing]).all()


def test_errors_and_side_effects():
    c = case("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    ips = np.array(c["ips"], np.uint32)
    # a first build, one call of every kind and a lazy row on both, so the diff builds nothing
    for t in (top, child):
        assert t.latency_ip(int(ips[0]), int(ips[1])) > 0
        t.trace_routes(ips[:8], ips[8:16])
        t.link_load(ips[:8], ips[8:16])
        t.link_crossings(ips[:8], ips[8:16], edges=[0, 1])
        t.link_timeline(ips[:8], ips[8:16], edges=[0, 1], nbins=4)
    state = lambda t: (t.stats(), t.trace_stats(), t.link_load_stats(), t.link_crossings_stats(),
                       t.link_timeline_stats(), [x.tolist() for x in t.lazy_rows()],
                       t.lazyMinimumLatency())
    snaps = [state(top), state(child)]
    assert_diff_equal(top.table_diff(child), c["exp"])
    assert [state(top), state(child)] == snaps
    assert_table_equal(top, c["t0"])
    assert_table_equal(child, c["t1"])
    assert [state(top)[0], state(child)[0]] == [snaps[0][0], snaps[1][0]]  # no rebuild
    # NULL topologies
    lib, _ = _lib.load()
    for a, b in ((None, top._h), (top._h, None), (None, None)):
        assert lib.shdtopo_table_diff(a, b, None, 0, None, None, None, None) == -1
    assert lib.shdtopo_table_diff_stats(None, None) == -1
    # one more host on a vertex that was no column: the attached lists differ
    st = 12345
    while True:
        v, st = child.attach_ip(host_ip(5000), st)
        if v not in c["verts"]:
            break
    assert len(child.attached_vertices()) == len(top.attached_vertices()) + 1
    with pytest.raises(RuntimeError) as e:
        top.table_diff(child)
    assert e.value.args[1] == -4


# ---- the paths of the pair loop (with_current_pair, topo_whatif.cpp) the tests above do not reach:
# ---- they build both tables first

def test_diff_builds_missing_tables():
    c = case("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    # no build and no getter so far: the call builds both tables
    assert_diff_equal(top.table_diff(child), c["exp"])
    assert build_counters(top)["sources"] > 0 and build_counters(child)["sources"] > 0
    snaps = [top.stats(), child.stats()]
    assert_diff_equal(top.table_diff(child), c["exp"])
    assert [top.stats(), child.stats()] == snaps  # the second call built nothing
    assert_table_equal(top, c["t0"])
    assert_table_equal(child, c["t1"])


def test_diff_rebuilds_stale_tables_with_equal_attached_sets():
    c = case("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    assert_diff_equal(top.table_diff(child), c["exp"])
    before = [build_counters(top), build_counters(child)]
    v = attach_off_column(c, top, child)
    A = len(c["t0"][0]) + 1
    assert len(top.attached_vertices()) == A and v in top.attached_vertices()
    # both tables are stale, the attached sets equal: neither -4 nor -5 (table_diff raises on a
    # negative return), the diff of the tables of the new set
    got = top.table_diff(child)
    after = [build_counters(top), build_counters(child)]
    for b, a in zip(before, after):
        assert a["paths_computed"] > b["paths_computed"] and a["targets"] == A
    t0, t1 = top.table(), child.table()  # (the snapshots afterwards: they rebuild nothing)
    assert [build_counters(top), build_counters(child)] == after
    assert len(t0[0]) == A
    assert got["total"] >= c["exp"]["total"] and len(got["row_changed"]) == A
    assert_diff_equal(got, expected_diff(t0, t1))


def test_diff_with_itself_builds_the_table():
    """a is b: nothing can differ, but the diff still demands a current table (the flow impact
    does not: test_flow_impact.test_same_topology_builds_no_table)."""
    c = case("real")
    top = product("real")
    A = len(c["t0"][0])
    assert build_counters(top)["paths_computed"] == 0
    got = top.table_diff(top)
    assert got["total"] == 0 and len(got["records"]) == 0 and not got["kind_count"].any()
    assert len(got["row_changed"]) == A and not got["row_changed"].any()
    assert len(got["row_worst_rise"]) == A and not got["row_worst_rise"].any()
    assert len(got["row_worst_col"]) == A and (got["row_worst_col"] == -1).all()
    st = top.table_diff_stats()
    assert st["pairs"] == A * A and st["changed"] == 0
    built = build_counters(top)
    assert built["paths_computed"] == A and built["targets"] == A
    # it left a current table behind
    lat, rel = np.empty((A, A), np.float64), np.empty((A, A), np.float64)
    hops = np.empty((A, A), np.uint16)
    lib, _ = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.shdtopo_table_to_host(top._h, p(lat), p(rel), p(hops)) == 0
    assert build_counters(top) == built
    assert np.array_equal(lat.view(np.uint64), c["t0"][1].view(np.uint64))
    assert_table_equal(top, c["t0"])
    assert build_counters(top) == built


def test_diff_stats_stay_with_the_first_argument():
    c = case("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    child.table_diff(top, cap=0)
    mine = child.table_diff_stats()
    assert mine["pairs"] == len(c["t0"][0]) ** 2 and mine["changed"] == c["exp"]["total"]
    fresh = top.table_diff_stats()
    assert fresh["pairs"] == 0 and fresh["changed"] == 0
    top.table_diff(child)
    assert child.table_diff_stats() == mine  # written to the first argument only
    assert top.table_diff_stats()["changed"] == c["exp"]["total"]
