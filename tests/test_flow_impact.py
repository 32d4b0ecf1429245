"""Flow impact on the GPU (shdtopo_flow_impact / shdtopo_flow_impact_device, topo_impact.hip): what
a link failure does to a set of flows, joined with the two resident tables on the device.

Reference: numpy on the oracle's two tables of the what-if cases (impact_helpers.expected_impact);
flows, weights and histogram edges are impact_helpers.impact_flows, computed once per case and
shared.  Every sum is a u64 that wraps (the weights are full-range), so every comparison is exact.
"""
import ctypes
import functools

import numpy as np
import pytest

from helpers import host_ip
from impact_helpers import (FLOW_CHANGE, UNATTACHED_IP, assert_impact_equal, assert_sums_equal,
                            columns_of, expected_impact, impact_flows, prefix, usum)
from shadow_amd import _lib
from whatif_helpers import (FELL, ROSE, assert_table_equal, attach_off_column, build_counters, case,
                            product)

pytestmark = pytest.mark.gpu

RECIPE = ("real", "int", "directed", "logu")
PARITY = RECIPE + ("parallel", "wide", "one_router", "one", "two")


@functools.lru_cache(maxsize=None)
def pair(name):
    """The product's parent and child of a case, built once (the tests only read their tables)."""
    top = product(name)
    return top, top.without(edges=case(name)["fail"])


def run(top, other, fl, n=None, **kw):
    n = len(fl["src_ip"]) if n is None else n
    return top.flow_impact(other, fl["src_ip"][:n], fl["dst_ip"][:n], weight=fl["weight"][:n],
                           rise_edges_ns=fl["edges"], **kw)


def cu(x):
    import torch
    x = np.ascontiguousarray(x)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(x.dtype)
    return torch.from_numpy(x.view(view) if view else x).cuda()


@pytest.mark.parametrize("name", RECIPE)
def test_inputs_exercise_the_impact(name):
    """Conditions on the input, from the oracle alone."""
    fl = impact_flows(name)
    exp, tt = fl["exp"], fl["exp"]["totals"]
    n = tt["flows"]
    assert tt["changed"] >= 100
    assert tt["compared"] - tt["changed"] >= 1000
    assert tt["unattached"] == 5
    assert np.array_equal(np.flatnonzero((fl["src_col"] < 0) | (fl["dst_col"] < 0)),
                          [0, 63, 64, n // 2, n - 1])
    assert (exp["rise_count"] > 0).sum() >= 3
    assert np.isin(exp["rises_ns"], fl["edges"]).sum() >= 1
    rec = exp["records"]
    if name == "int":
        assert (rec["lat0"].view(np.uint64) == rec["lat1"].view(np.uint64)).sum() >= 1
    flag = np.zeros(n, bool)
    flag[rec["flow"]] = True
    words = flag[:n // 64 * 64].reshape(-1, 64)
    assert words.all(axis=1).sum() >= 1 and (~words.any(axis=1)).sum() >= 1
    rose = rec[rec["kind"] & ROSE != 0]
    assert ((rose["lat1"] - rose["lat0"]) == tt["worstRise"]).sum() >= 2
    assert sum(int(x) for x in fl["weight"][rec["flow"]]) >= 2**64  # the sums do wrap


@pytest.mark.parametrize("name", PARITY)
def test_impact_matches_numpy_on_the_oracle_tables(name):
    c, fl = case(name), impact_flows(name)
    A = len(c["t0"][0])
    assert A == {"one": 1, "two": 2, "real": 41, "logu": 72}.get(name, A)
    if name == "one":
        assert fl["exp"]["total"] == 0
    top, child = pair(name)
    got = run(top, child, fl)
    assert_impact_equal(got, fl["exp"], what=name)
    assert got["records"].dtype.itemsize == FLOW_CHANGE.itemsize == 48
    st = top.flow_impact_stats()
    assert st["flows"] == len(fl["weight"]) and st["changed"] == fl["exp"]["total"]
    assert st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]
    # the tables themselves are still the oracle's
    assert_table_equal(top, c["t0"])
    assert_table_equal(child, c["t1"])


def test_tile_edges():
    c, fl = case("real"), impact_flows("real")
    top, child = pair("real")
    T = top.flow_impact_stats()["tile_flows"]
    assert T >= 256 and T % 256 == 0
    n_all = len(fl["weight"])
    assert n_all > T + 1
    for n in (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, n_all):
        assert_impact_equal(run(top, child, fl, n), prefix(fl, c, n), what=n)
        assert top.flow_impact_stats()["flows"] == n


@pytest.mark.parametrize("name", ("real", "logu"))
def test_cap(name):
    fl = impact_flows(name)
    exp = fl["exp"]
    total = exp["total"]
    top, child = pair(name)
    zero = run(top, child, fl, cap=0)
    assert zero["total"] == total and len(zero["records"]) == 0
    assert_sums_equal(zero, exp)
    assert top.flow_impact_stats()["words_skipped"] == (len(fl["weight"]) + 63) // 64
    # cap = total // 2 through the C ABI: exactly that prefix, the rest of the buffer untouched
    lib, _ = _lib.load()
    half = total // 2
    buf = np.full(total, 0xFF, np.uint8).repeat(FLOW_CHANGE.itemsize).view(FLOW_CHANGE)
    tt = _lib.ShdImpactTotals()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    r = lib.shdtopo_flow_impact(top._h, child._h, p(fl["src_ip"]), p(fl["dst_ip"]), p(fl["weight"]),
                                len(fl["weight"]), p(fl["edges"]), len(fl["edges"]), p(buf), half,
                                ctypes.byref(tt), None, None, None, None)
    assert r == total
    assert buf[:half].tobytes() == exp["records"][:half].tobytes()
    assert (buf[half:].view(np.uint8) == 0xFF).all()
    assert tt.changed == total and tt.delayRiseNs == exp["totals"]["delayRiseNs"]
    assert_impact_equal(run(top, child, fl, cap=half), exp, cap=half)
    # one record, and a cap beyond the total
    assert_impact_equal(run(top, child, fl, cap=1), exp, cap=1)
    assert_impact_equal(run(top, child, fl, cap=total + 7), exp)


def test_direction():
    c, fl = case("real"), impact_flows("real")
    top, child = pair("real")
    fwd = fl["exp"]
    back = run(child, top, fl)
    assert_impact_equal(back, expected_impact(c["t1"], c["t0"], fl["src_col"], fl["dst_col"],
                                              fl["weight"], fl["edges"]))
    assert np.array_equal(back["records"]["flow"], fwd["records"]["flow"])
    assert ((back["records"]["kind"] & FELL != 0) == (fwd["records"]["kind"] & ROSE != 0)).all()
    assert not (back["records"]["kind"] & ROSE).any()
    assert back["totals"]["delayFallNs"] == fwd["totals"]["delayRiseNs"]
    assert back["totals"]["delayRiseNs"] == 0
    assert back["totals"]["hopsFall"] == fwd["totals"]["hopsRise"]
    assert not back["rise_count"].any() and not back["rise_weight"].any()
    assert back["totals"]["worstFlow"] == -1 and back["totals"]["worstRise"] == 0.0


def test_order_independence():
    c, fl = case("real"), impact_flows("real")
    top, child = pair("real")
    n = len(fl["weight"])
    perm = np.random.default_rng(31).permutation(n)
    shuffled = {k: fl[k][perm] for k in ("src_ip", "dst_ip", "weight", "src_col", "dst_col")}
    shuffled["edges"] = fl["edges"]
    got = run(top, child, shuffled)
    exp = expected_impact(c["t0"], c["t1"], shuffled["src_col"], shuffled["dst_col"],
                          shuffled["weight"], fl["edges"])
    assert_impact_equal(got, exp)
    # sums, histograms and per-column arrays are those of the original order
    for k in ("rise_count", "rise_weight", "src_changed_weight", "dst_changed_weight"):
        assert np.array_equal(got[k], fl["exp"][k]), k
    for k, v in fl["exp"]["totals"].items():
        if k not in ("worstFlow", "kindCount", "kindWeight"):
            assert got["totals"][k] == v, k
    assert np.array_equal(got["totals"]["kindCount"], fl["exp"]["totals"]["kindCount"])
    assert np.array_equal(got["totals"]["kindWeight"], fl["exp"]["totals"]["kindWeight"])
    # the records are the original ones at their new indices, ascending
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    moved = fl["exp"]["records"].copy()
    moved["flow"] = inv[moved["flow"]]
    moved = moved[np.argsort(moved["flow"])]
    assert got["records"].tobytes() == moved.tobytes()
    assert (np.diff(got["records"]["flow"]) > 0).all()


def test_repeatability():
    fl = impact_flows("logu")
    top, child = pair("logu")
    a, b = run(top, child, fl), run(top, child, fl)
    assert a["total"] == b["total"] and a["records"].tobytes() == b["records"].tobytes()
    for k in ("rise_count", "rise_weight", "src_changed_weight", "dst_changed_weight"):
        assert a[k].tobytes() == b[k].tobytes()
    for k, v in a["totals"].items():
        x = b["totals"][k]
        assert (np.array_equal(v, x) if isinstance(v, np.ndarray) else
                np.float64(v).view(np.uint64) == np.float64(x).view(np.uint64) if k == "worstRise"
                else v == x), k


@pytest.mark.parametrize("name", ("real", "wide"))
def test_device_variant(name):
    import torch
    c, fl = case(name), impact_flows(name)
    top, child = pair(name)
    A = len(c["t0"][0])
    n = len(fl["weight"])
    col = {}
    for ip in np.unique(np.concatenate([fl["src_ip"], fl["dst_ip"]])):
        col[int(ip)] = top.column_of_ip(int(ip))
    sc = np.array([col[int(x)] for x in fl["src_ip"]], np.int32)
    dc = np.array([col[int(x)] for x in fl["dst_ip"]], np.int32)
    assert np.array_equal(sc, fl["src_col"]) and np.array_equal(dc, fl["dst_col"])
    # columns that are none, planted on changed and unchanged flows
    ch = fl["exp"]["records"]["flow"]
    planted = [int(ch[3]), int(ch[40]), 7, n - 2]
    sc[planted[0]] = -1
    dc[planted[1]] = A
    sc[planted[2]] = 2**31 - 1
    dc[planted[3]] = -(2**31)
    pay = np.random.default_rng(41).integers(0, 2**32, n, dtype=np.uint32)
    d_sc, d_dc, d_pay = cu(sc), cu(dc), cu(pay)
    exp = expected_impact(c["t0"], c["t1"], sc, dc, pay, fl["edges"])
    assert exp["totals"]["unattached"] == 5 + 4
    got = top.flow_impact_device(child, d_sc, d_dc, payload=d_pay, rise_edges_ns=fl["edges"])
    assert_impact_equal(got, exp, what="payload")
    # the host variant on the same flows with the same weights
    s, d = fl["src_ip"].copy(), fl["dst_ip"].copy()
    s[planted[0]] = s[planted[2]] = UNATTACHED_IP
    d[planted[1]] = d[planted[3]] = UNATTACHED_IP
    host = top.flow_impact(child, s, d, weight=pay.astype(np.uint64), rise_edges_ns=fl["edges"])
    assert_impact_equal(host, exp, what="host")
    assert host["records"].tobytes() == got["records"].tobytes()
    # no payload: 1 each; on a stream of the caller's
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    ones = top.flow_impact_device(child, d_sc, d_dc, rise_edges_ns=fl["edges"],
                                  stream=st.cuda_stream)
    assert_impact_equal(ones, expected_impact(c["t0"], c["t1"], sc, dc, None, fl["edges"]),
                        what="ones")
    assert ones["totals"]["changedWeight"] == ones["total"]
    assert top.flow_impact_stats()["resolve_ms"] == 0
    # the same topology twice: counted on the host from the copied columns
    same = top.flow_impact_device(top, d_sc, d_dc, payload=d_pay, rise_edges_ns=fl["edges"])
    assert same["total"] == 0
    assert same["totals"]["compared"] == exp["totals"]["compared"]
    assert same["totals"]["weight"] == exp["totals"]["weight"]


def test_errors_and_side_effects():
    c, fl = case("real"), impact_flows("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    ips = np.array(c["ips"], np.uint32)
    # a first build, one call of every kind and a lazy row on both, so the impact builds nothing
    for t in (top, child):
        assert t.latency_ip(int(ips[0]), int(ips[1])) > 0
        t.trace_routes(ips[:8], ips[8:16])
        t.link_load(ips[:8], ips[8:16])
        t.link_crossings(ips[:8], ips[8:16], edges=[0, 1])
        t.link_timeline(ips[:8], ips[8:16], edges=[0, 1], nbins=4)
    top.table_diff(child)
    child.table_diff(top)
    state = lambda t: (t.stats(), t.trace_stats(), t.link_load_stats(), t.link_crossings_stats(),
                       t.link_timeline_stats(), t.table_diff_stats(),
                       [x.tolist() for x in t.lazy_rows()], t.lazyMinimumLatency())
    snaps = [state(top), state(child)]
    got = run(top, child, fl)
    assert_impact_equal(got, fl["exp"])
    d_sc, d_dc = cu(fl["src_col"]), cu(fl["dst_col"])
    dev = top.flow_impact_device(child, d_sc, d_dc, rise_edges_ns=fl["edges"])
    assert dev["total"] == fl["exp"]["total"]
    assert [state(top), state(child)] == snaps
    assert top.flow_impact_stats()["changed"] == fl["exp"]["total"]
    assert child.flow_impact_stats()["flows"] == 0  # kept by the first argument
    assert_table_equal(top, c["t0"])
    assert_table_equal(child, c["t1"])
    # one more host on a vertex that was no column: the attached lists differ
    st = 12345
    while True:
        v, st = child.attach_ip(host_ip(5000), st)
        if v not in c["verts"]:
            break
    with pytest.raises(RuntimeError) as e:
        run(top, child, fl)
    assert e.value.args[1] == -4
    with pytest.raises(RuntimeError) as e:
        top.flow_impact_device(child, d_sc, d_dc)
    assert e.value.args[1] == -4


def test_identical_child():
    fl = impact_flows("real")
    top, _ = pair("real")
    same = top.without()
    got = run(top, same, fl)
    tt, want = got["totals"], fl["exp"]["totals"]
    assert got["total"] == 0 and len(got["records"]) == 0
    assert (tt["flows"], tt["compared"], tt["unattached"]) == (want["flows"], want["compared"], 5)
    assert tt["weight"] == want["weight"] and tt["weight"] != 0
    for k in ("changed", "changedWeight", "delayRiseNs", "delayFallNs", "hopsRise", "hopsFall"):
        assert tt[k] == 0, k
    assert not tt["kindCount"].any() and not tt["kindWeight"].any()
    assert tt["worstFlow"] == -1 and tt["worstRise"] == 0.0
    for k in ("rise_count", "rise_weight", "src_changed_weight", "dst_changed_weight"):
        assert not got[k].any(), k
    st = top.flow_impact_stats()
    assert st["words_skipped"] == (want["flows"] + 63) // 64 and st["kernel_ms"] > 0


# ---- the paths of the pair loop (with_current_pair, topo_whatif.cpp) the tests above do not reach:
# ---- they build both tables first

def test_impact_builds_missing_tables():
    c, fl = case("real"), impact_flows("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    # no build and no getter so far: the call builds both tables
    assert_impact_equal(run(top, child, fl), fl["exp"])
    assert build_counters(top)["sources"] > 0 and build_counters(child)["sources"] > 0
    snaps = [top.stats(), child.stats()]
    assert_impact_equal(run(top, child, fl), fl["exp"])
    assert [top.stats(), child.stats()] == snaps  # the second call built nothing
    assert_table_equal(top, c["t0"])
    assert_table_equal(child, c["t1"])


def test_impact_rebuilds_stale_tables_with_equal_attached_sets():
    c, fl = case("real"), impact_flows("real")
    top = product("real")
    child = top.without(edges=c["fail"])
    assert_impact_equal(run(top, child, fl), fl["exp"])
    before = [build_counters(top), build_counters(child)]
    extra = host_ip(5000)
    v = attach_off_column(c, top, child, ip=extra)
    A = len(c["t0"][0]) + 1
    # both tables are stale, the attached sets equal: neither -4 nor -5 (flow_impact raises on a
    # negative return), the impact between the tables of the new set; the new host sends and
    # receives one flow
    s = np.append(fl["src_ip"], [extra, fl["src_ip"][1]]).astype(np.uint32)
    d = np.append(fl["dst_ip"], [fl["dst_ip"][1], extra]).astype(np.uint32)
    w = np.append(fl["weight"], [3, 2**63 + 5]).astype(np.uint64)
    got = top.flow_impact(child, s, d, weight=w, rise_edges_ns=fl["edges"])
    after = [build_counters(top), build_counters(child)]
    for b, a in zip(before, after):
        assert a["paths_computed"] > b["paths_computed"] and a["targets"] == A
    t0, t1 = top.table(), child.table()  # (the snapshots afterwards: they rebuild nothing)
    assert [build_counters(top), build_counters(child)] == after
    assert len(t0[0]) == A and v in t0[0]
    moved = dict(c, ips=c["ips"] + (extra,), verts=c["verts"] + (v,))
    sc, dc = columns_of(moved, s, t0[0]), columns_of(moved, d, t0[0])
    assert sc[-2] >= 0 and dc[-1] >= 0 and (sc < 0).sum() + (dc < 0).sum() == 5
    exp = expected_impact(t0, t1, sc, dc, w, fl["edges"])
    assert exp["total"] >= fl["exp"]["total"]
    assert_impact_equal(got, exp)
    # the device variant: the host leaves again, both tables are stale once more
    top.detach_ip(extra), child.detach_ip(extra)
    before = [build_counters(top), build_counters(child)]
    dev = top.flow_impact_device(child, cu(fl["src_col"]), cu(fl["dst_col"]),
                                 rise_edges_ns=fl["edges"])
    for b, t in zip(before, (top, child)):
        assert build_counters(t)["paths_computed"] > b["paths_computed"]
    assert_table_equal(top, c["t0"])
    assert_table_equal(child, c["t1"])
    assert_impact_equal(dev, expected_impact(c["t0"], c["t1"], fl["src_col"], fl["dst_col"], None,
                                             fl["edges"]))


def test_same_topology_builds_no_table():
    """a is b: nothing can change, and the impact -- unlike the diff, which still demands a current
    table (test_whatif.test_diff_with_itself_builds_the_table) -- counts on the host."""
    fl = impact_flows("real")
    want = fl["exp"]["totals"]
    n = want["flows"]
    top = product("real")
    got = run(top, top, fl)
    tt = got["totals"]
    assert got["total"] == 0 and len(got["records"]) == 0
    assert (tt["flows"], tt["compared"], tt["unattached"]) == (n, want["compared"], 5)
    assert tt["weight"] == want["weight"] and tt["changed"] == 0 and tt["worstFlow"] == -1
    for k in ("rise_count", "rise_weight", "src_changed_weight", "dst_changed_weight"):
        assert not got[k].any(), k
    st = top.flow_impact_stats()
    assert st["flows"] == n and st["changed"] == 0 and st["kernel_ms"] == 0
    assert st["words_skipped"] == (n + 63) // 64
    pay = np.random.default_rng(43).integers(0, 2**32, n, dtype=np.uint32)
    ok = (fl["src_col"] >= 0) & (fl["dst_col"] >= 0)
    for payload, weight in ((pay, usum(pay[ok])), (None, int(ok.sum()))):
        dev = top.flow_impact_device(top, cu(fl["src_col"]), cu(fl["dst_col"]),
                                     payload=None if payload is None else cu(payload),
                                     rise_edges_ns=fl["edges"])
        tt = dev["totals"]
        assert dev["total"] == 0 and tt["changed"] == 0
        assert (tt["flows"], tt["compared"], tt["unattached"]) == (n, int(ok.sum()), 5)
        assert tt["weight"] == weight
    built = build_counters(top)
    assert built["paths_computed"] == 0 and built["sources"] == 0 and built["build_ms"] == 0
