"""Conditions on the inputs of test_bound_tables.py, from numpy and the oracle alone: every case
make_tables plants is present in the expected diff, the flows reach what the impact kernels
branch on, the packet route's reliabilities sit where the drop rule decides -- so a planted case
cannot silently vanish.  No GPU; the product is called only for its argument checks.
"""
import numpy as np
import pytest

import oracle
from helpers import graphml_doc
from impact_helpers import check_no_device_used, expected_impact
from shadow_amd import _lib
from table_helpers import (BIG, IMPACT_SIZES, REL_KINDS, ROUTE_JUMP, ROUTE_LATS, SIZES, TIE, U64,
                           attached_of, bound_flows, bound_topologies, glibc_chance, make_tables,
                           pinned_doc, rowmin_table, route_inputs)
from whatif_helpers import FELL, HOPS, REL, ROSE, expected_diff


def tile_flows():
    (top,), _ = bound_topologies(2, 1)
    T = top.flow_impact_stats()["tile_flows"]
    assert T >= 256 and T % 256 == 0
    return T


def test_graphml_doc_without_an_ip_is_what_it_was():
    nodes = [("pop-0", "pop", 0.0), ("poi-0", "client", 0.01)]
    edges = [("poi-0", "pop-0", 5.0, 0.0), ("poi-0", "poi-0", 1.0, 0.0)]
    doc = graphml_doc(nodes, edges)
    assert doc.count(b'<data key="d1">0.0.0.0</data>') == 2
    # the text of the schema as it always was, restated
    node = ('<node id="poi-0"><data key="d0">0.01</data><data key="d1">0.0.0.0</data>'
            '<data key="d2">US</data><data key="d3">10240</data><data key="d4">10240</data>'
            '<data key="d5">client</data></node>')
    assert node.encode() in doc
    with_ip = graphml_doc([nodes[0], nodes[1] + ("12.0.0.1",)], edges)
    assert with_ip == doc.replace(b'0.0.0.0</data><data key="d2">US</data><data key="d3">10240'
                                  b'</data><data key="d4">10240</data><data key="d5">client',
                                  b'12.0.0.1</data><data key="d2">US</data><data key="d3">10240'
                                  b'</data><data key="d4">10240</data><data key="d5">client')


@pytest.mark.parametrize("P", (1, 2, 65))
def test_pinned_topologies(P):
    g = oracle.OGraph.from_graphml(pinned_doc(P))
    assert g.V == P + 2 and g.is_strongly_connected() and not g.is_complete()
    tops, ips = bound_topologies(P)
    assert len(tops) == 2 and len(set(ips.tolist())) == P
    for top in tops:
        assert not top.is_complete
        assert np.array_equal(top.attached_vertices(), attached_of(P))
        assert [top.vertex_of_ip(int(ip)) for ip in ips] == list(range(2, P + 2))
        check_no_device_used(top)


def kinds_at(exp, A):
    k = np.zeros((A, A), np.uint32)
    k[exp["records"]["srcCol"], exp["records"]["dstCol"]] = exp["records"]["kind"]
    return k


@pytest.mark.parametrize("A", SIZES)
def test_tables_follow_the_recipe(A):
    t0, t1, _ = make_tables(A)
    for a, lat, rel, hops in (t0, t1):
        assert np.array_equal(a, attached_of(A)) and lat.shape == rel.shape == hops.shape == (A, A)
        assert np.isfinite(lat).all() and (lat > 0).all() and (lat <= 200 + BIG).all()
        assert (rel >= 0).all() and (rel <= 1).all() and hops.dtype == np.uint16
    lat0, hops0 = t0[1], t0[3]
    assert np.array_equal(lat0 * 2.0**20, np.round(lat0 * 2.0**20))  # differences are exact
    assert (lat0 * 4 != np.round(lat0 * 4)).sum() == (A >= 2) + 2 * (A >= 3)  # the one-ulp cells
    off = ~np.eye(A, dtype=bool)
    assert (lat0 != lat0.T)[off].all()
    usual = (hops0 >= 1) & (hops0 <= 40)
    assert (~usual).sum() == (2 if A >= 4 else 0)
    again = make_tables.__wrapped__(A)
    for x, y in zip(t0[1:] + t1[1:], again.t0[1:] + again.t1[1:]):
        assert x.tobytes() == y.tobytes()  # deterministic


@pytest.mark.parametrize("A", SIZES)
def test_planted_cases_are_in_the_expected_diff(A):
    t0, t1, plan = make_tables(A)
    exp = expected_diff(t0, t1)
    kind = kinds_at(exp, A)
    lat0, lat1 = t0[1], t1[1]
    # what this A has room for
    want = {"big": 1 if A == 1 else 2, "fall_beside_rise": A >= 2, "rel_only": A >= 5,
            "hops_only": A >= 5, "all_three": A >= 5, "ulp_up": (A >= 2) + (A >= 3),
            "ulp_down": A >= 3, "hops_0_to_max": A >= 4, "hops_max_to_0": A >= 4,
            "tie_adjacent": A >= 5, "row_all": A >= 7, "row_none": A >= 7, "row_col0": A >= 10,
            "row_last": A >= 10, "row_255_256": A >= 257, "tie_64": A >= 65, "tie_256": A >= 257,
            "tie_wave": A >= 139, "tie_wave_step": A >= 267}
    assert {k: len(plan.get(k, ())) for k in want} == {k: int(v) for k, v in want.items()}
    count = {k: 0 for k in want}
    for r, c in plan["big"]:
        assert kind[r, c] & ROSE and lat1[r, c] - lat0[r, c] == BIG
        count["big"] += 1
    rose = exp["records"][exp["records"]["kind"] & ROSE != 0]
    assert (rose["lat1"] - rose["lat0"]).max() == BIG
    assert ((rose["lat1"] - rose["lat0"]) == BIG).sum() == len(plan["big"])
    assert len({r for r, _ in plan["big"]}) == len(plan["big"])  # in different rows
    for r, c in plan.get("fall_beside_rise", ()):
        assert kind[r, c] & FELL and kind[r, 0] & ROSE and c // 64 == 0
        count["fall_beside_rise"] += 1
    for name, k in (("rel_only", REL), ("hops_only", HOPS), ("all_three", ROSE | REL | HOPS)):
        for r, c in plan.get(name, ()):
            assert kind[r, c] == k
            count[name] += 1
    ns = lambda x: np.ceil(x * 1e6)
    for name, k in (("ulp_up", ROSE), ("ulp_down", FELL)):
        for r, c in plan.get(name, ()):
            assert kind[r, c] == k
            assert abs(int(lat1[r, c].view(np.int64)) - int(lat0[r, c].view(np.int64))) == 1
            assert ns(lat0[r, c]) == ns(lat1[r, c])  # the delay does not move: a rise of 0 ns
            count[name] += 1
    for name, h in (("hops_0_to_max", (0, 65535)), ("hops_max_to_0", (65535, 0))):
        for r, c in plan.get(name, ()):
            assert kind[r, c] == HOPS and (t0[3][r, c], t1[3][r, c]) == h
            count[name] += 1
    for name in ("tie_adjacent", "tie_64", "tie_256", "tie_wave", "tie_wave_step"):
        for r, lo, hi in plan.get(name, ()):
            assert lo < hi and lat1[r, lo] - lat0[r, lo] == TIE == lat1[r, hi] - lat0[r, hi]
            assert exp["row_worst_rise"][r] == TIE and exp["row_worst_col"][r] == lo
            smaller = (kind[r] & ROSE != 0) & (lat1[r] - lat0[r] < TIE)
            assert smaller.any()
            count[name] += 1
    for r, lo, hi in plan.get("tie_64", ()):
        assert hi - lo == 64
    for r, lo, hi in plan.get("tie_256", ()):
        assert hi - lo == 256  # one thread of a 256-thread workgroup, two steps
    lane, wave, step = lambda c: c % 64, lambda c: c % 256 // 64, lambda c: c // 256
    for name in ("tie_wave", "tie_wave_step"):
        for r, lo, hi in plan.get(name, ()):
            small = int(np.flatnonzero((kind[r] & ROSE != 0) & (lat1[r] - lat0[r] < TIE))[0])
            assert lane(lo) > lane(hi) > lane(small) and wave(lo) > wave(small)
            assert (wave(lo) > wave(hi) and step(hi) > step(lo) if name == "tie_wave_step"
                    else wave(hi) > wave(lo))
    rc = exp["row_changed"]
    cols = lambda r: exp["records"]["dstCol"][exp["records"]["srcCol"] == r].tolist()
    for name, n, where in (("row_all", A, list(range(A))), ("row_none", 0, []),
                           ("row_col0", 1, [0]), ("row_last", 1, [A - 1]),
                           ("row_255_256", 2, [255, 256])):
        for r in plan.get(name, ()):
            assert rc[r] == n and cols(r) == where
            count[name] += 1
    if plan.get("row_all"):
        assert plan["row_none"][0] == plan["row_all"][0] + 1  # next to each other
    assert count == {k: int(v) for k, v in want.items()}
    # both directions, and in one row
    if A >= 2:
        assert exp["kind_count"][0] > 0 and exp["kind_count"][1] > 0
        both = ((kind & ROSE != 0).any(axis=1) & (kind & FELL != 0).any(axis=1))
        assert both.sum() >= 1
        word = (kind[:, :64] & ROSE != 0).any(axis=1) & (kind[:, :64] & FELL != 0).any(axis=1)
        assert word.sum() >= 1
    else:
        assert exp["total"] == 1 and exp["kind_count"][0] == 1  # one cell holds one change


@pytest.mark.parametrize("A", SIZES)
def test_rowmin_table(A):
    t, pos, mins = rowmin_table(A)
    lat = t[1]
    assert (np.diag(lat) > 0).all()
    assert np.array_equal(np.argmin(np.where(lat >= 0, lat, np.inf), axis=1), pos)
    assert (mins > 0).all() and len(np.unique(mins)) == A
    cyc = [0, 1, 63, 64, 65, 255, 256, A - 1]
    assert pos.tolist() == [min(cyc[i % 8], A - 1) for i in range(A)]
    if A >= 63:
        assert (lat == -1.0).sum() > A and ((lat == -1.0).any(axis=1)).all()
        assert set(np.unique(lat[lat < 0]).tolist()) == {-1.0}


@pytest.mark.parametrize("A", IMPACT_SIZES)
def test_flows_exercise_the_impact(A):
    T = tile_flows()
    t0, t1, plan = make_tables(A)
    fl = bound_flows(A, T)
    n = len(fl["weight"])
    s, d = fl["src_col"], fl["dst_col"]
    bad = (s < 0) | (s >= A) | (d < 0) | (d >= A)
    assert np.array_equal(np.flatnonzero(bad), [0, 63, 64, n // 2, n - 1])
    if A <= 65:
        pairs = set(zip(s[~bad].tolist(), d[~bad].tolist()))
        assert len(pairs) == A * A
    exp = expected_impact(t0, t1, s, d, fl["weight"], fl["edge_sets"]["exact"])
    tt = exp["totals"]
    assert tt["unattached"] == 5 and tt["changed"] >= 130
    assert tt["delayRiseNs"] != 0 and tt["delayFallNs"] != 0
    assert tt["hopsRise"] != 0 and tt["hopsFall"] != 0
    rises = exp["rises_ns"]
    assert (rises == 0).sum() >= 1  # a latency that rose without moving the delay
    edges = fl["edge_sets"]["exact"]
    assert np.isin(rises, edges).sum() >= 1 and np.isin(rises + U64(1), edges).sum() >= 1
    assert int(edges[-1]) == 2**63
    rec = exp["records"]
    # the sums do wrap
    for m in (rec["kind"] & ROSE != 0, rec["kind"] & FELL != 0, rec["kind"] & HOPS != 0):
        assert sum(int(x) for x in fl["weight"][rec["flow"][m]]) >= 2**64
    # the worst rise: reached in two tiles, and inside the first tile in one wavefront, in two
    # wavefronts and by one thread at two steps
    rose = rec[rec["kind"] & ROSE != 0]
    top_flows = rose["flow"][(rose["lat1"] - rose["lat0"]) == tt["worstRise"]]
    assert tt["worstRise"] == BIG and tt["worstFlow"] == 1 == fl["worst"][0]
    assert {1, 2, 70, 258, n - 3} <= set(top_flows.tolist())
    assert fl["worst"][1] - fl["worst"][0] > T
    assert len(set((top_flows // T).tolist())) >= 2
    assert 258 < T and 258 % 256 == 2
    # full and empty ballot words
    flag = np.zeros(n, bool)
    flag[rec["flow"]] = True
    words = flag[:n // 64 * 64].reshape(-1, 64)
    assert words.all(axis=1).sum() >= 1 and (~words.any(axis=1)).sum() >= (A > 2)
    # the edge sets
    es = fl["edge_sets"]
    assert len(es["none"]) == 0 and es["zero"].tolist() == [0] and len(es["max"]) == 1024
    assert (np.diff(es["max"].astype(object)) > 0).all()
    assert np.isin(rises, es["max"]).sum() >= 1
    big = expected_impact(t0, t1, s, d, fl["weight"], es["max"])
    assert (big["rise_count"] > 0).sum() >= (3 if A > 2 else 2)  # (A = 2: 0 ns and BIG)


def test_glibc_chance_is_the_oracles_draw():
    st = np.random.default_rng(3).integers(0, 2**32, 5000, dtype=np.uint64).astype(np.uint32)
    st[:4] = [0, 1, 2**31, 2**32 - 1]
    chance, nxt = glibc_chance(st)
    n = len(st)
    one, zero = np.ones(n), np.zeros(n, np.uint64)
    _, _, ost = oracle.route_packets(one, one, np.ones(n, np.uint32), st, zero, 0, 0)
    assert np.array_equal(nxt, ost)
    assert (chance >= 0).all() and (chance <= 1).all()
    # and the chance itself: delivered exactly when chance <= rel
    _, dl, _ = oracle.route_packets(one, chance, np.ones(n, np.uint32), st, zero, 0, 0)
    assert dl.all()
    below = np.nextafter(chance, -1.0)
    _, dl, _ = oracle.route_packets(one, below, np.ones(n, np.uint32), st, zero, 0, 0)
    assert not dl[chance > 0].any()


def test_route_inputs_sit_on_the_drop_rule():
    ri = route_inputs()
    _, lat, rel, _ = ri["t"]
    n = len(ri["state"])
    assert n == 4096 and lat.shape == (64, 64)
    assert (rel >= 0).all() and (rel <= 1).all() and (lat > 0).all() and np.isfinite(lat).all()
    s, d = ri["src_col"], ri["dst_col"]
    assert len(set(zip(s.tolist(), d.tolist()))) == n  # a pair per packet
    L, R = lat[s, d], rel[s, d]
    _, dl, st = oracle.route_packets(L, R, ri["payload"], ri["state"], ri["now"], ROUTE_JUMP, 1)
    assert np.array_equal(st, glibc_chance(ri["state"])[1])
    kind = np.array(REL_KINDS)[ri["rel_kind"]]
    paid = ri["payload"] > 0
    for k in REL_KINDS:
        for p in (True, False):
            assert ((kind == k) & (paid == p)).sum() >= 300, (k, p)
    eq, below, above = kind == "equal", kind == "ulp_below", kind == "ulp_above"
    assert np.array_equal(R[eq].view(U64), ri["chance"][eq].view(U64))
    assert np.array_equal(R[below], np.nextafter(ri["chance"][below], -1.0))
    assert dl[eq].all() and dl[above].all() and dl[kind == "one"].all()
    assert not dl[below & paid].any() and dl[below & ~paid].all()
    assert not dl[(kind == "zero") & paid].any() and dl[(kind == "zero") & ~paid].all()
    # every latency with every reliability kind and both payloads
    combos = set(zip(ri["lat_kind"].tolist(), ri["rel_kind"].tolist(), paid.tolist()))
    assert len(combos) == len(ROUTE_LATS) * 5 * 2
    for m in (1, 255, 256, 257):
        assert len(set(ri["rel_kind"][:m].tolist())) == min(m, 5)


def test_route_delays():
    lats = np.array(ROUTE_LATS)
    n = len(lats)
    t, dl, _ = oracle.route_packets(lats, np.ones(n), np.zeros(n, np.uint32),
                                    np.ones(n, np.uint32), np.zeros(n, np.uint64), 0, 0)
    assert dl.all()
    # (1e-6 * 1e6 is 1.0 exactly; one ulp above it the product is above 1.0: 2 ns)
    assert t.tolist() == [500000, 3000000, 3000001, 1, 1, 2, 107374182400000000, 2999999]
    # the clamp sees a delay below, at and above the jump
    assert {ROUTE_JUMP - 1, ROUTE_JUMP, ROUTE_JUMP + 1} <= set(t.tolist())
    tc, _, _ = oracle.route_packets(lats, np.ones(n), np.zeros(n, np.uint32),
                                    np.ones(n, np.uint32), np.zeros(n, np.uint64), ROUTE_JUMP, 1)
    assert np.array_equal(tc, np.maximum(t, np.uint64(ROUTE_JUMP)))


def test_bind_argument_checks():
    """NULL arguments: -1, and no device is initialised for it."""
    lib, _ = _lib.load()
    (top,), _ = bound_topologies(2, 1)
    buf = np.zeros(16, np.float64)
    p = buf.ctypes.data
    for f in (lib.shdtopo_bind_table, lib.shdtopo_bind_table_ref):
        assert f(None, p, p, 1.0, None) == -1
        assert f(None, None, None, 1.0, None) == -1
        assert f(top._h, None, p, 1.0, None) == -1
        assert f(top._h, p, None, 1.0, None) == -1
    check_no_device_used(top)
