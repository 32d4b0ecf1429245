"""Flow impact, host side (no device): shdtopo_flow_impact's argument checks, the -4 for unequal
attached sets, the a == b answer that needs no table, and the numpy reference of impact_helpers
against a plain Python loop.
"""
import ctypes
import math
import struct

import numpy as np
import pytest

import shadow_amd as sa
from helpers import host_ip, random_topology_graphml
from impact_helpers import (UNATTACHED_IP, check_no_device_used, columns_of, expected_impact,
                            impact_flows)
from shadow_amd import _lib
from whatif_helpers import FELL, HOPS, REL, ROSE, case, product_attach

M64 = (1 << 64) - 1


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pair(hosts_b=None):
    data = random_topology_graphml()
    a, b = sa.Topology.from_buffer(data), sa.Topology.from_buffer(data)
    ips, _, _ = product_attach(a, 20)
    product_attach(b, 20, only=hosts_b)
    return a, b, np.array(ips, np.uint32)


def test_bad_arguments_are_refused_before_any_device_is_used():
    lib, _ = _lib.load()
    a, b, ips = _pair()
    s, d = ips[:8].copy(), ips[8:16].copy()
    n = len(s)
    rec = np.zeros(4, sa.topology.FLOW_CHANGE_DTYPE)

    def host(ta=a._h, tb=b._h, src=_p(s), dst=_p(d), n=n, edges=None, nb=0, out=None, cap=0):
        return lib.shdtopo_flow_impact(ta, tb, src, dst, None, n, edges, nb, out, cap, None, None,
                                       None, None, None)

    def dev(ta=a._h, tb=b._h, src=_p(s), dst=_p(d), n=n, edges=None, nb=0, out=None, cap=0):
        # (the pointers are never read: every case fails the argument check)
        return lib.shdtopo_flow_impact_device(ta, tb, src, dst, None, n, edges, nb, out, cap, None,
                                              None, None, None, None, None)

    asc = np.array([1, 5, 9], np.uint64)
    for call in (host, dev):
        assert call(ta=None) == -1 and call(tb=None) == -1
        assert call(n=-1) == -1
        assert call(src=None) == -1 and call(dst=None) == -1
        assert call(cap=-1) == -1
        assert call(out=None, cap=4) == -1
        assert call(nb=-1, edges=_p(asc)) == -1
        assert call(nb=1025, edges=_p(np.arange(1025, dtype=np.uint64))) == -1
        assert call(nb=3, edges=None) == -1
        for bad in ([1, 1, 9], [5, 1, 9], [1, 9, 5], [0, 0]):
            e = np.array(bad, np.uint64)
            assert call(nb=len(e), edges=_p(e)) == -1, bad
    assert lib.shdtopo_flow_impact_stats(None, None) == -1
    assert lib.shdtopo_flow_impact_stats(a._h, None) == -1
    for t in (a, b):
        check_no_device_used(t)
        assert t.stats()["sources"] == 0 and t.stats()["build_ms"] == 0


def test_unequal_attached_sets_are_refused_before_any_device_is_used():
    """Two topologies of one document, the second with the first 10 hosts only."""
    a, b, ips = _pair(hosts_b=tuple(range(10)))
    assert len(a.attached_vertices()) != len(b.attached_vertices())
    for x, y in ((a, b), (b, a)):
        with pytest.raises(RuntimeError) as e:
            x.flow_impact(y, ips[:8], ips[8:16])
        assert e.value.args[1] == -4
    for t in (a, b):
        check_no_device_used(t)
        assert t.stats()["sources"] == 0 and t.stats()["build_ms"] == 0


def test_same_topology_is_answered_on_the_host():
    a, _, ips = _pair()
    rng = np.random.default_rng(5)
    n = 300
    s, d = ips[rng.integers(0, len(ips), n)], ips[rng.integers(0, len(ips), n)]
    s[[0, 70]] = UNATTACHED_IP
    d[[70, 299]] = UNATTACHED_IP
    w = rng.integers(0, 2**64, n, dtype=np.uint64)
    ok = (s != UNATTACHED_IP) & (d != UNATTACHED_IP)
    assert ok.sum() == n - 3
    A = len(a.attached_vertices())
    for weight, want in ((w, int(w[ok].sum(dtype=np.uint64))), (None, int(ok.sum()))):
        got = a.flow_impact(a, s, d, weight=weight, rise_edges_ns=[0, 10, 2**63])
        assert got["total"] == 0 and len(got["records"]) == 0
        tt = got["totals"]
        assert (tt["flows"], tt["compared"], tt["unattached"]) == (n, n - 3, 3)
        assert tt["weight"] == want
        assert tt["worstFlow"] == -1 and tt["worstRise"] == 0.0
        for k in ("changed", "changedWeight", "delayRiseNs", "delayFallNs", "hopsRise", "hopsFall"):
            assert tt[k] == 0, k
        assert not tt["kindCount"].any() and not tt["kindWeight"].any()
        assert len(got["rise_count"]) == 4 and not got["rise_count"].any()
        assert not got["rise_weight"].any()
        assert len(got["src_changed_weight"]) == A and not got["src_changed_weight"].any()
        assert not got["dst_changed_weight"].any()
    st = a.flow_impact_stats()
    assert st["flows"] == n and st["changed"] == 0 and st["kernel_ms"] == 0
    assert st["words_skipped"] == (n + 63) // 64
    assert st["tile_flows"] >= 256 and st["tile_flows"] % 256 == 0
    # no flows at all
    got = a.flow_impact(a, [], [])
    assert got["total"] == 0 and got["totals"]["flows"] == 0 and got["totals"]["compared"] == 0
    check_no_device_used(a)
    assert a.stats()["sources"] == 0 and a.stats()["build_ms"] == 0


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_numpy_reference_agrees_with_a_plain_loop():
    """200 flows of `real`, one at a time in Python integers (sums modulo 2^64)."""
    c = case("real")
    fl = impact_flows("real")
    rose_at = fl["exp"]["records"]["flow"][fl["exp"]["records"]["kind"] & ROSE != 0]
    lo = max(0, int(rose_at[0]) - 100)
    sel = np.arange(lo, lo + 200)
    sc, dc, w, edges = fl["src_col"][sel], fl["dst_col"][sel], fl["weight"][sel], fl["edges"]
    exp = expected_impact(c["t0"], c["t1"], sc, dc, w, edges)
    _, lat0, rel0, hops0 = c["t0"]
    _, lat1, rel1, hops1 = c["t1"]
    A = len(c["t0"][0])
    tot = dict(compared=0, unattached=0, changed=0, weight=0, changedWeight=0, delayRiseNs=0,
               delayFallNs=0, hopsRise=0, hopsFall=0)
    kc, kw = [0] * 4, [0] * 4
    hist_c, hist_w = [0] * (len(edges) + 1), [0] * (len(edges) + 1)
    srcw, dstw = [0] * A, [0] * A
    worst, worst_flow, recs = 0.0, -1, []
    for i in range(200):
        s, d, wi = int(sc[i]), int(dc[i]), int(w[i])
        if not (0 <= s < A and 0 <= d < A):
            tot["unattached"] += 1
            continue
        tot["compared"] += 1
        tot["weight"] = (tot["weight"] + wi) & M64
        l0, l1 = float(lat0[s, d]), float(lat1[s, d])
        r0, r1 = float(rel0[s, d]), float(rel1[s, d])
        h0, h1 = int(hops0[s, d]), int(hops1[s, d])
        kind = 0
        if _bits(l0) != _bits(l1):
            kind |= ROSE if l1 > l0 else (FELL if l1 < l0 else 0)
        if _bits(r0) != _bits(r1):
            kind |= REL
        if h0 != h1:
            kind |= HOPS
        if not (_bits(l0) != _bits(l1) or _bits(r0) != _bits(r1) or h0 != h1):
            continue
        recs.append((i, l0, l1, r0, r1, h0, h1, kind))
        tot["changed"] += 1
        tot["changedWeight"] = (tot["changedWeight"] + wi) & M64
        for b in range(4):
            if kind >> b & 1:
                kc[b] += 1
                kw[b] = (kw[b] + wi) & M64
        d0, d1 = math.ceil(l0 * 1000000.0), math.ceil(l1 * 1000000.0)
        if kind & ROSE:
            up = d1 - d0
            tot["delayRiseNs"] = (tot["delayRiseNs"] + wi * up) & M64
            b = sum(1 for e in edges if int(e) <= up)
            hist_c[b] += 1
            hist_w[b] = (hist_w[b] + wi) & M64
            if worst_flow < 0 or l1 - l0 > worst:
                worst, worst_flow = l1 - l0, i
        if kind & FELL:
            tot["delayFallNs"] = (tot["delayFallNs"] + wi * (d0 - d1)) & M64
        if h1 > h0:
            tot["hopsRise"] = (tot["hopsRise"] + wi * (h1 - h0)) & M64
        if h1 < h0:
            tot["hopsFall"] = (tot["hopsFall"] + wi * (h0 - h1)) & M64
        srcw[s] = (srcw[s] + wi) & M64
        dstw[d] = (dstw[d] + wi) & M64
    assert tot["changed"] >= 10 and tot["unattached"] + tot["compared"] == 200
    assert sum(hist_c) >= 10
    for k, v in tot.items():
        assert int(exp["totals"][k]) == v, k
    assert exp["totals"]["kindCount"].tolist() == kc and exp["totals"]["kindWeight"].tolist() == kw
    assert exp["totals"]["worstFlow"] == worst_flow
    assert _bits(exp["totals"]["worstRise"]) == _bits(worst)
    assert exp["rise_count"].tolist() == hist_c and exp["rise_weight"].tolist() == hist_w
    assert exp["src_changed_weight"].tolist() == srcw
    assert exp["dst_changed_weight"].tolist() == dstw
    assert exp["total"] == len(recs)
    for r, want in zip(exp["records"], recs):
        got = (int(r["flow"]), float(r["lat0"]), float(r["lat1"]), float(r["rel0"]),
               float(r["rel1"]), int(r["hops0"]), int(r["hops1"]), int(r["kind"]))
        assert got == want
    # the columns the reference was given are the hosts' (impact_helpers.columns_of)
    assert np.array_equal(columns_of(c, fl["src_ip"][sel]), sc)
