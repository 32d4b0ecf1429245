"""Expected values and shared inputs of the flow impact tests (test_flow_impact.py,
test_flow_impact_cpu.py).

Every expected value comes from the CPU oracle's two tables of a what-if case
(whatif_helpers.case: t0 the parent's, t1 the child's) through numpy: gather per flow, compare
bits, ``np.ceil(lat * 1e6).astype(np.uint64)`` for the delays.  Every sum is a uint64 sum that
wraps, in numpy as in the product.  Nothing in this file calls ``table_diff`` or ``flow_impact``.
"""
import functools

import numpy as np

from helpers import host_ip
from whatif_helpers import FELL, HOPS, REL, ROSE, case

# one record of the impact (ShdFlowChange), restated: the product's dtype is not the reference
FLOW_CHANGE = np.dtype([("flow", np.int64), ("lat0", np.float64), ("lat1", np.float64),
                        ("rel0", np.float64), ("rel1", np.float64), ("hops0", np.uint16),
                        ("hops1", np.uint16), ("kind", np.uint32)])
TOTALS = ("flows", "compared", "unattached", "changed", "weight", "changedWeight", "kindCount",
          "kindWeight", "delayRiseNs", "delayFallNs", "hopsRise", "hopsFall", "worstRise",
          "worstFlow")
UNATTACHED_IP = host_ip(1000)
U64 = np.uint64


def check_no_device_used(top):
    """No call initialised a device: dev_inits is 0 -- except where a device is visible, where
    creating a topology initialises it in the background, once, whatever is called later."""
    n = top.stats()["dev_inits"]
    if n:
        import torch
        assert n == 1 and torch.cuda.is_available()


def delay_ns(lat):
    """The packet route's delay."""
    return np.ceil(lat * 1e6).astype(U64)


def columns_of(c, ips, attached=None):
    """Columns of the hosts' IPs in the tables of case c (-1: not attached); attached: the columns'
    vertices where they are no longer the case's."""
    vert = dict(zip(c["ips"], c["verts"]))
    col = {int(v): k for k, v in enumerate(c["t0"][0] if attached is None else attached)}
    return np.array([col.get(vert.get(int(ip), -1), -1) for ip in ips], np.int32)


def usum(x):
    return int(np.asarray(x, U64).sum(dtype=U64))


def expected_impact(t0, t1, sc, dc, w, edges):
    """The impact of the flows (columns sc -> dc, outside [0, A): unattached; weights w or None)
    between two oracle tables, in numpy: a dict with the keys of Topology.flow_impact."""
    a0, lat0, rel0, hops0 = t0
    a1, lat1, rel1, hops1 = t1
    assert np.array_equal(a0, a1)
    A, n = len(a0), len(sc)
    sc, dc = np.asarray(sc, np.int64), np.asarray(dc, np.int64)
    w = np.ones(n, U64) if w is None else np.asarray(w).astype(U64)
    edges = np.asarray(edges, U64).reshape(-1)
    nb = len(edges)
    ok = (sc >= 0) & (sc < A) & (dc >= 0) & (dc < A)
    s, d = np.where(ok, sc, 0), np.where(ok, dc, 0)
    if A == 0:
        l0 = l1 = r0 = r1 = np.zeros(n)
        h0 = h1 = np.zeros(n, np.uint16)
    else:
        l0, l1, r0, r1 = lat0[s, d], lat1[s, d], rel0[s, d], rel1[s, d]
        h0, h1 = hops0[s, d].astype(np.uint16), hops1[s, d].astype(np.uint16)
    dl = ok & (l0.view(U64) != l1.view(U64))
    dr = ok & (r0.view(U64) != r1.view(U64))
    dh = ok & (h0 != h1)
    rose, fell = dl & (l1 > l0), dl & (l1 < l0)
    kind = (rose * ROSE + fell * FELL + dr * REL + dh * HOPS).astype(np.uint32)
    changed = dl | dr | dh
    idx = np.flatnonzero(changed)
    rec = np.zeros(len(idx), FLOW_CHANGE)
    rec["flow"] = idx
    rec["lat0"], rec["lat1"], rec["rel0"], rec["rel1"] = l0[idx], l1[idx], r0[idx], r1[idx]
    rec["hops0"], rec["hops1"], rec["kind"] = h0[idx], h1[idx], kind[idx]
    d0, d1 = delay_ns(np.where(ok, l0, 0.0)), delay_ns(np.where(ok, l1, 0.0))
    up, down = (d1 - d0)[rose], (d0 - d1)[fell]
    # (both imply "changed"; a flow that is not compared gathered pair (0, 0) above and counts for
    # nothing: "Flow i is compared when both ends are columns", include/shd_topology_abi.h)
    hup, hdown = ok & (h1 > h0), ok & (h1 < h0)
    hd = lambda m, x, y: (x[m].astype(U64) - y[m].astype(U64)) * w[m]
    bits = (ROSE, FELL, REL, HOPS)
    totals = {
        "flows": n, "compared": int(ok.sum()), "unattached": int(n - ok.sum()),
        "changed": len(idx), "weight": usum(w[ok]), "changedWeight": usum(w[changed]),
        "kindCount": np.array([(kind & b != 0).sum() for b in bits], U64),
        "kindWeight": np.array([usum(w[kind & b != 0]) for b in bits], U64),
        "delayRiseNs": usum(w[rose] * up), "delayFallNs": usum(w[fell] * down),
        "hopsRise": usum(hd(hup, h1, h0)), "hopsFall": usum(hd(hdown, h0, h1)),
        "worstRise": 0.0, "worstFlow": -1,
    }
    if rose.any():
        r = np.where(rose, l1 - l0, -np.inf)
        totals["worstRise"] = float(r.max())
        totals["worstFlow"] = int(np.flatnonzero(r == r.max())[0])
    b = np.searchsorted(edges, up, side="right")  # the number of edges <= the rise
    rise_count = np.bincount(b, minlength=nb + 1).astype(U64)
    rise_weight = np.zeros(nb + 1, U64)
    np.add.at(rise_weight, b, w[rose])
    srcw, dstw = np.zeros(A, U64), np.zeros(A, U64)
    np.add.at(srcw, sc[changed], w[changed])
    np.add.at(dstw, dc[changed], w[changed])
    return {"total": len(idx), "records": rec, "totals": totals, "rise_count": rise_count,
            "rise_weight": rise_weight, "src_changed_weight": srcw, "dst_changed_weight": dstw,
            "rises_ns": up}


def assert_impact_equal(got, exp, cap=None, what=""):
    """Every output of flow_impact against expected_impact; records are the first `cap`."""
    assert got["total"] == exp["total"], what
    n = exp["total"] if cap is None else min(cap, exp["total"])
    assert len(got["records"]) == n, what
    for f in FLOW_CHANGE.names:
        x, y = got["records"][f], exp["records"][f][:n]
        if x.dtype == np.float64:
            x, y = x.view(U64), np.ascontiguousarray(y).view(U64)
        assert np.array_equal(x, y), (what, f)
    assert_sums_equal(got, exp, what)


def assert_sums_equal(got, exp, what=""):
    """Everything but the records."""
    assert set(got["totals"]) == set(TOTALS)
    for k in TOTALS:
        x, y = got["totals"][k], exp["totals"][k]
        if k == "worstRise":
            assert np.float64(x).view(U64) == np.float64(y).view(U64), (what, k, x, y)
        elif k.startswith("kind"):
            assert np.array_equal(x, y), (what, k, x, y)
        else:
            assert int(x) == int(y), (what, k, x, y)
    for k in ("rise_count", "rise_weight", "src_changed_weight", "dst_changed_weight"):
        assert got[k].dtype == U64 and np.array_equal(got[k], exp[k]), (what, k)


@functools.lru_cache(maxsize=None)
def impact_flows(name, seed=23):
    """The flow recipe on whatif_helpers.case(name): dict with src_ip, dst_ip (uint32), weight
    (uint64, full range: every sum wraps), src_col, dst_col (-1: unattached), edges (uint64) and
    exp, the expected impact of all flows (computed once, shared, never modified)."""
    c = case(name)
    rng = np.random.default_rng(seed)
    ips = np.array(c["ips"], np.uint32)
    a = c["t0"][0]
    first_host = {}
    for ip, v in zip(c["ips"], c["verts"]):
        first_host.setdefault(int(v), ip)
    colip = np.array([first_host[int(v)] for v in a], np.uint32)
    H, A = len(ips), len(a)
    rec = c["exp"]["records"]
    # 1. random host pairs
    src, dst = [ips[rng.integers(0, H, 3000)]], [ips[rng.integers(0, H, 3000)]]
    # 2. one flow per changed pair, the first host on each vertex
    src.append(colip[rec["srcCol"]])
    dst.append(colip[rec["dstCol"]])
    # 3. full and empty ballot words in the middle of the array
    if len(rec):
        src.append(np.repeat(colip[rec["srcCol"][0]], 130))
        dst.append(np.repeat(colip[rec["dstCol"][0]], 130))
    ch = np.zeros((A, A), bool)
    ch[rec["srcCol"], rec["dstCol"]] = True
    same = np.argwhere(~ch & ~np.eye(A, dtype=bool))  # row-major: the first unchanged pair
    if len(same):
        src.append(np.repeat(colip[same[0][0]], 130))
        dst.append(np.repeat(colip[same[0][1]], 130))
    # 4. every host's self pair
    src.append(ips)
    dst.append(ips)
    # 5. two more copies of the pair with the worst latency rise
    rose = rec[rec["kind"] & ROSE != 0]
    if len(rose):
        k = int(np.argmax(rose["lat1"] - rose["lat0"]))
        src.append(np.repeat(colip[rose["srcCol"][k]], 2))
        dst.append(np.repeat(colip[rose["dstCol"][k]], 2))
    src, dst = np.concatenate(src), np.concatenate(dst)
    # 6. five flows with an unattached end at 0, 63, 64, the middle and the last index
    n = len(src) + 5
    at = np.array([0, 63, 64, n // 2, n - 1])
    keep = np.ones(n, bool)
    keep[at] = False
    s, d = np.empty(n, np.uint32), np.empty(n, np.uint32)
    s[keep], d[keep] = src, dst
    s[at], d[at] = ips[rng.integers(0, H, 5)], ips[rng.integers(0, H, 5)]
    s[at[[0, 2, 4]]] = UNATTACHED_IP
    d[at[[1, 3]]] = UNATTACHED_IP
    w = rng.integers(0, 2**64, n, dtype=U64)
    sc, dc = columns_of(c, s), columns_of(c, d)
    # histogram edges: 0, the quartiles of the expected rises, one rise exactly, 2^63
    rises = expected_impact(c["t0"], c["t1"], sc, dc, w, [])["rises_ns"]
    e = [0, 2**63]
    if len(rises):
        e += [int(x) for x in np.quantile(rises, [0.25, 0.5, 0.75], method="lower")]
        e.append(int(np.sort(rises)[len(rises) // 3]))
    edges = np.unique(np.array(e, U64))
    exp = expected_impact(c["t0"], c["t1"], sc, dc, w, edges)
    return dict(src_ip=s, dst_ip=d, weight=w, src_col=sc, dst_col=dc, edges=edges, exp=exp,
                unattached_at=at)


def prefix(fl, c, n):
    """The expected impact of the first n flows of fl."""
    return expected_impact(c["t0"], c["t1"], fl["src_col"][:n], fl["dst_col"][:n],
                           fl["weight"][:n], fl["edges"])
