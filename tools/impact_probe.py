"""Probe: what a flow impact costs on the C4 topology -- 1,000,000 vertices, 10,000,000 edges,
10,000 attached poi, 100,000 hosts: fail the 16 heaviest router-router edges (the failing set of
tools/whatif_probe.py), build the derived table and ask what that does to two sets of flows
(Topology.flow_impact, Topology.flow_impact_device), next to what a user does without the call.

Flow sets
  slice   the 2.56 M flows of tools/load_probe.py: 256 sources x all attached, weights U{1..1448}
  window  the 10 M packets of one scheduler window (synth_packets), weight = payload

In one process on one box, after one unmeasured round, --reps measured rounds of

  host     flow_impact by IPs and u64 weights with cap given (one call, no sizing pass): total_ms,
           resolve_ms, kernel_ms (count, scan, fill) and fill_ms from the call's own counters
           (shdtopo_flow_impact_stats)
  device   flow_impact_device on the sets' column and payload arrays in HBM: the same counters
  count    flow_impact_device with cap = 0 on the window: kernel_ms is the count pass and the scan
           alone; its random-request rate is 4 x compared flows / kernel_ms, next to
           packet_route_kernel's on the same columns (one request per packet, route_kernel_ms)
  tables   the first alternative: two table_to_host copies, then per set a numpy gather of both
           tables per flow and the comparison
  records  the second alternative: table_diff's records, then per set a numpy join of the flows
           on srcCol * A + dstCol (a searchsorted into the records' keys, which are ascending)

Both alternatives must find the changed flows the call reports, and the same changedWeight,
delayRiseNs and kind counts: "agrees" in the summary.  One JSON line per round, then one summary
line with the medians and the range.

usage: python tools/impact_probe.py [--reps N] [--fail N] [--small]
  --reps   measured rounds, default 5
  --fail   edges to fail, default 16
  --small  a 30,000-vertex topology with 300 poi and a 100,000-packet window (a dry run of the
           tool, not a measurement)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shadow_amd as sa  # noqa: E402

U64 = np.uint64


def med(xs):
    return [round(float(np.median(xs)), 4), round(float(min(xs)), 4), round(float(max(xs)), 4)]


def ns(lat):
    return np.ceil(lat * 1e6).astype(U64)


def sums(w, lat0, lat1, kind):
    """What both alternatives must reproduce, from the changed flows' values."""
    rose = kind & 1 != 0
    return {"changed": int(len(w)), "changedWeight": int(w.sum(dtype=U64)),
            "delayRiseNs": int((w[rose] * (ns(lat1[rose]) - ns(lat0[rose]))).sum(dtype=U64)),
            "kindCount": [int((kind & b != 0).sum()) for b in (1, 2, 4, 8)]}


def from_tables(t0, t1, sc, dc, w):
    """Alternative 1: gather both host tables per flow and compare."""
    _, lat0, rel0, hops0 = t0
    _, lat1, rel1, hops1 = t1
    l0, l1 = lat0[sc, dc], lat1[sc, dc]
    dl = l0.view(U64) != l1.view(U64)
    dr = rel0[sc, dc].view(U64) != rel1[sc, dc].view(U64)
    dh = hops0[sc, dc] != hops1[sc, dc]
    idx = np.flatnonzero(dl | dr | dh)
    l0, l1 = l0[idx], l1[idx]
    kind = ((dl[idx] & (l1 > l0)) * 1 + (dl[idx] & (l1 < l0)) * 2 + dr[idx] * 4 + dh[idx] * 8)
    return idx, sums(w[idx], l0, l1, kind.astype(np.uint32))


def from_records(rec, A, sc, dc, w):
    """Alternative 2: join the flows with the diff's records on srcCol * A + dstCol."""
    key = rec["srcCol"].astype(np.int64) * A + rec["dstCol"]  # row-major: ascending
    fk = sc.astype(np.int64) * A + dc
    pos = np.minimum(np.searchsorted(key, fk), max(len(key) - 1, 0))
    hit = key[pos] == fk if len(key) else np.zeros(len(fk), bool)
    idx = np.flatnonzero(hit)
    r = rec[pos[idx]]
    return idx, sums(w[idx], r["lat0"], r["lat1"], r["kind"])


def same(got, idx, s):
    tt = got["totals"]
    return bool(np.array_equal(got["records"]["flow"], idx) and s["changed"] == got["total"] and
                s["changedWeight"] == tt["changedWeight"] and
                s["delayRiseNs"] == tt["delayRiseNs"] and
                s["kindCount"] == [int(x) for x in tt["kindCount"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fail", type=int, default=16)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("impact_probe needs the GPU: tables are built and joined on the device")
    t0 = time.time()
    if args.small:
        top = sa.Topology.synthetic(seed=20261015, n_routers=29_700, n_poi=300, n_edges=300_000)
        hosts, packets = 3000, 100_000
    else:
        top = sa.Topology.synthetic(seed=20261015)
        hosts, packets = 100_000, 10_000_000
    pk = top.synth_packets(20261015, hosts, packets, 10**9, 10**7)  # host k < poi count: poi k
    attached = top.attached_vertices()
    A = len(attached)
    V, eu, ev, _, _, _ = top.export_graph()
    is_poi = np.zeros(V, bool)
    is_poi[attached] = True
    routers = np.flatnonzero(~is_poi[eu] & ~is_poi[ev] & (eu != ev))
    top.build()
    ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255, (k + 1) >> 8 & 255,
                                                        (k + 1) & 255)) for k in range(A)],
                     np.uint32)
    msrc = min(256, A)
    s_ip, d_ip = np.repeat(ips[:msrc], A), np.tile(ips, msrc)
    w = np.random.default_rng(1).integers(1, 1449, len(s_ip)).astype(U64)
    load = top.link_load(s_ip, d_ip, w)
    traffic = (load["edge_fwd"] + load["edge_rev"])[routers]
    fail = routers[np.argsort(np.iinfo(U64).max - traffic, kind="stable")[:args.fail]]
    child = top.without(edges=fail.astype(np.int32))
    child.build()
    col_of = {int(ip): top.column_of_ip(int(ip)) for ip in ips}
    cu = lambda x, view=None: torch.from_numpy(
        np.ascontiguousarray(x).view(view) if view else np.ascontiguousarray(x)).cuda()
    sets = {
        "slice": dict(src_ip=s_ip, dst_ip=d_ip, w=w,
                      sc=np.array([col_of[int(x)] for x in ips[:msrc]], np.int32).repeat(A),
                      dc=np.tile(np.array([col_of[int(x)] for x in ips], np.int32), msrc),
                      pay=w.astype(np.uint32)),
        "window": dict(src_ip=pk["src_ip"], dst_ip=pk["dst_ip"], w=pk["payload"].astype(U64),
                       sc=pk["src_col"], dc=pk["dst_col"], pay=pk["payload"]),
    }
    for x in sets.values():
        x["d_sc"], x["d_dc"], x["d_pay"] = cu(x["sc"]), cu(x["dc"]), cu(x["pay"], np.int32)
    edges = [0] + [int(10**k) for k in range(3, 9)]  # 1 us .. 100 ms, in decades
    wd = sets["window"]
    n_w = len(wd["sc"])
    route_in = [wd["d_sc"], wd["d_dc"], wd["d_pay"], cu(pk["state_in"], np.int32),
                cu(pk["now"], np.int64)]
    route_out = [torch.empty(n_w, dtype=torch.int64, device="cuda"),
                 torch.empty(n_w, dtype=torch.int32, device="cuda"),
                 torch.empty(n_w, dtype=torch.uint8, device="cuda")]
    jump = int(top.getMinimumLatency()) * 1_000_000
    head = {"topology": "C4", "small": args.small, "vertices": top.num_vertices,
            "edges": top.num_edges, "attached": A, "reps": args.reps,
            "failed_edges": [int(e) for e in fail], "rise_edges_ns": edges,
            "flows": {k: len(v["sc"]) for k, v in sets.items()},
            "tile_flows": top.flow_impact_stats()["tile_flows"], "setup_s": round(time.time() - t0, 2)}
    print(json.dumps(head), flush=True)

    t = {}
    info = {k: {} for k in sets}
    agree = True
    for rep in range(-1, args.reps):  # round -1 is not measured
        row = {}
        got = {}
        for name, x in sets.items():
            cap = max(1, info[name].get("changed") or
                      top.flow_impact(child, x["src_ip"], x["dst_ip"], cap=0)["total"])
            t1 = time.time()
            out = top.flow_impact(child, x["src_ip"], x["dst_ip"], weight=x["w"],
                                  rise_edges_ns=edges, cap=cap)
            row[name + "_host_wall"] = 1e3 * (time.time() - t1)
            st = top.flow_impact_stats()
            for k in ("total_ms", "resolve_ms", "kernel_ms", "fill_ms"):
                row["%s_host_%s" % (name, k)] = st[k]
            t1 = time.time()
            dev = top.flow_impact_device(child, x["d_sc"], x["d_dc"], payload=x["d_pay"],
                                         rise_edges_ns=edges, cap=cap)
            row[name + "_device_wall"] = 1e3 * (time.time() - t1)
            st = top.flow_impact_stats()
            for k in ("total_ms", "resolve_ms", "kernel_ms", "fill_ms"):
                row["%s_device_%s" % (name, k)] = st[k]
            agree = agree and out["records"].tobytes() == dev["records"].tobytes() and \
                out["totals"]["delayRiseNs"] == dev["totals"]["delayRiseNs"]
            tt = out["totals"]
            info[name].update(
                changed=out["total"], compared=tt["compared"], unattached=tt["unattached"],
                changed_weight=tt["changedWeight"], weight=tt["weight"],
                delay_rise_ns=tt["delayRiseNs"], hops_rise=tt["hopsRise"],
                kind_count=[int(v) for v in tt["kindCount"]], worst_rise=tt["worstRise"],
                worst_flow=tt["worstFlow"], rise_count=[int(v) for v in out["rise_count"]],
                words_skipped=st["words_skipped"], words=(len(x["sc"]) + 63) // 64,
                bytes_model=st["bytes_model"])
            got[name] = out
        # the count pass alone, next to the packet route on the same columns
        z = top.flow_impact_device(child, wd["d_sc"], wd["d_dc"], payload=wd["d_pay"],
                                   rise_edges_ns=edges, cap=0)
        row["count_kernel"] = top.flow_impact_stats()["kernel_ms"]
        row["count_g_requests_per_s"] = 4 * z["totals"]["compared"] / row["count_kernel"] / 1e6
        top.route_batch_device(*route_in, jump, 1, *route_out)
        torch.cuda.synchronize()
        row["route_kernel"] = top.stats()["route_kernel_ms"]
        row["route_g_requests_per_s"] = n_w / row["route_kernel"] / 1e6
        # alternative 1: both tables on the host
        t1 = time.time()
        t_parent, t_child = top.table(), child.table()
        row["tables_copy"] = 1e3 * (time.time() - t1)
        for name, x in sets.items():
            t1 = time.time()
            idx, s = from_tables(t_parent, t_child, x["sc"], x["dc"], x["w"])
            row[name + "_tables_gather"] = 1e3 * (time.time() - t1)
            agree = agree and same(got[name], idx, s)
        del t_parent, t_child
        # alternative 2: the diff's records
        total = info.get("pairs_changed") or top.table_diff(child, cap=0)["total"]
        info["pairs_changed"] = total
        t1 = time.time()
        rec = top.table_diff(child, cap=max(1, total))["records"]
        row["records_diff"] = 1e3 * (time.time() - t1)
        for name, x in sets.items():
            t1 = time.time()
            idx, s = from_records(rec, A, x["sc"], x["dc"], x["w"])
            row[name + "_records_join"] = 1e3 * (time.time() - t1)
            agree = agree and same(got[name], idx, s)
        del rec, got
        if rep < 0:
            continue
        for k, v in row.items():
            t.setdefault(k, []).append(v)
        print(json.dumps({"rep": rep, **{k: round(v, 4) for k, v in row.items()}}), flush=True)
    summary = {"summary": "medians of %d rounds [median, min, max]; ms unless named" % args.reps,
               "failed": len(fail), **info, "alternatives_agree": bool(agree)}
    for k, v in t.items():
        summary[k] = med(v)
    for name in sets:
        summary[name + "_tables_ms"] = med([a + b for a, b in
                                            zip(t["tables_copy"], t[name + "_tables_gather"])])
        summary[name + "_records_ms"] = med([a + b for a, b in
                                             zip(t["records_diff"], t[name + "_records_join"])])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
