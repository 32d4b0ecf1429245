"""Probe: what a load shift costs on the C4 topology -- 1,000,000 vertices, 10,000,000 edges,
10,000 attached poi, 100,000 hosts: fail the 16 heaviest router-router edges (the failing set of
tools/whatif_probe.py and tools/impact_probe.py) and ask where the traffic of two sets of flows
goes (Topology.load_shift), next to what a user does without the call.

Flow sets
  slice   the 2.56 M flows of tools/load_probe.py: 256 sources x all attached, weights U{1..1448}
  one     one source to all attached (load_probe's call (a)), the same weights

In one process on one box, after one unmeasured round, --reps measured rounds of

  shift    load_shift with cap given (one call, no sizing pass): total_ms, resolve_ms, the two
           accumulations' wall times (load_a_ms, load_b_ms), kernel_ms (count, reduce, scan, fill)
           and the rate bytes_model / kernel_ms, from the call's own counters
           (shdtopo_load_shift_stats)
  numpy    the alternative: link_load on the parent, link_load on the child, edge_origin, and the
           join in numpy (scatter the child's loads to the root's ids, compare, nonzero)

Both must find the same entries with the same loads: "agrees" in the summary.  One JSON line per
round, then one summary line with the medians and the range.

usage: python tools/shift_probe.py [--reps N] [--fail N] [--small]
  --reps   measured rounds, default 5
  --fail   edges to fail, default 16
  --small  a 30,000-vertex topology with 300 poi (a dry run of the tool, not a measurement)
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


def numpy_join(la, lb, origin, R, V):
    """The alternative's last step: both loads in the root's numbering, and the entries that
    differ (x, before, after)."""
    before = np.concatenate([la["edge_fwd"], la["edge_rev"], la["vertex"]])
    after = np.zeros(2 * R + V, U64)
    after[origin] = lb["edge_fwd"]
    after[R + origin] = lb["edge_rev"]
    after[2 * R:] = lb["vertex"]
    x = np.flatnonzero(before != after)
    return x, before[x], after[x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fail", type=int, default=16)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("shift_probe needs the GPU: the loads are accumulated and compared on the device")
    t0 = time.time()
    if args.small:
        top = sa.Topology.synthetic(seed=20261015, n_routers=29_700, n_poi=300, n_edges=300_000)
        hosts = 3000
    else:
        top = sa.Topology.synthetic(seed=20261015)
        hosts = 100_000
    top.synth_packets(20261015, hosts, 1000, 10**9, 10**7)  # attaches: host k < poi count: poi k
    attached = top.attached_vertices()
    A = len(attached)
    V, eu, ev, _, _, _ = top.export_graph()
    R = top.num_edges
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
    sets = {"slice": dict(src_ip=s_ip, dst_ip=d_ip, w=w),
            "one": dict(src_ip=np.repeat(ips[5], A), dst_ip=ips, w=w[:A].copy())}
    head = {"topology": "C4", "small": args.small, "vertices": V, "edges": R, "attached": A,
            "reps": args.reps, "failed_edges": [int(e) for e in fail],
            "flows": {k: len(v["w"]) for k, v in sets.items()}, "entries": 2 * R + V,
            "tile_entries": top.load_shift_stats()["tile_entries"],
            "setup_s": round(time.time() - t0, 2)}
    print(json.dumps(head), flush=True)

    t = {}
    info = {k: {} for k in sets}
    agree = True
    for rep in range(-1, args.reps):  # round -1 is not measured
        row = {}
        for name, x in sets.items():
            cap = max(1, info[name].get("changed") or
                      top.load_shift(child, x["src_ip"], x["dst_ip"], weight=x["w"],
                                     cap=0)["total"])
            t1 = time.time()
            out = top.load_shift(child, x["src_ip"], x["dst_ip"], weight=x["w"], cap=cap)
            row[name + "_shift_wall"] = 1e3 * (time.time() - t1)
            st = top.load_shift_stats()
            for k in ("total_ms", "resolve_ms", "load_a_ms", "load_b_ms", "kernel_ms"):
                row["%s_shift_%s" % (name, k)] = st[k]
            row[name + "_kernel_tb_per_s"] = st["bytes_model"] / st["kernel_ms"] / 1e9
            info[name].update(
                changed=out["total"], by_kind=[int(v) for v in out["changed"]],
                gained=[int(v) for v in out["gained"]], lost=[int(v) for v in out["lost"]],
                newly_used=[int(v) for v in out["newlyUsed"]],
                abandoned=[int(v) for v in out["abandoned"]], displaced=int(out["displaced"]),
                worst_gain=int(out["worstGain"]), worst_gain_index=int(out["worstGainIndex"]),
                peak_before=int(out["peakBefore"]), peak_after=int(out["peakAfter"]),
                peak_after_index=int(out["peakAfterIndex"]),
                hop_weight=[int(out["hopWeightA"]), int(out["hopWeightB"])],
                words_skipped=st["words_skipped"], words=(st["entries"] + 63) // 64,
                bytes_model=st["bytes_model"])
            # the alternative: two link_load calls, edge_origin and the join in numpy
            t1 = time.time()
            la = top.link_load(x["src_ip"], x["dst_ip"], x["w"])
            t2 = time.time()
            lb = child.link_load(x["src_ip"], x["dst_ip"], x["w"])
            t3 = time.time()
            origin = child.edge_origin()
            xs, before, after = numpy_join(la, lb, origin, R, V)
            t4 = time.time()
            row[name + "_numpy_load_a"] = 1e3 * (t2 - t1)
            row[name + "_numpy_load_b"] = 1e3 * (t3 - t2)
            row[name + "_numpy_join"] = 1e3 * (t4 - t3)
            row[name + "_numpy_ms"] = 1e3 * (t4 - t1)
            rec = out["records"]
            gx = np.where(rec["kind"] == 2, 2 * R, rec["kind"].astype(np.int64) * R) + rec["id"]
            agree = agree and bool(np.array_equal(gx, xs) and np.array_equal(rec["before"], before)
                                   and np.array_equal(rec["after"], after))
            assert agree, "load_shift and the numpy join disagree on %s" % name
            del la, lb, out
        if rep < 0:
            continue
        for k, v in row.items():
            t.setdefault(k, []).append(v)
        print(json.dumps({"rep": rep, **{k: round(v, 4) for k, v in row.items()}}), flush=True)
    summary = {"summary": "medians of %d rounds [median, min, max]; ms unless named" % args.reps,
               "failed": len(fail), **info, "alternatives_agree": bool(agree)}
    for k, v in t.items():
        summary[k] = med(v)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
