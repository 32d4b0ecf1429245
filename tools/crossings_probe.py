"""Probe: what a link-crossings call (shdtopo_link_crossings) costs on the C4 topology --
1,000,000 vertices, 10,000,000 edges, 10,000 attached poi, the table built -- next to a link load
of the same flows (existing code, the yardstick) and next to what a user does without it: trace
every flow and filter the routes in numpy.

Three sets of flows (those of tools/load_probe.py): (a) one source to all attached, (b) 256
sources x all attached (a 2.56 M-flow slice of a traffic matrix), (c) 5,000 sources with one pair
each; weights U{1..1448}.  The watches are the 16 heaviest edges and the 16 heaviest vertices of a
link load of the same flows.  Per case, in one process on one box, after one unmeasured call of
each kind, --reps alternating rounds of

  crossings     Topology.link_crossings with cap given (one call, no sizing pass): total_ms,
                kernel_ms and batch_ms from the call's own counters (shdtopo_link_crossings_stats)
  load          Topology.link_load: total_ms and load_kernel_ms (shdtopo_link_load_stats)
  trace+filter  Topology.trace_routes with cap given, then the same records from its vertices and
                edges in numpy: wall time of both steps, and of the trace alone

One JSON line per round and kind, then one summary line per case with the medians and the range.
The records of the numpy filter are compared with the call's (a dry check; the tests compare with
the oracle).

usage: python tools/crossings_probe.py [--reps N] [--sources N] [--matrix-sources N] [--small]
  --reps            measured rounds per case, default 5
  --sources         distinct sources of case (c), default 5000
  --matrix-sources  sources of case (b), default 256
  --small           a 30,000-vertex topology with 300 poi (a dry run of the tool, not a measurement)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shadow_amd as sa  # noqa: E402


def filter_routes(tr, eu, V, edges, vertices):
    """The call's records from a trace of the same flows, on the host: every hop of every written
    route tested against the watch lists (numpy; sorted by flow, hop, edge before vertex)."""
    ne = len(edges)
    hops = np.where(tr["status"] == 0, tr["hops"], 0).astype(np.int64)
    n = len(hops)
    flow = np.repeat(np.arange(n), hops)
    first = np.repeat(tr["offset"], hops)
    hop = np.arange(len(flow)) - np.repeat(np.cumsum(hops) - hops, hops)
    pos = first + hop
    e, a, b = tr["edges"][pos], tr["vertices"][pos], tr["vertices"][pos + 1]
    emap = np.full(len(eu), -1, np.int32)
    emap[edges] = np.arange(ne)
    vmap = np.full(V, -1, np.int32)
    vmap[vertices] = ne + np.arange(len(vertices))
    ke, kv = emap[e], vmap[b]
    he, hv = ke >= 0, kv >= 0
    rec = np.zeros(int(he.sum() + hv.sum()), sa.CROSSING_DTYPE)
    m = int(he.sum())
    rec["flow"][:m], rec["watch"][:m], rec["hop"][:m] = flow[he], ke[he], hop[he]
    rec["reverse"][:m] = (eu[e[he]] != a[he]) & (a[he] != b[he])
    rec["flow"][m:], rec["watch"][m:], rec["hop"][m:] = flow[hv], kv[hv], hop[hv]
    kind = np.concatenate([np.zeros(m, np.int64), np.ones(len(rec) - m, np.int64)])
    return rec[np.lexsort((kind, rec["hop"], rec["flow"]))]


def med(xs):
    return round(float(np.median(xs)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sources", type=int, default=5000)
    ap.add_argument("--matrix-sources", type=int, default=256)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("crossings_probe needs the GPU: the chains of an SSSP topology are on the device")
    t0 = time.time()
    if args.small:
        top = sa.Topology.synthetic(seed=20261015, n_routers=29_700, n_poi=300, n_edges=300_000)
        hosts = 3000
    else:
        top = sa.Topology.synthetic(seed=20261015)
        hosts = 100_000
    top.synth_packets(20261015, hosts, 1000, 10**9, 10**7)  # host k < poi count sits on poi k
    A = len(top.attached_vertices())
    t1 = time.time()
    top.build()
    build_s = round(time.time() - t1, 2)
    eu = top.export_graph()[1]
    ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255, (k + 1) >> 8 & 255,
                                                       (k + 1) & 255)) for k in range(A)], np.uint32)
    print(json.dumps({"topology": "C4", "small": args.small, "vertices": top.num_vertices,
                      "edges": top.num_edges, "attached": A, "table_build_s": build_s,
                      "reps": args.reps, "setup_s": round(time.time() - t0, 2)}), flush=True)
    nsrc = min(args.sources, A - 1)
    msrc = min(args.matrix_sources, A)
    rng = np.random.default_rng(1)
    cases = [
        ("(a) one source to all %d attached" % A, np.repeat(ips[5], A), ips),
        ("(b) %d sources x all %d attached" % (msrc, A), np.repeat(ips[:msrc], A),
         np.tile(ips, msrc)),
        ("(c) %d distinct sources, one pair each" % nsrc, ips[:nsrc],
         ips[(np.arange(nsrc) + 1 + rng.integers(0, A - 1, nsrc)) % A]),
    ]
    # the first call of a topology also uploads the replay's CSR and the edge ids
    top.link_load(ips[[1]], ips[[2]])
    for name, s, d in cases:
        w = rng.integers(1, 1449, len(s)).astype(np.uint64)  # payload bytes
        load = top.link_load(s, d, w)  # (also the load's unmeasured call)
        heavy = lambda x: np.argsort(np.iinfo(np.uint64).max - x, kind="stable")[:16]
        edges = heavy(load["edge_fwd"] + load["edge_rev"]).astype(np.int32)
        vertices = heavy(load["vertex"]).astype(np.int32)
        sized = top.link_crossings(s, d, edges, vertices, w)  # sizing + filling: unmeasured
        cap, tcap = max(int(sized["total"]), 1), 16 * len(s)
        tr = top.trace_routes(s, d, cap=tcap)
        rec = filter_routes(tr, eu, top.num_vertices, edges, vertices)
        same = rec.tobytes() == sized["records"].tobytes()
        t = {k: [] for k in ("x_total", "x_kernel", "x_batch", "x_wall", "l_total", "l_kernel",
                             "l_wall", "tf_wall", "t_wall", "t_total")}
        for rep in range(args.reps):
            t1 = time.time()
            out = top.link_crossings(s, d, edges, vertices, w, cap=cap)
            t["x_wall"].append(1e3 * (time.time() - t1))
            cs = top.link_crossings_stats()
            t["x_total"].append(cs["total_ms"])
            t["x_kernel"].append(cs["kernel_ms"])
            t["x_batch"].append(cs["batch_ms"])
            t1 = time.time()
            top.link_load(s, d, w)
            t["l_wall"].append(1e3 * (time.time() - t1))
            ls = top.link_load_stats()
            t["l_total"].append(ls["total_ms"])
            t["l_kernel"].append(ls["load_kernel_ms"])
            t1 = time.time()
            tr = top.trace_routes(s, d, cap=tcap)
            t["t_wall"].append(1e3 * (time.time() - t1))
            rec = filter_routes(tr, eu, top.num_vertices, edges, vertices)
            t["tf_wall"].append(1e3 * (time.time() - t1))
            t["t_total"].append(top.trace_stats()["total_ms"])
            same = same and rec.tobytes() == out["records"].tobytes()
            print(json.dumps({"case": name, "rep": rep,
                              **{k: round(v[-1], 3) for k, v in t.items()}}), flush=True)
        print(json.dumps({
            "case": name, "summary": "medians of %d rounds [min, max]" % args.reps,
            "requests": int(len(s)), "watched_edges": len(edges), "watched_vertices": len(vertices),
            "crossings": cs["crossings"], "flows_hit": cs["flows_hit"], "routed": cs["routed"],
            "sources": cs["sources"], "chunks": cs["chunks"],
            "batch_sources": cs["batch_sources"], "batch_fallback": cs["batch_fallback"],
            "route_entries": int(tr["total"]), "filter_agrees": bool(same),
            "crossings_total_ms": [med(t["x_total"]), round(min(t["x_total"]), 3), round(max(t["x_total"]), 3)],
            "crossings_kernel_ms": [med(t["x_kernel"]), round(min(t["x_kernel"]), 3), round(max(t["x_kernel"]), 3)],
            "crossings_batch_ms": med(t["x_batch"]),
            "crossings_python_wall_ms": med(t["x_wall"]),
            "load_total_ms": [med(t["l_total"]), round(min(t["l_total"]), 3), round(max(t["l_total"]), 3)],
            "load_kernel_ms": [med(t["l_kernel"]), round(min(t["l_kernel"]), 3), round(max(t["l_kernel"]), 3)],
            "load_python_wall_ms": med(t["l_wall"]),
            "trace_and_filter_wall_ms": [med(t["tf_wall"]), round(min(t["tf_wall"]), 3), round(max(t["tf_wall"]), 3)],
            "trace_alone_wall_ms": med(t["t_wall"]), "trace_total_ms": med(t["t_total"]),
        }), flush=True)


if __name__ == "__main__":
    main()
