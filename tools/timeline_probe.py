"""Probe: what a link-timeline call (shdtopo_link_timeline) costs on the C4 topology -- 1,000,000
vertices, 10,000,000 edges, 10,000 attached poi, the table built -- next to link crossings of the
same flows and watches (existing code, the yardstick: the same walks without the prefix
latencies) and next to what a user does without it: trace every flow and bin the hops in numpy.

The three sets of flows and the watches of tools/crossings_probe.py: (a) one source to all
attached, (b) 256 sources x all attached (a 2.56 M-flow slice of a traffic matrix), (c) 5,000
sources with one pair each; weights U{1..1448}; the 16 heaviest edges and the 16 heaviest vertices
of a link load of the same flows.  Emission times are uniform over a 10 ms window, the bins 1 ms
wide from the window's start (--bins of them).  Per case, in one process on one box, after one
unmeasured call of each kind, --reps alternating rounds of

  timeline     Topology.link_timeline: total_ms, kernel_ms and batch_ms from the call's own
               counters (shdtopo_link_timeline_stats)
  crossings    Topology.link_crossings with cap given (one call, no sizing pass): total_ms and
               kernel_ms (shdtopo_link_crossings_stats)
  trace+numpy  Topology.trace_routes with cap given, then the same bins from its vertices and
               edges in numpy (one IEEE add per hop from the source): wall time of both steps, and
               of the trace alone

One JSON line per round and kind, then one summary line per case with the medians and the range.
Every round the numpy bins are compared with the call's and the call's hits with the crossings'
total (a dry check; the tests compare with the oracle).

usage: python tools/timeline_probe.py [--reps N] [--sources N] [--matrix-sources N] [--bins N]
                                      [--small]
  --reps            measured rounds per case, default 5
  --sources         distinct sources of case (c), default 5000
  --matrix-sources  sources of case (b), default 256
  --bins            1 ms bins, default 64
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

MS = 1_000_000


def numpy_timeline(tr, eu, elat, V, edges, vertices, w, now, t0, bin_ns, nbins):
    """The call's bins from a trace of the same flows, on the host: hop k of every written route
    at once, the latency accumulated flow by flow with one add per hop from the source.  Returns
    (bins[rows][nbins], outside[rows][2], hits)."""
    ne, nv = len(edges), len(vertices)
    rows = 2 * ne + nv
    emap = np.full(len(eu), -1, np.int64)
    emap[edges] = np.arange(ne)
    vmap = np.full(V, -1, np.int64)
    vmap[vertices] = 2 * ne + np.arange(nv)
    acc = np.zeros(rows * (nbins + 2), np.uint64)  # per row: the bins, before, after
    hits = 0

    def put(row, t, wt):
        late = t >= np.uint64(t0)
        b = np.where(late, t - np.uint64(t0), np.uint64(0)) // np.uint64(bin_ns)
        b = np.minimum(b, np.uint64(nbins + 1)).astype(np.int64)
        slot = np.where(~late, nbins, np.where(b >= nbins, nbins + 1, b))
        np.add.at(acc, row * (nbins + 2) + slot, wt)
        return len(row)

    hops = np.where(tr["status"] == 0, tr["hops"], 0).astype(np.int64)
    lat = np.zeros(len(hops))
    live = np.nonzero(hops > 0)[0]
    k = 0
    while len(live):
        pos = tr["offset"][live] + k
        e, a, b = tr["edges"][pos], tr["vertices"][pos], tr["vertices"][pos + 1]
        enter = now[live] + np.ceil(lat[live] * 1000000.0).astype(np.uint64)
        lat[live] = lat[live] + elat[e]
        arrive = now[live] + np.ceil(lat[live] * 1000000.0).astype(np.uint64)
        ke = emap[e]
        he = ke >= 0
        rev = (eu[e] != a) & (a != b)
        hits += put(ke[he] + ne * rev[he], enter[he], w[live][he])
        kv = vmap[b]
        hv = kv >= 0
        hits += put(kv[hv], arrive[hv], w[live][hv])
        k += 1
        live = live[hops[live] > k]
    acc = acc.reshape(rows, nbins + 2)
    return acc[:, :nbins], acc[:, [nbins, nbins + 1]], hits


def flat(out):
    o = out["outside"]
    return (np.concatenate([out["edge_fwd"], out["edge_rev"], out["vertex"]]),
            np.concatenate([o["edge_fwd"], o["edge_rev"], o["vertex"]]))


def med(xs):
    return round(float(np.median(xs)), 3)


def span(xs):
    return [med(xs), round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sources", type=int, default=5000)
    ap.add_argument("--matrix-sources", type=int, default=256)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("timeline_probe needs the GPU: the chains of an SSSP topology are on the device")
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
    graph = top.export_graph()
    eu, elat = graph[1], graph[3]
    ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255, (k + 1) >> 8 & 255,
                                                       (k + 1) & 255)) for k in range(A)], np.uint32)
    print(json.dumps({"topology": "C4", "small": args.small, "vertices": top.num_vertices,
                      "edges": top.num_edges, "attached": A, "table_build_s": build_s,
                      "reps": args.reps, "bins": args.bins, "bin_ms": 1, "window_ms": 10,
                      "setup_s": round(time.time() - t0, 2)}), flush=True)
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
    base, nb = 10**9, args.bins
    for name, s, d in cases:
        w = rng.integers(1, 1449, len(s)).astype(np.uint64)  # payload bytes
        now = (base + rng.integers(0, 10 * MS, len(s))).astype(np.uint64)
        load = top.link_load(s, d, w)
        heavy = lambda x: np.argsort(np.iinfo(np.uint64).max - x, kind="stable")[:16]
        edges = heavy(load["edge_fwd"] + load["edge_rev"]).astype(np.int32)
        vertices = heavy(load["vertex"]).astype(np.int32)
        kw = dict(edges=edges, vertices=vertices, weight=w, t0=base, bin_ns=MS, nbins=nb)
        # one unmeasured call of each kind
        top.link_timeline(s, d, now, **kw)
        sized = top.link_crossings(s, d, edges, vertices, w)
        cap, tcap = max(int(sized["total"]), 1), 16 * len(s)
        top.trace_routes(s, d, cap=tcap)
        same = True
        t = {k: [] for k in ("tl_total", "tl_kernel", "tl_batch", "tl_wall", "x_total", "x_kernel",
                             "x_wall", "tn_wall", "t_wall")}
        for rep in range(args.reps):
            t1 = time.time()
            out = top.link_timeline(s, d, now, **kw)
            t["tl_wall"].append(1e3 * (time.time() - t1))
            ts = top.link_timeline_stats()
            t["tl_total"].append(ts["total_ms"])
            t["tl_kernel"].append(ts["kernel_ms"])
            t["tl_batch"].append(ts["batch_ms"])
            t1 = time.time()
            x = top.link_crossings(s, d, edges, vertices, w, cap=cap)
            t["x_wall"].append(1e3 * (time.time() - t1))
            cs = top.link_crossings_stats()
            t["x_total"].append(cs["total_ms"])
            t["x_kernel"].append(cs["kernel_ms"])
            t1 = time.time()
            tr = top.trace_routes(s, d, cap=tcap)
            t["t_wall"].append(1e3 * (time.time() - t1))
            bins, outside, hits = numpy_timeline(tr, eu, elat, top.num_vertices, edges, vertices,
                                                 w, now, base, MS, nb)
            t["tn_wall"].append(1e3 * (time.time() - t1))
            got = flat(out)
            same = (same and np.array_equal(got[0], bins) and np.array_equal(got[1], outside)
                    and out["hits"] == hits == x["total"])
            print(json.dumps({"case": name, "rep": rep,
                              **{k: round(v[-1], 3) for k, v in t.items()}}), flush=True)
        ratio = [a / b for a, b in zip(t["tl_kernel"], t["x_kernel"])]
        print(json.dumps({
            "case": name, "summary": "medians of %d rounds [min, max]" % args.reps,
            "requests": int(len(s)), "watched_edges": len(edges), "watched_vertices": len(vertices),
            "hits": ts["hits"], "flows_hit": ts["flows_hit"], "in_range": ts["in_range"],
            "before": ts["before"], "after": ts["after"], "staged_hops": ts["staged_hops"],
            "routed": ts["routed"], "sources": ts["sources"], "chunks": ts["chunks"],
            "batch_sources": ts["batch_sources"], "batch_fallback": ts["batch_fallback"],
            "route_entries": int(tr["total"]), "numpy_and_crossings_agree": bool(same),
            "timeline_total_ms": span(t["tl_total"]), "timeline_kernel_ms": span(t["tl_kernel"]),
            "timeline_batch_ms": med(t["tl_batch"]), "timeline_python_wall_ms": med(t["tl_wall"]),
            "crossings_total_ms": span(t["x_total"]), "crossings_kernel_ms": span(t["x_kernel"]),
            "crossings_python_wall_ms": med(t["x_wall"]),
            "kernel_ms_ratio_timeline_over_crossings": span(ratio),
            "trace_and_numpy_wall_ms": span(t["tn_wall"]), "trace_alone_wall_ms": med(t["t_wall"]),
        }), flush=True)


if __name__ == "__main__":
    main()
