"""Probe: what a link load (shdtopo_link_load) costs on the C4 topology -- 1,000,000 vertices,
10,000,000 edges, 10,000 attached poi -- and what the tree accumulation buys over the per-request
walk.

Three sets of flows, one call each with option load_walk = 0 (leaf-to-root tree accumulation) and
1 (per-request walk, two atomics per hop): (a) one source to all attached, (b) 256 sources x all
attached (a 2.56 M-pair slice of a traffic matrix), (c) 5,000 sources with one pair each.  Per
call one JSON line from the call's own counters (shdtopo_link_load_stats): wall time, the event
time of the heap-replay launches and of the accumulation kernels, the tree vertices.  For the
same requests on the same box a third line gives the trace (shdtopo_trace_routes) and the event
time of its kernels -- the existing code the accumulation is compared against.  The two modes'
arrays are compared with each other (a dry check; the tests compare with the oracle).

With --batch 1 or both the table is built first and every call runs with option trace_batch as
asked (both: 0 then 1 -- the replay path and the batch path in one process on one box); the lines
then carry the keep launches' event time and the sources served from pair records.  --batch 0
(the default) is the probe as it was: no table, replay only.

usage: python tools/load_probe.py [--integer] [--sources N] [--matrix-sources N] [--small]
                                  [--batch 0|1|both]
  --integer         C4-int (latencies U{1..100}: u32 heap keys) instead of C4
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--integer", action="store_true")
    ap.add_argument("--sources", type=int, default=5000)
    ap.add_argument("--matrix-sources", type=int, default=256)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--batch", choices=["0", "1", "both"], default="0")
    args = ap.parse_args()
    modes = {"0": [0], "1": [1], "both": [0, 1]}[args.batch]
    import torch
    if not torch.cuda.is_available():
        sys.exit("load_probe needs the GPU: a link load of an SSSP topology runs the heap replay")
    t0 = time.time()
    if args.small:
        top = sa.Topology.synthetic(seed=20261015, n_routers=29_700, n_poi=300, n_edges=300_000,
                                    integer_latency=args.integer)
        hosts = 3000
    else:
        top = sa.Topology.synthetic(seed=20261015, integer_latency=args.integer)
        hosts = 100_000
    # replay only: the batched SSSP's workspace is not needed, its HBM goes to the replay's slots
    if modes == [0]:
        top.set_option("prepare_on_attach", 0)
    top.synth_packets(20261015, hosts, 1000, 10**9, 10**7)  # host k < poi count sits on poi k
    A = len(top.attached_vertices())
    build_s = None
    if modes != [0]:
        t1 = time.time()
        top.build()
        build_s = round(time.time() - t1, 2)
    ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255, (k + 1) >> 8 & 255,
                                                       (k + 1) & 255)) for k in range(A)], np.uint32)
    print(json.dumps({"topology": "C4-int" if args.integer else "C4", "small": args.small,
                      "vertices": top.num_vertices, "edges": top.num_edges, "attached": A,
                      "table_build_s": build_s, "setup_s": round(time.time() - t0, 2)}),
          flush=True)
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
    # the first call of a topology also prepares the graph, the replay's CSR and the edge ids
    t1 = time.time()
    top.link_load(ips[[1]], ips[[2]])
    ls = top.link_load_stats()
    print(json.dumps({"case": "warm-up: first load of the topology, one pair",
                      "python_wall_s": round(time.time() - t1, 4),
                      "call_total_ms": round(ls["total_ms"], 3),
                      "edge_id_upload_ms": round(ls["ids_ms"], 3)}), flush=True)
    for name, s, d in cases:
        w = rng.integers(1, 1449, len(s)).astype(np.uint64)  # payload bytes
        outs = []
        for walk, mode in [(wk, m) for wk in (0, 1) for m in modes]:
            top.set_option("load_walk", walk)
            top.set_option("trace_batch", mode)
            t1 = time.time()
            out = top.link_load(s, d, w)
            wall = time.time() - t1
            ls = top.link_load_stats()
            outs.append(out)
            print(json.dumps({
                "case": name, "load_walk": walk, "trace_batch": mode, "requests": int(len(s)),
                "batch_sources": ls["batch_sources"], "batch_fallback": ls["batch_fallback"],
                "batch_ms": round(ls["batch_ms"], 3),
                "sources": ls["sources"], "chunks": ls["chunks"], "routed": ls["routed"],
                "broken": ls["broken"], "tree_vertices": ls["tree_vertices"],
                "hop_weight": ls["hop_weight"],
                "weighted_mean_hops": round(ls["hop_weight"] / max(int(w.sum()), 1), 2),
                "python_wall_s": round(wall, 4),
                "total_ms": round(ls["total_ms"], 3),
                "replay_ms": round(ls["replay_ms"], 3),
                "load_kernel_ms": round(ls["load_kernel_ms"], 3),
                "load_kernel_share": round(ls["load_kernel_ms"] / max(ls["total_ms"], 1e-9), 6),
            }), flush=True)
        top.set_option("load_walk", 0)
        same = all(np.array_equal(outs[0][k], o[k]) for o in outs[1:]
                   for k in ("edge_fwd", "edge_rev", "vertex"))
        for mode in modes:
            top.set_option("trace_batch", mode)
            t1 = time.time()
            tr = top.trace_routes(s, d, cap=16 * len(s))  # one call: no sizing pass
            wall = time.time() - t1
            ts = top.trace_stats()
            print(json.dumps({
                "case": name, "trace": True, "trace_batch": mode, "modes_agree": bool(same),
                "batch_sources": ts["batch_sources"], "batch_fallback": ts["batch_fallback"],
                "batch_ms": round(ts["batch_ms"], 3), "requests": int(len(s)),
                "entries": int(tr["total"]), "not_written": int((tr["status"] != 0).sum()),
                "python_wall_s": round(wall, 4),
                "total_ms": round(ts["total_ms"], 3),
                "replay_ms": round(ts["replay_ms"], 3),
                "trace_kernel_ms": round(ts["trace_kernel_ms"], 3),
            }), flush=True)


if __name__ == "__main__":
    main()
