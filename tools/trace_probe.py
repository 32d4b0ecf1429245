"""Probe: what a route trace (shdtopo_trace_routes) costs on the C4 topology -- 1,000,000
vertices, 10,000,000 edges, 10,000 attached poi.

Times three calls: (a) one pair, (b) one source to all 10,000 targets, (c) 5,000 distinct sources
with one pair each.  Per call one JSON line: the call's wall time (host clock around the call,
which ends in a device synchronise) and, from the trace's own counters, the event time of the
heap-replay launches and of route_trace_kernel with its scans, placement and scatter.  The first
call of a topology also prepares the graph, the replay's CSR and the edge ids; that is reported
as a line of its own (a one-pair warm-up) so that (a) is the steady-state cost of one pair.

With --batch 1 or both the table is built first (the batch path needs the relaxation copy of the
current attached set and the batch workspace) and every case runs with option trace_batch as
asked -- both: 0 then 1, the replay path and the batch path in one process on one box.  Each line
then carries the keep launches' event time and the sources served from pair records / replayed
after a keep launch.  --batch 0 (the default) is the probe as it was: no table, replay only.

usage: python tools/trace_probe.py [--integer] [--sources N] [--small] [--batch 0|1|both]
  --integer   C4-int (latencies U{1..100}: u32 heap keys) instead of C4
  --sources   distinct sources of case (c), default 5000
  --small     a 30,000-vertex topology with 300 poi (a dry run of the tool, not a measurement)
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
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--batch", choices=["0", "1", "both"], default="0")
    args = ap.parse_args()
    modes = {"0": [0], "1": [1], "both": [0, 1]}[args.batch]
    import torch
    if not torch.cuda.is_available():
        sys.exit("trace_probe needs the GPU: a trace of an SSSP topology runs the heap replay")
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
    # host k has IP 11.0.0.1 + k
    ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255, (k + 1) >> 8 & 255,
                                                       (k + 1) & 255)) for k in range(A)], np.uint32)
    assert len({top.vertex_of_ip(int(x)) for x in ips[:50]}) == 50
    print(json.dumps({"topology": "C4-int" if args.integer else "C4", "small": args.small,
                      "vertices": top.num_vertices, "edges": top.num_edges, "attached": A,
                      "table_build_s": build_s, "setup_s": round(time.time() - t0, 2)}),
          flush=True)
    nsrc = min(args.sources, A - 1)
    rng = np.random.default_rng(1)
    cases = [
        ("warm-up: first trace of the topology, one pair", ips[[1]], ips[[2]]),
        ("(a) one pair", ips[[3]], ips[[4]]),
        ("(b) one source to all %d targets" % A, np.repeat(ips[5], A), ips),
        ("(c) %d distinct sources, one pair each" % nsrc, ips[:nsrc],
         ips[(np.arange(nsrc) + 1 + rng.integers(0, A - 1, nsrc)) % A]),
    ]
    runs = [(c, m) for c in cases for m in (modes[:1] if c[0].startswith("warm-up") else modes)]
    for (name, s, d), mode in runs:
        top.set_option("trace_batch", mode)
        t1 = time.time()
        tr = top.trace_routes(s, d, cap=256 * len(s))  # one call: no sizing pass
        wall = time.time() - t1
        ts = top.trace_stats()
        ok = tr["status"] == 0
        print(json.dumps({
            "case": name, "trace_batch": mode, "requests": int(len(s)), "sources": ts["sources"],
            "batch_sources": ts["batch_sources"], "batch_fallback": ts["batch_fallback"],
            "batch_event_ms": round(ts["batch_ms"], 3),
            "chunks": ts["chunks"], "entries": int(tr["total"]),
            "mean_hops": round(float(tr["hops"][ok].mean()), 2), "max_hops": int(tr["hops"].max()),
            "not_ok": int((~ok).sum()),
            "python_wall_s": round(wall, 4),
            "call_total_ms": round(ts["total_ms"], 3),
            "replay_event_ms": round(ts["replay_ms"], 3),
            "route_trace_kernel_event_ms": round(ts["trace_kernel_ms"], 3),
            "edge_id_upload_ms": round(ts["ids_ms"], 3),
            "trace_kernel_share": round(ts["trace_kernel_ms"] / max(ts["total_ms"], 1e-9), 6),
        }), flush=True)


if __name__ == "__main__":
    main()
