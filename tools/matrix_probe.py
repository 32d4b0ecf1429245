"""Probe: what a traffic matrix (shdtopo_matrix_*) costs on the C4 topology -- 1,000,000 vertices,
10,000,000 edges, the 10,000 attached poi of shdtopo_synth_packets -- and what it buys the flow
calls that take its export.

Two sets of packets, each --reps times after one unmeasured round, in one process on one box:

  (w) window   the --packets packet Tor-like window of shdtopo_synth_packets, weight = payload
  (b) slice    --matrix-sources sources x all attached (a 2.56 M-flow slice), weights U{1..1448}

Per round:

  matrix     reset, feed_device of the columns resident in device memory (feed_kernel_ms: the
             event time of the feed kernel), a sizing read (cap = 0: the count pass and the scan,
             read_kernel_ms) and a full read (count, scan, fill: read_kernel_ms, and the wall time
             with the copy of the records to the host)
  flows      link_load(*matrix.flows()[:3]) end to end -- the read, vertex_ips and the link load of
             the aggregated flows -- against link_load of the raw packets by IP (wall times and
             the calls' own total_ms); the two loads are compared byte for byte
  numpy      the alternative without the library: np.unique over the packets' (source column,
             destination column) keys and np.add.at of the weights, on the host

One JSON line per round, then one summary line per case with the medians and the range.

usage: python tools/matrix_probe.py [--reps N] [--matrix-sources N] [--packets N] [--small]
  --small   a 30,000-vertex topology with 300 poi (a dry run of the tool, not a measurement)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shadow_amd as sa  # noqa: E402


def med(xs):
    return round(float(np.median(xs)), 3)


def span(xs):
    return [med(xs), round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--matrix-sources", type=int, default=256)
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("matrix_probe needs the GPU: it times the matrix's kernels")
    t0 = time.time()
    if args.small:
        top = sa.Topology.synthetic(seed=20261015, n_routers=29_700, n_poi=300, n_edges=300_000)
        hosts, npk = 3000, min(args.packets, 100_000)
    else:
        top = sa.Topology.synthetic(seed=20261015)
        hosts, npk = 100_000, args.packets
    pk = top.synth_packets(20261015, hosts, npk, 10**9, 10_000_000)
    A = len(top.attached_vertices())
    top.build()
    ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255, (k + 1) >> 8 & 255,
                                                       (k + 1) & 255)) for k in range(A)], np.uint32)
    cols = np.asarray([top.column_of_ip(int(ip)) for ip in ips], np.int32)
    top.link_load(ips[[1]], ips[[2]])  # the first call uploads the replay's CSR and the edge ids
    print(json.dumps({"topology": "C4", "small": args.small, "vertices": top.num_vertices,
                      "edges": top.num_edges, "attached": A, "reps": args.reps,
                      "setup_s": round(time.time() - t0, 2)}), flush=True)
    msrc = min(args.matrix_sources, A)
    rng = np.random.default_rng(1)
    si, di = np.repeat(np.arange(msrc), A), np.tile(np.arange(A), msrc)
    w = rng.integers(1, 1449, len(si)).astype(np.uint32)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cases = [
        ("(w) the %d-packet synthetic window" % npk, pk["src_ip"], pk["dst_ip"], pk["src_col"],
         pk["dst_col"], pk["payload"]),
        ("(b) %d sources x all %d attached" % (msrc, A), ips[si], ips[di], cols[si], cols[di], w),
    ]
    m = top.traffic_matrix()
    for name, sip, dip, sc, dc, pay in cases:
        d = [cu(sc), cu(dc), cu(pay.view(np.int32))]
        w64 = pay.astype(np.uint64)
        n = len(sc)
        torch.cuda.synchronize()

        def matrix_round():
            r = {}
            m.reset()
            t1 = time.time()
            m.feed_device(d[0], d[1], payload=d[2])
            st = m.stats()  # (waits for the feed)
            r["feed_wall"] = 1e3 * (time.time() - t1)
            r["feed_kernel"] = st["feed_kernel_ms"]
            m.read(cap=0)
            r["count_scan_kernel"] = m.stats()["read_kernel_ms"]
            t1 = time.time()
            rec, _, tot = m.read()
            r["read_wall"] = 1e3 * (time.time() - t1)
            st = m.stats()
            r["read_kernel"] = st["read_kernel_ms"]
            return r, rec, tot, st

        def flows_round():
            r = {}
            t1 = time.time()
            agg = top.link_load(*m.flows()[:3])
            r["load_of_flows_wall"] = 1e3 * (time.time() - t1)
            r["load_of_flows_total"] = top.link_load_stats()["total_ms"]
            t1 = time.time()
            raw = top.link_load(sip, dip, w64)
            r["load_of_packets_wall"] = 1e3 * (time.time() - t1)
            r["load_of_packets_total"] = top.link_load_stats()["total_ms"]
            same = all(agg[k].tobytes() == raw[k].tobytes()
                       for k in ("edge_fwd", "edge_rev", "vertex"))
            return r, same

        def numpy_round():
            t1 = time.time()
            key = sc.astype(np.int64) * A + dc
            uniq, inv = np.unique(key, return_inverse=True)
            wsum = np.zeros(len(uniq), np.uint64)
            np.add.at(wsum, inv, w64)
            cnt = np.bincount(inv, minlength=len(uniq))
            return {"numpy_wall": 1e3 * (time.time() - t1)}, uniq, wsum, cnt

        # one unmeasured round of each kind
        matrix_round()
        flows_round()
        t, same, cells_ok = {}, True, True
        for rep in range(args.reps):
            r, rec, tot, st = matrix_round()
            r2, ok = flows_round()
            r3, uniq, wsum, cnt = numpy_round()
            same = same and ok
            mv = m.vertices()
            # (mv is the attached set: an index in mv is a column)
            cells_ok = (cells_ok and len(mv) == A and len(rec) == len(uniq)
                        and np.array_equal(rec["srcIndex"].astype(np.int64) * A + rec["dstIndex"],
                                           uniq)
                        and np.array_equal(rec["weight"], wsum)
                        and np.array_equal(rec["packets"], cnt.astype(np.uint64)))
            r.update(r2)
            r.update(r3)
            for k, v in r.items():
                t.setdefault(k, []).append(v)
            print(json.dumps({"case": name, "rep": rep, **{k: round(v, 3) for k, v in r.items()}}),
                  flush=True)
        M = st["size"]
        count_ms = med(t["count_scan_kernel"])
        print(json.dumps({
            "case": name, "summary": "medians of %d rounds [min, max]" % args.reps, "packets": n,
            "size": M, "cells": tot["cells"], "fed": st["fed"], "bad_columns": st["bad_columns"],
            "matrix_bytes": st["bytes"], "read_bytes_model": st["bytes_model"],
            "peak_weight": tot["peakWeight"], "peak_cell_packets": int(rec["packets"].max()),
            "cells_equal_numpy": bool(cells_ok), "loads_equal": bool(same),
            "feed_kernel_ms": span(t["feed_kernel"]), "feed_wall_ms": span(t["feed_wall"]),
            "packets_per_us": round(n / max(med(t["feed_kernel"]), 1e-9) / 1e3, 1),
            "count_and_scan_kernel_ms": span(t["count_scan_kernel"]),
            "count_model_GBps": round(16.0 * M * M / max(count_ms, 1e-9) / 1e6, 1),
            "read_kernel_ms": span(t["read_kernel"]), "read_wall_ms": span(t["read_wall"]),
            "link_load_of_flows_wall_ms": span(t["load_of_flows_wall"]),
            "link_load_of_flows_total_ms": span(t["load_of_flows_total"]),
            "link_load_of_packets_wall_ms": span(t["load_of_packets_wall"]),
            "link_load_of_packets_total_ms": span(t["load_of_packets_total"]),
            "numpy_unique_add_at_wall_ms": span(t["numpy_wall"]),
        }), flush=True)


if __name__ == "__main__":
    main()
