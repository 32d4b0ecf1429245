"""Probe: what a link monitor (shdtopo_monitor_*) costs on the C4 topology -- 1,000,000 vertices,
10,000,000 edges, 10,000 attached poi, the table built -- next to link_timeline calls on the same
flows, watches and bins (existing code, the yardstick: it walks every flow's route).

The watches are the 16 heaviest edges and the 16 heaviest vertices of a link load of the matrix
slice.  The monitor is prepared once (prepare_ms with its breakdown, index_records, index_bytes),
then two sets of packets are fed, each --reps times after one unmeasured round:

  (b) slice    --matrix-sources sources x all attached (a 2.56 M-flow slice of a traffic matrix),
               weights U{1..1448}, emission times uniform over a 10 ms window
  (w) window   the --packets packet Tor-like window of shdtopo_synth_packets, weight = payload

Per round, in one process on one box:

  monitor    reset, feed_device of the columns resident in device memory, read: the wall time of
             feed + read, and feed_kernel_ms (the event time of the feed kernel)
  timeline   Topology.link_timeline of the identical flows by IP: total_ms and kernel_ms from the
             call's own counters (shdtopo_link_timeline_stats)

and the monitor's bins are compared with the call's, byte for byte.  One JSON line per round, then
one summary line per case with the medians and the range.

usage: python tools/monitor_probe.py [--reps N] [--matrix-sources N] [--packets N] [--bins N]
                                     [--small]
  --reps            measured rounds per case, default 5
  --matrix-sources  sources of the slice, default 256
  --packets         packets of the window, default 10,000,000
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
PREP_KEYS = ("prepare_ms", "replay_ms", "kernel_ms", "batch_ms", "sources", "chunks",
             "batch_sources", "batch_fallback", "broken_pairs", "index_pairs", "index_records",
             "index_bytes", "prepares")


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
    ap.add_argument("--matrix-sources", type=int, default=256)
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("monitor_probe needs the GPU: the chains of an SSSP topology are on the device")
    t0 = time.time()
    if args.small:
        top = sa.Topology.synthetic(seed=20261015, n_routers=29_700, n_poi=300, n_edges=300_000)
        hosts, npk = 3000, min(args.packets, 100_000)
    else:
        top = sa.Topology.synthetic(seed=20261015)
        hosts, npk = 100_000, args.packets
    base, nb = 10**9, args.bins
    pk = top.synth_packets(20261015, hosts, npk, base, 10 * MS)  # host k < poi count sits on poi k
    A = len(top.attached_vertices())
    t1 = time.time()
    top.build()
    build_s = round(time.time() - t1, 2)
    ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255, (k + 1) >> 8 & 255,
                                                       (k + 1) & 255)) for k in range(A)], np.uint32)
    cols = np.asarray([top.column_of_ip(int(ip)) for ip in ips], np.int32)
    print(json.dumps({"topology": "C4", "small": args.small, "vertices": top.num_vertices,
                      "edges": top.num_edges, "attached": A, "table_build_s": build_s,
                      "reps": args.reps, "bins": nb, "bin_ms": 1, "window_ms": 10,
                      "setup_s": round(time.time() - t0, 2)}), flush=True)
    msrc = min(args.matrix_sources, A)
    rng = np.random.default_rng(1)
    si, di = np.repeat(np.arange(msrc), A), np.tile(np.arange(A), msrc)
    w = rng.integers(1, 1449, len(si)).astype(np.uint32)  # payload bytes
    now = (base + rng.integers(0, 10 * MS, len(si))).astype(np.uint64)
    # the first call of a topology also uploads the replay's CSR and the edge ids
    top.link_load(ips[[1]], ips[[2]])
    load = top.link_load(ips[si], ips[di], w.astype(np.uint64))
    heavy = lambda x: np.argsort(np.iinfo(np.uint64).max - x, kind="stable")[:16]
    edges = heavy(load["edge_fwd"] + load["edge_rev"]).astype(np.int32)
    vertices = heavy(load["vertex"]).astype(np.int32)
    kw = dict(edges=edges, vertices=vertices, t0=base, bin_ns=MS, nbins=nb)

    mon = top.link_monitor(**kw)
    t1 = time.time()
    records = mon.prepare()
    st = mon.stats()
    print(json.dumps({"prepare": "all %d x %d column pairs" % (A, A), "records": records,
                      "python_wall_ms": round(1e3 * (time.time() - t1), 3),
                      "watched_edges": len(edges), "watched_vertices": len(vertices),
                      **{k: (round(st[k], 3) if isinstance(st[k], float) else st[k])
                         for k in PREP_KEYS}}), flush=True)

    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cases = [
        ("(b) %d sources x all %d attached" % (msrc, A), ips[si], ips[di], cols[si], cols[di], w,
         now),
        ("(w) the %d-packet synthetic window" % npk, pk["src_ip"], pk["dst_ip"], pk["src_col"],
         pk["dst_col"], pk["payload"], pk["now"]),
    ]
    for name, sip, dip, sc, dc, pay, tnow in cases:
        d = [cu(sc), cu(dc), cu(tnow.view(np.int64)), cu(pay.view(np.int32))]
        w64 = pay.astype(np.uint64)
        torch.cuda.synchronize()

        def monitor_round():
            mon.reset()
            t1 = time.time()
            mon.feed_device(d[0], d[1], d[2], payload=d[3])
            out = mon.read()
            return out, 1e3 * (time.time() - t1), mon.stats()
        # one unmeasured round of each kind
        monitor_round()
        top.link_timeline(sip, dip, tnow, weight=w64, **kw)
        same = True
        t = {k: [] for k in ("mon_kernel", "mon_wall", "tl_total", "tl_kernel", "tl_batch")}
        for rep in range(args.reps):
            out, wall, ms = monitor_round()
            t["mon_wall"].append(wall)
            t["mon_kernel"].append(ms["feed_kernel_ms"])
            ref = top.link_timeline(sip, dip, tnow, weight=w64, **kw)
            ts = top.link_timeline_stats()
            t["tl_total"].append(ts["total_ms"])
            t["tl_kernel"].append(ts["kernel_ms"])
            t["tl_batch"].append(ts["batch_ms"])
            same = (same and out["hits"] == ref["hits"]
                    and all(x.tobytes() == y.tobytes() for x, y in zip(flat(out), flat(ref))))
            print(json.dumps({"case": name, "rep": rep,
                              **{k: round(v[-1], 3) for k, v in t.items()}}), flush=True)
        ratio = [a / b for a, b in zip(t["tl_kernel"], t["mon_kernel"])]
        print(json.dumps({
            "case": name, "summary": "medians of %d rounds [min, max]" % args.reps,
            "packets": int(len(sc)), "hits": ms["hits"], "flows_hit": ms["flows_hit"],
            "in_range": ms["in_range"], "before": ms["before"], "after": ms["after"],
            "bad_columns": ms["bad_columns"], "bins_equal_the_timelines": bool(same),
            "monitor_feed_kernel_ms": span(t["mon_kernel"]),
            "monitor_feed_and_read_wall_ms": span(t["mon_wall"]),
            "timeline_total_ms": span(t["tl_total"]), "timeline_kernel_ms": span(t["tl_kernel"]),
            "timeline_batch_ms": med(t["tl_batch"]),
            "kernel_ms_ratio_timeline_over_monitor": span(ratio),
            "total_over_monitor_wall": round(med(t["tl_total"]) / max(med(t["mon_wall"]), 1e-9), 1),
        }), flush=True)


if __name__ == "__main__":
    main()
