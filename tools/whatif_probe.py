"""Probe: what a link-failure what-if costs on the C4 topology -- 1,000,000 vertices, 10,000,000
edges, 10,000 attached poi: derive a topology without the 16 heaviest links, build its table and
diff the two tables on the device (Topology.without, Topology.table_diff), next to what a user
does without the diff: copy both tables to the host and compare them in numpy.

The failing set: the 16 heaviest edges of a link load of 256 sources x all attached (the 2.56
M-flow slice of tools/load_probe.py, weights U{1..1448}) among the edges that join two routers
(an uplink of an attached poi cannot be failed: it would cut the poi off).

In one process on one box, after one unmeasured round, --reps measured rounds of

  derive       Topology.without(edges): wall time (filtered copy of the graph, connectivity of the
               rest, validation, the hosts carried over)
  child build  the derived topology's first build(): wall time, next to the parent's cold build
               (measured once, before the rounds) -- each includes waiting for its background
               preparation
  diff         Topology.table_diff with cap given (one call, no sizing pass): total_ms, kernel_ms
               and bytes_read from the call's own counters (shdtopo_table_diff_stats); the
               kernels' achieved rate is bytes_read / kernel_ms
  host diff    Topology.table() of both topologies and the same changed pairs in numpy: wall time
               of the copies and of the comparison

With SHDTOPO_LOG=2 the library prints its own breakdown of every derive (validation and
connectivity, copy, graph checks, hosts carried over) and of every graph preparation on stderr.

The child is freed at the end of every round.  One JSON line per round, then one summary line with
the medians and the range, the device memory held by one and by two topologies, and whether the
numpy diff agrees with the device's.  If the child cannot build next to the parent with default
options the probe halves the child's "slots" until it does and reports the value.

usage: python tools/whatif_probe.py [--reps N] [--fail N] [--small] [--derive-only]
  --reps         measured rounds, default 5
  --fail         edges to fail, default 16
  --small        a 30,000-vertex topology with 300 poi (a dry run of the tool, not a measurement)
  --derive-only  time the derive alone (needs no device; the failing set is then the lowest-
                 latency router edges, as no link load is available)
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
    return [round(float(np.median(xs)), 3), round(float(min(xs)), 3), round(float(max(xs)), 3)]


def host_diff(t0, t1):
    """The changed pairs of two host tables: (count, flat indices)."""
    _, lat0, rel0, hops0 = t0
    _, lat1, rel1, hops1 = t1
    ch = ((lat0.view(np.uint64) != lat1.view(np.uint64)) |
          (rel0.view(np.uint64) != rel1.view(np.uint64)) | (hops0 != hops1))
    idx = np.flatnonzero(ch)
    return len(idx), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fail", type=int, default=16)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--derive-only", action="store_true")
    args = ap.parse_args()
    if not args.derive_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit("whatif_probe needs the GPU: tables are built and compared on the device")
        used = lambda: int(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0])
    t0 = time.time()
    if args.small:
        top = sa.Topology.synthetic(seed=20261015, n_routers=29_700, n_poi=300, n_edges=300_000)
        hosts = 3000
    else:
        top = sa.Topology.synthetic(seed=20261015)
        hosts = 100_000
    top.synth_packets(20261015, hosts, 1000, 10**9, 10**7)  # host k < poi count sits on poi k
    attached = top.attached_vertices()
    A = len(attached)
    V, eu, ev, elat, _, _ = top.export_graph()
    is_poi = np.zeros(V, bool)
    is_poi[attached] = True
    routers = np.flatnonzero(~is_poi[eu] & ~is_poi[ev] & (eu != ev))
    head = {"topology": "C4", "small": args.small, "vertices": top.num_vertices,
            "edges": top.num_edges, "attached": A, "reps": args.reps}
    slots = 0
    if args.derive_only:
        fail = routers[np.argsort(elat[routers], kind="stable")[:args.fail]].astype(np.int32)
    else:
        mem0 = used()
        t1 = time.time()
        top.build()
        head["parent_cold_build_ms"] = round(1e3 * (time.time() - t1), 3)
        head["parent_build_wall_ms_stat"] = round(top.stats()["build_wall_ms"], 3)
        head["parent_workspace_bytes"] = int(top.stats()["workspace_bytes"])
        head["device_bytes_one_topology"] = used() - mem0
        ips = np.asarray([sa.ip_to_network("11.%d.%d.%d" % ((k + 1) >> 16 & 255,
                                                           (k + 1) >> 8 & 255, (k + 1) & 255))
                          for k in range(A)], np.uint32)
        msrc = min(256, A)
        s, d = np.repeat(ips[:msrc], A), np.tile(ips, msrc)
        w = np.random.default_rng(1).integers(1, 1449, len(s)).astype(np.uint64)
        load = top.link_load(s, d, w)
        traffic = (load["edge_fwd"] + load["edge_rev"])[routers]
        order = np.argsort(np.iinfo(np.uint64).max - traffic, kind="stable")[:args.fail]
        fail = routers[order].astype(np.int32)
        head["failed_edge_traffic"] = [int(x) for x in traffic[order]]
        head["device_bytes_after_link_load"] = used() - mem0
    head["failed_edges"] = [int(e) for e in fail]
    head["setup_s"] = round(time.time() - t0, 2)
    print(json.dumps(head), flush=True)

    t = {k: [] for k in ("derive", "child_build", "child_build_wait", "child_prep",
                         "child_prep_init", "child_prep_graph", "child_prep_scan",
                         "child_prep_workspace", "diff_total", "diff_kernel", "diff_wall",
                         "diff_rate", "host_copy", "host_compare")}
    info = {}
    agree = True
    for rep in range(-1, args.reps):  # round -1 is not measured
        t1 = time.time()
        child = top.without(edges=fail)
        row = {"derive": 1e3 * (time.time() - t1)}
        if not args.derive_only:
            while True:
                if slots:
                    child.set_option("slots", slots)
                t1 = time.time()
                try:
                    child.build()
                    break
                except RuntimeError as e:  # no room next to the parent: fewer slots
                    slots = (slots or int(top.stats()["slots"])) // 2
                    if slots < 1:
                        raise
                    print(json.dumps({"child_build_failed": str(e), "retry_slots": slots}),
                          flush=True)
                    child.free()
                    child = top.without(edges=fail)
            row["child_build"] = 1e3 * (time.time() - t1)
            info["device_bytes_two_topologies"] = used() - mem0
            info["child_workspace_bytes"] = int(child.stats()["workspace_bytes"])
            cst = child.stats()
            row["child_build_wait"] = cst["build_wait_ms"]  # of it: for the background preparation
            row["child_prep"] = cst["attach_prep_ms"]       # that thread's wall time
            for i, k in enumerate(("init", "graph", "scan", "workspace")):
                row["child_prep_" + k] = cst["attach_prep_step_ms"][i]
            info["child_slots"] = int(cst["slots"])
            info["parent_slots"] = int(top.stats()["slots"])
            cap = max(1, top.table_diff(child, cap=0)["total"]) if rep < 0 else info["changed"]
            t1 = time.time()
            out = top.table_diff(child, cap=max(1, cap))
            row["diff_wall"] = 1e3 * (time.time() - t1)
            ds = top.table_diff_stats()
            row["diff_total"], row["diff_kernel"] = ds["total_ms"], ds["kernel_ms"]
            row["diff_rate"] = ds["bytes_read"] / ds["kernel_ms"] / 1e6 if ds["kernel_ms"] else 0.0
            info.update(pairs=ds["pairs"], changed=ds["changed"], bytes_read=ds["bytes_read"],
                        kind_count=[int(x) for x in out["kind_count"]],
                        rows_changed=int((out["row_changed"] > 0).sum()),
                        worst_rise=float(out["row_worst_rise"].max()))
            t1 = time.time()
            t_parent, t_child = top.table(), child.table()
            row["host_copy"] = 1e3 * (time.time() - t1)
            t1 = time.time()
            n, idx = host_diff(t_parent, t_child)
            row["host_compare"] = 1e3 * (time.time() - t1)
            rec = out["records"]
            agree = agree and n == out["total"] and np.array_equal(
                idx, rec["srcCol"].astype(np.int64) * A + rec["dstCol"])
            del t_parent, t_child, out, rec
        child.free()
        if rep < 0:
            continue
        for k, v in row.items():
            t[k].append(v)
        print(json.dumps({"rep": rep, **{k: round(v, 3) for k, v in row.items()}}), flush=True)
    summary = {"summary": "medians of %d rounds [median, min, max]" % args.reps,
               "failed": len(fail), **info, "host_diff_agrees": bool(agree),
               "child_slots_option": slots}
    for k, v in t.items():
        if v:
            summary[k + ("_gb_per_s" if k == "diff_rate" else "_ms")] = med(v)
    if t["host_copy"]:
        summary["host_diff_ms"] = med([a + b for a, b in zip(t["host_copy"], t["host_compare"])])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
