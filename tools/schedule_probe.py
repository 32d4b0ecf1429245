"""Probe: what a route schedule costs on the C4 topology -- 1,000,000 vertices, 10,000,000 edges,
10,000 attached poi, 100,000 hosts: fail the 16 heaviest router-router edges (the failing set of
tools/whatif_probe.py), build the derived table and route the 10 M packets of one scheduler window
(synth_packets) through the schedules [p], [p, c] and [p, c, p] (p: the parent, c: the derived
topology), the epochs cutting the window's emission times into near-equal parts.

In one process on one box, after one unmeasured round, --reps measured rounds of

  floor     (a) route_batch_device on the parent alone: one table, one launch
  baseline  (b) what a user does without the call: per epoch a torch mask over `now`, the
            compaction of the five input arrays, one route_batch_device on the epoch's topology
            and the scatter of its three outputs back into emission order (one epoch: the plain
            route, nothing to split)
  schedule  (c) RouteSchedule.route_device: one launch; with and without the epoch output

Each is enqueued on one torch stream between two events of that stream (event time: the device's
work and the launch gaps between its pieces); the schedule also reports its own kernel_ms
(shdtopo_route_schedule_stats).  (b) and (c) must give the same bytes: "agrees" in the summary.
One JSON line per round, then one summary line with the medians and the range.

usage: python tools/schedule_probe.py [--reps N] [--fail N] [--small]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fail", type=int, default=16)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("schedule_probe needs the GPU: tables are built and read on the device")
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
    w = np.random.default_rng(1).integers(1, 1449, msrc * A).astype(U64)
    load = top.link_load(np.repeat(ips[:msrc], A), np.tile(ips, msrc), w)
    traffic = (load["edge_fwd"] + load["edge_rev"])[routers]
    fail = routers[np.argsort(np.iinfo(U64).max - traffic, kind="stable")[:args.fail]]
    child = top.without(edges=fail.astype(np.int32))
    child.build()

    n = len(pk["now"])
    cu = lambda x, view=None: torch.from_numpy(
        np.ascontiguousarray(x).view(view) if view else np.ascontiguousarray(x)).cuda()
    ins = [cu(pk["src_col"]), cu(pk["dst_col"]), cu(pk["payload"], np.int32),
           cu(pk["state_in"], np.int32), cu(pk["now"], np.int64)]
    d_now = ins[4]

    def outputs():
        return [torch.empty(n, dtype=torch.int64, device="cuda"),
                torch.empty(n, dtype=torch.int32, device="cuda"),
                torch.empty(n, dtype=torch.uint8, device="cuda")]

    out_a, out_b, out_c = outputs(), outputs(), outputs()
    d_epoch = torch.empty(n, dtype=torch.uint8, device="cuda")
    jump = int(top.getMinimumLatency()) * 1_000_000
    # one stream of the probe's own for all three: the default stream's handle is 0, which the
    # library takes for "the topology's own stream", and torch's work would not be ordered with it
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    assert sp != 0
    snow = np.sort(pk["now"])
    schedules = {}
    for name, tops in (("p", [top]), ("p_c", [top, child]), ("p_c_p", [top, child, top])):
        k = len(tops)
        from_ns = [0] + [int(snow[(n * e) // k]) for e in range(1, k)]
        schedules[name] = (tops, from_ns, sa.RouteSchedule(tops, from_ns))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def floor():
        top.route_batch_device(*ins, jump, 1, *out_a, stream=sp)

    def baseline(tops, from_ns):
        if len(tops) == 1:
            tops[0].route_batch_device(*ins, jump, 1, *out_b, stream=sp)
            return
        for e, t in enumerate(tops):
            m = d_now >= from_ns[e]
            if e + 1 < len(tops):
                m &= d_now < from_ns[e + 1]
            idx = m.nonzero().squeeze(1)
            part = [x.index_select(0, idx) for x in ins]
            po = [torch.empty(len(idx), dtype=x.dtype, device="cuda") for x in out_b]
            t.route_batch_device(*part, jump, 1, *po, stream=sp)
            for x, y in zip(out_b, po):
                x.index_copy_(0, idx, y)

    head = {"topology": "C4", "small": args.small, "vertices": top.num_vertices,
            "edges": top.num_edges, "attached": A, "reps": args.reps, "packets": n,
            "failed_edges": [int(e) for e in fail], "jump_ns": jump,
            "schedules": {k: v[1] for k, v in schedules.items()},
            "setup_s": round(time.time() - t0, 2)}
    print(json.dumps(head), flush=True)

    t = {}
    info = {}
    agree = True
    for rep in range(-1, args.reps):  # round -1 is not measured
        row = {"floor": timed(floor)}
        for name, (tops, from_ns, sched) in schedules.items():
            row[name + "_baseline"] = timed(lambda: baseline(tops, from_ns))
            row[name + "_schedule"] = timed(lambda: sched.route_device(
                *ins, jump, 1, *out_c, stream=sp))
            st = sched.stats()
            row[name + "_schedule_kernel"] = st["kernel_ms"]
            agree = agree and all(torch.equal(x, y) for x, y in zip(out_b, out_c))
            row[name + "_schedule_epoch"] = timed(lambda: sched.route_device(
                *ins, jump, 1, *out_c, epoch=d_epoch, stream=sp))
            st = sched.stats()
            row[name + "_schedule_epoch_kernel"] = st["kernel_ms"]
            agree = agree and all(torch.equal(x, y) for x, y in zip(out_b, out_c))
            k = len(tops)
            info[name] = {"epoch_packets": [int(x) for x in st["epoch_packets"][:k]],
                          "epoch_delivered": [int(x) for x in st["epoch_delivered"][:k]],
                          "not_routed": st["not_routed"], "bytes_model": st["bytes_model"]}
        if rep < 0:
            continue
        for k, v in row.items():
            t.setdefault(k, []).append(v)
        print(json.dumps({"rep": rep, **{k: round(v, 4) for k, v in row.items()}}), flush=True)
    summary = {"summary": "medians of %d rounds [median, min, max], ms" % args.reps,
               "failed": len(fail), **info, "baseline_and_schedule_agree": bool(agree)}
    for k, v in t.items():
        summary[k] = med(v)
    fl = float(np.median(t["floor"]))
    for name in schedules:
        c, b = float(np.median(t[name + "_schedule"])), float(np.median(t[name + "_baseline"]))
        summary[name + "_schedule_over_baseline"] = round(c / b, 4)
        summary[name + "_schedule_over_floor"] = round(c / fl, 4)
        summary[name + "_schedule_gb_per_s"] = round(
            53e-6 * n / float(np.median(t[name + "_schedule_kernel"])), 1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
