"""Expected values of the link-timeline tests (test_link_timeline.py, test_link_timeline_cpu.py).

Expected bins come from the CPU oracle alone: load_helpers.ExpectedLoad gives every flow's vertex
chain and get_eid edges (g.dijkstra for the parents, g.get_eid for each hop's edge); the prefix
latencies are accumulated here with Python floats, one add per hop from the source, and converted
with math.ceil(lat * 1000000.0); the sums are numpy uint64.  Nothing in this file calls
trace_routes, link_load, link_crossings or link_timeline.
"""
import math

import numpy as np

STAT_KEYS = ("requests", "routed", "unattached", "broken", "sources", "hits", "flows_hit",
             "in_range", "before", "after")
U64 = (1 << 64) - 1


def ns(lat):
    """The packet kernel's conversion: milliseconds -> nanoseconds, rounded up."""
    return int(math.ceil(lat * 1000000.0))


class ExpectedTimeline:
    """Timeline of the flows of `exp` (an ExpectedLoad, or anything with its .verts and .edges)
    with weights `w` (None: 1 each) and emission times `now` (None: 0 each) over the watched
    `edges` (edge ids) and `vertices` (original ids).

    bins     uint64[2 ne + nv][nbins]: rows [0, ne) an edge watch's hops leaving eu[e] (and every
             self loop), [ne, 2 ne) its other hops, [2 ne, 2 ne + nv) the arrivals at a vertex
    outside  uint64[2 ne + nv][2]: before t0, at or after the last bin
    hit_row / hit_bin / hit_flow / hit_time  one entry per hit, in flow and hop order, the edge
             hit of a hop before its vertex hit (hit_bin: -1 before, nbins after)
    """

    def __init__(self, g, exp, w, now, edges, vertices, t0, bin_ns, nbins):
        m = len(exp.verts)
        w = np.ones(m, np.uint64) if w is None else np.asarray(w, np.uint64)
        now = np.zeros(m, np.uint64) if now is None else np.asarray(now, np.uint64)
        assert len(w) == m == len(now)
        edges = [int(e) for e in edges]
        vertices = [int(v) for v in vertices]
        ne, nv = len(edges), len(vertices)
        ewatch = {e: k for k, e in enumerate(edges)}
        vwatch = {v: k for k, v in enumerate(vertices)}
        assert len(ewatch) == ne and len(vwatch) == nv
        rows = 2 * ne + nv
        self.bins = np.zeros((rows, nbins), np.uint64)
        self.outside = np.zeros((rows, 2), np.uint64)
        hit_row, hit_bin, hit_flow, hit_time = [], [], [], []

        def put(row, t, i):
            t &= U64
            if t < t0:
                b = -1
                self.outside[row, 0] += w[i]
            elif nbins == 0 or (t - t0) // bin_ns >= nbins:
                b = nbins
                self.outside[row, 1] += w[i]
            else:
                b = (t - t0) // bin_ns
                self.bins[row, b] += w[i]
            hit_row.append(row)
            hit_bin.append(b)
            hit_flow.append(i)
            hit_time.append(t)

        with np.errstate(over="ignore"):
            for i, (chain, es) in enumerate(zip(exp.verts, exp.edges)):
                lat = 0.0
                t_i = int(now[i])
                for a, b, e in zip(chain[:-1], chain[1:], es):
                    enter = t_i + ns(lat)
                    lat = lat + float(g.elat[e])
                    if e in ewatch:
                        rev = a != b and int(g.eu[e]) != a
                        put(ewatch[e] + (ne if rev else 0), enter, i)
                    if b in vwatch:
                        put(2 * ne + vwatch[b], t_i + ns(lat), i)
        self.hit_row = np.asarray(hit_row, np.int64)
        self.hit_bin = np.asarray(hit_bin, np.int64)
        self.hit_flow = np.asarray(hit_flow, np.int64)
        self.hit_time = hit_time
        self.hits = len(hit_row)
        self.before = int((self.hit_bin < 0).sum())
        self.after = int((self.hit_bin >= nbins).sum())
        self.in_range = self.hits - self.before - self.after
        per_flow = np.bincount(self.hit_flow, minlength=m) if self.hits else np.zeros(m, np.int64)
        self.per_flow = per_flow
        self.flows_hit = int((per_flow > 0).sum())
        self.routed = m
        self.ne, self.nv, self.nbins = ne, nv, nbins

    # what the input exercises (asserted by the tests with margin, from these hits alone)
    def cells_with_several(self):
        """(row, bin) cells of the bins that hold at least two hits."""
        inr = (self.hit_bin >= 0) & (self.hit_bin < self.nbins)
        if not inr.any():
            return 0
        cell = self.hit_row[inr] * max(self.nbins, 1) + self.hit_bin[inr]
        return int((np.unique(cell, return_counts=True)[1] >= 2).sum())

    def flows_with_several(self):
        return int((self.per_flow >= 2).sum())

    def reverse_rows_nonzero(self):
        rev = slice(self.ne, 2 * self.ne)
        return int(((self.bins[rev].sum(1) + self.outside[rev].sum(1)) != 0).sum())

    def conditions(self):
        return dict(hits=self.hits, in_range=self.in_range, before=self.before, after=self.after,
                    cells=self.cells_with_several(), flows2=self.flows_with_several(),
                    rev_rows=self.reverse_rows_nonzero())


def flat(out):
    """A Topology.link_timeline result as (bins[rows][nbins], outside[rows][2])."""
    bins = np.concatenate([out["edge_fwd"], out["edge_rev"], out["vertex"]])
    o = out["outside"]
    return bins, np.concatenate([o["edge_fwd"], o["edge_rev"], o["vertex"]])


def check_timeline(out, xt):
    """A link_timeline result equals the oracle's, exactly."""
    bins, outside = flat(out)
    assert out["hits"] == xt.hits
    assert bins.shape == xt.bins.shape and outside.shape == xt.outside.shape
    assert np.array_equal(outside, xt.outside)
    assert np.array_equal(bins, xt.bins)
    assert len(out["edge_fwd"]) == len(out["edge_rev"]) == xt.ne and len(out["vertex"]) == xt.nv


def check_stats(ts, xt, requests, sources, unattached=0):
    want = dict(requests=requests, routed=xt.routed, unattached=unattached, broken=0,
                sources=sources, hits=xt.hits, flows_hit=xt.flows_hit, in_range=xt.in_range,
                before=xt.before, after=xt.after)
    assert {k: ts[k] for k in STAT_KEYS} == want
    assert ts["hits"] == ts["in_range"] + ts["before"] + ts["after"]


def bytes_equal(a, b):
    assert a["hits"] == b["hits"]
    for x, y in zip(flat(a), flat(b)):
        assert x.tobytes() == y.tobytes()
