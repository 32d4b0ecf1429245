"""Shared pieces of the traffic-matrix tests (test_traffic_matrix.py, test_traffic_matrix_cpu.py,
test_traffic_matrix_window.py).

Expected values come from numpy alone: np.add.at on two dense u64 arrays indexed by (source
vertex, destination vertex) over all V vertices of the graph, cut down to the matrix's vertex list
mv -- which the tests take from the oracle's attach -- when a read is checked.  Nothing here calls
the product.
"""
import numpy as np

FLOW = np.dtype([("srcVertex", np.int32), ("dstVertex", np.int32), ("srcIndex", np.int32),
                 ("dstIndex", np.int32), ("packets", np.uint64), ("weight", np.uint64)])
SUMS = ("sentPackets", "sentWeight", "recvPackets", "recvWeight")


class ExpectedMatrix:
    """Packets and weight per (source vertex, destination vertex), u64 and wrapping, and the
    counters of the feeds."""

    def __init__(self, V):
        self.V = V
        self.reset()

    def reset(self):
        self.P = np.zeros((self.V, self.V), np.uint64)
        self.W = np.zeros((self.V, self.V), np.uint64)
        self.fed = self.skipped = self.unattached = 0

    def add(self, sv, dv, weight=None, delivered=None):
        """One feed: vertices (-1: an end that is no column).  Returns the packets it counts."""
        sv, dv = np.asarray(sv, np.int64), np.asarray(dv, np.int64)
        w = np.ones(len(sv), np.uint64) if weight is None else np.asarray(weight).astype(np.uint64)
        dl = np.ones(len(sv), bool) if delivered is None else np.asarray(delivered) != 0
        on = (sv >= 0) & (dv >= 0)
        k = dl & on
        with np.errstate(over="ignore"):
            np.add.at(self.P, (sv[k], dv[k]), np.uint64(1))
            np.add.at(self.W, (sv[k], dv[k]), w[k])
        self.fed += int(k.sum())
        self.skipped += int((~dl).sum())
        self.unattached += int((dl & ~on).sum())
        return int(k.sum())

    def view(self, mv):
        """What a read returns for the vertex list mv: (records, sums, totals).  Every non-zero
        cell must lie inside mv x mv."""
        mv = np.asarray(mv, np.int64)
        M = len(mv)
        rep = (self.P != 0) | (self.W != 0)
        inside = np.zeros((self.V, self.V), bool)
        inside[np.ix_(mv, mv)] = True
        assert not (rep & ~inside).any()
        P, W, R = self.P[np.ix_(mv, mv)], self.W[np.ix_(mv, mv)], rep[np.ix_(mv, mv)]
        i, j = np.nonzero(R)  # row-major: ascending (i, j), so ascending (srcVertex, dstVertex)
        rec = np.zeros(len(i), FLOW)
        rec["srcVertex"], rec["dstVertex"] = mv[i], mv[j]
        rec["srcIndex"], rec["dstIndex"] = i, j
        rec["packets"], rec["weight"] = P[i, j], W[i, j]
        with np.errstate(over="ignore"):
            sums = dict(sentPackets=P.sum(1, dtype=np.uint64), sentWeight=W.sum(1, dtype=np.uint64),
                        recvPackets=P.sum(0, dtype=np.uint64), recvWeight=W.sum(0, dtype=np.uint64))
            d = np.arange(M)
            tot = dict(size=M, cells=len(i), packets=int(P.sum(dtype=np.uint64)),
                       weight=int(W.sum(dtype=np.uint64)), selfCells=int(R[d, d].sum()),
                       selfPackets=int(P[d, d].sum(dtype=np.uint64)),
                       selfWeight=int(W[d, d].sum(dtype=np.uint64)),
                       activeSources=int(R.any(1).sum()), activeDestinations=int(R.any(0).sum()),
                       peakWeight=0, peakCell=-1)
        if len(i):
            lin = i * M + j
            top = W[i, j].max()
            tot["peakWeight"] = int(top)
            tot["peakCell"] = int(lin[W[i, j] == top].min())
        return rec, sums, tot


def bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes()


def reads_equal(x, y):
    """Two read() results are the same bytes."""
    bytes_equal(x[0], y[0])
    for k in SUMS:
        bytes_equal(x[1][k], y[1][k])
    assert x[2] == y[2]


def check_read(m, exp, mv, cap=None):
    """m.read(cap) equals numpy's view of the expected matrix on mv, byte for byte; with a cap
    the records are the first cap of them and everything else is complete.  Returns the read."""
    rec, sums, tot = exp.view(mv)
    assert np.array_equal(m.vertices(), np.asarray(mv, np.int32))
    got = m.read(cap)
    reads_equal(got, (rec if cap is None else rec[:cap], sums, tot))
    assert m.stats()["cells"] == len(rec) and m.stats()["size"] == len(mv)
    return got


def check_counters(st, exp, bad=0, feeds=None):
    want = dict(fed=exp.fed, skipped_undelivered=exp.skipped, unattached=exp.unattached,
                bad_columns=bad)
    assert {k: st[k] for k in want} == want
    if feeds is not None:
        assert st["feeds"] == feeds
