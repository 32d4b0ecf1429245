"""Shared pieces of the link-monitor tests (test_link_monitor.py, test_link_monitor_cpu.py,
test_link_monitor_window.py).

Expected values come from the CPU oracle alone, through load_helpers.ExpectedLoad (or one-hop
chains over g.get_eid) and timeline_helpers.ExpectedTimeline: a monitor's hit index is the
(hit_row, hit_time) list of a timeline over every ordered pair of attached vertices with now = 0
and t0 = 0; its bins after any sequence of feeds are the timeline of all packets that were fed.
Nothing here calls link_timeline.
"""
import numpy as np

from timeline_helpers import ExpectedTimeline, flat


def pair_grid(av):
    """Every ordered pair of the attached vertices `av` (ascending = column order), row-major:
    pair s * A + d is (av[s], av[d])."""
    av = np.asarray(av, np.int32)
    return np.repeat(av, len(av)), np.tile(av, len(av))


def expected_index(g, chains, edges, vertices):
    """The index the oracle implies for the A x A chains `chains` (an ExpectedLoad over
    pair_grid): (pair_off int64[A*A + 1], row int64[R], off_ns list[R])."""
    xt = ExpectedTimeline(g, chains, None, None, edges, vertices, 0, 1, 0)
    npairs = len(chains.verts)
    off = np.zeros(npairs + 1, np.int64)
    np.cumsum(xt.per_flow, out=off[1:])
    return off, xt.hit_row, list(xt.hit_time), xt


def check_index(mon, g, chains, edges, vertices, min_hits, min_empty=1):
    """export_index() equals the oracle's index pair by pair, in order; the input has pairs with
    no record (at least min_empty) and pairs with several.  Returns the oracle's all-pairs
    timeline."""
    off, row, ns, xt = expected_index(g, chains, edges, vertices)
    assert xt.hits >= min_hits, xt.hits
    assert int((xt.per_flow == 0).sum()) >= min_empty and int((xt.per_flow >= 2).sum()) >= 1
    goff, grow, gns = mon.export_index()
    assert np.array_equal(goff, off)
    assert np.array_equal(grow.astype(np.int64), row)
    assert [int(x) for x in gns] == ns
    st = mon.stats()
    assert st["index_pairs"] == len(chains.verts) and st["index_records"] == xt.hits
    assert st["index_bytes"] == 8 * (len(chains.verts) + 1) + 16 * xt.hits
    assert st["broken_pairs"] == 0
    return xt


def zero_bins(out):
    bins, outside = flat(out)
    return not bins.any() and not outside.any()


def check_counters(st, xts, fed, skipped=0, unattached=0, bad=0):
    """The cumulative counters are the sums over the fed windows' expectations `xts`."""
    want = dict(hits=sum(x.hits for x in xts), flows_hit=sum(x.flows_hit for x in xts),
                in_range=sum(x.in_range for x in xts), before=sum(x.before for x in xts),
                after=sum(x.after for x in xts), fed=fed, skipped_undelivered=skipped,
                unattached=unattached, bad_columns=bad)
    assert {k: st[k] for k in want} == want


def check_last(st, xt, fed, skipped=0, unattached=0, bad=0):
    want = dict(last_hits=xt.hits, last_flows_hit=xt.flows_hit, last_in_range=xt.in_range,
                last_before=xt.before, last_after=xt.after, last_fed=fed,
                last_skipped_undelivered=skipped, last_unattached=unattached,
                last_bad_columns=bad)
    assert {k: st[k] for k in want} == want
