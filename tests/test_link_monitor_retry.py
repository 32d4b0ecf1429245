"""GPU test of the link monitor's index when the first block of source columns is wider than a
chunk (monitor_index_replay's retry, topo_monitor_host.cpp).  Graph, expectations and helpers are
those of test_link_monitor.py; the test sits in its own file so that file stays as it was.
"""
import pytest

from monitor_helpers import check_index
from test_link_monitor import KW, all_chains, index_bytes, windows
from test_link_timeline import real_case, real_graphml
from timeline_helpers import bytes_equal

pytestmark = pytest.mark.gpu


def test_real_graph_index_when_the_first_block_is_wider_than_a_chunk():
    """The first block of source columns is a guess (256 of them when "trace_chunk" is 0).  With
    two replay slots a chunk holds two sources, so the guess is wider than a chunk and the block is
    taken again one chunk wide: the index and the bins it feeds are those of the default options."""
    top, g, sip, dip, sv, dv, w, now, exp, xc, edges, vertices = real_case()
    av = top.attached_vertices()
    A = len(av)
    assert A >= 5  # input condition: several chunks of two
    g2, chains = all_chains(real_graphml(), tuple(int(v) for v in av))
    top.table()
    mon = top.link_monitor(edges, vertices, **KW)
    xt = check_index(mon, g, chains, edges, vertices, min_hits=300)
    a = index_bytes(mon)
    i = windows(len(sip))[0][0]
    hits = mon.feed(sip[i], dip[i], now[i], w[i])
    assert hits >= 30
    bins = mon.read()
    top.set_option("trace_chunk", 0)
    top.set_option("replay_slots", 2)
    try:
        for batch in (0, 1):
            top.set_option("trace_batch", batch)
            assert mon.prepare() == xt.hits
            st = mon.stats()
            assert st["sources"] == A and st["broken_pairs"] == 0
            if batch == 0:
                assert st["chunks"] == (A + 1) // 2 and st["batch_sources"] == 0
            assert index_bytes(mon) == a
            check_index(mon, g, chains, edges, vertices, min_hits=300)
            mon.reset()
            assert mon.feed(sip[i], dip[i], now[i], w[i]) == hits
            bytes_equal(mon.read(), bins)
    finally:
        top.set_option("trace_batch", 1)
        top.set_option("replay_slots", 0)
        top.set_option("trace_chunk", 0)
