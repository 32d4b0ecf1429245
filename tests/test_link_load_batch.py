"""Link load from the batch kernel's parent records (option "trace_batch").

The per-request walk (load_walk = 1) takes the chains of the sources whose row crosses no tie from
the batch slots' pair records; the tree accumulation (load_walk = 0) keeps its state in the
replay's records and replays every source.  Loads are compared exactly with the oracle's
(load_helpers.ExpectedLoad) and, byte for byte, with the replay path (trace_batch = 0).
"""
import functools

import numpy as np
import pytest

import oracle
import shadow_amd as sa
from helpers import random_topology_graphml
from load_helpers import ExpectedLoad, check_load, pairs_crossing_ties, random_hosts

pytestmark = pytest.mark.gpu
NSRC = 5


def real_graphml():
    return random_topology_graphml(600, 60, 2400, seed=3)


def flows(av, aip):
    """NSRC sources x every attached vertex, then duplicates and self pairs, weights up to 2^40;
    an unattached end is added by the test.  Returns (sip, dip, sv, dv, w)."""
    k = len(av)
    si = np.concatenate([np.repeat(np.arange(NSRC), k), [0, 0, 1, 3, 3, 2], [0, 1, 2]])
    di = np.concatenate([np.tile(np.arange(k), NSRC), [9, 9, 8, 7, 7, 11], [0, 1, 2]])
    w = np.random.default_rng(33).integers(1, 2**40, len(si), endpoint=True).astype(np.uint64)
    w[:3] = [2**40, 1, 2**40 - 1]
    return aip[si], aip[di], av[si], av[di], w


@functools.lru_cache(maxsize=None)
def real_expected(av):
    g = oracle.OGraph.from_graphml(real_graphml())
    v = np.asarray(av, np.int32)
    sip, dip, sv, dv, w = flows(v, np.zeros(len(v), np.uint32))
    exp = ExpectedLoad(g, sv, dv, w, v)
    return exp, pairs_crossing_ties(g, exp)


def load_both(top, sip, dip, w):
    top.set_option("trace_batch", 0)
    try:
        a = top.link_load(sip, dip, w)
        la = top.link_load_stats()
        assert la["batch_sources"] == 0 and la["batch_fallback"] == 0 and la["batch_ms"] == 0
    finally:
        top.set_option("trace_batch", 1)
    b = top.link_load(sip, dip, w)
    return a, la, b, top.link_load_stats()


@pytest.mark.parametrize("walk", [1, 0])
def test_real_latency_loads(walk):
    top, g, av, aip = random_hosts(real_graphml(), 300, [("load_walk", walk)])
    sip, dip, sv, dv, w = flows(av, aip)
    exp, crossing = real_expected(tuple(int(v) for v in av))
    assert crossing == 0  # input condition: no requested chain crosses a tie
    stranger = sa.ip_to_network("10.9.8.7")
    sip = np.concatenate([sip, [stranger]]).astype(np.uint32)
    dip = np.concatenate([dip, [aip[0]]]).astype(np.uint32)
    w = np.concatenate([w, [2**39]]).astype(np.uint64)
    top.table()
    a, la, b, lb = load_both(top, sip, dip, w)
    check_load(b, exp)
    for k in ("edge_fwd", "edge_rev", "vertex"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["routed"] == b["routed"] == len(sip) - 1
    for k in ("requests", "routed", "unattached", "broken", "sources", "chunks", "hop_weight",
              "tree_vertices"):
        assert la[k] == lb[k], k
    assert lb["unattached"] == 1 and lb["broken"] == 0 and lb["sources"] == NSRC
    assert lb["hop_weight"] == exp.hop_weight
    assert lb["tree_vertices"] == (0 if walk else exp.tree_vertices)
    if walk:
        assert lb["batch_sources"] == NSRC and lb["batch_fallback"] == 0
        assert lb["replay_ms"] == 0 and lb["batch_ms"] > 0
    else:
        assert lb["batch_sources"] == 0 and lb["batch_fallback"] == 0 and lb["batch_ms"] == 0


def test_chunked_batch_load_is_byte_identical():
    top, g, av, aip = random_hosts(real_graphml(), 300)
    sip, dip, sv, dv, w = flows(av, aip)
    exp, _ = real_expected(tuple(int(v) for v in av))
    top.table()
    a = top.link_load(sip, dip, w)
    assert top.link_load_stats()["chunks"] == 1
    top.set_option("trace_chunk", 2)
    try:
        b = top.link_load(sip, dip, w)
        ls = top.link_load_stats()
        assert ls["chunks"] == 3 and ls["sources"] == NSRC and ls["batch_sources"] == NSRC
    finally:
        top.set_option("trace_chunk", 0)
    for k in ("edge_fwd", "edge_rev", "vertex"):
        assert a[k].tobytes() == b[k].tobytes(), k
    check_load(b, exp)


def test_multi_device_topology_loads_either_way():
    top, g, av, aip = random_hosts(real_graphml(), 300, [("devices", 2)])
    sip, dip, sv, dv, w = flows(av, aip)
    exp, _ = real_expected(tuple(int(v) for v in av))
    top.table()
    st0 = top.stats()
    assert st0["devices"] == 2
    check_load(top.link_load(sip, dip, w), exp)
    assert top.stats() == st0
