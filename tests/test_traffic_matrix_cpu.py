"""The traffic matrix on complete topologies and its argument checks (no GPU): a complete
topology's host feeds add into host cells and a read with only host cells is answered on the
host, so no device is initialised.  Expected values are numpy's (matrix_helpers.ExpectedMatrix:
np.add.at on dense u64 arrays indexed by vertex pair) over the oracle's attach; nothing expected
comes from the product.
"""
import ctypes
import socket
import struct

import numpy as np
import pytest

from helpers import attach_hosts, bundled_pair, host_ip
from matrix_helpers import FLOW, ExpectedMatrix, bytes_equal, check_counters, check_read
from shadow_amd import _lib
from test_link_monitor_cpu import check_no_device_used

NAMES = ["topology.simple", "topology", "topology.plab"]


def packets(ips, verts, n, seed):
    """n packets between random hosts, self pairs and duplicates among them, weights up to 2^40."""
    rng = np.random.default_rng(seed)
    k = len(ips)
    si, di = rng.integers(0, k, n), rng.integers(0, k, n)
    si[:6], di[:6] = [0, 0, 1, 1, 2, 2], [0, 0, 1, 3, 2, 3]
    w = rng.integers(0, 2**40, n, endpoint=True).astype(np.uint64)
    w[:3] = [2**40, 0, 1]
    ips, verts = np.asarray(ips, np.uint32), np.asarray(verts, np.int32)
    return ips[si], ips[di], verts[si], verts[di], w


def host_order(ip):
    return struct.unpack("!I", struct.pack("=I", int(ip)))[0]


@pytest.mark.parametrize("name", NAMES)
def test_complete_topology_host_feeds(name):
    top, g = bundled_pair(name)
    assert top.is_complete and g.is_complete()
    otop, ips, verts = attach_hosts(top, g, 120)
    mv = sorted(set(verts))
    n = 900
    sip, dip, sv, dv, w = packets(ips, verts, n, 7)
    m = top.traffic_matrix()
    assert len(m.vertices()) == 0 and m.read()[2]["peakCell"] == -1
    exp = ExpectedMatrix(g.V)
    # two windows by IP, one stranger in the second
    h = n // 2
    assert m.feed(sip[:h], dip[:h], w[:h]) == exp.add(sv[:h], dv[:h], w[:h]) == h
    check_read(m, exp, mv)
    stranger = np.asarray([0x01020304], np.uint32)
    assert m.feed(np.concatenate([stranger, sip[h:]]), np.concatenate([dip[:1], dip[h:]]),
                  np.concatenate([w[:1], w[h:]])) == \
        exp.add(np.concatenate([[-1], sv[h:]]), np.concatenate([dv[:1], dv[h:]]),
                np.concatenate([w[:1], w[h:]])) == n - h
    # then by vertex with a delivered mask
    keep = np.random.default_rng(5).integers(0, 2, n).astype(np.uint8)
    keep[:4] = [1, 0, 1, 0]
    assert m.feed_vertices(sv, dv, w, keep) == exp.add(sv, dv, w, keep) == int(keep.sum())
    rec, sums, tot = check_read(m, exp, mv)
    assert tot["cells"] >= 3 and tot["selfCells"] >= 1 and tot["packets"] == n + int(keep.sum())
    st = m.stats()
    check_counters(st, exp, feeds=3)
    assert exp.unattached == 1 and exp.skipped == n - int(keep.sum())
    assert st["last_fed"] == int(keep.sum()) and st["last_skipped_undelivered"] == exp.skipped
    assert st["last_unattached"] == 0 and st["last_bad_columns"] == 0
    assert st["feed_kernel_ms"] == 0 and st["relayouts"] == 0
    assert st["bytes"] == 16 * len(mv) ** 2
    # the cap: a sizing call; a small cap with a sentinel beyond it untouched; totals complete
    lib, h_ = m._lib, top._h
    total = lib.shdtopo_matrix_read(h_, m.id, None, 0, None, None, None, None, None)
    assert total == len(rec) >= 3
    cap = total // 2
    buf = np.zeros(total, FLOW)
    buf[cap:] = 0x5A
    tt = _lib.ShdMatrixTotals()
    assert lib.shdtopo_matrix_read(h_, m.id, buf.ctypes.data, cap, None, None, None, None,
                                   ctypes.byref(tt)) == total
    bytes_equal(buf[:cap], rec[:cap])
    sentinel = np.zeros(total - cap, FLOW)
    sentinel[:] = 0x5A
    bytes_equal(buf[cap:], sentinel)
    assert {k: getattr(tt, k) for k, _ in _lib.ShdMatrixTotals._fields_} == tot
    check_read(m, exp, mv, cap=1)
    # reset keeps mv; weight = NULL gives weight == packets
    m.reset()
    exp.reset()
    check_read(m, exp, mv)
    check_counters(m.stats(), exp)
    assert m.feed(sip, dip) == exp.add(sv, dv) == n
    rec, sums, tot = check_read(m, exp, mv)
    assert np.array_equal(rec["weight"], rec["packets"]) and tot["weight"] == tot["packets"] == n
    bytes_equal(sums["sentWeight"], sums["sentPackets"])
    m.free()
    check_no_device_used(top)


def test_sums_wrap():
    top, g = bundled_pair("topology")
    otop, ips, verts = attach_hosts(top, g, 20)
    m = top.traffic_matrix()
    exp = ExpectedMatrix(g.V)
    a, b = sorted(set(verts))[:2]
    big = np.asarray([2**63 + 5, 2**63 + 9, 3], np.uint64)
    s, d = np.asarray([a, a, b], np.int32), np.asarray([b, b, a], np.int32)
    assert m.feed_vertices(s, d, big) == exp.add(s, d, big) == 3
    rec, sums, tot = check_read(m, exp, sorted(set(verts)))
    cell = rec[(rec["srcVertex"] == a) & (rec["dstVertex"] == b)]
    assert len(cell) == 1 and int(cell["weight"][0]) == 14 and int(cell["packets"][0]) == 2
    assert tot["weight"] == 17 and tot["peakWeight"] == 14
    check_no_device_used(top)


@pytest.mark.parametrize("name", ["topology", "topology.plab"])
def test_growth_moves_every_cell_and_detached_vertices_keep_their_rows(name):
    top, g = bundled_pair(name)
    otop, ips, verts = attach_hosts(top, g, 30)
    mv0 = sorted(set(verts))
    sip, dip, sv, dv, w = packets(ips, verts, 400, 11)
    m = top.traffic_matrix()
    exp = ExpectedMatrix(g.V)
    assert m.feed(sip, dip, w) == exp.add(sv, dv, w)
    check_read(m, exp, mv0)
    # late attaches: new vertices, some below old ones, so old columns shift and old cells move
    st = 12345
    ips2, verts2 = [], []
    for k in range(60):
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        ip = host_ip(5000 + k)
        v1, _ = top.attach_ip(ip, st)
        v2, _ = otop.attach(ip, st)
        assert v1 == v2
        ips2.append(ip)
        verts2.append(v1)
    mv1 = sorted(set(mv0) | set(verts2))
    new = sorted(set(mv1) - set(mv0))
    assert len(new) >= 5 and new[0] < mv0[-1] and any(v > mv0[0] for v in new)
    assert np.array_equal(m.vertices(), np.asarray(mv0, np.int32))  # grows with the next feed
    ips_all, verts_all = list(ips) + ips2, list(verts) + verts2
    sip, dip, sv, dv, w = packets(ips_all, verts_all, 500, 12)
    assert m.feed(sip, dip, w) == exp.add(sv, dv, w) == 500
    rec, _, _ = check_read(m, exp, mv1)
    assert m.stats()["relayouts"] == 1 and m.stats()["bytes"] == 16 * len(mv1) ** 2
    assert set(rec["srcVertex"]) & set(new) and set(rec["srcVertex"]) & set(mv0)
    # a vertex whose hosts were all detached keeps its row and its totals
    gone = verts[0]
    for ip, v in zip(ips_all, verts_all):
        if v == gone:
            top.detach_ip(ip)
    assert gone not in top.attached_vertices()
    left = [(ip, v) for ip, v in zip(ips_all, verts_all) if v != gone]
    sip, dip, sv, dv, w = packets([x[0] for x in left], [x[1] for x in left], 100, 13)
    gone_ip = np.asarray([ips[0]], np.uint32)  # no column any more: unattached
    assert m.feed(np.concatenate([gone_ip, sip]), np.concatenate([dip[:1], dip]),
                  np.concatenate([w[:1], w])) == \
        exp.add(np.concatenate([[-1], sv]), np.concatenate([dv[:1], dv]),
                np.concatenate([w[:1], w])) == 100
    rec, sums, _ = check_read(m, exp, mv1)
    assert gone in rec["srcVertex"] and m.stats()["relayouts"] == 1
    assert m.stats()["unattached"] == 1
    # flows(): the detached vertex has no host to stand for it, its records are dropped
    fs, fd, fw, fp = m.flows()
    keep = (rec["srcVertex"] != gone) & (rec["dstVertex"] != gone)
    assert m.dropped == int((~keep).sum()) >= 1
    low = {}
    for ip, v in left:
        if v not in low or host_order(ip) < host_order(low[v]):
            low[v] = ip
    assert np.array_equal(fs, np.asarray([low[v] for v in rec["srcVertex"][keep]], np.uint32))
    assert np.array_equal(fd, np.asarray([low[v] for v in rec["dstVertex"][keep]], np.uint32))
    bytes_equal(fw, rec["weight"][keep])
    bytes_equal(fp, rec["packets"][keep])
    check_no_device_used(top)


def test_matrix_mb_too_small_leaves_the_matrix_untouched():
    top, g = bundled_pair("topology")
    otop, ips, verts = attach_hosts(top, g, 30)
    mv0 = sorted(set(verts))
    sip, dip, sv, dv, w = packets(ips, verts, 300, 3)
    m = top.traffic_matrix()
    exp = ExpectedMatrix(g.V)
    lib, h = m._lib, top._h
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    # the first growth does not fit: nothing is counted, mv stays empty
    top.set_option("matrix_mb", (16 * len(mv0) ** 2 - 1) / 1048576.0)
    assert lib.shdtopo_matrix_feed(h, m.id, p(sip), p(dip), p(w), None, len(sip)) == -5
    assert lib.shdtopo_matrix_feed_vertices(h, m.id, p(sv), p(dv), p(w), None, len(sv)) == -5
    assert len(m.vertices()) == 0 and m.read()[2]["cells"] == 0 and m.stats()["fed"] == 0
    top.set_option("matrix_mb", 16 * len(mv0) ** 2 / 1048576.0)  # exactly enough
    assert m.feed(sip, dip, w) == exp.add(sv, dv, w)
    before = check_read(m, exp, mv0)
    # a later growth does not fit: contents and mv unchanged
    st = 99
    ips2, verts2 = [], []
    for k in range(40):
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        v1, _ = top.attach_ip(host_ip(7000 + k), st)
        v2, _ = otop.attach(host_ip(7000 + k), st)
        assert v1 == v2
        ips2.append(host_ip(7000 + k))
        verts2.append(v1)
    mv1 = sorted(set(mv0) | set(verts2))
    assert len(mv1) > len(mv0)
    assert lib.shdtopo_matrix_feed(h, m.id, p(sip), p(dip), p(w), None, len(sip)) == -5
    check_read(m, exp, mv0)
    assert m.stats()["fed"] == exp.fed and m.stats()["relayouts"] == 0
    # the option raised: the same feed grows the matrix and counts
    top.set_option("matrix_mb", 0)
    assert m.feed(sip, dip, w) == exp.add(sv, dv, w)
    after = check_read(m, exp, mv1)
    assert m.stats()["relayouts"] == 1 and after[2]["packets"] == 2 * before[2]["packets"]
    assert lib.shdtopo_set_option(h, b"matrix_mb", -1.0) == -1
    check_no_device_used(top)


@pytest.mark.parametrize("name", NAMES)
def test_vertex_ips_lowest_ip_per_vertex(name):
    top, g = bundled_pair(name)
    otop, ips, verts = attach_hosts(top, g, 120)
    low = {}
    for ip, v in zip(ips, verts):  # the oracle's attach map
        if v not in low or host_order(ip) < host_order(low[v]):
            low[v] = ip
    assert any(verts.count(v) >= 2 for v in low)
    ask = np.ascontiguousarray(np.arange(g.V, dtype=np.int32)[::-1])
    want = np.asarray([low.get(int(v), 0) for v in ask], np.uint32)
    assert np.array_equal(top.vertex_ips(ask), want)
    if g.V > 2:
        assert (want == 0).any()
    lib = top._lib
    out = np.zeros(g.V, np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert lib.shdtopo_vertex_ips(top._h, p(ask), g.V, p(out)) == len(low)
    assert socket.inet_ntoa(struct.pack("=I", int(out[ask == verts[0]][0]))).startswith("11.")
    for bad in (-1, g.V):
        assert lib.shdtopo_vertex_ips(top._h, p(np.asarray([0, bad], np.int32)), 2, p(out)) == -1
    assert lib.shdtopo_vertex_ips(None, p(ask), 1, p(out)) == -1
    assert lib.shdtopo_vertex_ips(top._h, None, 1, p(out)) == -1
    assert lib.shdtopo_vertex_ips(top._h, p(ask), 1, None) == -1
    assert lib.shdtopo_vertex_ips(top._h, p(ask), -1, p(out)) == -1
    assert lib.shdtopo_vertex_ips(top._h, None, 0, None) == 0
    check_no_device_used(top)


def test_bad_arguments_and_stale_ids_return_minus_one():
    lib, _ = _lib.load()
    top, g = bundled_pair("topology.simple")
    otop, ips, verts = attach_hosts(top, g, 4)
    other, g2 = bundled_pair("topology.simple")
    attach_hosts(other, g2, 4)
    a = np.asarray(ips[:2], np.uint32)
    v = np.asarray(verts[:2], np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    ok = lib.shdtopo_matrix_new(top._h)
    assert ok >= 0 and lib.shdtopo_matrix_new(None) == -1
    st = _lib.ShdMatrixStats()
    tot = _lib.ShdMatrixTotals()
    rec = np.zeros(8, FLOW)
    mvb = np.zeros(8, np.int32)

    def every_call(top_h, m):
        return [lib.shdtopo_matrix_feed(top_h, m, p(a), p(a), None, None, 2),
                lib.shdtopo_matrix_feed_vertices(top_h, m, p(v), p(v), None, None, 2),
                lib.shdtopo_matrix_feed_device(top_h, m, None, None, None, None, 0, None),
                lib.shdtopo_matrix_vertices(top_h, m, p(mvb), 8),
                lib.shdtopo_matrix_read(top_h, m, p(rec), 8, None, None, None, None,
                                        ctypes.byref(tot)),
                lib.shdtopo_matrix_reset(top_h, m),
                lib.shdtopo_matrix_stats(top_h, m, ctypes.byref(st))]
    assert all(r >= 0 for r in every_call(top._h, ok))
    # a NULL IP / vertex array with n > 0, a negative or too large n, NULL outputs
    assert lib.shdtopo_matrix_feed(top._h, ok, None, p(a), None, None, 2) == -1
    assert lib.shdtopo_matrix_feed(top._h, ok, p(a), None, None, None, 2) == -1
    assert lib.shdtopo_matrix_feed(top._h, ok, p(a), p(a), None, None, -1) == -1
    assert lib.shdtopo_matrix_feed(top._h, ok, p(a), p(a), None, None, 2**31 - 1) == -1
    assert lib.shdtopo_matrix_feed_vertices(top._h, ok, None, p(v), None, None, 2) == -1
    assert lib.shdtopo_matrix_feed_vertices(top._h, ok, p(v), p(v), None, None, 2**31 - 1) == -1
    assert lib.shdtopo_matrix_feed_device(top._h, ok, None, None, None, None, 2, None) == -1
    assert lib.shdtopo_matrix_feed_device(top._h, ok, None, None, None, None, -1, None) == -1
    assert lib.shdtopo_matrix_stats(top._h, ok, None) == -1
    assert lib.shdtopo_matrix_read(top._h, ok, None, 4, None, None, None, None, None) == -1
    assert lib.shdtopo_matrix_read(top._h, ok, p(rec), -1, None, None, None, None, None) == -1
    assert lib.shdtopo_matrix_vertices(top._h, ok, p(mvb), -1) == -1
    assert lib.shdtopo_matrix_feed(top._h, ok, None, None, None, None, 0) == 0
    # an id of another topology, an id never handed out, a NULL topology, a freed id
    theirs = lib.shdtopo_matrix_new(other._h)
    assert theirs >= 0 and theirs != ok
    assert every_call(top._h, theirs) == [-1] * 7 and lib.shdtopo_matrix_free(top._h, theirs) == -1
    assert every_call(other._h, ok) == [-1] * 7
    assert every_call(top._h, 1 << 20) == [-1] * 7 and every_call(top._h, -1) == [-1] * 7
    assert every_call(None, ok) == [-1] * 7 and lib.shdtopo_matrix_free(None, ok) == -1
    assert all(r >= 0 for r in every_call(other._h, theirs))
    assert lib.shdtopo_matrix_free(top._h, ok) == 0
    assert every_call(top._h, ok) == [-1] * 7 and lib.shdtopo_matrix_free(top._h, ok) == -1
    other.free()  # topology_free releases what is left (theirs)
    check_no_device_used(top)
