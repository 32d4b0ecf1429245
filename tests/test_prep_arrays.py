"""Every prepared array of the graph preparation (topo_prep.hip) and of the target
preparation (topo_sssp_batch.hip: leaf targets, target marks, the kappa fixpoint, the re-sort, the
records' kappa field) read back through Topology.export_prep and compared bit for
bit with the numpy restatement of prep_helpers.py.  No tolerances.

A. Rounding range: the latency domains put pi and kappa0 at zero, among the half subnormals, at
   both signs and past 65504; besides the restated bits the contract "bounds never tighten" is
   checked on its own.
B. Shapes: rows of exactly 4096 / 4097 / 8192 / 9001 entries (one segment, several, a cut at a
   segment end), V > 16565 so the tail takes the thread-per-row paths with every row length 1..9,
   several self loops on one vertex, a directed twin with a hub long only in its in-row, a small
   multigraph.
C. Target preparation per option, and a changed target set against a fresh topology (the restore
   of the plain copy before a new set's keys).

The fixtures' coverage preconditions are asserted in test_prep_cpu.py, from the restatement alone.

Division of work with test_prep.py: that module reads shdtopo_export_csr on two undirected
power-law graphs (3,150 and 40,400 vertices, both sides of the tail grouping's threshold) and
covers perm, rowptr, the adjacency columns, pi and the h0-tree parent, and that the attach-time
preparation yields the build-time table.  Everything else that is prepared -- the records'
{f16 pi, f16 kappa0} field, aloss, the self loops, spt, the kappa-sorted copy and its probes, the
hub segments, directed topologies, multigraphs and the target preparation -- is covered here.
"""
import numpy as np
import pytest

import prep_helpers as ph
import shadow_amd as sa
from helpers import host_ip

pytestmark = pytest.mark.gpu

GRAPH_ARRAYS = ("perm", "inv", "rowptr", "adj", "aloss", "vloss", "self_lat", "self_loss", "pot",
                "pi_max", "spt_parent", "spt", "adjk", "kap", "ksum", "kap0", "kf_kap",
                "hub_seg", "hub_multi")
DIRECTED_ARRAYS = ("rowptr_in", "adj_out", "pot_src")
TARGET_ARRAYS = ("tbits", "tbits_eff", "dead", "tleaf", "kfix")
COPY_ARRAYS = ("adjk", "kap", "ksum", "kap0")


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def assert_same(name, got, want, rowptr=None):
    """bitwise equality; a failure names the first differing record and its row"""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, "%s: shape %s, restated %s" % (name, g.shape, w.shape)
    if g.dtype != w.dtype:
        g, w = g.astype(np.int64), w.astype(np.int64)
    ne = g != w
    if not ne.any():
        return
    i = tuple(int(x) for x in np.argwhere(ne)[0])
    where = "index %s" % (i,)
    if rowptr is not None and len(g) == int(rowptr[-1]):
        row = int(np.searchsorted(rowptr, i[0], side="right")) - 1
        where = "record %d of row %d, word %s" % (i[0] - int(rowptr[row]), row, i[1:])
    raise AssertionError("%s: %d words differ; first at %s: device %#x, restated %#x"
                         % (name, int(ne.sum()), where, int(g[i]), int(w[i])))


def check_graph(top, R, graph=None):
    """every graph array of the topology against the restatement R"""
    directed = R["directed"]
    assert top.is_directed == directed
    if graph is not None:  # the restatement was made from the very graph the library parsed
        for x, y in zip(top.export_graph()[1:], graph[1:]):
            assert_same("parsed graph", x, y)
    got = top.export_prep()
    names = GRAPH_ARRAYS + (DIRECTED_ARRAYS if directed else ())
    assert set(names) <= set(got), sorted(set(names) - set(got))
    if not directed:
        assert not set(DIRECTED_ARRAYS) & set(got)
        with pytest.raises(KeyError):
            top.export_prep(["adj_out"])
    assert not set(TARGET_ARRAYS) & set(got)  # no build yet
    assert got["state"] == R["state"]
    assert_same("perm", got["perm"], R["perm"])  # first: every other array is in its ids
    rp_out = R["out"].rowptr
    rp_in = R["inn"].rowptr
    per_row = dict(adj=rp_in, aloss=rp_in, adj_out=rp_out, adjk=rp_out, kap=rp_out, kf_kap=rp_out)
    for name in names:
        assert_same(name, got[name], R[name], per_row.get(name))
    return got


def check_bounds(got, R):
    """The contract of the records' field and of kap, from the restated pi / kappa0 and the
    device's own records: a bound never tightens, and it is the nearest representable one."""
    rec = got["adj_out"] if R["directed"] else got["adj"]
    col = rec[:, 0].astype(np.int64)
    for arr in (rec, got["adjk"]):  # the plain copy carries the same fields
        c = (arr[:, 0] & 0x3FFFFFFF).astype(np.int64)
        pi, k0 = R["pot"][c], R["kap0d"][c]
        hi = (arr[:, 1] >> 16).astype(np.uint16).view(np.float16)
        lo = (arr[:, 1] & 0xFFFF).astype(np.uint16).view(np.float16)
        with np.errstate(over="ignore"):
            hi_below = np.nextafter(hi, np.float16(-np.inf)).astype(np.float64)
            lo_above = np.nextafter(lo, np.float16(np.inf)).astype(np.float64)
        assert bool((hi.astype(np.float64) >= pi).all()), "a pi field below pi"
        assert bool((hi_below < pi).all()), "a pi field looser than the next half"
        assert bool((lo.astype(np.float64) <= k0).all()), "a kappa0 field above kappa0"
        assert bool((lo_above > k0).all()), "a kappa0 field looser than the next half"
    k = got["adjk"]
    w = (k[:, 2].astype(np.uint64) | (k[:, 3].astype(np.uint64) << 32)).view(np.float64)
    kappa = w - R["pot"][(k[:, 0] & 0x3FFFFFFF).astype(np.int64)]
    kap = got["kap"]
    with np.errstate(over="ignore"):
        above = np.nextafter(kap, np.float32(np.inf)).astype(np.float64)
    assert bool((kap.astype(np.float64) <= kappa).all()) and bool((above > kappa).all())
    assert len(col) == R["out"].n


# ----------------------------------------------------------------------------------------------
# A. rounding range
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain,directed", [
    ("real", False), ("int", False), ("real_dn30", False), ("real_up30", False),
    ("bimodal", False), ("logu", False), ("real", True), ("real_up30", True)])
def test_graph_arrays_across_latency_domains(domain, directed):
    data, graph, _ = ph.domain_graph(domain, directed)
    top = sa.Topology.from_buffer(data)
    assert top is not None and not top.is_complete
    R = ph.domain_restated(domain, directed)
    got = check_graph(top, R, graph)
    check_bounds(got, R)


# ----------------------------------------------------------------------------------------------
# B. shapes
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
def test_graph_arrays_of_the_shapes_graph(directed):
    data, graph = ph.shapes_graph(directed)
    top = sa.Topology.from_buffer(data)
    assert top is not None
    R = ph.shapes_restated(directed)
    got = check_graph(top, R, graph)
    check_bounds(got, R)
    assert got["state"]["hub_seg_len"] == ph.HUB_SEG and got["state"]["group_hubs"] < R["V"]


def test_graph_arrays_of_a_multigraph():
    """parallel edges: rows ordered by edge id within a neighbour, the tree record at the lowest
    slot of the parent's entries"""
    data, graph = ph.multigraph()
    top = sa.Topology.from_buffer(data)
    R = ph.restate(graph)
    out = R["out"]
    dup = (out.row[1:] == out.row[:-1]) & (out.col[1:] == out.col[:-1])
    assert int(dup.sum()) >= 300
    check_graph(top, R, graph)


# ----------------------------------------------------------------------------------------------
# C. target preparation
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shard():
    """build_shard, with torch and its device context set up once for the module"""
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    return build_shard


def build_shard(top, rows=8):
    """a few rows of the table: the target preparation runs, the kernel time stays small"""
    import torch
    A = len(top.attached_vertices())
    rows = min(rows, A)
    lr = torch.empty((rows, A, 2), dtype=torch.float64, device="cuda")
    hp = torch.empty((rows, A), dtype=torch.int16, device="cuda")
    top.build_rows_into(0, rows, lr, hp)
    torch.cuda.synchronize()


def attach_poi(top, ks):
    for k in ks:
        v, _ = top.attach_ip(host_ip(k + 1), (k * 2654435761 + 12345) & 0xFFFFFFFF,
                             typeHint="t%d" % k)
        assert v == ph.shapes_poi_vertex(k)


def check_targets(top, R, opts, got=None):
    """the target-derived state after a build, against the restatement for the attached set"""
    att = top.attached_vertices()
    tg = R["inv"][att].astype(np.int64)  # the table's column order
    T = ph.restate_targets(R, tg, leaf=opts.get("leaf_targets", 1),
                           nit=opts.get("target_kappa", ph.TARGET_KAPPA),
                           resort=opts.get("target_resort", 1), skip=opts.get("target_skip", 1))
    got = got if got is not None else top.export_prep()
    assert top.stats()["peeled_targets"] == T["peeled"]
    assert got["state"] == T["state"]
    for name in TARGET_ARRAYS:
        assert (name in got) == (name in T), name
        if name in T:
            assert_same(name, got[name], T[name])
    rp = R["out"].rowptr
    for name in COPY_ARRAYS:
        assert_same(name, got[name], T[name], rp)
    # what the target preparation must not touch
    for name in ("adj", "rowptr", "spt", "kf_kap") + (("adj_out",) if R["directed"] else ()):
        assert_same(name, got[name], R[name])
    return T, got


def _cases():
    """target_kappa in {default, 0, 1} x leaf_targets x target_resort (an option at its default
    is left unset), and target_skip = 0"""
    out = []
    for kappa in (None, 0, 1):
        for leaf in (1, 0):
            for resort in (1, 0):
                o = {} if kappa is None else dict(target_kappa=kappa)
                if not leaf:
                    o["leaf_targets"] = 0
                if not resort:
                    o["target_resort"] = 0
                out.append(o)
    return out + [dict(target_skip=0)]


SHAPE_CASES = _cases()


def case_id(o):
    return ",".join("%s=%d" % (k.split("_")[1], v) for k, v in o.items()) or "default"


@pytest.mark.parametrize("opts", SHAPE_CASES, ids=case_id)
def test_target_preparation_on_the_shapes_graph(opts, shard):
    top = sa.Topology.from_buffer(ph.shapes_graph()[0])
    for k, v in opts.items():
        top.set_option(k, v)
    attach_poi(top, ph.SHAPE_SET1)
    shard(top)
    T, _ = check_targets(top, ph.shapes_restated(), opts)
    if opts.get("leaf_targets", 1):
        assert T["peeled"] > 0


def test_target_preparation_on_the_directed_twin(shard):
    top = sa.Topology.from_buffer(ph.shapes_graph(True)[0])
    attach_poi(top, ph.SHAPE_SET1)
    shard(top)
    T, got = check_targets(top, ph.shapes_restated(True), {})
    assert T["peeled"] == 0 and "tleaf" not in got and got["state"]["leaf"] == 0


@pytest.mark.parametrize("opts", [dict(), dict(target_kappa=1, leaf_targets=0)], ids=case_id)
def test_target_preparation_on_a_domain_graph(opts, shard):
    data, graph, _ = ph.domain_graph("real")
    top = sa.Topology.from_buffer(data)
    for k, v in opts.items():
        top.set_option(k, v)
    st, hints = 1, ("client", "relay", "server")
    for k in range(ph.DOMAIN_TARGET_HOSTS):  # helpers.attach_hosts' stream
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        top.attach_ip(host_ip(k + 1), st, typeHint=hints[k % 3])
    assert tuple(int(v) for v in top.attached_vertices()) == ph.domain_targets("real")
    shard(top)
    check_targets(top, ph.domain_restated("real"), opts)


def test_changed_target_set_equals_a_fresh_preparation(shard):
    """Detach some hosts, attach others, build again: a new target set re-derives the plain copy
    first (stale keys of the older set would cut rows that lead to the new targets), so the
    state equals, bit for bit, that of a topology prepared for the second set alone."""
    data = ph.shapes_graph()[0]
    R = ph.shapes_restated()
    a = sa.Topology.from_buffer(data)
    attach_poi(a, ph.SHAPE_SET1)
    shard(a)
    first = a.export_prep()
    for k in sorted(set(ph.SHAPE_SET1) - set(ph.SHAPE_SET2)):
        a.detach_ip(host_ip(k + 1))
    attach_poi(a, sorted(set(ph.SHAPE_SET2) - set(ph.SHAPE_SET1)))
    shard(a)
    b = sa.Topology.from_buffer(data)
    attach_poi(b, ph.SHAPE_SET2)
    shard(b)
    assert np.array_equal(a.attached_vertices(), b.attached_vertices())
    ga, gb = a.export_prep(), b.export_prep()
    assert set(ga) == set(gb) and ga["state"] == gb["state"]
    for name in ga:
        if name != "state":
            assert_same(name, ga[name], gb[name])
    assert not np.array_equal(first["adjk"], ga["adjk"])  # the two sets' copies differ
    check_targets(a, R, {}, ga)
