"""A numpy restatement of the graph preparation (topo_prep.hip) and of the target
preparation (topo_sssp_batch.hip), and the fixtures of test_prep_cpu.py /
test_prep_arrays.py.

Everything here is computed from the parsed graph (V, eu, ev, elat, eloss, vloss: document order,
as Topology.export_graph or oracle.OGraph give it) and the attached vertices alone; no exported
device array enters.  Each arithmetic step is one IEEE double operation, as in the library (built
with -ffp-contract=off), so every array is compared bit for bit.
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

from helpers import domain_graphml, graphml_doc, random_topology_graphml

GROUP_HUBS = 16565   # kGroupHubs (topo_core.cpp)
HUB_SEG = 4096       # kHubSeg (topo_device.h)
KPROBES = 8          # kKProbes
SEG_WAVE, SEG_BLOCK = 64, 4096  # kSegWave, kSegBlock: the segmented sort's size classes
NO_LEAF = 0xFFFFFFFF
TARGET_KAPPA = 6     # option target_kappa's default
NINF, PINF = -np.inf, np.inf


# ----------------------------------------------------------------------------------------------
# directed roundings, from numpy's own single-rounding conversions
# ----------------------------------------------------------------------------------------------
def _half(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16)


def _half_floor(x):
    """largest half <= x (+inf stays +inf; below -65504: -inf); NaN untouched"""
    x = np.asarray(x, np.float64)
    h = _half(x)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = h.astype(np.float64) > x
        return np.where(hi, np.nextafter(h, np.float16(NINF)), h).astype(np.float16)


def _half_ceil(x):
    x = np.asarray(x, np.float64)
    h = _half(x)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = h.astype(np.float64) < x
        return np.where(lo, np.nextafter(h, np.float16(PINF)), h).astype(np.float16)


def half_dn(x):
    """f16_dn: bits of the largest half <= x; a bound is never +inf (+inf -> 65504, 0x7BFF);
    NaN -> -inf."""
    x = np.asarray(x, np.float64)
    b = _half_floor(x).view(np.uint16).astype(np.uint32)
    b = np.where(b == 0x7C00, 0x7BFF, b)
    return np.where(np.isnan(x), 0xFC00, b).astype(np.uint32)


def half_up(x):
    """f16_up: bits of the smallest half >= x; -inf -> -65504 (0xFBFF); NaN -> +inf."""
    x = np.asarray(x, np.float64)
    b = _half_ceil(x).view(np.uint16).astype(np.uint32)
    b = np.where(b == 0xFC00, 0xFBFF, b)
    return np.where(np.isnan(x), 0x7C00, b).astype(np.uint32)


def half_down(x):
    """f16_down (kfix_store): as half_dn, but +inf stays +inf (the pair skip's explicit drop)."""
    x = np.asarray(x, np.float64)
    b = _half_floor(x).view(np.uint16).astype(np.uint32)
    return np.where(np.isnan(x), 0xFC00, b).astype(np.uint32)


def f32_dn(x):
    """largest float <= x (NaN -> -inf)"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
        hi = f.astype(np.float64) > x
        f = np.where(hi, np.nextafter(f, np.float32(NINF)), f).astype(np.float32)
    return np.where(np.isnan(x), np.float32(NINF), f).astype(np.float32)


def f32_order(f):
    """u32 image of a float that orders like the value (-0.0 below +0.0)"""
    u = np.asarray(f, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def radix_f32(f):
    """the segmented sort's image: as f32_order, but -0.0 and +0.0 equal"""
    f = np.asarray(f, np.float32)
    return f32_order(np.where(f == 0, np.float32(0.0), f))


def half_value(bits):
    return np.asarray(bits, np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)


def split64(x):
    """f64 array -> (low, high) u32 words"""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return (b & 0xFFFFFFFF).astype(np.uint32), (b >> 32).astype(np.uint32)


# ----------------------------------------------------------------------------------------------
# graph preparation
# ----------------------------------------------------------------------------------------------
class Rows:
    """CSR rows sorted by (row, neighbour, edge id), self loops excluded."""

    def __init__(self, V, row, col, w, loss, eid):
        o = np.lexsort((eid, col, row))
        self.row, self.col, self.w, self.loss, self.eid = row[o], col[o], w[o], loss[o], eid[o]
        self.rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=V))]).astype(np.int64)
        self.n = len(row)

    def row_min(self, x, V):
        """min of x over every row (+inf for an empty one)"""
        out = np.full(V, PINF)
        ne = self.rowptr[1:] > self.rowptr[:-1]
        if self.n:
            out[ne] = np.minimum.reduceat(x, self.rowptr[:-1][ne])
        return out


def hub_segments(rowptr, rows):
    """HubSegs of rows [0, rows): {row, first entry} per segment of at most HUB_SEG entries (an
    empty row keeps one), {row, first segment, segments, 0} per row cut in several."""
    seg, multi = [], []
    for v in range(rows):
        r0, r1 = int(rowptr[v]), int(rowptr[v + 1])
        first = len(seg)
        starts = list(range(r0, r1, HUB_SEG)) or [r0]
        seg += [(v, b) for b in starts]
        if len(starts) > 1:
            multi.append((v, first, len(starts), 0))
    return (np.asarray(seg, np.uint32).reshape(-1, 2), np.asarray(multi, np.uint32).reshape(-1, 4))


def _distances(rows, V):
    """d(0, .) over rows (row -> col), parallel entries merged to their minimum"""
    first = np.ones(rows.n, bool)
    first[1:] = (rows.row[1:] != rows.row[:-1]) | (rows.col[1:] != rows.col[:-1])
    idx = np.nonzero(first)[0]
    w = np.minimum.reduceat(rows.w, idx)
    g = sp.csr_matrix((w, (rows.row[idx], rows.col[idx])), shape=(V, V))
    assert bool((w > 0).all())
    return dijkstra(g, directed=True, indices=[0])[0]


def _records(rows, field):
    lo, hi = split64(rows.w)
    return np.stack([rows.col.astype(np.uint32), field.astype(np.uint32), lo, hi], axis=1)


def restate(graph, directed=False):
    """Every prepared graph array from the parsed graph; keys as Topology.export_prep's, plus the
    intermediate values the tests and preconditions read (out / inn: the Rows)."""
    V, eu, ev, elat, eloss, vloss = graph
    eu, ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
    elat, eloss = np.asarray(elat, np.float64), np.asarray(eloss, np.float64)
    nl = eu != ev
    a, b, w, lo, e = eu[nl], ev[nl], elat[nl], eloss[nl], np.nonzero(nl)[0]
    # relabel: degree (in + out) descending, stable; the tail grouped by its best hub neighbour
    deg = np.bincount(a, minlength=V) + np.bincount(b, minlength=V)
    perm = np.argsort(-deg, kind="stable")
    H = min(GROUP_HUBS, V)
    if H < V:
        big = np.iinfo(np.int32).max
        hubrank = np.full(V, big, np.int64)
        hubrank[perm[:H]] = np.arange(H)
        primary = np.full(V, big, np.int64)
        np.minimum.at(primary, a, hubrank[b])
        np.minimum.at(primary, b, hubrank[a])
        tail = perm[H:]
        perm = np.concatenate([perm[:H], tail[np.argsort(primary[tail], kind="stable")]])
    inv = np.empty(V, np.int64)
    inv[perm] = np.arange(V)
    R = dict(V=V, directed=directed, perm=perm.astype(np.int32), inv=inv.astype(np.int32),
             vloss=np.asarray(vloss, np.float64)[perm])
    # self loops: the lowest edge id of each vertex
    self_lat, self_loss = np.full(V, np.nan), np.zeros(V)
    li = np.nonzero(~nl)[0][::-1]  # assigned last to first: the lowest edge id stays
    self_lat[inv[eu[li]]] = elat[li]
    self_loss[inv[eu[li]]] = eloss[li]
    R["self_lat"], R["self_loss"] = self_lat, self_loss
    # rows
    if directed:
        out = Rows(V, inv[a], inv[b], w, lo, e)
        inn = Rows(V, inv[b], inv[a], w, lo, e)
    else:
        out = inn = Rows(V, np.concatenate([inv[a], inv[b]]), np.concatenate([inv[b], inv[a]]),
                         np.concatenate([w, w]), np.concatenate([lo, lo]), np.concatenate([e, e]))
    R["out"], R["inn"] = out, inn
    R["rowptr"] = out.rowptr.astype(np.uint32)
    R["aloss"] = inn.loss
    R["hub_seg"], R["hub_multi"] = hub_segments(out.rowptr, H)
    # pi = d(h0, .) over the out-rows; directed: d(., h0) over the in-rows too
    pot = _distances(out, V)
    assert bool(np.isfinite(pot).all())
    R["pot"] = pot
    R["pi_max"] = np.asarray([pot.max()])
    if directed:
        R["rowptr_in"] = inn.rowptr.astype(np.uint32)
        R["pot_src"] = _distances(inn, V)
    # h0 tree over the in-rows: argmin (d(u), u) over the tight entries, the lowest position
    v, u, k = inn.row, inn.col, np.arange(inn.n)
    tight = (pot[u] < pot[v]) & (pot[u] + inn.w == pot[v]) & (u != v) & (v != 0)
    tv, tu, tk = v[tight], u[tight], k[tight]
    o = np.lexsort((tk, tu, pot[tu], tv))
    tv, tu, tk = tv[o], tu[o], tk[o]
    first = np.ones(len(tv), bool)
    first[1:] = tv[1:] != tv[:-1]
    parent = np.full(V, 0xFFFFFFFF, np.uint32)
    parent[tv[first]] = tu[first]
    R["spt_parent"] = parent
    R["tight_parents"] = np.bincount(tv, minlength=V)
    spt = np.zeros((V, 8), np.uint32)
    spt[:, :4] = 0xFFFFFFFF
    sv, sk = tv[first], tk[first]
    spt[sv, 0], spt[sv, 1] = tu[first], sk
    spt[sv, 2], spt[sv, 3] = split64(inn.w[sk])
    spt[sv, 4], spt[sv, 5] = split64(inn.loss[sk])
    R["spt"] = spt
    # kappa(x, y) = w - pi(y) over the out-rows, kappa0 = the row minimum, the records' field
    kap = out.w - pot[out.col]
    kap0d = out.row_min(kap, V)
    R["kf_kap"], R["kap0d"] = kap, kap0d
    field = (half_up(pot[out.col]) << 16) | half_dn(kap0d[out.col])
    if directed:
        R["adj_out"] = _records(out, field)
        R["adj"] = _records(inn, np.zeros(inn.n, np.uint32))
    else:
        R["adj"] = _records(out, field)
    # the plain relaxation copy: rows stably sorted by the image of f32_dn(kappa)
    kf = f32_dn(kap)
    o = np.lexsort((f32_order(kf), out.row))
    adjk = _records(out, field)[o]
    flag = parent[out.col[o]] == out.row[o]
    adjk[:, 0] |= np.where(flag, np.uint32(0x80000000), np.uint32(0))
    R["adjk"], R["kap"] = adjk, kf[o]
    R["ksum"], R["kap0"] = probes(out.rowptr, R["kap"])
    R["state"] = dict(adjk_plain=1, flagged=0, resorted=0, leaf=0, kprobes=KPROBES, kap_in_rec=1,
                      hub_seg_len=HUB_SEG, group_hubs=GROUP_HUBS)
    return R


def probes(rowptr, kap):
    """ksum [V, KPROBES] (kappa at row positions 2^q - 1, +inf past the row) and kap0"""
    V = len(rowptr) - 1
    n = rowptr[1:] - rowptr[:-1]
    ksum = np.full((V, KPROBES), PINF, np.float32)
    for q in range(KPROBES):
        pq = (1 << q) - 1
        has = pq < n
        ksum[has, q] = kap[rowptr[:-1][has] + pq]
    return ksum, ksum[:, 0].copy()


# ----------------------------------------------------------------------------------------------
# target preparation
# ----------------------------------------------------------------------------------------------
def bitmap(V, verts):
    out = np.zeros((V + 31) // 32, np.uint32)
    verts = np.asarray(verts, np.int64)
    np.bitwise_or.at(out, verts >> 5, (np.uint32(1) << (verts & 31).astype(np.uint32)))
    return out


def bits_of(bm, V):
    return ((bm[np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1).astype(bool)


def restate_leaves(R, targets):
    """leaf_targets_kernel: the 32-B record of every target, the effective target mask, the dead
    mask and the peeled count.  A target is peeled when its row holds one entry (u, w), u != t,
    and u's row holds more than one."""
    V, rows = R["V"], R["inn"]
    rp = rows.rowptr
    eff = np.zeros(V, bool)
    eff[targets] = True
    dead = np.zeros(V, bool)
    rec = np.zeros((len(targets), 8), np.uint32)
    rec[:, 0] = targets
    rec[:, 1] = NO_LEAF
    t = np.asarray(targets, np.int64)
    one = rp[t + 1] - rp[t] == 1
    u = np.where(one, rows.col[np.minimum(rp[t], max(rows.n - 1, 0))], 0)
    peel = one & (u != t) & (rp[u + 1] - rp[u] > 1)
    k = rp[t][peel]
    rec[peel, 1] = u[peel]
    rec[peel, 2], rec[peel, 3] = split64(rows.w[k])
    rec[peel, 4], rec[peel, 5] = split64(rows.loss[k])
    eff[t[peel]] = False
    dead[t[peel]] = True
    eff[u[peel]] = True
    return rec, eff, dead, int(peel.sum())


def kfix_iterates(R, tmask, dead, nit):
    """[K_0, ..., K_nit] and the matching Kt = target ? -inf : K.  One step:
    K(x) = min over x's out-row of target(y) ? kap : max(kap, (Kt(y) + w (1 - 2e-5)) - 1e-9),
    dead vertices forced to +inf."""
    V, out = R["V"], R["out"]
    kap = R["kf_kap"]

    def put(K):
        if dead is not None:
            K = np.where(dead, PINF, K)
        return K, np.where(tmask, NINF, K)

    Ks = [put(out.row_min(kap, V))]
    for _ in range(nit):
        Kt = Ks[-1][1]
        ky = (Kt[out.col] + out.w * (1.0 - 2e-5)) - 1e-9
        term = np.where(ky > kap, ky, kap)
        Ks.append(put(out.row_min(term, V)))
    return Ks


def restate_targets(R, targets, leaf=True, nit=TARGET_KAPPA, resort=True, skip=True):
    """The target-derived state after a build for `targets` (relabelled ids in the order of the
    table's columns).  leaf applies to undirected topologies only."""
    V, out = R["V"], R["out"]
    leaf = bool(leaf) and not R["directed"]
    T = {}
    tb = np.zeros(V, bool)
    tb[targets] = True
    T["peeled"] = 0
    dead = None
    tmask = tb
    if leaf:
        T["tleaf"], tmask, dead, T["peeled"] = restate_leaves(R, np.asarray(targets, np.int64))
        T["tbits_eff"] = bitmap(V, np.nonzero(tmask)[0])
        T["dead"] = bitmap(V, np.nonzero(dead)[0])
    T["tmask"], T["deadmask"] = tmask, dead
    if not skip:  # the copy stays the plain one
        T.update(adjk=R["adjk"], kap=R["kap"], ksum=R["ksum"], kap0=R["kap0"],
                 state=dict(R["state"]))
        return T
    T["tbits"] = bitmap(V, targets)
    Ks = kfix_iterates(R, tmask, dead, nit)
    T["iterates"] = Ks
    K, Kt = Ks[-1]
    T["kfix"] = np.concatenate([K, Kt])
    adjk = R["adjk"].copy()
    kap = R["kap"]
    col = (adjk[:, 0] & 0x3FFFFFFF).astype(np.int64)
    adjk[:, 0] = (adjk[:, 0] & ~np.uint32(0x40000000)) | (tmask[col].astype(np.uint32) << 30)
    row = out.row  # rows keep their ranges in every order
    order = np.arange(out.n)
    if resort:
        w = (adjk[:, 2].astype(np.uint64) | (adjk[:, 3].astype(np.uint64) << 32)).view(np.float64)
        t = w - R["pot"][col]
        ky = (K[col] + w * (1.0 - 2e-5)) - 1e-9
        t = np.where(~tmask[col] & (ky > t), ky, t)
        key = f32_dn(t)
        order = np.lexsort((radix_f32(key), row))  # stable, from the plain copy's order
        adjk, kap, col = adjk[order], key[order], col[order]
    T["order"] = order
    adjk[:, 1] = (adjk[:, 1] & 0xFFFF0000) | half_down(K[col])
    T["adjk"], T["kap"] = adjk, kap
    T["ksum"], T["kap0"] = probes(out.rowptr, kap)
    T["state"] = dict(R["state"], adjk_plain=0, flagged=1, resorted=int(bool(resort)),
                      leaf=int(leaf))
    return T


# ----------------------------------------------------------------------------------------------
# fixtures
# ----------------------------------------------------------------------------------------------
def doc_graph(nodes, edges):
    """The parsed graph of graphml_doc(nodes, edges): vertex ids in node order, edge ids in list
    order (what Topology.export_graph returns for the document)."""
    idx = {n[0]: i for i, n in enumerate(nodes)}
    eu = np.asarray([idx[e[0]] for e in edges], np.int32)
    ev = np.asarray([idx[e[1]] for e in edges], np.int32)
    elat = np.asarray([float(e[2]) for e in edges], np.float64)
    eloss = np.asarray([float(e[3]) for e in edges], np.float64)
    vloss = np.asarray([float(n[2]) for n in nodes], np.float64)
    return len(nodes), eu, ev, elat, eloss, vloss


@functools.lru_cache(maxsize=None)
def domain_graph(domain, directed=False):
    """(graphml bytes, parsed graph) of helpers.domain_graphml"""
    import oracle
    data = domain_graphml(domain, directed)
    g = oracle.read_graphml(data)
    ea, va = g["eattrs"], g["vattrs"]
    graph = (g["V"], g["eu"], g["ev"], np.asarray(ea["latency"], np.float64),
             np.asarray(ea["packetloss"], np.float64), np.asarray(va["packetloss"], np.float64))
    return data, graph, tuple(va["type"])


@functools.lru_cache(maxsize=None)
def domain_restated(domain, directed=False):
    return restate(domain_graph(domain, directed)[1], directed)


LATTICE = 16600
HUB_ROWS = (4096, 4097, 8192, 9001)
EXTRAS = 1500
SHAPE_POI = 48
SELF_LOOP_AT = 5   # lattice vertex with several self loops
IN_ONLY_HUB = 3    # directed twin: this hub's out-row keeps IN_ONLY_OUT entries
IN_ONLY_OUT = 10


@functools.lru_cache(maxsize=None)
def shapes_lists(directed=False):
    """(nodes, edges) of the shapes graph.
    * a ring lattice of LATTICE vertices (each joined to its next four: degree 8);
    * four hubs whose rows hold HUB_ROWS entries: spokes dealt round the lattice, so the first
      lattice vertices take two spokes and the rest one (degree 9-10);
    * EXTRAS vertices of degree 1 + j % 9 and SHAPE_POI pendant poi (type t<k>: host k is pinned
      to poi k; poi 1 mod 8 has a second uplink) hanging off one-spoke lattice vertices, at most
      one each: lattice degrees stay 9-10.  Listed after the lattice, so in the degree order they
      are the tail together with a few degree-9 lattice vertices: every tail-row length 1..9;
    * four self loops of different latency on one lattice vertex, one on every poi;
    * edge ids shuffled.
    directed: every edge becomes two arcs of independent latency and loss, except that hub
    IN_ONLY_HUB keeps only IN_ONLY_OUT out-arcs (long only in its in-row)."""
    rng = np.random.default_rng(20261020)
    lat = lambda: float(rng.uniform(1, 100))
    loss = lambda: float(rng.uniform(0, 0.01))
    N = LATTICE
    nodes = [("pop-%d" % i, "pop", 0.0) for i in range(N)]
    nodes += [("hub-%d" % h, "pop", 0.0) for h in range(len(HUB_ROWS))]
    nodes += [("x-%d" % j, "pop", 0.0) for j in range(EXTRAS)]
    nodes += [("poi-%d" % k, "t%d" % k, float(rng.uniform(0, 0.05))) for k in range(SHAPE_POI)]
    edges = []

    def both(a, b, out_arc=True):
        """the edge {a, b}; directed: the arcs a -> b (unless out_arc is False) and b -> a"""
        if not directed:
            edges.append((a, b, lat(), loss()))
            return
        if out_arc:
            edges.append((a, b, lat(), loss()))
        edges.append((b, a, lat(), loss()))

    for i in range(N):
        for d in range(1, 5):
            both("pop-%d" % i, "pop-%d" % ((i + d) % N))
    c = 0
    for h, n in enumerate(HUB_ROWS):
        for j in range(n):
            both("hub-%d" % h, "pop-%d" % (c % N),
                 out_arc=not (directed and h == IN_ONLY_HUB and j >= IN_ONLY_OUT))
            c += 1
    free = iter(range(c % N, N))  # lattice vertices with one spoke
    for j in range(EXTRAS):
        for _ in range(1 + j % 9):
            both("x-%d" % j, "pop-%d" % next(free))
    for k in range(SHAPE_POI):
        both("poi-%d" % k, "pop-%d" % next(free))
        if k % 8 == 1:
            both("poi-%d" % k, "pop-%d" % next(free))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0 + k, 0.001 * (k + 1)))
    for s in range(4):
        edges.append(("pop-%d" % SELF_LOOP_AT, "pop-%d" % SELF_LOOP_AT, 2.0 + s, 0.002 * (s + 1)))
    order = rng.permutation(len(edges))
    return nodes, [edges[i] for i in order]


@functools.lru_cache(maxsize=None)
def shapes_graph(directed=False):
    """(graphml bytes, parsed graph) of the shapes graph"""
    nodes, edges = shapes_lists(directed)
    return graphml_doc(nodes, edges, directed), doc_graph(nodes, edges)


@functools.lru_cache(maxsize=None)
def shapes_restated(directed=False):
    return restate(shapes_graph(directed)[1], directed)


def shapes_poi_vertex(k):
    return LATTICE + len(HUB_ROWS) + EXTRAS + k


# the two attached sets of the shapes tests (poi numbers): the second drops some of the first and
# adds others
SHAPE_SET1 = tuple(range(0, 30))
SHAPE_SET2 = tuple(range(12, 44))


@functools.lru_cache(maxsize=None)
def multigraph():
    """(graphml bytes, parsed graph) of a small multigraph: 300 parallel edges"""
    import oracle
    data = random_topology_graphml(n_routers=400, n_poi=40, extra=1600, seed=17, integer=True,
                                   parallel=300)
    g = oracle.read_graphml(data)
    ea, va = g["eattrs"], g["vattrs"]
    return data, (g["V"], g["eu"], g["ev"], np.asarray(ea["latency"], np.float64),
                  np.asarray(ea["packetloss"], np.float64),
                  np.asarray(va["packetloss"], np.float64))


DOMAIN_TARGET_HOSTS = 90


@functools.lru_cache(maxsize=None)
def domain_targets(domain, directed=False, n_hosts=DOMAIN_TARGET_HOSTS, seed=1):
    """The vertices helpers.attach_hosts(top, g, n_hosts, seed, type_hints=client/relay/server)
    attaches on the domain graph (the oracle's half of it), ascending and distinct."""
    import oracle
    from helpers import host_ip
    g = oracle.OGraph.from_graphml(domain_graph(domain, directed)[0])
    otop = oracle.OracleTopology(g)
    st, verts = seed, []
    hints = ("client", "relay", "server")
    for k in range(n_hosts):
        st = (st * 1103515245 + 12345) & 0xFFFFFFFF
        v, _ = otop.attach(host_ip(k + 1), st, type_hint=hints[k % 3])
        verts.append(v)
    return tuple(sorted(set(verts)))


# ----------------------------------------------------------------------------------------------
# coverage preconditions (conditions on the restatement, not measurements of the library)
# ----------------------------------------------------------------------------------------------
def resort_classes(R, T):
    """rows whose order changes in the re-sort, per size class of the segmented sort"""
    rp = R["out"].rowptr
    moved = T["order"] != np.arange(len(T["order"]))
    per_row = np.add.reduceat(moved, rp[:-1][rp[1:] > rp[:-1]]) > 0
    n = (rp[1:] - rp[:-1])[rp[1:] > rp[:-1]]
    return dict(wave=int((per_row & (n <= SEG_WAVE)).sum()),
                block=int((per_row & (n > SEG_WAVE) & (n <= SEG_BLOCK)).sum()),
                big=int((per_row & (n > SEG_BLOCK)).sum()))


def iterates_differ(T):
    """K_0 != K_1 and K_1 != the last iterate (bitwise)"""
    Ks = [k for k, _ in T["iterates"]]
    same = lambda x, y: np.array_equal(x.view(np.uint64), y.view(np.uint64))
    return len(Ks) > 2 and not same(Ks[0], Ks[1]) and not same(Ks[1], Ks[-1])
