"""Hand-made A x A tables installed behind a topology (shdtopo_bind_table / shdtopo_bind_table_ref),
the shared inputs of test_bound_tables.py and test_bound_tables_cpu.py.

Every kernel that reads the finished table -- the diff, the flow impact, the packet route, the row
minima, the getters' row copy -- reads it through one pointer pair, and bind_table* put a caller's
table there.  A test of such a kernel therefore needs no graph search: it makes the two tables it
wants in numpy (make_tables plants the cases a link failure never produces), installs them
(install) into topologies whose columns are pinned (bound_topologies) and compares with the numpy
references that take any pair of tables (whatif_helpers.expected_diff,
impact_helpers.expected_impact, oracle.route_packets, numpy.min).

Nothing here imports torch at module level; install does, when called.
"""
import collections
import functools

import numpy as np

import shadow_amd as sa
from helpers import graphml_doc, host_ip
from impact_helpers import UNATTACHED_IP, expected_impact

U64 = np.uint64
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)   # the edges of a 64-lane word and a 256-column step
IMPACT_SIZES = (2, 65, 257)
BIG = 64.0       # the largest planted rise, in two rows
TIE = 2.0        # the rise of every planted row tie
OFF_GRID = 2.0 ** -20  # added to the old latency of a one-ulp cell: lat * 1e6 is then no integer


# ---- topologies whose columns are known in advance ----
def poi_ip(k):
    return "12.%d.%d.%d" % ((k >> 16) & 255, (k >> 8) & 255, k & 255)


@functools.lru_cache(maxsize=None)
def pinned_doc(P):
    """One router and P poi vertices, each poi with an uplink to the router, a self loop and an ip
    of its own: strongly connected, not complete, and a host attached with ipHint = poi_ip(k + 1)
    lands on poi k whatever its random stream says.  (A stub router behind the router keeps the
    graph of P = 1, two vertices and their edge, from being complete.)"""
    nodes = [("pop-0", "pop", 0.0), ("pop-1", "pop", 0.0)]
    nodes += [("poi-%d" % k, "client", 0.0, poi_ip(k + 1)) for k in range(P)]
    edges = [("pop-0", "pop-1", 1.0, 0.0)]
    for k in range(P):
        edges.append(("poi-%d" % k, "pop-0", 5.0, 0.0))
        edges.append(("poi-%d" % k, "poi-%d" % k, 1.0, 0.0))
    return graphml_doc(nodes, edges)


def bound_topologies(P, k=2):
    """k independent topologies of pinned_doc(P) with one host per poi (host h on poi h, so column
    h of every table is host_ip(h + 1)): (topologies, ips uint32[P])."""
    ips = np.array([host_ip(h + 1) for h in range(P)], np.uint32)
    tops = []
    for _ in range(k):
        top = sa.Topology.from_buffer(pinned_doc(P))
        assert top is not None and not top.is_complete
        for h in range(P):
            v, _ = top.attach_ip(int(ips[h]), 1, ipHint=poi_ip(h + 1))
            assert v == h + 2
        a = top.attached_vertices()
        assert len(a) == P
        tops.append(top)
    for top in tops[1:]:
        assert np.array_equal(top.attached_vertices(), tops[0].attached_vertices())
    assert np.array_equal(tops[0].attached_vertices(), attached_of(P))
    return tops, ips


def attached_of(A):
    """The attached vertices of bound_topologies(A): the routers are vertices 0 and 1."""
    return np.arange(2, A + 2, dtype=np.int32)


# ---- the two tables ----
Tables = collections.namedtuple("Tables", "t0 t1 plan")


@functools.lru_cache(maxsize=None)
def make_tables(A, seed=5):
    """(t0, t1, plan): two tables (attached, lat, rel, hops) in the form expected_diff and
    expected_impact take, computed once and shared (never modified).

    t0: latencies k / 4 in [0.25, 200] with an even k above the diagonal and an odd k below it (so
    lat[i, j] != lat[j, i]), reliabilities k / 1024 in [0, 1], hops in [1, 40] -- apart from the
    cells a planted change needs otherwise (the one-ulp cells are off the 1/4 grid, the hop-limit
    cells hold 0 and 65535).  Every latency is a multiple of 2^-20 below 2^8, so every planted
    difference is exact.

    t1 is t0 plus the changes below, each in a row of its own; an item whose row or columns do not
    exist at this A is left out, and plan says what was planted: name -> list of cells (row, col)
    or of rows, empty when left out.

      row 0   rise BIG with hops up at column 0, fall with hops down at column 1 (one 64-column
              word), reliability only at 2, hops only at 3, all three at 4
      row 1   a one-ulp rise at column 0 (0 ns), rise BIG at column 1: the largest rise twice
      row 2   one ulp up at column 0, one ulp down at column 1: ceil(lat * 1e6) does not move
      row 3   hops 0 -> 65535 at column 0, 65535 -> 0 at column 1
      row 4   rise TIE at columns 2 and 3, a smaller rise at 0
      row 5   changed in every column (rises and falls alternate); row 6 changed in none
      row 7   changed at column 0 only; row 8 at column A - 1 only; row 9 at 255 and 256 only
      row 10  rise TIE at columns 0 and 64 (two wavefronts), a smaller rise at 1
      row 11  rise TIE at columns 0 and 256 (one thread, two steps), a smaller rise at 1
      row 12  rise TIE at 114 and 138, a smaller one at 5: the lower column of the tie is in lane
              50 of wavefront 1, the other in lane 10 of wavefront 2, the smaller rise in lane 5
              of wavefront 0
      row 13  the same with 266 for 138: lane 10 of wavefront 0 at the second step
      rows 16 and up, those not divisible by 3: about one cell in 20 changed, kinds at random,
              rises of at most 16"""
    rng = np.random.default_rng([seed, A])
    k = rng.integers(1, 401, (A, A))
    i, j = np.indices((A, A))
    k = np.where(i < j, 2 * k, np.where(i > j, 2 * k - 1, k))
    lat0 = k * 0.25
    rel0 = rng.integers(0, 1025, (A, A)) / 1024.0
    hops0 = rng.integers(1, 41, (A, A)).astype(np.uint16)
    plan = collections.defaultdict(list)

    # cells of t0 that a planted change needs off the general recipe
    if A >= 2:
        lat0[1, 0] += OFF_GRID
    if A >= 3:
        lat0[2, 0] += OFF_GRID
        lat0[2, 1] += OFF_GRID
    if A >= 4:
        hops0[3, 0], hops0[3, 1] = 0, 65535
    lat1, rel1, hops1 = lat0.copy(), rel0.copy(), hops0.copy()

    def other_rel(x):
        return np.where(x < 1.0, x + 1.0 / 2048, x - 1.0 / 2048)

    def rise(r, c, by, name=None):
        lat1[r, c] = lat0[r, c] + by
        if name:
            plan[name].append((r, c))

    def fall(r, c, name=None):
        lat1[r, c] = lat0[r, c] - 0.125
        if name:
            plan[name].append((r, c))

    # row 0
    rise(0, 0, BIG, "big")
    hops1[0, 0] = hops0[0, 0] + 3
    if A >= 2:
        fall(0, 1, "fall_beside_rise")
        hops1[0, 1] = hops0[0, 1] - 1
    if A >= 5:
        rel1[0, 2] = other_rel(rel0[0, 2])
        plan["rel_only"].append((0, 2))
        hops1[0, 3] = hops0[0, 3] + 1
        plan["hops_only"].append((0, 3))
        rise(0, 4, 1.0, "all_three")
        rel1[0, 4] = other_rel(rel0[0, 4])
        hops1[0, 4] = hops0[0, 4] + 2
    # row 1
    if A >= 2:
        lat1[1, 0] = np.nextafter(lat0[1, 0], np.inf)
        plan["ulp_up"].append((1, 0))
        rise(1, 1, BIG, "big")
    # row 2
    if A >= 3:
        lat1[2, 0] = np.nextafter(lat0[2, 0], np.inf)
        plan["ulp_up"].append((2, 0))
        lat1[2, 1] = np.nextafter(lat0[2, 1], -np.inf)
        plan["ulp_down"].append((2, 1))
    # row 3
    if A >= 4:
        hops1[3, 0], hops1[3, 1] = 65535, 0
        plan["hops_0_to_max"].append((3, 0))
        plan["hops_max_to_0"].append((3, 1))

    def tie(name, r, lo, hi, small):
        """rise TIE at columns lo < hi of row r, a smaller rise at `small`: (row, lo, hi)"""
        if r < A and hi < A:
            rise(r, lo, TIE)
            rise(r, hi, TIE)
            rise(r, small, 1.0)
            plan[name].append((r, lo, hi))

    tie("tie_adjacent", 4, 2, 3, 0)
    if A >= 7:
        for c in range(A):
            (rise(5, c, 0.5) if c % 2 == 0 else fall(5, c))
        plan["row_all"].append(5)
        plan["row_none"].append(6)
    if A >= 10:
        rise(7, 0, 1.0)
        plan["row_col0"].append(7)
        fall(8, A - 1)
        plan["row_last"].append(8)
    if A >= 257:
        rise(9, 255, 1.0)
        fall(9, 256)
        plan["row_255_256"].append(9)
    tie("tie_64", 10, 0, 64, 1)
    tie("tie_256", 11, 0, 256, 1)
    tie("tie_wave", 12, 114, 138, 5)
    tie("tie_wave_step", 13, 114, 266, 5)
    # rows 16 and up
    for r in range(16, A):
        if r % 3 == 0:
            continue
        cols = np.flatnonzero(rng.random(A) < 0.05)
        kinds = rng.integers(0, 4, len(cols))
        by = rng.integers(1, 65, len(cols)) * 0.25
        for c, kd, b in zip(cols, kinds, by):
            if kd == 0:
                rise(r, c, b)
            elif kd == 1:
                fall(r, c)
            elif kd == 2:
                rel1[r, c] = other_rel(rel0[r, c])
            else:
                hops1[r, c] = hops0[r, c] + 1
    for x in (lat0, rel0, hops0, lat1, rel1, hops1):
        x.setflags(write=False)
    a = attached_of(A)
    a.setflags(write=False)
    return Tables((a, lat0, rel0, hops0), (a, lat1, rel1, hops1), dict(plan))


@functools.lru_cache(maxsize=None)
def rowmin_table(A, seed=9):
    """(t, pos, mins): a table whose row i has its minimum latency at column pos[i] -- pos cycles
    through 0, 1, 63, 64, 65, 255, 256, A - 1, clipped to A -- and the "no edge" value -1.0 (with
    reliability -1.0) in about one cell in 8 off the diagonal and off pos.  mins[i] = the minimum
    over the non-negative entries of row i; the rows' minima are distinct and > 0."""
    rng = np.random.default_rng([seed, A])
    lat = rng.integers(4 * (A + 2), 4 * (A + 2) + 800, (A, A)) * 0.25
    rel = rng.integers(0, 1025, (A, A)) / 1024.0
    hops = rng.integers(1, 41, (A, A)).astype(np.uint16)
    cyc = np.array([0, 1, 63, 64, 65, 255, 256, A - 1])
    pos = np.minimum(cyc[np.arange(A) % len(cyc)], A - 1)
    rows = np.arange(A)
    hole = rng.random((A, A)) < 0.125
    hole[rows, rows] = False
    hole[rows, pos] = False
    lat[hole] = -1.0
    rel[hole] = -1.0
    lat[rows, pos] = 0.25 * (rng.permutation(A) + 1)  # distinct, below every other entry
    mins = np.where(lat >= 0, lat, np.inf).min(axis=1)
    assert np.array_equal(mins, lat[rows, pos]) and len(set(mins.tolist())) == A
    return (attached_of(A), lat, rel, hops), pos, mins


def pack(t):
    """The device layout of a table: (lr f64 [A, A, 2], hops as int16 [A, A]), numpy."""
    _, lat, rel, hops = t
    lr = np.ascontiguousarray(np.stack([lat, rel], axis=-1), np.float64)
    return lr, np.array(hops, np.uint16).view(np.int16)  # (a copy: the shared tables are read-only)


def install(top, t, how="copy"):
    """Put table t behind top: bind_table (how="copy") or bind_table_ref (how="ref") with
    lat.min() as the global minimum.  Returns the device tensors (lr, hops) that were bound."""
    import torch
    lr, hops = (torch.from_numpy(x).cuda() for x in pack(t))
    torch.cuda.synchronize()
    bind = {"copy": top.bind_table, "ref": top.bind_table_ref}[how]
    bind(lr, hops, float(t[1].min()))
    return lr, hops


# ---- the flows of the impact tests ----
@functools.lru_cache(maxsize=None)
def bound_flows(A, T, seed=17):
    """Flows over make_tables(A), T = the impact tile (the tile_flows stat): dict with src_col /
    dst_col (int32; -1 or A: unattached), weight (uint64, full range), payload (uint32), worst (the
    two planted positions of the largest rise, more than T apart), unattached_at and edge_sets
    (name -> uint64 edges).  Computed once, shared, never modified.

      320 random pairs; 3 T + 17 more with 130 copies of a changed pair and 130 of an unchanged
      one in their middle; one flow per planted cell of make_tables' plan; every pair once when
      A <= 65; 8 random pairs.  Five flows with an unattached end are then inserted so that they
      sit at 0, 63, 64, n / 2 and n - 1, and pair (0, 0) -- the largest rise -- replaces the
      random pair at flows 1, 2 (one wavefront) and 258 (flow 2's thread, one step later), pair
      (1, 1), the same rise, those at 70 (the next wavefront) and at n - 3 (another tile)."""
    t0, t1, plan = make_tables(A)
    rng = np.random.default_rng([seed, A])
    rnd = lambda m: (rng.integers(0, A, m), rng.integers(0, A, m))
    half = (3 * T + 17) // 2
    changed = (t0[1].view(U64) != t1[1].view(U64)) | (t0[2].view(U64) != t1[2].view(U64)) | \
        (t0[3] != t1[3])
    ch, same = np.argwhere(changed), np.argwhere(~changed)
    parts = [rnd(320), rnd(half), (np.repeat(ch[len(ch) // 2][0], 130),
                                   np.repeat(ch[len(ch) // 2][1], 130))]
    if len(same):
        parts.append((np.repeat(same[len(same) // 2][0], 130),
                      np.repeat(same[len(same) // 2][1], 130)))
    parts.append(rnd(3 * T + 17 - half))
    cells = [x for v in plan.values() for x in v if isinstance(x, tuple)]
    cells = [(x[0], c) for x in cells for c in x[1:]]  # (row, col) and (row, lo, hi)
    parts.append((np.array([r for r, _ in cells]), np.array([c for _, c in cells])))
    if A <= 65:
        parts.append(tuple(np.divmod(np.arange(A * A), A)))
    parts.append(rnd(8))
    src = np.concatenate([x for x, _ in parts]).astype(np.int32)
    dst = np.concatenate([y for _, y in parts]).astype(np.int32)
    big = plan["big"]
    # (positions before the insertion: 1 -> 0, 2 -> 1, 70 -> 67, 258 -> 255, n - 3 -> len - 2)
    for at, (r, c) in ((0, big[0]), (1, big[0]), (255, big[0]), (67, big[-1]),
                       (len(src) - 2, big[-1])):
        src[at], dst[at] = r, c
    n = len(src) + 5
    assert n > 3 * T
    at = np.array([0, 63, 64, n // 2, n - 1])
    keep = np.ones(n, bool)
    keep[at] = False
    s, d = np.zeros(n, np.int32), np.zeros(n, np.int32)
    s[keep], d[keep] = src, dst
    s[at[[0, 2, 4]]] = -1
    d[at[[1, 3]]] = A
    w = rng.integers(0, 2**64, n, dtype=U64)
    pay = rng.integers(0, 2**32, n, dtype=np.uint32)
    rises = np.unique(expected_impact(t0, t1, s, d, w, [])["rises_ns"])
    exact = np.unique(np.concatenate([rises, rises + U64(1), np.array([2**63], U64)]))
    keep = exact[:-1][:300]  # (every one of them at these sizes)
    filler = np.setdiff1d(np.arange(1024, dtype=U64) * U64(7919) + U64(3), keep)
    many = np.sort(np.concatenate([keep, filler[:1023 - len(keep)], np.array([2**63], U64)]))
    assert len(many) == 1024 and (np.diff(many.astype(object)) > 0).all()
    for x in (s, d, w, pay):
        x.setflags(write=False)
    return dict(src_col=s, dst_col=d, weight=w, payload=pay, worst=(1, n - 3), unattached_at=at,
                edge_sets={"none": np.zeros(0, U64), "zero": np.zeros(1, U64), "exact": exact,
                           "max": many})


def flow_ips(ips, col):
    """Host IPs of flow columns (a column outside [0, A) becomes an address that is not attached)."""
    col = np.asarray(col)
    ok = (col >= 0) & (col < len(ips))
    return np.where(ok, ips[np.where(ok, col, 0)], np.uint32(UNATTACHED_IP)).astype(np.uint32)


# ---- the packet route's inputs ----
def glibc_chance(state):
    """glibc's rand_r and Shadow's random_nextDouble, restated in numpy: (chance f64, next state
    u32) of uint32 states -- three steps of the 1103515245 / 12345 generator giving 11 + 10 + 10
    bits, divided by RAND_MAX."""
    with np.errstate(over="ignore"):
        s = np.asarray(state, np.uint32).copy()
        s = s * np.uint32(1103515245) + np.uint32(12345)
        r = (s // np.uint32(65536)) % np.uint32(2048)
        s = s * np.uint32(1103515245) + np.uint32(12345)
        r = (r << np.uint32(10)) ^ ((s // np.uint32(65536)) % np.uint32(1024))
        s = s * np.uint32(1103515245) + np.uint32(12345)
        r = (r << np.uint32(10)) ^ ((s // np.uint32(65536)) % np.uint32(1024))
    return r.astype(np.float64) / 2147483647.0, s


ROUTE_A = 64
ROUTE_JUMP = 3_000_000
REL_KINDS = ("equal", "ulp_below", "ulp_above", "zero", "one")
# the issue's latencies and one more, 2.9999985 ms = ROUTE_JUMP - 1 ns, so that the clamp sees a
# delay one below, at and one above the jump
ROUTE_LATS = (0.5, 3.0, float(np.nextafter(3.0, 4.0)), 1e-300, 1e-6, float(np.nextafter(1e-6, 1.0)),
              100.0 * 2.0 ** 30, 2.9999985)


@functools.lru_cache(maxsize=None)
def route_inputs(seed=29):
    """The packet route's table and window: a 64 x 64 table and 4096 packets, packet k on pair
    (k // 64, k % 64) alone, so each pair's reliability is made from its packet's own draw:
    rel kind k % 5 (REL_KINDS), latency (k // 5) % 8 (ROUTE_LATS), payload 0 when (k // 40) % 2 else
    1448.  dict: t, src_col, dst_col, payload, state, now, chance, rel_kind, lat_kind."""
    A = ROUTE_A
    n = A * A
    rng = np.random.default_rng(seed)
    state = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    chance, _ = glibc_chance(state)
    while True:  # a draw of exactly 0 or 1 has no neighbour inside [0, 1]
        bad = (chance <= 0.0) | (chance >= 1.0)
        if not bad.any():
            break
        state[bad] = rng.integers(0, 2**32, int(bad.sum()), dtype=np.uint64).astype(np.uint32)
        chance, _ = glibc_chance(state)
    kidx = np.arange(n)
    rel_kind, lat_kind = kidx % 5, (kidx // 5) % len(ROUTE_LATS)
    rel = np.select([rel_kind == 0, rel_kind == 1, rel_kind == 2, rel_kind == 3],
                    [chance, np.nextafter(chance, -1.0), np.nextafter(chance, 2.0), 0.0], 1.0)
    lat = np.array(ROUTE_LATS)[lat_kind]
    payload = np.where((kidx // 40) % 2 == 1, 0, 1448).astype(np.uint32)
    now = rng.integers(10**9, 2 * 10**9, n).astype(np.uint64)
    hops = np.ones((A, A), np.uint16)
    t = (attached_of(A), lat.reshape(A, A), rel.reshape(A, A), hops)
    return dict(t=t, src_col=(kidx // A).astype(np.int32), dst_col=(kidx % A).astype(np.int32),
                payload=payload, state=state, now=now, chance=chance, rel_kind=rel_kind,
                lat_kind=lat_kind)
