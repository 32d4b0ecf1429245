"""CPU companion of test_latency_domains.py: what the latency domains of helpers.LATENCY_DOMAINS
put in front of the kernels, measured on the oracle over the very graphs the GPU tests use
(helpers.domain_oracle), and the oracle itself pinned in the new domains.

1. Preconditions of the generator, so that a later edit cannot silently empty a domain: the
   decimal domain has vertices with several bitwise parent candidates AND near-miss vertices (an
   in-neighbour whose f64 sum d(u) + w differs from d(v) but lies within 8 ulp: equal as reals, no
   candidate for the reference); quarter and int x 2^-30 have heap-order ties; bimodal straddles
   the f16 range; logu spans more than six decades; the tie-free domains have no vertex with two
   candidates.
2. The oracle against scipy (helpers.scipy_rows, independent of it) where the magnitudes are new.
3. The oracle's own power-of-two metamorphism: scaling every latency by 2^k scales every distance
   by 2^k exactly and changes no parent, so hops and reliability are bit-identical.
"""
import numpy as np
import pytest

from helpers import TIE_FREE_DOMAINS, domain_oracle, parent_candidates, scipy_rows
from load_helpers import tied_vertices

NSRC = 10  # the first 10 attached vertices


def counts(domain, directed):
    """Per source, averaged over the first NSRC attached vertices: vertices with >= 2 bitwise
    parent candidates, near-miss vertices, heap-order ties; and the largest candidate count."""
    g, ips, verts, (a, lat, rel, hops) = domain_oracle(domain, directed)
    multi = near = ties = most = 0
    for s in a[:NSRC]:
        d = g.dijkstra(int(s))[0]
        assert bool((d >= 0).all())  # connected
        exact, nearv = parent_candidates(g, d, int(s))
        assert bool((np.delete(exact, int(s)) >= 1).all())  # every vertex has its parent
        multi += int((exact >= 2).sum())
        near += int((nearv >= 1).sum())
        ties += int(tied_vertices(g, d, int(s)).sum())
        most = max(most, int(exact.max()))
    return multi / NSRC, near / NSRC, ties / NSRC, most


def test_parent_candidates_agree_with_the_oracles_tie_count():
    """The numpy candidate count used below against oracle.c's orc_parent_ties on the integer
    graph: a vertex the oracle sees tied at the minimal d(u) has >= 2 bitwise candidates."""
    g, ips, verts, (a, lat, rel, hops) = domain_oracle("int_dn30", False)
    s = int(a[0])
    d = g.dijkstra(s)[0]
    exact, _ = parent_candidates(g, d, s)
    pt = g.parent_ties(d, s)
    assert bool((exact >= pt).all()) and int((pt >= 2).sum()) > 0
    assert np.array_equal(pt >= 2, tied_vertices(g, d, s))


def test_decimal_domain_has_ties_and_near_misses():
    """k/10 latencies, undirected, per source of 3,100 vertices: 41.3 vertices with >= 2 bitwise
    candidates, 48.5 near-miss vertices, 2.0 heap-order ties (measured; floors of 10 leave room
    for another seed)."""
    multi, near, ties, _ = counts("dec", False)
    print("dec undirected: multi %.1f near %.1f ties %.1f" % (multi, near, ties))
    assert multi >= 10 and near >= 10


def test_decimal_domain_directed():
    """Directed k/10 graph, per source: 25.3 vertices with >= 2 bitwise candidates, 24.4
    near-miss vertices, 0.6 heap-order ties (measured)."""
    multi, near, ties, _ = counts("dec", True)
    print("dec directed: multi %.1f near %.1f ties %.1f" % (multi, near, ties))
    assert multi > 0 and near > 0


def chains_crossing(pv, s, targets, mask):
    """Targets whose parent chain from s crosses a vertex of mask (the target included)."""
    n = 0
    for t in targets:
        v, hit = int(t), False
        while v != s and not hit:
            hit = bool(mask[v])
            v = int(pv[v])
        n += hit
    return n


def test_decimal_near_misses_sit_on_table_chains():
    """What a parent rule looser than bitwise equality gets wrong, on the table's own pairs.  A
    decoy is a vertex with a near-miss in-neighbour u closer to the source than its parent: a
    rule that accepts sums within a few ulp and takes the smallest d(u) picks u, silently.
    Of the 69 x 69 table, 63 pairs in 40 rows (undirected) and 42 pairs in 33 rows (directed)
    have a decoy on their chain (measured; the floors of 10 pairs and 5 rows leave room for
    another seed)."""
    for directed in (False, True):
        g, ips, verts, (a, lat, rel, hops) = domain_oracle("dec", directed)
        pairs = rows = 0
        for s in a:
            s = int(s)
            d, pv, _, _ = g.dijkstra(s)
            nl = g.eu != g.ev
            u, v, w = g.eu[nl], g.ev[nl], g.elat[nl]
            if not directed:
                u, v, w = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([w, w])
            keep = v != s
            u, v, w = u[keep], v[keep], w[keep]
            sm = d[u] + w
            gap = np.abs(sm.view(np.int64) - d[v].view(np.int64))
            near = (sm != d[v]) & (gap <= 8) & (d[u] < d[pv[v]])
            decoy = np.zeros(g.V, bool)
            decoy[v[near]] = True
            k = chains_crossing(pv, s, a, decoy)
            pairs += k
            rows += k > 0
        print("dec directed=%d: pairs over a decoy %d, rows %d" % (directed, pairs, rows))
        assert pairs >= 10 and rows >= 5


@pytest.mark.parametrize("domain", ["quarter", "int_dn30"])
def test_dyadic_domains_have_heap_order_ties(domain):
    """Exact non-integer ties, undirected, per source: quarter 21.7 vertices with >= 2 candidates
    and 0.4 heap-order ties; int x 2^-30 89.3 and 3.5; no near miss in either (every sum is
    exact).  No latency is an integer in int x 2^-30, a quarter of them in quarter."""
    multi, near, ties, _ = counts(domain, False)
    print("%s undirected: multi %.1f near %.1f ties %.1f" % (domain, multi, near, ties))
    assert ties * NSRC >= 1 and multi > 0 and near == 0
    g, _, _, (a, _, _, _) = domain_oracle(domain, False)
    assert bool((g.elat != np.floor(g.elat)).any())  # the replay cannot take integer keys
    # table rows with a heap-order tie on a target's chain (the rows the batch kernel must flag
    # for the replay): int x 2^-30 6 of 69, quarter 0 (measured)
    rows = 0
    for s in a:
        d, pv, _, _ = g.dijkstra(int(s))
        rows += chains_crossing(pv, int(s), a, tied_vertices(g, d, int(s))) > 0
    print("%s: table rows crossing a heap-order tie %d" % (domain, rows))
    if domain == "int_dn30":
        assert rows >= 1


def test_bimodal_and_logu_ranges():
    g = domain_oracle("bimodal", False)[0]
    assert g.elat.max() > 65504 and g.elat.min() < 0.1  # above f16's maximum, below 0.1
    g = domain_oracle("logu", False)[0]
    assert g.elat.max() / g.elat.min() > 1e6


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("domain", TIE_FREE_DOMAINS)
def test_tie_free_domains_have_one_candidate_per_vertex(domain, directed):
    multi, near, ties, most = counts(domain, directed)
    assert multi == 0 and ties == 0 and most == 1


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("domain", ["logu", "bimodal", "real_dn30", "real_up30"])
def test_oracle_rows_equal_scipy(domain, directed):
    """8 oracle rows against scipy's Dijkstra + the helper over its predecessor trees: latency,
    reliability and hops bit for bit (tie-free domains: the shortest-path tree is unique)."""
    g, ips, verts, (a, lat, rel, hops) = domain_oracle(domain, directed)
    graph = (g.V, g.eu, g.ev, g.elat, g.eloss, g.vloss)
    slat, srel, shops = scipy_rows(graph, [int(s) for s in a[:8]], a, directed=directed)
    assert np.array_equal(slat.view(np.uint64), lat[:8].view(np.uint64))
    assert np.array_equal(srel.view(np.uint64), rel[:8].view(np.uint64))
    assert np.array_equal(shops, hops[:8])


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("base", ["real", "int"])
def test_oracle_power_of_two_metamorphism(base, directed):
    """Every latency times 2^k (k = -30, +30; no overflow, no subnormal): every f64 sum scales
    exactly, so the heap makes the same decisions -- hops and reliability bit-identical, latency
    the base latency times 2^k exactly."""
    g0, _, v0, (a0, lat0, rel0, hops0) = domain_oracle(base, directed)
    for tag, k in (("_dn30", -30), ("_up30", 30)):
        g, _, v, (a, lat, rel, hops) = domain_oracle(base + tag, directed)
        assert np.array_equal(g.elat, g0.elat * 2.0 ** k) and v == v0 and np.array_equal(a, a0)
        assert np.array_equal(lat.view(np.uint64), (lat0 * 2.0 ** k).view(np.uint64))
        assert np.array_equal(rel.view(np.uint64), rel0.view(np.uint64))
        assert np.array_equal(hops, hops0)
