"""The host function behind option "h0_seed" (shdtopo_test_h0_seed): the seed of the batch kernel's
landmark bound for a source at prepared distance p from the landmark h0 on a V-vertex graph is
p (1 + m) rounded up, m = max(1e-9, 4 V 2^-53).  No device use."""
import math

import numpy as np

from shadow_amd import _lib as L

U = 2.0 ** -53


def seed(p, V):
    lib, _ = L.load()
    return float(lib.shdtopo_test_h0_seed(float(p), int(V)))


def margin(V):
    return max(1e-9, 4.0 * V * U)


def test_zero_stays_zero():
    for V in (1, 1000, 10**6, 10**9):
        assert seed(0.0, V) == 0.0


def test_infinity_stays_infinity():
    for V in (1, 1000, 10**6, 10**9):
        assert seed(math.inf, V) == math.inf


def test_at_least_p_and_within_twice_the_margin():
    rng = np.random.default_rng(5)
    ps = np.concatenate([10.0 ** rng.uniform(-6, 9, 400), [1e-300, 1.0, 1e300]])  # normal numbers
    for V in (1, 7, 1000, 990_000, 3_000_000, 10**9):
        m = margin(V)
        for p in ps:
            s = seed(p, V)
            assert s > p  # rounded up: never p itself
            assert s <= p * (1.0 + 2.0 * m)
            # past the rounding of both summation orders over fewer than V hops: 2 V u
            assert s >= p * (1.0 + 2.0 * V * U)


def test_monotone_in_the_vertex_count():
    rng = np.random.default_rng(6)
    Vs = (1, 1000, 10**6, 2 * 10**6, 3 * 10**6, 10**8, 10**12)
    for p in 10.0 ** rng.uniform(-3, 6, 200):
        s = [seed(p, V) for V in Vs]
        assert all(a <= b for a, b in zip(s, s[1:]))
        assert s[-1] > s[0]  # the V term takes over past 1e-9 / (4 u) = 2.25 M vertices


def test_monotone_in_p():
    ps = np.sort(10.0 ** np.random.default_rng(7).uniform(-3, 6, 300))
    s = [seed(p, 990_000) for p in ps]
    assert all(a <= b for a, b in zip(s, s[1:]))
