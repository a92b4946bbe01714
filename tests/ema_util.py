"""Shared by the moving-average tests: the float64 oracle of one update, its exactness proof, the test inputs.

Oracle: ``E' = float32(float64(e) + float64(w) * float64(float32(p - e)))``.  The product of two float32 values is exact
in float64 (24 + 24 significant bits); the sum is rounded to float64 and then to float32, which can differ from the
single rounding of a fused multiply-add only where the float64 sum falls within 2^-29 of its own size of a float32
rounding boundary.  `correctly_rounded` decides with exact rational arithmetic whether that happened; the host test
proves that it does not for any element the GPU tests compare, so they compare bit for bit with nothing excluded."""

from fractions import Fraction

import numpy as np

# the three weights of the tests: 1 - decay for decay 0.9, 0.9998 and 2/11 (the first warm-up update), formed in double
# and rounded once, as ema.weight_of does
WEIGHTS = [float(np.float32(1.0 - 0.9)), float(np.float32(1.0 - 0.9998)), float(np.float32(1.0 - 2.0 / 11.0))]
SEED, N_SEEDED = 20261, 18000

# (e, p, what the kernel must leave in e, as float32 bits, or None: the oracle's value) - the same for every w
_NEG0, _POS0 = np.float32(-0.0), np.float32(0.0)
PLANTED = [
    (np.float32(1.5), np.float32(1.5), np.float32(1.5)),                      # p == e: e keeps its bits
    (np.float32(-3.25e-3), np.float32(-3.25e-3), np.float32(-3.25e-3)),
    (np.float32(3.0e38), np.float32(3.0e38), np.float32(3.0e38)),
    (_POS0, _POS0, _POS0),
    (_NEG0, _NEG0, _POS0),        # the one exception: (-0) - (-0) = +0, w * (+0) + (-0) = +0 in round-to-nearest
    (_POS0, _NEG0, _POS0),
    (_NEG0, _POS0, _POS0),
    (np.float32(1e-40), np.float32(3e-40), None),                             # a denormal pair: nothing is flushed
    (np.float32(-2e-41), np.float32(1e-44), None),
    (np.float32(1e30), np.float32(0.0), None),
    (np.float32(-1e30), np.float32(1e30), None),
    (np.float32(1e30), np.float32(1.0000001e30), None),
]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits1(x):
    """The bits of one float32 value as an int."""
    return int(np.float32(x).view(np.uint32))


def oracle(e, p, w):
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    d = (p - e).astype(np.float32)                       # float32 subtraction, rounded once
    return (e.astype(np.float64) + np.float64(np.float32(w)) * d.astype(np.float64)).astype(np.float32)


def seeded(n, seed=SEED, scale=0.01):
    """n normal values and the same values perturbed at `scale`: a weight buffer and what a few optimizer steps later
    stands in its place."""
    rng = np.random.RandomState(seed)
    e = rng.standard_normal(n).astype(np.float32)
    p = (e + np.float32(scale) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    return e, p


def inputs(n):
    """The GPU test's arrays of n elements: the N_SEEDED seeded pairs, repeated when n is larger (so every element is
    one the host test has proven), with the planted cases written over the front (as many as fit)."""
    e, p = seeded(N_SEEDED)
    e, p = np.resize(e, n).copy(), np.resize(p, n).copy()
    for i, (pe, pp, _) in enumerate(PLANTED[:n]):
        e[i], p[i] = pe, pp
    return e, p


def correctly_rounded(e, p, w, r):
    """Is float32 r the correctly rounded (nearest, ties to even) value of e + w * float32(p - e), computed exactly?"""
    e, p, w, r = np.float32(e), np.float32(p), np.float32(w), np.float32(r)
    d = np.float32(p - e)
    exact = Fraction(float(e)) + Fraction(float(w)) * Fraction(float(d))
    if not np.isfinite(r):
        return False
    err = abs(exact - Fraction(float(r)))
    for nb in (np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))):
        if not np.isfinite(nb):
            continue
        other = abs(exact - Fraction(float(nb)))
        if other < err or (other == err and int(r.view(np.uint32)) & 1):     # a tie goes to the even mantissa
            return False
    return True
