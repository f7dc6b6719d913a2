"""Plain references for the aggregation tests, with inputs whose results are known exactly.

numpy, math.fsum, fractions.Fraction and Python ints only: this module imports neither quickstep_amd nor the oracle.  Every
generator asserts the invariant its data must keep, so that a test fed data that breaks it fails instead of passing quietly.

Family A (exact by construction): DOUBLE / FLOAT values are integer multiples of 2^-e, and every value, every expression node and
the sum of |x| over every group stays below 2^(53-e) (FLOAT values below 2^(24-e)).  Every partial sum of every subset of a group
is then a multiple of 2^-e below 2^(53-e), hence representable: every summation order, atomics included, gives the same double bit
for bit, and np.bincount is an exact reference.  A correct path only ever adds values of one group together (the whole input is
the one group of a single state), so the bound per group is the one that matters.

Family B (realistic decimals): TPC-H-like prices and hundredths.  Per group the bound tol_g = 2 gamma(2 n_g + k) S_g holds for any
summation tree and for the factored rewrite (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 4.2): n_g rows, k
roundings in one term's expression, S_g = sum |term| over the group (float64, times 1 + gamma(n_g)).  The factor 2 covers the
reference's own error.  Where it is used, tol_g < min |term| over the group: one lost, doubled or swapped row exceeds it.

Family C (integers): INT arguments at INT32_MIN / INT32_MAX / -1 / 0 and over the full range, group sums beyond +-2^32; LONG
arguments odd, of magnitude in [2^40, 2^41), a sign per group, group sums beyond +-2^53 that a double cannot hold.

Family D (MIN / MAX extremes): infinities, the largest and smallest normal and subnormal values, signed zeros, INT64 and INT32
extremes, and groups whose only value is an accumulator's identity.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                          # unit roundoff of float64
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
HEAVY_ROWS = 4096                       # groups with more rows than this get an odd row count (family C, LONG)

# The group layouts tests/test_gpu_agg_exact.py draws: name -> (rows, groups, order, heavy groups).  Row counts are no multiple of
# a tile; where every group is heavy the row count has the parity of the group count (make_gids makes heavy counts odd).
LAYOUTS = {
    "single": (300_001, 1, "random", 0),
    "q1": (2_000_006, 4, "random", 0),
    "q1_small": (300_006, 4, "random", 0),
    "five": (300_005, 5, "random", 0),
    "few": (300_007, 37, "random", 0),
    "dense": (300_001, 5_000, "random", 2),
    "midsize": (600_001, 3_000, "random", 2),
    "directory": (1_000_003, 9_000, "random", 2),
    "growth": (400_003, 50_000, "random", 2),
    "two_level": (600_001, 120_000, "random", 2),
    "lds_flush": (1_500_001, 150_000, "clustered", 2),
}


def gamma(m):
    """gamma(m) = m u / (1 - m u), u = 2^-53."""
    mu = m * U
    assert mu < 1
    return mu / (1 - mu)


# ---- group numbers ---------------------------------------------------------------------------------------------------------
def make_gids(rng, n, groups, order="random", heavy=0):
    """The group number of every row, int64.  Every group gets at least two rows; the first `heavy` groups share half of the rows
    beyond those; the rest are spread at random.  Every group with more than HEAVY_ROWS rows gets an ODD row count (a sum of that
    many odd LONG values is odd, and beyond 2^53 an odd integer is no double).  order: "random" or "clustered" (sorted)."""
    assert n >= 2 * groups, "every group needs two rows"
    counts = np.full(groups, 2, dtype=np.int64)
    rest = n - 2 * groups
    if heavy:
        h = rest // 2
        counts[:heavy] += h // heavy
        counts[0] += h - h // heavy * heavy
        rest -= h
    counts += np.bincount(rng.integers(0, groups, size=rest), minlength=groups)
    even = [int(g) for g in np.nonzero((counts > HEAVY_ROWS) & (counts % 2 == 0))[0]]
    while len(even) >= 2:                              # move one row between two even heavy groups: both become odd
        a, b = even.pop(), even.pop()
        counts[a] += 1
        counts[b] -= 1
    if even:
        light = np.nonzero(counts < HEAVY_ROWS)[0]
        assert light.size, "no light group to take a row: choose n with the parity of the group count"
        counts[even[0]] -= 1
        counts[light[0]] += 1
    gid = np.repeat(np.arange(groups, dtype=np.int64), counts)
    if order == "random":
        rng.shuffle(gid)
    else:
        assert order == "clustered"
    got = np.bincount(gid, minlength=groups)
    assert gid.size == n and got.min() >= 2
    assert not np.any((got > HEAVY_ROWS) & (got % 2 == 0))
    return gid


def group_counts(gid, groups):
    return np.bincount(gid, minlength=groups).astype(np.int64)


def int_group_sums(gid, m, groups):
    """Exact per-group sums of an int64 array as Python ints (two 32-bit halves, each summed in int64 without overflow)."""
    m = np.asarray(m, dtype=np.int64)
    assert gid.size < 2**31
    hi, lo = m >> 32, m & 0xFFFFFFFF
    shi, slo = np.zeros(groups, np.int64), np.zeros(groups, np.int64)
    np.add.at(shi, gid, hi)
    np.add.at(slo, gid, lo)
    return [(int(a) << 32) + int(b) for a, b in zip(shi, slo)]


def assert_exact_multiples(x, e, limit_bits=53):
    """Every value of x is an integer multiple of 2^-e below 2^(limit_bits - e) in magnitude; returns the integers m = x 2^e."""
    scaled = np.ldexp(np.asarray(x, dtype=np.float64), e)
    assert np.all(np.isfinite(scaled)) and np.all(scaled == np.trunc(scaled)), f"values are not multiples of 2^-{e}"
    assert np.all(np.abs(scaled) < 2.0 ** limit_bits), f"a value reaches 2^({limit_bits}-{e})"
    return scaled.astype(np.int64)


def assert_exact_sums(x, e, gid, groups):
    """Family A's invariant for one term: multiples of 2^-e, and sum |x| 2^e < 2^53 over every group (exact integer arithmetic)."""
    m = assert_exact_multiples(x, e)
    sums = int_group_sums(gid, np.abs(m), groups)
    assert max(sums) < 2**53, f"a group's sum of |x| reaches 2^(53-{e}): its sums would round"
    return m


def exact_group_sums(x, gid, groups):
    """np.bincount over family-A values (every order of the additions gives these doubles)."""
    return np.bincount(gid, weights=np.asarray(x, dtype=np.float64), minlength=groups)


# ---- family A: exact by construction ------------------------------------------------------------------------------------------
def q1_terms(cols):
    """The Q1 expression nodes over a dict of columns: t1 = price * (1 - disc), t3 = t1 * (1 + tax)."""
    t1 = cols["price"] * (1.0 - cols["disc"])
    return {"t1": t1, "t3": t1 * (1.0 + cols["tax"])}


def family_a(rng, gid, groups):
    """Q1-like columns (price = a/2, a in [1800, 210000]; disc = b/64, b in 0..6; tax = c/64, c in 0..5; qty in 1..50) and a
    FLOAT column `fl` of multiples of 1/16 whose group sums a float32 cannot hold.  Exponents: price 1, disc and tax 6, t1 7,
    t3 13, fl 4."""
    n = gid.size
    a = rng.integers(1800, 210001, size=n)
    b = rng.integers(0, 7, size=n)
    c = rng.integers(0, 6, size=n)
    cols = dict(qty=rng.integers(1, 51, size=n).astype(np.float64), price=a / 2.0, disc=b / 64.0, tax=c / 64.0)
    cols.update(q1_terms(cols))
    assert np.array_equal(assert_exact_multiples(cols["t3"], 13), a * (64 - b) * (64 + c))      # the nodes computed without rounding
    for name, e in (("qty", 0), ("price", 1), ("disc", 6), ("tax", 6), ("t1", 7), ("t3", 13)):
        assert_exact_sums(cols[name], e, gid, groups)
    # FLOAT: k / 16 with |k| in [2^23, 2^24 - 2], a sign per group: |value| < 2^20 = 2^(24 - 4), exact in float32
    sign = np.where(rng.random(groups) < 0.5, -1, 1)[gid]
    k = rng.integers(2**23, 2**24 - 2, size=n) * sign
    sums = int_group_sums(gid, k, groups)
    first = np.full(groups, -1, dtype=np.int64)
    first[gid[::-1]] = np.arange(n - 1, -1, -1)                     # first row of every group
    for g in range(groups):                                         # a group sum that float32 holds: move one row by 1/16
        if float(np.float32(sums[g] / 16.0)) == sums[g] / 16.0:
            k[first[g]] += 1 if k[first[g]] > 0 else -1
    cols["fl"] = (k / 16.0).astype(np.float32)
    assert np.array_equal(cols["fl"].astype(np.float64) * 16.0, k.astype(np.float64))
    m = assert_exact_sums(cols["fl"], 4, gid, groups)
    assert np.all(np.abs(m) < 2**24), "a FLOAT value is not exact in float32"
    s = exact_group_sums(cols["fl"], gid, groups)
    assert np.all(s.astype(np.float32).astype(np.float64) != s), "a FLOAT group sum fits float32: a float32 accumulator would pass"
    return cols


def family_a_subnormal(rng, gid, groups):
    """`sd`: DOUBLE m 2^-1074 with 0 < |m| < 2^40 (every value subnormal), a sign per group, |m| scaled per group so that sum |m|
    < 2^53 (every partial sum is a multiple of 2^-1074 below 2^-1021: exact).  Groups of 8192 rows and more have a NORMAL sum.
    `sf`: FLOAT k 2^-149 with 0 < |k| < 2^23 (float32 subnormals), sum |k| < 2^53 per group (exact in double)."""
    n = gid.size
    cnt = group_counts(gid, groups)
    top = np.minimum(2**40 - 1, (2**53 - 1) // np.maximum(cnt, 1))           # per group: |m| <= top, sum |m| < 2^53
    sign = np.where(rng.random(groups) < 0.5, -1, 1)
    hi = top[gid]
    m = (rng.integers(0, 2**62, size=n) % (hi // 3 + 1) + hi - hi // 3) * sign[gid]   # |m| in [2 top / 3, top]
    sd = np.ldexp(m.astype(np.float64), -1074)
    assert np.array_equal(np.ldexp(sd, 1074).astype(np.int64), m), "a subnormal value did not survive the conversion"
    assert np.all(np.abs(sd) < np.finfo(np.float64).tiny) and np.all(sd != 0)
    sums = int_group_sums(gid, np.abs(m), groups)
    assert max(sums) < 2**53
    k = rng.integers(1, 2**23, size=n) * sign[gid]
    sf = (k.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert np.array_equal((sf.astype(np.float64) * 2.0**149).astype(np.int64), k)
    assert np.all(np.abs(sf) < np.finfo(np.float32).tiny)
    assert max(int_group_sums(gid, np.abs(k), groups)) < 2**53
    return dict(sd=sd, sf=sf)


def subnormal_groups_with_normal_sums(cols, gid, groups):
    """Groups whose values are all subnormal but whose exact sum is a normal double."""
    s = exact_group_sums(cols["sd"], gid, groups)
    return np.nonzero(np.abs(s) >= np.finfo(np.float64).tiny)[0]


# ---- family B: realistic decimals -----------------------------------------------------------------------------------------------
def family_b(rng, gid, groups):
    """TPC-H-like: price with two decimals in [900, 105000], disc in 0.01..0.10, tax in 0.01..0.08, qty in 1..50 (no zero term:
    the bound must stay below the smallest term)."""
    n = gid.size
    cols = dict(qty=rng.integers(1, 51, size=n).astype(np.float64), price=rng.integers(90_000, 10_500_001, size=n) / 100.0,
                disc=rng.integers(1, 11, size=n) / 100.0, tax=rng.integers(1, 9, size=n) / 100.0)
    cols.update(q1_terms(cols))
    return cols


# roundings inside one term: 1 - disc, price * that (t1); 1 + tax, t1 * that (t3).  For the factored rewrite the coefficient's own
# roundings plus one give the same counts.
FAMILY_B_ROUNDINGS = {"qty": 0, "price": 0, "disc": 0, "tax": 0, "t1": 2, "t3": 4}


def family_b_reference(x, gid, groups):
    """math.fsum per group (correctly rounded) for at most 64 groups, np.bincount otherwise (its own error is within
    gamma(n_g) S_g, which the factor 2 of the bound covers)."""
    x = np.asarray(x, dtype=np.float64)
    if groups > 64:
        return np.bincount(gid, weights=x, minlength=groups)
    order = np.argsort(gid, kind="stable")
    edges = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=groups))])
    xs = x[order]
    return np.array([math.fsum(xs[edges[g]:edges[g + 1]]) for g in range(groups)])


def family_b_tolerance(x, gid, groups, k):
    """tol_g = 2 gamma(2 n_g + k) S_g, S_g = sum |x| (float64) (1 + gamma(n_g)); asserts tol_g < min |x| over every group."""
    x = np.asarray(x, dtype=np.float64)
    cnt = group_counts(gid, groups)
    s = np.bincount(gid, weights=np.abs(x), minlength=groups) * np.array([1 + gamma(int(c)) for c in cnt])
    tol = np.array([2 * gamma(2 * int(c) + k) for c in cnt]) * s
    smallest = np.full(groups, np.inf)
    np.minimum.at(smallest, gid, np.abs(x))
    assert np.all(tol < smallest), "the family-B bound is not below the smallest term: one lost row could pass"
    return tol


# ---- family C: integers ---------------------------------------------------------------------------------------------------------
def family_c(rng, gid, groups):
    """`i` INT: about 10 % of the rows INT32_MIN / INT32_MAX / -1 / 0, 20 % the full range, the rest within 2^27 of INT32_MAX or
    INT32_MIN by the group's sign.  `l` LONG: odd, |l| in [2^40, 2^41), a sign per group."""
    n = gid.size
    sign = np.where(np.arange(groups) % 2 == 0, 1, -1)[gid]
    i = np.where(sign > 0, rng.integers(INT32_MAX - 2**27, INT32_MAX, size=n, endpoint=True),
                 rng.integers(INT32_MIN, INT32_MIN + 2**27, size=n, endpoint=True))
    r = rng.random(n)
    full = r < 0.2
    i[full] = rng.integers(INT32_MIN, INT32_MAX, size=int(full.sum()), endpoint=True)
    special = r > 0.9
    i[special] = rng.choice(np.array([INT32_MIN, INT32_MAX, -1, 0]), size=int(special.sum()))
    i = i.astype(np.int32)
    for v in (INT32_MIN, INT32_MAX, -1, 0):
        assert np.any(i == v)
    lsign = np.where(rng.random(groups) < 0.5, -1, 1)
    lsign[:2] = [1, -1][:groups]                                           # (the heavy groups of a layout: one of each sign)
    lsign = lsign[gid]
    mag = rng.integers(2**39, 2**40, size=n) * 2 + 1                       # odd, in [2^40, 2^41)
    l = (mag * lsign).astype(np.int64)
    assert np.all(np.abs(l) >= 2**40) and np.all(np.abs(l) < 2**41) and np.all(l % 2 != 0)
    assert max(int_group_sums(gid, np.abs(l), groups)) < 2**63, "a LONG group sum of |x| reaches 2^63: partial sums could wrap"
    return dict(i=i, l=l)


def family_c_sums(cols, gid, groups):
    """Python-int group sums of `i` and `l`."""
    return int_group_sums(gid, cols["i"].astype(np.int64), groups), int_group_sums(gid, cols["l"], groups)


def assert_family_c_ranges(cols, gid, groups):
    """Some INT group sums below -2^32 and some above 2^32; some LONG group sums in (2^53, 2^63) and some in (-2^63, -2^53), every
    one of them beyond what a double holds."""
    si, sl = family_c_sums(cols, gid, groups)
    assert any(s < -2**32 for s in si) and any(s > 2**32 for s in si), "no INT group sum beyond 32 bits"
    big = [s for s in sl if abs(s) > 2**53]
    assert any(2**53 < s < 2**63 for s in big) and any(-2**63 < s < -2**53 for s in big), "no LONG group sum beyond 2^53"
    assert all(int(float(s)) != s for s in big), "a LONG group sum beyond 2^53 is a double: a double accumulator would pass"
    return si, sl


def avg_of_int_sum(s, c):
    """The exact AVG of an integer group: Fraction(S, c) rounded once when |S| < 2^53 (the kernel's double(S) / double(c) is then
    one rounding of the exact quotient)."""
    return float(Fraction(s, c))


def assert_int_avg(got, s, c):
    """AVG over an integer sum: exact when |S| < 2^53, else within two roundings (double(sum) / double(count))."""
    want = avg_of_int_sum(s, c)
    if abs(s) < 2**53:
        assert got == want, (got, want, s, c)
    else:
        assert abs(Fraction(got) - Fraction(s, c)) <= Fraction(2.0001 * U) * abs(Fraction(s, c)), (got, s, c)


# ---- family D: MIN / MAX extremes -----------------------------------------------------------------------------------------------
DOUBLE_EXTREMES = np.array([-np.inf, -np.finfo(np.float64).max, -1.0, -2.0**-1074, -0.0, 0.0, 2.0**-1074, np.finfo(np.float64).tiny,
                            1.0, np.finfo(np.float64).max, np.inf])
FLOAT_EXTREMES = np.array([-np.inf, -np.finfo(np.float32).max, -1.0, -2.0**-149, -0.0, 0.0, 2.0**-149, np.finfo(np.float32).tiny,
                           1.0, np.finfo(np.float32).max, np.inf], dtype=np.float32)
LONG_EXTREMES = np.array([INT64_MIN, INT64_MIN + 1, -1, 0, INT64_MAX - 1, INT64_MAX], dtype=np.int64)
INT_EXTREMES = np.array([INT32_MIN, -1, 0, INT32_MAX], dtype=np.int32)


def family_d(rng, gid, groups, identity_only=None):
    """Every value drawn from the extremes above.  Group 0: every value the MIN accumulators' identity (INT64_MAX, +inf);
    group 1: the MAX identities (INT64_MIN, -inf); group 2: INT64_MAX / -inf; group 3: INT64_MIN / +inf.  No NaN.  identity_only:
    every row of every group one of those four (a single state's one group: groups = 1)."""
    n = gid.size
    cols = dict(l=rng.choice(LONG_EXTREMES, size=n), d=rng.choice(DOUBLE_EXTREMES, size=n), f=rng.choice(FLOAT_EXTREMES, size=n),
                i=rng.choice(INT_EXTREMES, size=n))
    if identity_only is not None:
        lv, dv = ((INT64_MAX, np.inf), (INT64_MIN, -np.inf), (INT64_MAX, -np.inf), (INT64_MIN, np.inf))[identity_only]
        cols["l"][:], cols["d"][:], cols["f"][:] = lv, dv, np.float32(dv)
        return cols
    for g, (lv, dv) in enumerate(((INT64_MAX, np.inf), (INT64_MIN, -np.inf), (INT64_MAX, -np.inf), (INT64_MIN, np.inf))[:groups - 1]):
        rows = gid == g
        cols["l"][rows] = lv
        cols["d"][rows] = dv
        cols["f"][rows] = np.float32(dv)
    for name, want in (("l", LONG_EXTREMES), ("d", DOUBLE_EXTREMES), ("f", FLOAT_EXTREMES), ("i", INT_EXTREMES)):
        assert not np.any(np.isnan(cols[name].astype(np.float64)))
        assert set(np.unique(cols[name]).tolist()) == set(np.unique(want).tolist()), f"not every extreme of {name} occurs"
    return cols


def group_min_max(x, gid, groups, valid=None):
    """Per-group MIN and MAX (numpy's ufunc.at: the value itself, no rounding) over the rows where valid is True, and the
    number of such rows."""
    x = np.asarray(x)
    if valid is not None:
        x, gid = x[valid], gid[valid]
    if np.issubdtype(x.dtype, np.floating):
        lo, hi = np.full(groups, np.inf, dtype=x.dtype), np.full(groups, -np.inf, dtype=x.dtype)
    else:
        info = np.iinfo(x.dtype)
        lo, hi = np.full(groups, info.max, dtype=x.dtype), np.full(groups, info.min, dtype=x.dtype)
    np.minimum.at(lo, gid, x)
    np.maximum.at(hi, gid, x)
    return lo, hi, np.bincount(gid, minlength=groups)
