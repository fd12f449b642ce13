"""Float64 restatement of precision / recall / density / coverage (csrc/prdc.hip, metrics.Prdc), its error bound and the
case tables of tests/test_prdc.py and tests/test_gpu_prdc.py.  numpy only.

Definitions, all on squared distances d(a, b) = sum_j (a_j - b_j)^2 (Kynkaanniemi et al. 2019; Naeem et al. 2020):

    rad_k(x; X)   the k-th smallest d(x, x') over x' in X without x itself - the row of the same index; another row of
                  equal content counts, ties count with multiplicity
    precision     (1/M) #{j : exists i, d(f_j, r_i) <= rad_k(r_i; R)}
    density       (1/(k M)) sum_j #{i : d(f_j, r_i) <= rad_k(r_i; R)}
    recall        (1/N) #{i : exists j, d(r_i, f_j) <= rad_k(f_j; F)}
    coverage      (1/N) #{i : min_j d(r_i, f_j) <= rad_k(r_i; R)}

``<=`` is inclusive everywhere.  The selections and counts are direct loops over a float64 distance matrix; for the exact
operands (multiples of 1/8) the matrix is made in integers, so that nothing is rounded at all.

The bound is that of tests/nn_ref.py: the device distance is the same arithmetic, |d - d64| <= gamma(D) d64 with
gamma(D) = (D + 2) u / (1 - (D + 2) u), u = 2^-24.  A membership test d <= rad compares two such numbers, so it may go either
way only when |d - rad| <= 2 gamma(D) max(d, rad) in float64: such a pair is *undecided*.  Derived, not fitted.

The ``mutate`` argument of the references names one deliberate mistake; tests/test_prdc.py shows that every one of them
changes a result on the case tables below."""
import numpy as np

from tests.nn_ref import U, bf16_round, gamma  # noqa: F401  (the bound and bf16 rounding, shared with the search)

MUTATIONS = ("strict", "self", "k_plus_one", "padded_query")

# ---------------------------------------------------------------- case tables
# radii (N, D, k): N = k + 1; one full block; one row past a block; the second LDS chunk and the lane tail with three equal
# rows; 13 blocks
RADII_CASES = [(9, 64, 8), (16, 64, 1), (17, 192, 3), (61, 2112, 3), (203, 576, 5)]
# cover (Q, N, D): one pair; one tile and one block; a ragged tile with an all-zero set row; the second LDS chunk with
# ragged tiles and blocks; ten tiles, nine blocks
COVER_CASES = [(1, 1, 64), (8, 16, 64), (13, 17, 192), (197, 203, 2112), (75, 130, 576)]
# generic (N, M, D, k), case number = position
GENERIC_CASES = [(203, 197, 192, 3), (203, 197, 2112, 5), (130, 75, 576, 1)]
UNDECIDED_SHARE = 0.002              # of the pairs of a cover pass; a condition on the cases, checked before the device is


# ---------------------------------------------------------------- distances
def distances(q, s):
    """float64 [Q,N] of sum_j (q - s)^2, as differences."""
    q, s = np.asarray(q, dtype=np.float64), np.asarray(s, dtype=np.float64)
    return np.stack([((s - row[None]) ** 2).sum(axis=1) for row in q])


def distances_exact(q, s):
    """The same for operands that are multiples of 1/8, in int64: exact."""
    q8, s8 = np.rint(np.asarray(q) * 8).astype(np.int64), np.rint(np.asarray(s) * 8).astype(np.int64)
    assert np.array_equal(q8 / 8.0, q) and np.array_equal(s8 / 8.0, s)
    d = np.stack([((s8 - row[None]) ** 2).sum(axis=1) for row in q8])
    assert d.max() < 2 ** 24                      # in units of 1/64: every fp32 partial sum is exact in any order
    return d / 64.0


# ---------------------------------------------------------------- the references, as direct loops
def radii(x, k, dist=distances, mutate=None):
    """float64 [N]: the k-th smallest distance of row n to the rows m != n."""
    d = dist(x, x)
    N = len(d)
    kk = k + 1 if mutate == "k_plus_one" else k
    out = np.empty(N, dtype=np.float64)
    for n in range(N):
        others = sorted(float(d[n, m]) for m in range(N) if m != n or mutate == "self")
        out[n] = others[min(kk, len(others)) - 1]
    return out


def cover(q, radius_q, s, dist=distances, mutate=None):
    """(count int64 [N], dmin float64 [N]): count[n] = #{i : d(q_i, s_n) <= radius_q[i]}, dmin[n] = min_i d(q_i, s_n)."""
    q, radius_q = np.asarray(q, dtype=np.float64), np.asarray(radius_q, dtype=np.float64)
    if mutate == "padded_query":                  # the zero rows that fill the last tile of 8 take part, with radius 0
        pad = -len(q) % 8
        q = np.concatenate([q, np.zeros((pad, q.shape[1]))])
        radius_q = np.concatenate([radius_q, np.zeros(pad)])
    d = dist(q, s)
    Q, N = d.shape
    count, dmin = np.zeros(N, dtype=np.int64), np.full(N, np.inf)
    for n in range(N):
        for i in range(Q):
            inside = d[i, n] < radius_q[i] if mutate == "strict" else d[i, n] <= radius_q[i]
            count[n] += 1 if inside else 0
            dmin[n] = min(dmin[n], d[i, n])
    return count, dmin


def reduce4(count_f, count_r, dmin_r, radius_r, mutate=None):
    inside = (lambda a, b: a < b) if mutate == "strict" else (lambda a, b: a <= b)
    return [sum(1 for c in count_f if c > 0), sum(int(c) for c in count_f), sum(1 for c in count_r if c > 0),
            sum(1 for a, b in zip(dmin_r, radius_r) if inside(a, b))]


def ratios(out4, k, N, M):
    return {"precision": out4[0] / float(M), "recall": out4[2] / float(N), "density": out4[1] / float(k * M),
            "coverage": out4[3] / float(N)}


def scores(real, fake, k, dist=distances, mutate=None):
    """The four scores of two descriptor sets, composed as an event composes them."""
    rr, rf = radii(real, k, dist, mutate), radii(fake, k, dist, mutate)
    count_f, _ = cover(real, rr, fake, dist, mutate)
    count_r, dmin_r = cover(fake, rf, real, dist, mutate)
    return ratios(reduce4(count_f, count_r, dmin_r, rr, mutate), k, len(real), len(fake))


# ---------------------------------------------------------------- undecided pairs
def undecided(d, rad, D):
    """Boolean, elementwise: the comparison of d with rad may go either way on the device."""
    d, rad = np.asarray(d, dtype=np.float64), np.asarray(rad, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        close = np.abs(d - rad) <= 2.0 * gamma(D) * np.maximum(d, rad)
    return close & np.isfinite(rad) & ~((d == 0) & (rad == 0))     # inf is never reached; 0 against 0 is exact


def cover_bands(q, radius_q, s):
    """(sure int64 [N], open int64 [N], dmin float64 [N], undecided share): the device's count[n] lies in
    [sure[n], sure[n] + open[n]]."""
    D = np.asarray(q).shape[1]
    d = distances(q, s)
    rad = np.asarray(radius_q, dtype=np.float64)[:, None]
    und = undecided(d, rad, D)
    sure = ((d <= rad) & ~und).sum(axis=0)
    return sure.astype(np.int64), und.sum(axis=0).astype(np.int64), d.min(axis=0), float(und.mean())


def score_bands(real, fake, k):
    """{name: (lowest, highest)}: what the device's scores may be, the undecided pairs going either way.  Radii in
    float64; a device radius within the bound moves a comparison only inside the undecided band."""
    D = np.asarray(real).shape[1]
    N, M = len(real), len(fake)
    rr, rf = radii(real, k), radii(fake, k)
    sf, of, _, _ = cover_bands(real, rr, fake)
    sr, orr, dmin_r, _ = cover_bands(fake, rf, real)
    cu = undecided(dmin_r, rr, D)
    c_lo, c_hi = int(((dmin_r <= rr) & ~cu).sum()), int(((dmin_r <= rr) | cu).sum())
    return {"precision": ((sf > 0).sum() / float(M), (sf + of > 0).sum() / float(M)),
            "recall": ((sr > 0).sum() / float(N), (sr + orr > 0).sum() / float(N)),
            "density": (sf.sum() / float(k * M), (sf + of).sum() / float(k * M)),
            "coverage": (c_lo / float(N), c_hi / float(N))}


# ---------------------------------------------------------------- operands
def exact_rows(rng, n, D):
    """Multiples of 1/8 in [-1, 1]: bf16 holds them, every squared difference is a multiple of 1/64 up to 4, and with
    D <= 2112 every sum stays below 2^24 / 64, so fp32 is exact in any order."""
    return rng.integers(-8, 9, size=(n, D)) / 8.0


def radii_operands(case):
    N, D, k = RADII_CASES[case]
    x = exact_rows(np.random.default_rng(10 + case), N, D)
    if N > 40:
        x[5] = x[6] = x[40]                        # three equal rows: neighbours of each other at distance 0
    return x


def cover_operands(case):
    """(q, radius_q, set).  Set row 3 equals query 1, whose radius is 0 (the pair counts); query 2 has radius +inf; the
    radius of query 0 is exactly its distance to set row N // 2 (the pair counts); the other radii are a third of the way
    from the nearest to the farthest row.  With N > 7, set row 7 is all zeros: no query is, so its dmin is positive."""
    Q, N, D = COVER_CASES[case]
    rng = np.random.default_rng(20 + case)
    q, s = exact_rows(rng, Q, D), exact_rows(rng, N, D)
    if Q > 1 and N > 3:
        s[3] = q[1]
    if N > 7:
        s[7] = 0.0
    d = distances_exact(q, s)
    rad = d.min(axis=1) + (d.max(axis=1) - d.min(axis=1)) / 3.0
    rad[0] = d[0, N // 2]
    if Q > 1:
        rad[1] = 0.0
    if Q > 2:
        rad[2] = np.inf
    return q, rad.astype(np.float32).astype(np.float64), s


def generic_operands(case):
    """(real [N,D], fake [M,D], k) of bf16-representable rows: 8 centres from N(0, 0.5); real rows around all 8 in turn,
    fake rows around the first 4 in turn, noise of sigma 0.15; clipped to [-1, 1]; the first M // 8 fake rows replaced by
    U(-1, 1).  The fakes miss half of the modes and an eighth of them lies off the data."""
    N, M, D, k = GENERIC_CASES[case]
    rng = np.random.default_rng(100 + case)
    centres = rng.normal(0.0, 0.5, size=(8, D))
    real = centres[np.arange(N) % 8] + rng.normal(0.0, 0.15, size=(N, D))
    fake = centres[np.arange(M) % 4] + rng.normal(0.0, 0.15, size=(M, D))
    real, fake = np.clip(real, -1.0, 1.0), np.clip(fake, -1.0, 1.0)
    fake[:M // 8] = rng.uniform(-1.0, 1.0, size=(M // 8, D))
    return bf16_round(real), bf16_round(fake), k
