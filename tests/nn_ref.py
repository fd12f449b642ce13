"""Float64 restatement of the nearest-training-image search (csrc/nearest.hip, neighbours.py), its error bound and the
case tables of tests/test_nn.py and tests/test_gpu_nn.py.  numpy only.

The bound.  A device distance is sum_j fl(fl(q_j - s_j)^2 + acc): one rounding in the subtraction, one in the fma, and at
most D additions in whatever order the kernel sums, all terms non-negative.  With u = 2^-24 every term carries a factor
within (1 +- u)^(D + 2) of its true value, so |d - d64| <= g d64 with g = (D + 2) u / (1 - (D + 2) u) (Higham,
"Accuracy and Stability of Numerical Algorithms", lemma 3.1).  Derived, not fitted."""
import numpy as np

U = 2.0 ** -24

# (Q, N, D): one lone row; N and Q across tile edges; D below / at / off the wave stride of 512; two query tiles
SHAPES = [(1, 1, 192), (3, 17, 192), (17, 1000, 1024), (16, 1000, 3072), (40, 257, 16384), (5, 5000, 768)]
SMALL_SHAPES = [(1, 1, 192), (3, 17, 192), (17, 40, 1024), (16, 20, 3072)]       # for the emulation and the mutations


# ---------------------------------------------------------------- bf16
def bf16_bits(x):
    """float array -> uint16 bf16 bit patterns, rounded to nearest even from the fp32 value (finite input)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """uint16 bf16 bit patterns -> float64 values."""
    return (np.asarray(bits, dtype=np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def bf16_ulp(x):
    """The spacing of bf16 numbers at |x| (8 significant bits), for normal x."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 7)


# ---------------------------------------------------------------- pack
def box_mean(x, f, mirror=False):
    """x [B,S,S,C] -> float64 [B, (S/f)(S/f)C]: the f x f box mean of the (mirrored) image, unrounded."""
    x = np.asarray(x, dtype=np.float64)
    if mirror:
        x = x[:, :, ::-1]
    B, S, _, C = x.shape
    s = S // f
    return x.reshape(B, s, f, s, f, C).mean(axis=(2, 4)).reshape(B, s * s * C)


# ---------------------------------------------------------------- distances
def distances(q, s):
    """float64 [Q,N] of sum_j (q - s)^2, as differences."""
    q, s = np.asarray(q, dtype=np.float64), np.asarray(s, dtype=np.float64)
    return np.stack([((s - row[None]) ** 2).sum(axis=1) for row in q])


def distances_loop(q, s):
    """The same by the definition, one element at a time (python floats are float64)."""
    return np.array([[sum((float(a) - float(b)) ** 2 for a, b in zip(qi, sn)) for sn in s] for qi in q])


def gamma(D):
    return (D + 2) * U / (1.0 - (D + 2) * U)


def bound(D, d64):
    return gamma(D) * np.asarray(d64, dtype=np.float64)


def distances_fp32_sequential(q, s, drop_last=0, row_shift=0, mirror_cols=None, reuse_tile=None):
    """An fp32 emulation that sums fully sequentially (the longest chain the bound allows), and the mutations of
    tests/test_nn.py: ``drop_last`` elements of every row left out, set rows read ``row_shift`` further (wrapping),
    ``mirror_cols`` = (side, C): the set rows' columns reversed, ``reuse_tile`` = QT: queries of the second tile of QT
    take the first tile's."""
    q32, s32 = np.asarray(q, dtype=np.float32), np.asarray(s, dtype=np.float32)
    if row_shift:
        s32 = np.roll(s32, -row_shift, axis=0)
    if mirror_cols is not None:
        side, C = mirror_cols
        s32 = s32.reshape(len(s32), side, side, C)[:, :, ::-1].reshape(len(s32), -1)
    if reuse_tile is not None:
        q32 = q32.copy()
        q32[reuse_tile:2 * reuse_tile] = q32[:len(q32[reuse_tile:2 * reuse_tile])]
    D = q32.shape[1] - drop_last
    acc = np.zeros((len(q32), len(s32)), dtype=np.float32)
    for j in range(D):
        d = (q32[:, j, None] - s32[None, :, j]).astype(np.float32)
        acc = (d.astype(np.float64) * d.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)   # one fma rounding
    return acc


def random_operands(rng, Q, N, D):
    """bf16-representable uniform values in [-1, 1]; with more than one query, the last one equals set row
    min(3, N - 1) (``planted_equal``)."""
    q, s = bf16_round(rng.uniform(-1, 1, size=(Q, D))), bf16_round(rng.uniform(-1, 1, size=(N, D)))
    if Q > 1:
        q[Q - 1] = s[min(3, N - 1)]
    return q, s


def planted_equal(Q, N):
    """(query, row) of the equal pair of ``random_operands``, None for a single query."""
    return (Q - 1, min(3, N - 1)) if Q > 1 else None


def exact_operands(rng, Q, N, D):
    """Operands from {-1, -1/2, 0, 1/2, 1}: every squared difference is a multiple of 1/4 up to 4 and every partial sum an
    integer multiple of 1/4 below 2^24 / 4, so fp32 is exact in any order."""
    vals = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    return vals[rng.randint(0, 5, size=(Q, D))], vals[rng.randint(0, 5, size=(N, D))]


# ---------------------------------------------------------------- selection and merge
def topk(dist, k):
    """(values [Q,k], indices [Q,k]) ascending by (value, index); (+inf, -1) past N."""
    dist = np.asarray(dist)
    Q, N = dist.shape
    v, i = np.full((Q, k), np.inf, dtype=dist.dtype), np.full((Q, k), -1, dtype=np.int64)
    for r in range(Q):
        order = np.lexsort((np.arange(N), dist[r]))[:k]
        v[r, :len(order)], i[r, :len(order)] = dist[r, order], order
    return v, i


def merge(plain, mirrored, k):
    """[(distance, index, mirrored)]: union, one entry per index (smaller distance, the plain one on equality), sorted
    by (distance, index), the first k."""
    rows = [(d, i, 0) for d, i in plain if i >= 0] + [(d, i, 1) for d, i in (mirrored or []) if i >= 0]
    rows.sort(key=lambda r: (r[1], r[0], r[2]))
    kept = [r for n, r in enumerate(rows) if n == 0 or rows[n - 1][1] != r[1]]
    return [(d, i, bool(m)) for d, i, m in sorted(kept, key=lambda r: (r[0], r[1]))][:k]


def nearest(queries, set_desc, side, C, k, mirror):
    """The composed search in float64 on descriptors: per query [(distance, index, mirrored)] and the full merged
    distance rows (min over plain / mirrored per index) for the gap check."""
    plain = distances(queries, set_desc)
    flipped = None
    if mirror:
        qm = np.asarray(queries).reshape(len(queries), side, side, C)[:, :, ::-1].reshape(len(queries), -1)
        flipped = distances(qm, set_desc)
    out, rows = [], []
    for r in range(len(queries)):
        pv, pi = topk(plain[r:r + 1], k)
        m = None
        if flipped is not None:
            mv, mi = topk(flipped[r:r + 1], k)
            m = list(zip(mv[0], mi[0]))
        out.append(merge(list(zip(pv[0], pi[0])), m, k))
        rows.append(plain[r] if flipped is None else np.minimum(plain[r], flipped[r]))
    return out, np.stack(rows)


# ---------------------------------------------------------------- the planted case of the composed test
PLANTED = dict(Q=5, N=300, side=32, C=3, k=8, a=0.02, seed=3)


def planted_case(seed=PLANTED["seed"]):
    """Images [.,32,32,3] with bf16-representable values (so that packing with f = 1 is exact) around which the order of
    the neighbours is decided by gaps far above the kernel's error: amid uniform fill, query i has the rows
    bf16(q_i + a 1.5^j noise), j < 8, planted at scattered indices, those of odd j as mirror images (only the mirrored
    search finds them), and the j = 2 row planted twice (an exact tie, decided by the index)."""
    p = PLANTED
    rng = np.random.RandomState(seed)
    shape = (p["side"], p["side"], p["C"])
    queries = bf16_round(rng.uniform(-1, 1, size=(p["Q"],) + shape))
    images = bf16_round(rng.uniform(-1, 1, size=(p["N"],) + shape))
    slots = rng.permutation(p["N"])[:p["Q"] * 9].reshape(p["Q"], 9)
    for i in range(p["Q"]):
        for j in range(8):
            row = bf16_round(queries[i] + p["a"] * 1.5 ** j * rng.standard_normal(shape))
            images[slots[i, j]] = row[:, ::-1] if j % 2 else row
            if j == 2:
                images[slots[i, 8]] = images[slots[i, j]]
    return dict(queries=queries.astype(np.float32), images=images.astype(np.float32), slots=slots, **p)


def gaps_are_decided(case):
    """The precondition of the composed test: for every query, every adjacent gap among the first k + 1 merged float64
    distances is exactly 0 or at least 100 x the bound.  Returns (ok, smallest non-zero gap / bound)."""
    D = case["side"] ** 2 * case["C"]
    q = case["queries"].reshape(case["Q"], D)
    s = case["images"].reshape(case["N"], D)
    _, rows = nearest(q, s, case["side"], case["C"], case["k"], True)
    worst = np.inf
    for r in rows:
        first = np.sort(r)[:case["k"] + 1]
        gap, b = np.diff(first), bound(D, first[1:])
        live = gap != 0
        if live.any():
            worst = min(worst, float((gap[live] / b[live]).min()))
    return worst >= 100.0, worst
