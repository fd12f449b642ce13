"""The diversity score (mean MS-SSIM of image pairs; DESIGN.md, "In-training diversity score") restated for the tests.

``pair_scores`` is the float64 reference: the DIRECT 2-D window of 121 taps (scipy.signal.correlate2d, deliberately not
the separable form that the kernel uses), the 2 x 2-mean pyramid and the per-pair score.  ``emulate_fp32`` is the same
definition in float32 numpy arithmetic in a second summation order (separable, horizontal pass first, one rounding per
multiply and per add).  It is not compared with the device; it only sizes the gate:

    the two fp32 orders - the kernel's fused multiply-adds and this file's separate multiplies and adds - differ by
    reassociation and rounding placement only, so their distances to the float64 value are of one magnitude.  The gate
    of tests/test_gpu_msssim.py is 4 x the largest distance between ``emulate_fp32`` and ``pair_scores`` over exactly
    the inputs that the GPU tests use (``gate_cases``).  A tap or stride that is off by one pixel moves a mean by more than
    ten gates on these inputs (tests/test_msssim.py checks it).

MEAN_GAP / SCORE_GAP below are that measured distance (for the per-(pair, channel) means of cs and ssim, and for the
per-pair scores); tests/test_msssim.py recomputes both and fails if either is exceeded, so the constants cannot go stale.
bf16 inputs add nothing: the reference is fed the bf16-rounded values."""
import functools

import numpy as np
import scipy.signal

WEIGHTS5 = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2
TAPS, SIGMA = 11, 1.5
U32 = 2.0 ** -24                                           # unit round-off of fp32

# Measured by measure_gaps() over gate_cases() (numpy 1.x / 2.x give the same figures: the emulation is elementwise).
MEAN_GAP = 3.4e-5            # largest |fp32 emulation - float64| of a per-(pair, channel) mean of cs or ssim, any level
                             # (measured 3.314e-5)
SCORE_GAP = 3.0e-5           # the same for a pair's score (measured 2.995e-5)
MEAN_GATE = 4 * MEAN_GAP     # what the device's means may differ from float64 by
SCORE_GATE = 4 * SCORE_GAP


def window():
    d = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    g = np.exp(-d * d / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def sides(S):
    assert S >= 16 and S & (S - 1) == 0
    L = min(5, int(np.log2(S)) - 3)
    return [S >> i for i in range(L)]


def weights(L):
    w = np.asarray(WEIGHTS5[:L], dtype=np.float64)
    return w / w.sum()


def pool(x):
    """2 x 2 mean of [P, s, s, C]."""
    return 0.25 * (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2])


def pool_bound(x):
    """|fp32 pooled - exact| for fp32 inputs p00, p01, p10, p11 and the kernel's ((p00 + p01) + (p10 + p11)) * 0.25:
    s1 = (p00 + p01)(1 + e1), s2 = (p10 + p11)(1 + e2), s = (s1 + s2)(1 + e3), |e| <= u, and the scaling by 2^-2 is exact,
    so the error is at most u (|p00 + p01| + |p10 + p11|)(1 + u) + u |p00 + p01 + p10 + p11|, all times 0.25; (1 + 4u)
    covers the second-order terms."""
    x = np.asarray(x, dtype=np.float64)
    t, b = x[:, 0::2, 0::2] + x[:, 0::2, 1::2], x[:, 1::2, 0::2] + x[:, 1::2, 1::2]
    return 0.25 * U32 * (1 + 4 * U32) * (np.abs(t) + np.abs(b) + np.abs(t + b))


def _filter2d(u):
    """E[u] under the 121-tap window at every valid position: [P, s, s, C] -> [P, s-10, s-10, C]."""
    g = window()
    W = np.outer(g, g)
    out = np.empty((u.shape[0], u.shape[1] - TAPS + 1, u.shape[2] - TAPS + 1, u.shape[3]))
    for p in range(u.shape[0]):
        for c in range(u.shape[3]):
            out[p, :, :, c] = scipy.signal.correlate2d(u[p, :, :, c], W, mode="valid")
    return out


def level_means(xa, xb):
    """x-unit images [P, s, s, C] float64 -> (mean cs, mean ssim), each [P, C], over the (s - 10)^2 positions."""
    a, b = (xa + 1.0) / 2.0, (xb + 1.0) / 2.0
    mua, mub = _filter2d(a), _filter2d(b)
    va, vb, cab = _filter2d(a * a) - mua * mua, _filter2d(b * b) - mub * mub, _filter2d(a * b) - mua * mub
    cs = (2 * cab + C2) / (va + vb + C2)
    l = (2 * mua * mub + C1) / (mua * mua + mub * mub + C1)
    return cs.mean(axis=(1, 2)), (l * cs).mean(axis=(1, 2))


def combine(cs_means, ssim_last):
    """cs_means: [L-1] arrays [P, C]; ssim_last [P, C] -> scores [P]."""
    L = len(cs_means) + 1
    w = weights(L)
    prod = np.ones_like(ssim_last, dtype=np.float64)
    for i, m in enumerate(list(cs_means) + [ssim_last]):
        prod = prod * np.power(np.maximum(m, 0.0), w[i])
    return prod.mean(axis=1)


def pair_scores(xa, xb):
    """The float64 reference.  xa, xb [P, S, S, C] in [-1, 1] -> dict(scores [P], cs [L][P, C], ssim [L][P, C],
    pyramid [(a_i, b_i)] of every level)."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    cs, ss, pyr = [], [], []
    for i, _ in enumerate(sides(xa.shape[1])):
        pyr.append((xa, xb))
        m_cs, m_ss = level_means(xa, xb)
        cs.append(m_cs)
        ss.append(m_ss)
        xa, xb = pool(xa), pool(xb)
    return dict(scores=combine(cs[:-1], ss[-1]), cs=cs, ssim=ss, pyramid=pyr)


# ---------------------------------------------------------------- the fp32 emulation (sizes the gate only)
def _sep32(u, g):
    """Separable window in float32: horizontal pass then vertical, taps ascending, a rounding after every operation."""
    n = u.shape[2] - TAPS + 1
    h = np.zeros(u.shape[:2] + (n,) + u.shape[3:], dtype=np.float32)
    for k in range(TAPS):
        h = h + g[k] * u[:, :, k:k + n]
    m = u.shape[1] - TAPS + 1
    v = np.zeros((u.shape[0], m) + h.shape[2:], dtype=np.float32)
    for k in range(TAPS):
        v = v + g[k] * h[:, k:k + m]
    return v


def emulate_fp32(xa, xb):
    """The same definition in float32 (means over positions, powers and products in float64, as on the device)."""
    f = np.float32
    g = window().astype(f)
    xa, xb = np.asarray(xa, dtype=f), np.asarray(xb, dtype=f)
    cs_l, ss_l = [], []
    for _ in sides(xa.shape[1]):
        a, b = xa * f(0.5) + f(0.5), xb * f(0.5) + f(0.5)
        mua, mub = _sep32(a, g), _sep32(b, g)
        va, vb, cab = _sep32(a * a, g) - mua * mua, _sep32(b * b, g) - mub * mub, _sep32(a * b, g) - mua * mub
        cs = (f(2) * cab + f(C2)) / (va + vb + f(C2))
        l = (f(2) * mua * mub + f(C1)) / (mua * mua + mub * mub + f(C1))
        assert cs.dtype == f and l.dtype == f
        cs_l.append(cs.astype(np.float64).mean(axis=(1, 2)))
        ss_l.append((l * cs).astype(np.float64).mean(axis=(1, 2)))
        xa = ((xa[:, 0::2, 0::2] + xa[:, 0::2, 1::2]) + (xa[:, 1::2, 0::2] + xa[:, 1::2, 1::2])) * f(0.25)
        xb = ((xb[:, 0::2, 0::2] + xb[:, 0::2, 1::2]) + (xb[:, 1::2, 0::2] + xb[:, 1::2, 1::2])) * f(0.25)
    return dict(scores=combine(cs_l[:-1], ss_l[-1]), cs=cs_l, ssim=ss_l)


def gaps(xa, xb, ref=None):
    """(largest gap of a cs / ssim mean, largest gap of a score) between the emulation and the reference."""
    ref = pair_scores(xa, xb) if ref is None else ref
    emu = emulate_fp32(xa, xb)
    mean_gap = max(max(np.abs(e - r).max() for e, r in zip(emu[k], ref[k])) for k in ("cs", "ssim"))
    return float(mean_gap), float(np.abs(emu["scores"] - ref["scores"]).max())


# ---------------------------------------------------------------- the inputs of the GPU tests
KINDS = ("lowpass", "identical", "negated", "constant", "white")


def _lowpass(rng, S, C):
    """Uniform noise under a 5 x 5 box (wrapped), scaled back up and clipped to [-1, 1]."""
    x = rng.uniform(-1, 1, size=(S, S, C))
    acc = np.zeros_like(x)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            acc += np.roll(x, (dy, dx), axis=(0, 1))
    return np.clip(acc / 25.0 * 4.0, -1, 1)


def bf16_round(x):
    """float32 values rounded to the nearest bf16 (ties to even), as float32."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32)


def make_pairs(S, C, P, seed):
    """fp32 (a, b) [P, S, S, C]: pair p is of kind KINDS[p % 5] - two independent low-pass images; the same image twice;
    an image and its negative; two constants; two white-noise images."""
    rng = np.random.RandomState(seed)
    a, b = np.empty((P, S, S, C)), np.empty((P, S, S, C))
    for p in range(P):
        kind = KINDS[p % len(KINDS)]
        a[p] = _lowpass(rng, S, C)
        if kind == "lowpass":
            b[p] = _lowpass(rng, S, C)
        elif kind == "identical":
            b[p] = a[p]
        elif kind == "negated":
            b[p] = -a[p]
        elif kind == "constant":
            a[p], b[p] = 0.25, -0.5
        else:
            a[p], b[p] = rng.uniform(-1, 1, size=(S, S, C)), rng.uniform(-1, 1, size=(S, S, C))
    return a.astype(np.float32), b.astype(np.float32)


LEVEL_CASES = [(S, C, (1, 3, 5)[(i + j) % 3]) for i, S in enumerate((16, 32, 64, 128)) for j, C in enumerate((1, 3, 4))]
E2E_CASE = (64, 3, 6)


@functools.lru_cache(maxsize=None)
def case(S, C, P, dtype="fp32"):
    """The inputs of one GPU test and their float64 reference, computed once and shared; treat as read-only."""
    a, b = make_pairs(S, C, P, seed=1000 * S + 10 * C + P)
    if dtype == "bf16":
        a, b = bf16_round(a), bf16_round(b)
    return dict(a=a, b=b, ref=pair_scores(a, b), kinds=[KINDS[p % len(KINDS)] for p in range(P)])


def gate_cases():
    return [(S, C, P, d) for (S, C, P) in LEVEL_CASES + [E2E_CASE] for d in ("fp32", "bf16")]


def measure_gaps():
    worst = (0.0, 0.0)
    for key in gate_cases():
        k = case(*key)
        g = gaps(k["a"], k["b"], k["ref"])
        worst = (max(worst[0], g[0]), max(worst[1], g[1]))
    return worst
