"""The radial power spectrum (csrc/powerspec.hip, metrics.PowerSpectrum) restated once in float64, the kernel's algorithm
restated in NumPy fp32, the inputs of the tests and the gates that follow from them.  Nothing here is fitted to the device.

Definition.  NHWC images in [-1, 1]; C = 1 is used as it is, C = 3 / 4 through Y = 0.299 R + 0.587 G + 0.114 B (alpha is
ignored).  F = DFT2(Y), unnormalised, signed frequencies ky, kx in [-S/2, S/2); P = |F|^2 / S^4, so that sum P =
mean(Y^2); no window, no mean subtraction.  Bin r = (isqrt(4 (ky^2 + kx^2)) + 1) // 2, which is round(sqrt(.)) in integers
and has no ties; NB(S) = (isqrt(2 S^2) + 1) // 2 + 1 bins reach the corner (S/2, S/2).  The profile of an image is the
mean of P over the coefficients of the FULL plane in each bin.  The reference bins the full ``fft2``; the device and the
restatement keep the columns kx = 0 .. S/2 and count 0 < kx < S/2 twice: an independent formulation.

Gate per coefficient - derived (``power_bound``).  u = 2^-24 is the unit round-off of fp32.
  * One radix-2 stage of a Cooley-Tukey transform with twiddles of absolute error mu multiplies the relative 2-norm error
    by at most 1 + eta, eta = mu + gamma_4 (sqrt 2 + mu), gamma_4 = 4u / (1 - 4u) (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., theorem 24.2): gamma_4 covers one complex multiplication (error <= sqrt 5 u) and one
    complex addition.  The twiddles are rounded once from fp64: each component is off by at most u, so mu <= u (the
    restatement's table is the same; a component that is itself rounded twice, fp64 then fp32, stays within u).
    eta <= u + 4 sqrt 2 u + O(u^2) = 6.66 u < 7 u: c = 7.
  * A radix-4 pass is two such stages with fewer roundings (one twiddle multiplication per output, the other rotation
    is by -i, exact), so log2(S^2) = 2 log2 S stages bound the 2-D transform.  Packing two real rows into one complex
    transform Z keeps the norms: ||A||^2 + ||B||^2 = ||Z||^2 for the true values and for the errors (parallelogram law);
    the split itself is one complex addition and an exact halving per output, (1 + u), which the slack 0.34 u per stage
    (at least 8 stages) covers.  Hence ||F^ - F||_2 <= 7 u log2(S^2) ||F||_2.
  * Luminance: three products and two sums of values in [-1, 1] with coefficients rounded to fp32 (or fused, which only
    removes roundings): |Y^ - Y| <= 3u per pixel, ||dY||_2 <= 3u S, and the DFT2 has norm S: 3u S^2 on top.
  * So |F^_k - F_k| <= delta = 7 u log2(S^2) ||F||_2 + 3 u S^2 for every k, and with P^ = fl(fl(re^2 + im^2) / S^4), three
    roundings and an exact scaling: |P^ - P| <= ((2 |F_k| delta + delta^2) (1 + 3u) + 3u |F_k|^2) / S^4.
  The bound is rigorous, not tight: the fp32 restatement uses a few thousandths of it (``test_ps.py`` prints the ratio).

Gate per profile bin - measured (``PROFILE_GAP``).  The restatement's worst relative gap |p^[r] - p[r]| / p[r] to float64
over the bins that hold signal (``significant``), over every case of the table below, times 16: the device's fused
multiply-adds and its order of operations differ from NumPy's.  Bins without signal (all but one bin of a single cosine)
are held to the mean of the per-coefficient bounds instead, which is rigorous for a mean."""
import functools
import math

import numpy as np

U32 = 2.0 ** -24
C_FFT = 7.0
SIDES = (16, 32, 64, 128, 256, 512)
NB_TABLE = {16: 12, 32: 24, 64: 46, 128: 92, 256: 182, 512: 363}
LUMA = (0.299, 0.587, 0.114)
FLOOR = 1e-30
SIGNIFICANT = 1e-6            # a bin holds signal when its mean power is at least this fraction of mean(Y^2) / S^2

# Measured by ``measure_profile_gap()`` (NumPy fp32 restatement against float64, all cases of STRUCTURE_CASES,
# CONTENT_CASES and the boundary case, significant bins only): 2.076e-05, at the DC-heavy bf16 input S = 64, n = 3, C = 3
# (white and 1/f inputs stay below 1.5e-06).  test_ps.py re-measures it and fails if it rose above the record or fell more
# than 25 % below it.
PROFILE_GAP = 2.1e-5
PROFILE_GATE = 16 * PROFILE_GAP

STRUCTURE_CASES = [(S, 2, 3) for S in SIDES]                                        # (S, n, C), fp32, white
CONTENT_CASES = [(S, n, C) for S in (16, 64) for n in (1, 3, 5) for C in (1, 3, 4)]   # x dtype x kind
KINDS = ("white", "pink", "dc")
DTYPES = ("fp32", "bf16")
BOUNDARY_SIDE = 64


# ---------------------------------------------------------------- bins
def n_bins(S):
    return (math.isqrt(2 * S * S) + 1) // 2 + 1


def bin_of(ky, kx):
    return (math.isqrt(4 * (ky * ky + kx * kx)) + 1) // 2


@functools.lru_cache(maxsize=None)
def full_bins(S, rule="round"):
    """int64 [S, S] in DFT order (row ky, column kx, both 0 .. S/2 - 1 then -S/2 .. -1)."""
    f = np.arange(S)
    f = np.where(f < S // 2, f, f - S)
    out = np.empty((S, S), dtype=np.int64)
    for i, ky in enumerate(f):
        for j, kx in enumerate(f):
            m = int(ky * ky + kx * kx)
            out[i, j] = bin_of(int(ky), int(kx)) if rule == "round" else math.isqrt(m)
    return out


def counts(S):
    return np.bincount(full_bins(S).reshape(-1), minlength=n_bins(S)).astype(np.int64)


# ---------------------------------------------------------------- the float64 reference
def luminance(x, weights=LUMA):
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] == 1:
        return x[..., 0]
    return weights[0] * x[..., 0] + weights[1] * x[..., 1] + weights[2] * x[..., 2]


def power_full(x):
    """x [n,S,S,C] -> P float64 [n,S,S] over the full plane, DFT order."""
    Y = luminance(x)
    S = Y.shape[1]
    F = np.fft.fft2(Y, axes=(1, 2))
    return (F.real ** 2 + F.imag ** 2) / float(S) ** 4


def profiles_from_full(P):
    n, S, _ = P.shape
    b, nb = full_bins(S).reshape(-1), n_bins(S)
    c = counts(S).astype(np.float64)
    return np.stack([np.bincount(b, weights=P[i].reshape(-1), minlength=nb) / c for i in range(n)])


def reference(x):
    """{"power": float64 [n,S,S/2+1] (the half plane the device keeps), "profiles": [n,NB], "Y": luminance, "F": fft2}."""
    Y = luminance(x)
    S = Y.shape[1]
    F = np.fft.fft2(Y, axes=(1, 2))
    P = (F.real ** 2 + F.imag ** 2) / float(S) ** 4
    return {"power": P[:, :, :S // 2 + 1], "profiles": profiles_from_full(P), "Y": Y, "F": F[:, :, :S // 2 + 1]}


def set_profile(profiles):
    return np.asarray(profiles, dtype=np.float64).mean(axis=0)


def log_profile(m):
    return np.log10(np.maximum(m, FLOOR))


def scores(m_real, m_fake, S):
    D = log_profile(m_fake) - log_profile(m_real)
    lo = S // 4
    at = lo + int(np.argmax(D[lo:]))
    return {"ps_dist": float(np.sqrt(np.mean(D[1:] ** 2))), "ps_hf": float(np.mean(D[lo:])), "ps_peak": float(D[at]),
            "ps_peak_at": at / float(S)}


def image_scores(real, fake):
    """Scores of two image sets [n,S,S,C] through the reference."""
    S = real.shape[1]
    return scores(set_profile(reference(real)["profiles"]), set_profile(reference(fake)["profiles"]), S)


# ---------------------------------------------------------------- the derived gate per coefficient
def power_bound(ref):
    """float64 [n,S,S/2+1]: the bound on |P^ - P| of the module docstring."""
    F, Y = ref["F"], ref["Y"]
    S = Y.shape[1]
    normF = S * np.sqrt((Y ** 2).sum(axis=(1, 2)))                       # ||F||_2 = S ||Y||_2
    delta = (C_FFT * U32 * math.log2(S * S) * normF + 3 * U32 * S * S)[:, None, None]
    a = np.abs(F)
    return ((2 * a * delta + delta ** 2) * (1 + 3 * U32) + 3 * U32 * a ** 2) / float(S) ** 4


def half_weights(S):
    w = np.full(S // 2 + 1, 2.0)
    w[0] = w[-1] = 1.0
    return w


def profile_bound(ref):
    """float64 [n,NB]: the mean of the coefficient bounds over every bin: a rigorous bound on |p^[r] - p[r]| (the fp64 sums
    add 2^-53 relative per term, which the (1 + 3u) factors of the coefficient bounds cover)."""
    bound = power_bound(ref)
    n, S, W = bound.shape
    b = full_bins(S)[:, :W].reshape(-1)
    w = np.tile(half_weights(S), S)
    c = counts(S).astype(np.float64)
    return np.stack([np.bincount(b, weights=w * bound[i].reshape(-1), minlength=n_bins(S)) / c for i in range(n)])


def significant(ref):
    """bool [n,NB]: bins whose mean power is at least SIGNIFICANT x the mean power per coefficient, mean(Y^2) / S^2."""
    Y = ref["Y"]
    S = Y.shape[1]
    level = SIGNIFICANT * (Y ** 2).mean(axis=(1, 2)) / float(S * S)
    return ref["profiles"] >= level[:, None]


def check_power(got, ref):
    """Worst |P^ - P| / bound over all coefficients (<= 1 passes)."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref["power"]) / power_bound(ref)).max())


def check_profiles(got, ref):
    """(worst relative gap over the significant bins, worst |gap| / bound over all bins)."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref["profiles"].shape:
        return float("inf"), float("inf")
    gap = np.abs(got - ref["profiles"])
    sig = significant(ref)
    rel = float((gap[sig] / ref["profiles"][sig]).max()) if sig.any() else 0.0
    return rel, float((gap / profile_bound(ref)).max())


def passes(got_power, got_profiles, ref):
    """Do a power array and its profiles pass every gate against ``ref``?"""
    rel, frac = check_profiles(got_profiles, ref)
    return check_power(got_power, ref) <= 1.0 and rel <= PROFILE_GATE and frac <= 1.0


# ---------------------------------------------------------------- the kernel's algorithm in NumPy fp32
def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def _twiddles(S, sign=-1.0):
    k = np.arange(S, dtype=np.float64)
    return (np.cos(2 * np.pi * k / S) + 1j * sign * np.sin(2 * np.pi * k / S)).astype(np.complex64)


def _stockham(x, tw):
    """x complex64 [M, S] -> its DFT along the last axis by the kernel's passes: radix-4 (n, s) = (S, 1), (S/4, 4), ... and
    a last radix-2 pass for odd log2 S; w^p of a sub-transform of n points is tw[p s]."""
    M, S = x.shape
    n, s = S, 1
    j = np.complex64(1j)
    while n >= 4:
        n1 = n // 4
        X = x.reshape(M, 4, n1, s)
        a, b, c, d = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
        apc, amc, bpd, jbmd = a + c, a - c, b + d, j * (b - d)
        p = np.arange(n1) * s
        w1, w2, w3 = tw[p][None, :, None], tw[2 * p][None, :, None], tw[3 * p][None, :, None]
        x = np.stack([apc + bpd, w1 * (amc - jbmd), w2 * (apc - bpd), w3 * (amc + jbmd)], axis=2).reshape(M, S)
        n, s = n1, 4 * s
    if n == 2:
        X = x.reshape(M, 2, s)
        x = np.stack([X[:, 0] + X[:, 1], X[:, 0] - X[:, 1]], axis=1).reshape(M, S)
    return x.astype(np.complex64)


MUTATIONS = ("mirror_weight", "floor_bins", "bins_to_half", "twiddle_sign", "swap_rb", "s_squared")


def emulate(x, mutation=None):
    """x [n,S,S,C] fp32 values -> (power fp32 [n,S,S/2+1], profiles float64 [n,NB]) by the device's route in fp32: fp32
    luminance, two real rows per complex transform, Stockham passes with twiddles rounded once from fp64, the split, the
    column transforms, (re^2 + im^2) / S^4, then the half-plane sums in float64.  ``mutation``: one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS
    f = np.float32
    x = np.asarray(x, dtype=np.float32)
    n, S, _, C = x.shape
    W = S // 2 + 1
    if C == 1:
        Y = x[..., 0]
    else:
        wr, wg, wb = (f(LUMA[2]), f(LUMA[1]), f(LUMA[0])) if mutation == "swap_rb" else (f(LUMA[0]), f(LUMA[1]), f(LUMA[2]))
        Y = wb * x[..., 2] + (wg * x[..., 1] + wr * x[..., 0])
    tw = _twiddles(S, +1.0 if mutation == "twiddle_sign" else -1.0)
    z = (Y[:, 0::2, :] + np.complex64(1j) * Y[:, 1::2, :]).astype(np.complex64).reshape(n * S // 2, S)
    Z = _stockham(z, tw)
    Zm = np.conj(Z[:, (-np.arange(W)) % S])
    Zk = Z[:, :W]
    A = f(0.5) * (Zk + Zm)
    D = Zk - Zm
    B = (f(0.5) * D.imag + np.complex64(1j) * (f(-0.5) * D.real)).astype(np.complex64)
    spec = np.stack([A.reshape(n, S // 2, W), B.reshape(n, S // 2, W)], axis=2).reshape(n, S, W)
    cols = _stockham(np.ascontiguousarray(spec.transpose(0, 2, 1)).reshape(n * W, S), tw).reshape(n, W, S).transpose(0, 2, 1)
    scale = f(1.0) / (f(S) ** (2 if mutation == "s_squared" else 4))
    power = ((cols.real * cols.real + cols.imag * cols.imag) * scale).astype(np.float32)
    # the half-plane profile
    rule = "floor" if mutation == "floor_bins" else "round"
    b = full_bins(S, rule)[:, :W].reshape(-1)
    w = np.ones(W) if mutation == "mirror_weight" else half_weights(S)
    wt = np.tile(w, S)
    nb = n_bins(S)
    cnt = np.bincount(b, weights=wt, minlength=nb)
    prof = np.stack([np.bincount(b, weights=wt * power[i].reshape(-1).astype(np.float64), minlength=nb)[:nb] /
                     np.maximum(cnt[:nb], 1) for i in range(n)])
    if mutation == "bins_to_half":
        prof = prof[:, :S // 2 + 1]
    return power, prof


# ---------------------------------------------------------------- inputs
def make_images(S, n, C, kind, seed=0):
    """float32 [n,S,S,C] in [-1, 1]: ``white`` uniform noise, ``pink`` 1/f noise (every channel on its own, scaled to a
    peak of 0.95), ``dc`` 0.9 + 0.05 x white: the DC-heavy case."""
    rng = np.random.RandomState(1000 * S + 100 * n + 10 * C + KINDS.index(kind) + 7 * seed)
    white = rng.uniform(-1.0, 1.0, size=(n, S, S, C))
    if kind == "white":
        x = white
    elif kind == "dc":
        x = 0.9 + 0.05 * white
    else:
        f = np.fft.fftfreq(S) * S
        r = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
        r[0, 0] = 1.0
        x = np.fft.ifft2(np.fft.fft2(white, axes=(1, 2)) / r[None, :, :, None], axes=(1, 2)).real
        x = 0.95 * x / np.abs(x).max(axis=(1, 2), keepdims=True)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(S, n, C, kind="white", dtype="fp32"):
    """{"x": fp32 values (bf16-exact for dtype bf16), "ref": reference(x)}: computed once and shared; do not modify."""
    x = make_images(S, n, C, kind)
    if dtype == "bf16":
        x = bf16_round(x)
    x.setflags(write=False)
    return {"x": x, "ref": reference(x)}


@functools.lru_cache(maxsize=None)
def boundary_frequencies(S=BOUNDARY_SIDE, each=4):
    """The (ky, kx), 0 < kx < S/2, 0 < |ky| < S/2, whose sqrt(ky^2 + kx^2) lies nearest a half-integer: ``each`` from below
    (they round down) and ``each`` from above (they round up), found by search; one per distinct radius."""
    below, above, seen = [], [], set()
    for ky in range(-S // 2 + 1, S // 2):
        for kx in range(1, S // 2):
            m = ky * ky + kx * kx
            if ky == 0 or m in seen:
                continue
            seen.add(m)
            rho = math.sqrt(m)
            frac = rho - math.floor(rho)
            (below if frac < 0.5 else above).append((abs(frac - 0.5), ky, kx))
    picks = sorted(below)[:each] + sorted(above)[:each]
    return tuple((ky, kx) for _, ky, kx in picks)


def cosine_images(S, freqs, dtype=np.float32):
    """[len(freqs),S,S,1]: image i is cos(2 pi (ky y + kx x) / S)."""
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    return np.stack([np.cos(2 * np.pi * (ky * y + kx * x) / S) for ky, kx in freqs])[..., None].astype(dtype)


@functools.lru_cache(maxsize=None)
def boundary_case():
    x = cosine_images(BOUNDARY_SIDE, boundary_frequencies())
    x.setflags(write=False)
    return {"x": x, "ref": reference(x), "freqs": boundary_frequencies()}


def all_cases():
    """Every case the GPU tests run, as (label, case)."""
    for S, n, C in STRUCTURE_CASES:
        yield "structure S=%d" % S, case(S, n, C)
    for S, n, C in CONTENT_CASES:
        for dtype in DTYPES:
            for kind in KINDS:
                yield "content S=%d n=%d C=%d %s %s" % (S, n, C, dtype, kind), case(S, n, C, kind, dtype)
    yield "boundary", boundary_case()


def measure_profile_gap():
    """(worst relative gap of the restatement's profiles over the significant bins, its label, worst |P^ - P| / bound,
    worst profile |gap| / bound) over all cases."""
    worst, where, worst_power, worst_frac = 0.0, None, 0.0, 0.0
    for label, k in all_cases():
        power, prof = emulate(k["x"])
        rel, frac = check_profiles(prof, k["ref"])
        if rel > worst:
            worst, where = rel, label
        worst_power = max(worst_power, check_power(power, k["ref"]))
        worst_frac = max(worst_frac, frac)
    return worst, where, worst_power, worst_frac
