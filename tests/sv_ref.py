"""The singular-value monitor (csrc/spectrum.hip) written once in NumPy and evaluated twice: in float64 as the reference
and in fp32 as a stand-in for the kernels (the dot products of pass A in the kernel's own order, Q and Y stored in fp32,
everything that the kernels do in fp64 done in float64).  Truth is LAPACK (``torch.linalg.svdvals`` in float64 on the CPU)
of the fp32-rounded matrix.  Nothing here is fitted to a device: every bound below is a count of rounding points.

The algorithm.  W is [rows, cols], Q is [cols, 8] with orthonormal columns, b = min(8, rows, cols); columns >= b are zero.
  one iteration     Y = W Q   (fp32 dot products of length cols, stored in fp32)
                    Z = W^T Y (fp64 products and sums: exact for the purposes below)
                    Q = orth(Z): classical Gram-Schmidt with one re-orthogonalisation in fp64, a column whose remaining
                    squared norm is <= 2^-80 of its squared norm becomes zero; stored in fp32
  Ritz step         Y = W Q; H = Y^T Y; H = V diag(lambda) V^T, descending; sv = sqrt(max(lambda, 0));
                    Q <- Q V (stored in fp32), Y <- Y V; Z = W^T Y; resid_i = ||Z_i - lambda_i Q_i|| / lambda_0

Rounding points, u = 2^-24.
  * A dot product of pass A.  A lane of the kernel adds ``steps`` products one after the other (4 per trip of 256 columns
    when cols % 4 == 0, otherwise 1 per trip of 64 columns), then the 64 lanes are added by a butterfly of depth 6.  The
    stand-in rounds the product and the sum (2 per step), the kernel uses fused multiply-adds (1 per step); with the
    larger count every result passes through at most d = 2 steps + 6 roundings, so
        |dy_ri| <= g sum_c |w_rc| |q_ci| <= g ||w_r|| ||q_i||,   g = d u / (1 - d u),
    and ||dY||_2 <= ||dY||_F <= sqrt(8) g ||W||_F (1 + 8 u) =: EY.
  * Q in fp32: every entry has relative error u, so (Q^T Q - I)_ij is at most (2 u + u^2) in magnitude after pass C (Cauchy-
    Schwarz on the exact orthonormal columns) and ||Q^T Q - I||_2 <= 8 (2 u + u^2); the singular values of Q lie in 1 +- 8.1 u.
  * fp64 sums (pass B, Gram-Schmidt, H, Jacobi, the rotation, the residual) are 2^29 times finer and count as exact; 1e-13
    is added where a bound would otherwise be compared with an fp64 rounding.

(b) orthonormality.  After pass C the defect max |Q^T Q - I| over the nonzero columns is <= 2 u + u^2.  The Ritz step
    rotates by an orthogonal V (|V^T E V|_ij <= ||E||_2 <= 8 (2 u + u^2)) and rounds again (2 u + u^2):
        DEFECT = 9 (2 u + u^2) + 1e-13.
(c) the fp32 floor of resid.  With B the basis before the rotation, the reported residual vector is
        Z_i - l_i q_i = [W^T W B V_i - l_i B V_i] + W^T dY V_i - l_i dq_i.
    The bracket is the residual in exact arithmetic of the pair that H yields; H differs from the exact B^T W^T W B by
    dH = Y^T dY + dY^T Y + dY^T dY, which moves the bracket by at most ||dH|| (1 + 8.1 u) <= 2.01 s0 EY; the second term is
    at most s0 EY, the third at most l_0 u (1 + 8.1 u); a basis that is off orthonormal by 8 (2 u + u^2) adds at most
    17 u l_0.  Divided by l_0 = s0^2:
        FLOOR = 3.01 EY / s0 + 18.1 u.
    A reported residual therefore differs from the residual of (sv_i^2, q_i / ||q_i||) in exact arithmetic by at most FLOOR.
(a) the Ritz values.  The singular values of Y + dY differ from those of W B by at most EY, and those from the Ritz values
    of the orthonormalised basis by a factor 1 +- 8.1 u, so with sv in units of s0
        |sv_i^2 - ritz_i^2| <= LOCAL l_0,   LOCAL = 2.01 (EY / s0 + 8.1 u).
    This part is pure rounding.  Two runs from the same start (device and float64) also stand on slightly different
    subspaces: each pass rounds Y and Q again.  For that part the theorem is used, not a rounding count: for symmetric
    A = W^T W and a unit q some eigenvalue of A lies within ||A q - l q|| of l.  A run whose residual is r_i therefore has
    sv_i^2 within (r_i + FLOOR + LOCAL) l_0 of a true sigma^2, and two runs that are both near the same sigma^2 (the
    cases keep the first values apart by more than the caps) differ by at most the sum:
        GAP_i = (CAP_i + r64_i + FLOOR + 2 LOCAL) l_0.
(d) the reported residual against the pair's own.  For q~_i = B V_i + dq_i the residual vector in exact arithmetic is
    [bracket] + W^T W dq_i - l_i dq_i, the reported one [bracket] + W^T dY V_i - l_i dq_i: they differ by at most
    s0 EY + l_0 u (1 + 8.1 u), and taking q~_i / ||q~_i|| instead of q~_i (norm 1 +- 9.1 u, residual at most 2.01 l_0) adds
    18.3 u l_0:
        RESID_ERR = EY / s0 + 19.4 u.
    The gate evaluates the residual of every returned pair in float64 on the host and holds the reported one to it: this
    is what keeps the theorem honest for the values that have not converged, whose residuals are far above the floor.
The cap.  A loose residual would make the theorem vacuous, so every case is chosen such that the float64 run's residual
    of the first K = 4 values is at least 100 times below FLOOR, and the device's residual must stay below CAP_i.  What
    the fp32 run adds to the float64 run's residual: the floor itself, and the tilt of q_i that the last pass's rounding
    leaves (earlier tilts are damped by the iteration): dZ_i = W^T dY_i has norm <= s0 EY against ||Z_i|| ~ l_i, a tilt
    of EY s0 / l_i, which a unit vector turns into a residual of at most (tilt) max|mu - l_i| / l_0 <= tilt; the rounding
    of Q adds u.  So
        CAP_i = min(2.01, FLOOR + r64_i + (EY / s0) (l_0 / l_i) + u),
    the multiple of the floor being 1 + (l_0 / l_i) / 3 (1.3 for the largest value, 22 for sigma_3 = sigma_0 / 8); 2.01 is
    what ||A q - l q|| / l_0 can be at all for a unit q and 0 <= l <= l_0, with the slack of the fp32 basis.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
BLOCK = 8
K = 4                       # values that the cap and the gap are asked of (--sv_k is at most 4)
EPS64 = 1e-13


# ---------------------------------------------------------------- inputs and truth
def make_matrix(rows, cols, spectrum, seed):
    """U diag(s) V^T with U, V from a QR of seeded Gaussians in float64, rounded to fp32."""
    rng = np.random.RandomState(seed)
    s = np.asarray(spectrum, dtype=np.float64)
    k = len(s)
    assert k <= min(rows, cols)
    u, _ = np.linalg.qr(rng.standard_normal((rows, k)))
    v, _ = np.linalg.qr(rng.standard_normal((cols, k)))
    return ((u * s) @ v.T).astype(np.float32)


def make_basis(cols, seed, rows=None):
    """A start basis [cols, 8] fp32 with orthonormal columns (zero beyond b = min(8, rows, cols))."""
    rng = np.random.RandomState(seed)
    b = min(BLOCK, cols, cols if rows is None else rows)
    q = np.zeros((cols, BLOCK), dtype=np.float64)
    q[:, :b], _ = np.linalg.qr(rng.standard_normal((cols, b)))
    return q.astype(np.float32)


def truth(w):
    """LAPACK singular values of the fp32 matrix in float64, descending."""
    return torch.linalg.svdvals(torch.from_numpy(np.asarray(w, dtype=np.float64))).numpy()


def true_basis(w):
    """The top-8 right singular vectors of the fp32 matrix as a basis [cols, 8] fp32 (zero beyond b)."""
    w64 = np.asarray(w, dtype=np.float64)
    _, _, vt = np.linalg.svd(w64, full_matrices=False)
    b = min(BLOCK, *w64.shape)
    q = np.zeros((w64.shape[1], BLOCK))
    q[:, :b] = vt[:b].T
    return q.astype(np.float32)


def pow2(n):
    return [2.0 ** -i for i in range(n)]


def pow15(n):
    return [1.5 ** -i for i in range(n)]


# (name, rows, cols, spectrum, iterations): the shape cases of tests/test_gpu_sv.py
CASES = [
    ("rank1_8x8", 8, 8, [1.0], 3),
    ("3x1", 3, 1, pow2(1), 3),
    ("2x7", 2, 7, pow2(2), 3),
    ("27x3", 27, 3, pow2(3), 3),
    ("37x5", 37, 5, pow2(5), 3),
    ("64x256", 64, 256, pow2(64), 3),
    ("65x257", 65, 257, pow15(65), 6),
    ("16x1024", 16, 1024, pow2(16), 3),
    ("1030x24", 1030, 24, pow2(24), 3),
    ("equal_40x12", 40, 12, [1.0, 1.0] + pow2(12)[2:], 3),
]
# the further case (every grid-stride loop takes a second trip) is 65600 x 2052: the device test builds it there
_cache = {}


def case(name):
    """The case's matrix, start basis, truth and both host runs, computed once."""
    if name not in _cache:
        i = [c[0] for c in CASES].index(name)
        _, rows, cols, spec, iters = CASES[i]
        w = make_matrix(rows, cols, spec, 100 + i)
        q0 = make_basis(cols, 200 + i, rows)
        k = dict(name=name, w=w, q0=q0, iters=iters, truth=truth(w), rows=rows, cols=cols)
        k["ref"] = run(w, q0, iters, np.float64)
        k["sim"] = run(w, q0, iters, np.float32)
        k["bounds"] = bounds(w, k["truth"], k["ref"]["resid"])
        for v in (w, q0, k["truth"]):
            v.setflags(write=False)
        _cache[name] = k
    return _cache[name]


# ---------------------------------------------------------------- the algorithm
def steps_of(cols):
    """Products that one lane of pass A adds one after the other."""
    return 4 * ((cols + 255) // 256) if cols % 4 == 0 else (cols + 63) // 64


def dot_kernel_order(w, q):
    """W Q in fp32 in the order of pass A: 64 lanes, each a running sum over its columns, then a butterfly over the lanes."""
    rows, cols = w.shape
    f = np.float32
    if cols % 4 == 0:
        trips = (cols + 255) // 256
        wp = np.zeros((rows, trips * 256), dtype=f)
        qp = np.zeros((trips * 256, BLOCK), dtype=f)
        wp[:, :cols], qp[:cols] = w, q
        wp, qp = wp.reshape(rows, trips, 64, 4), qp.reshape(trips, 64, 4, BLOCK)
        acc = np.zeros((rows, 64, BLOCK), dtype=f)
        for t in range(trips):
            for e in range(4):
                acc = acc + wp[:, t, :, e, None] * qp[None, t, :, e, :]
    else:
        trips = (cols + 63) // 64
        wp = np.zeros((rows, trips * 64), dtype=f)
        qp = np.zeros((trips * 64, BLOCK), dtype=f)
        wp[:, :cols], qp[:cols] = w, q
        wp, qp = wp.reshape(rows, trips, 64), qp.reshape(trips, 64, BLOCK)
        acc = np.zeros((rows, 64, BLOCK), dtype=f)
        for t in range(trips):
            acc = acc + wp[:, t, :, None] * qp[None, t]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o, :]
    return acc[:, 0, :]


def orth(z, b):
    """Pass C in float64: (Q, squared norms that remained).  Columns >= b, zero, non-finite or dependent columns -> 0."""
    z = np.array(z, dtype=np.float64)
    rn = np.zeros(BLOCK)
    for j in range(BLOCK):
        orig = float(z[:, j] @ z[:, j])
        keep = j < b and orig > 0.0 and np.isfinite(orig)
        rem = orig
        if keep and j > 0:
            for _ in range(2):
                for_k = [k for k in range(j) if rn[k] > 0.0]
                coef = np.array([(z[:, k] @ z[:, j]) / rn[k] for k in for_k])
                if for_k:
                    z[:, j] = z[:, j] - z[:, for_k] @ coef
            rem = float(z[:, j] @ z[:, j])
            keep = rem > np.ldexp(orig, -80) and np.isfinite(rem)
        if not keep:
            rem = 0.0
            z[:, j] = 0.0
        rn[j] = rem
    scale = np.where(rn > 0.0, 1.0 / np.sqrt(np.where(rn > 0.0, rn, 1.0)), 0.0)
    return z * scale, rn


MUTATIONS = ("q_transposed", "no_orth", "column_norms", "drop_last_rows", "resid_by_lambda_i")


def run(w, q0, iters, dtype=np.float64, mutate=None):
    """``iters`` iterations and the Ritz step from the basis ``q0``.  dtype float64: the reference; float32: the stand-in
    for the kernels.  ``mutate``: one of MUTATIONS, a fault that the gates must catch.  Returns sv, resid [8] float64, the
    basis q [cols, 8] float64 (holding dtype values) and lam."""
    assert mutate is None or mutate in MUTATIONS
    w = np.asarray(w, dtype=np.float32)
    rows, cols = w.shape
    b = min(BLOCK, rows, cols)
    w64 = w.astype(np.float64)
    q = np.array(q0, dtype=dtype)
    q[:, b:] = 0

    def project(q):
        if mutate == "q_transposed":
            q = np.ascontiguousarray(q).reshape(BLOCK, cols).T
        if dtype == np.float64:
            return w64 @ np.asarray(q, dtype=np.float64)
        return dot_kernel_order(w, np.asarray(q, dtype=np.float32)).astype(np.float64)

    def backproject(y):
        if mutate == "drop_last_rows" and rows % 256:
            n = rows // 256 * 256
            return w64[:n].T @ y[:n]
        return w64.T @ y

    for _ in range(iters):
        z = backproject(project(q))
        if mutate == "no_orth":
            qn = z.copy()
            qn[:, b:] = 0
        else:
            qn, _ = orth(z, b)
        q = qn.astype(dtype)
    y = project(q)
    h = y.T @ y
    lam = np.zeros(BLOCK)
    v = np.eye(BLOCK)
    if mutate == "column_norms":
        lam[:b] = np.diag(h)[:b]
    else:
        e, vec = np.linalg.eigh(h[:b, :b])
        order = np.argsort(-e, kind="stable")
        lam[:b], v[:b, :b] = e[order], vec[:, order]
    lam = np.where((lam > 0.0) & np.isfinite(lam), lam, 0.0)
    q = (q.astype(np.float64) @ v).astype(dtype)
    z = backproject(y @ v)
    d = z - q.astype(np.float64) * lam
    norm = np.sqrt((d * d).sum(axis=0))
    resid = np.zeros(BLOCK)
    if lam[0] > 0.0:
        den = np.where(lam > 0.0, lam, np.inf) if mutate == "resid_by_lambda_i" else lam[0]
        resid[:b] = (norm / den)[:b]
    return dict(sv=np.sqrt(lam), resid=resid, q=q.astype(np.float64), lam=lam)


# ---------------------------------------------------------------- the bounds (module docstring)
def bounds(w, sigma, resid64=None):
    """FLOOR, LOCAL, DEFECT and, per index, CAP and GAP (relative to l_0 = sigma_0^2) for the matrix ``w`` with LAPACK
    singular values ``sigma``; ``resid64``: the float64 run's residuals (None: 0)."""
    w64 = np.asarray(w, dtype=np.float64)
    rows, cols = w64.shape
    s0 = float(sigma[0])
    fro = float(np.sqrt((w64 * w64).sum()))
    d = 2 * steps_of(cols) + 6
    g = d * U32 / (1.0 - d * U32)
    ey = np.sqrt(8.0) * g * (fro / s0) * (1 + 8 * U32) if s0 > 0 else 0.0       # EY / s0
    floor = 3.01 * ey + 18.1 * U32
    local = 2.01 * (ey + 8.1 * U32)
    defect = 9 * (2 * U32 + U32 * U32) + EPS64
    r64 = np.zeros(BLOCK) if resid64 is None else np.asarray(resid64, dtype=np.float64)
    lam = np.zeros(BLOCK)
    n = min(BLOCK, len(sigma))
    lam[:n] = np.asarray(sigma[:n], dtype=np.float64) ** 2
    ratio = np.where(lam > 0.0, (s0 * s0) / np.where(lam > 0.0, lam, 1.0), np.inf)
    cap = np.minimum(2.01, floor + r64 + ey * ratio + U32)
    gap = cap + r64 + floor + 2 * local
    return dict(floor=floor, local=local, defect=defect, cap=cap, gap=gap, s0=s0, d=d, resid_err=ey + 19.4 * U32)


def pair_resid(apply_a, q, sv):
    """|| A q_i / ||q_i|| - sv_i^2 q_i / ||q_i|| || / sv_0^2 per column in float64 (0 for zero columns or sv_0 = 0);
    ``apply_a``: x [cols, 8] float64 -> W^T W x."""
    q = np.asarray(q, dtype=np.float64)
    sv = np.asarray(sv, dtype=np.float64)
    nrm = np.sqrt((q * q).sum(axis=0))
    qn = q / np.where(nrm > 0, nrm, 1.0)
    d = apply_a(qn) - qn * sv ** 2
    r = np.sqrt((d * d).sum(axis=0))
    return np.where(nrm > 0, r, 0.0) / sv[0] ** 2 if sv[0] > 0 else np.zeros(BLOCK)


def apply_gram(w):
    w64 = np.asarray(w, dtype=np.float64)
    return lambda x: w64.T @ (w64 @ x)


def theorem_miss(sv, resid, sigma, extra):
    """Per index: distance of sv_i^2 from the nearest true sigma^2, minus what the theorem allows, (resid_i + extra) sv_0^2.
    <= 0 is a pass.  ``sigma`` is padded with the zeros that a rank below 8 implies."""
    sv, resid = np.asarray(sv, dtype=np.float64), np.asarray(resid, dtype=np.float64)
    s2 = np.concatenate([np.asarray(sigma, dtype=np.float64) ** 2, [0.0]])
    dist = np.abs(sv[:, None] ** 2 - s2[None, :]).min(axis=1)
    return dist - (resid + extra) * sv[0] ** 2


def defect_of(q):
    """max |Q^T Q - I| over the nonzero columns of q, and whether the other columns are exactly zero."""
    q = np.asarray(q, dtype=np.float64)
    nz = np.abs(q).max(axis=0) > 0
    g = q[:, nz].T @ q[:, nz]
    return (float(np.abs(g - np.eye(int(nz.sum()))).max()) if nz.any() else 0.0), nz


def gate(k, out):
    """The checks that tests/test_gpu_sv.py applies to a run ``out`` (sv, resid, q) of case ``k``: a list of the failures
    (empty: the run passes).  Used on the device's outputs and, in tests/test_sv.py, on the stand-in and its mutants."""
    bd, ref = k["bounds"], k["ref"]
    b = min(BLOCK, k["rows"], k["cols"])
    kk = min(K, b)
    fails = []
    sv, resid = np.asarray(out["sv"], dtype=np.float64), np.asarray(out["resid"], dtype=np.float64)
    if not (np.isfinite(sv).all() and np.isfinite(resid).all() and np.isfinite(out["q"]).all()):
        return ["not finite"]
    if (sv[b:] != 0).any() or (resid[b:] != 0).any() or (np.asarray(out["q"])[:, b:] != 0).any():
        fails.append("outputs beyond b_eff are not zero")
    if (np.diff(sv[:b]) > 0).any():
        fails.append("sv not descending")
    l0 = bd["s0"] ** 2
    gap = np.abs(sv ** 2 - ref["sv"] ** 2)[:kk]
    if (gap > bd["gap"][:kk] * l0).any():
        fails.append("sv off the float64 run: %s > %s" % (gap / l0, bd["gap"][:kk]))
    miss = theorem_miss(sv, resid, k["truth"], bd["floor"] + bd["local"])[:b]
    if (miss > 0).any():
        fails.append("theorem missed by %s" % (miss / l0))
    if (resid[:kk] > bd["cap"][:kk]).any():
        fails.append("resid %s above the cap %s" % (resid[:kk], bd["cap"][:kk]))
    own = pair_resid(k.get("apply_a") or apply_gram(k["w"]), out["q"], sv)
    if (np.abs(resid - own)[:b] > bd["resid_err"]).any():
        fails.append("resid %s is not the pair's own %s" % (resid[:b], own[:b]))
    dfc, nz = defect_of(out["q"])
    if dfc > bd["defect"]:
        fails.append("defect %.3g > %.3g" % (dfc, bd["defect"]))
    return fails
