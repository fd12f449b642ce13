"""float64 references, error bounds and the case table of the kernels that run once per weight per step: spectral norm
(single and multi-tensor form, packed bf16 copies), the orthogonal regularisers (Gram-side kernels and the low-rank form)
and the TF-Adam + EMA update.

Test helper, not product code.  The pattern of tests/elementwise_ref.py:

* references - plain float64 restatements of the header comments of ``include/biggan_hip.h`` and of the formula comments
  above the kernels (csrc/elementwise.hip, csrc/augment_loss.hip), device-agnostic, written in the kernels' order of
  operations; ``tests/test_weight_gate.py`` checks them against float64 autograd through ``oracle/ref_ops.py``.
* bounds - never anything a kernel returned:
    - a reduction of length K: ``launch_replay.bound(A, K)`` with A the same sum over absolute values, plus ``U32 |term|``
      for every fp32 rounding inside a term;
    - elementwise formulas (spectral-norm backward, low-rank finish, 'ortho' dA, Adam): a named count of roundings times
      ``U32`` times the absolute-value form;
    - chains of reductions (l2-normalisations, the cosine regulariser's rows, the low-rank columns) carry (value, error)
      pairs through the formula to first order (class ``Fe``): every product / sum / quotient adds its own rounding, every
      reduction its ``bound``, and the error of an operand is propagated with the partial derivative's absolute value;
    - the spectral-norm chain is gated stage by stage, each stage against the float64 function of the call's OWN earlier
      outputs, so that each bound covers one reduction: v from the inputs, u from the returned v, sigma from the returned
      u and v, w_norm and the packed copies from the returned sigma (one division);
    - the device's ``rsqrtf``, ``sqrtf``, ``/`` and ``1.f / x`` take a measured allowance (RSQRT_U .. RCP_U below).
  Acceptance is ``launch_replay.gate``.
* CASES - the table both test modules walk: the smallest shapes that enter each dispatch branch.
"""
import math

import torch

from tests import launch_replay as R

U32 = R.U32
D64 = torch.float64
F32 = torch.float32
EPS = 1e-12                  # the clamp of l2_normalize
AMBIGUITY_CAP = 1e-4         # share of outputs a case may leave out (none of the cases below leaves any out)
POISON = 1.0e30              # finite poison: the first moment a beta1 == 0 update must not read
ERR_ARG = 1

# Device math allowances, in units of U32 = 2^-24 relative error.  The ROCm installation documents no accuracy table, so
# they were measured on an MI355X against float64 (2^24 arguments 2^e (1 + m), e in [-46, 30], the library's compile
# flags) and doubled, because the sample is finite:
RSQRT_U = 3.2                # rsqrtf: measured 1.5767
SQRT_U = 2.0                 # sqrtf:  measured 1.0000 (correctly rounded)
DIV_U = 2.0                  # a / b:  measured 0.9999 (correctly rounded)
RCP_U = 2.0                  # 1.f / x: measured 1.0000 (correctly rounded)

# Named rounding counts (fp32 roundings on the longest path of one output element)
SN_SS_M = 10        # sum v_^2 in the finalize block: per-thread partial cast to fp32 (1), 8 levels of block_sum_256, 1 spare
SN_V_M = SN_SS_M / 2 + RSQRT_U + 2      # rs_v = rsqrtf(ss) (half of ss's relative error + rsqrtf), v_ * rs_v (1), 1e-12f (1)
SN_T_M = 2          # t = (float) u_raw * rs_v: the cast from the fp64 accumulator (1), the product (1)
SN_BWD_M = 5 + RCP_U            # d v (1), * u (2), g - . (3), * inv_sigma (4), inv_sigma = 1.f / sigma (RCP_U); + 1
SN_DIV_M = DIV_U                # w / sigma: one division
LRF_M = 5           # 2 dW exact; s a (1), + (2), + W alpha (3), 2 P exact, * b (1), + (4); + 1 second-order
ID_DA_M = 2         # r = A - I (1), scale r (2)
ADAM_G_M = 1        # gi = g gscale
ADAM_M_M = 4        # gi (1), (1 - b1) gi (2), the sum (3); + 1 second-order   [b1 m: (1) on its own term]
ADAM_V_M = 6        # gi twice (2), (1 - b2) gi (3), * gi (4), the sum (5); + 1 second-order
ADAM_UPD_M = 2 + DIV_U          # lr m (1), the quotient (DIV_U); + 1 second-order
ADAM_EMA_M = 3      # decay ema | (1 - decay) p (1), the sum (2); + 1 second-order


def f32r(x):
    """A Python float as the fp32 value a c_float argument carries."""
    return float(torch.tensor(x, dtype=F32))


# ------------------------------------------------------------------------------------------
# (value, first-order error) pairs
# ------------------------------------------------------------------------------------------
class Fe:
    """float64 value v with an absolute error bound e of its fp32 counterpart."""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def lift(x, like):
        if isinstance(x, Fe):
            return x
        if not torch.is_tensor(x):
            x = torch.tensor(float(x), dtype=D64, device=like.v.device)
        return Fe(x)

    def __mul__(self, o):
        o = Fe.lift(o, self)
        r = self.v * o.v
        return Fe(r, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + U32 * r.abs())

    def exact(self, k):
        """Times a power of two (or a sign): no rounding."""
        return Fe(self.v * k, self.e * abs(k))

    def _addsub(self, o, sign):
        o = Fe.lift(o, self)
        return Fe(self.v + sign * o.v, self.e + o.e + U32 * (self.v.abs() + o.v.abs()))

    def __add__(self, o):
        return self._addsub(o, 1.0)

    def __sub__(self, o):
        return self._addsub(o, -1.0)

    def __truediv__(self, o):
        o = Fe.lift(o, self)
        r = self.v / o.v
        return Fe(r, (self.e + r.abs() * o.e) / o.v.abs() + DIV_U * U32 * r.abs())

    def sum(self, dim, K, keepdim=False):
        """An fp32 reduction over K terms in any order and association."""
        return Fe(self.v.sum(dim, keepdim=keepdim),
                  R.bound(self.v.abs().sum(dim, keepdim=keepdim), K) + self.e.sum(dim, keepdim=keepdim))

    def where(self, cond, o):
        o = Fe.lift(o, self)
        return Fe(torch.where(cond, self.v, o.v), torch.where(cond, self.e, o.e))


def fe_rsqrt_clamped(ss):
    """rsqrtf(fmaxf(ss, 1e-12f)) of a non-negative Fe -> (Fe, clamped mask, ambiguous mask)."""
    clamped = ss.v < EPS
    amb = (ss.v - EPS).abs() <= ss.e + U32 * EPS
    arg = torch.clamp(ss.v, min=EPS)
    r = arg.rsqrt()
    e_arg = torch.where(clamped, torch.full_like(arg, U32 * EPS), ss.e)        # 1e-12f is not 1e-12
    return Fe(r, 0.5 * r * e_arg / arg + RSQRT_U * U32 * r), clamped, amb


# ------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------
def l2n(t):
    """tf.nn.l2_normalize over the whole tensor: t rsqrt(max(sum t^2, 1e-12))."""
    return t * torch.clamp((t * t).sum(), min=EPS).rsqrt()


def l2n_bound(raw, E_raw, m):
    """l2n of a raw vector known to E_raw, to first order: d v^ <= rs E_raw + |v^| rs ||E_raw||_2 (the projection term,
    absent when the clamp is taken: rs is then a constant) + m roundings.  -> (ref, E, ambiguous clamp)."""
    ss = (raw * raw).sum()
    rs = torch.clamp(ss, min=EPS).rsqrt()
    ref = raw * rs
    proj = 0.0 if float(ss) < EPS else rs * E_raw.norm()
    amb = abs(float(ss) - EPS) <= 2.0 * float(raw.norm() * E_raw.norm()) + 1e-3 * EPS
    return ref, rs * E_raw + ref.abs() * (proj + m * U32), amb


def sn_u_m(cols):
    """Roundings of u_out beyond t: ss = sum t^2 - the square (1), ceil(cols / 256) serial adds per thread, 8 levels of
    block_sum_256, halved by the square root - rsqrtf, the product t rs_u (1), 1e-12f and second order (1)."""
    return (1 + (cols + 255) // 256 + 8) / 2 + RSQRT_U + 2


def sn_sigma_m(cols):
    """sigma = ss rs_u against sum_c raw_c u_c = rs_u sum_c raw_c t_c: ss as above without the halving, the product with
    rs_u (1), u's own final rounding (1), second order (1).  (rs_u is the same number on both sides.)"""
    return 1 + (cols + 255) // 256 + 8 + 3


def sn_fwd_ref(w, u):
    """One power iteration in float64: v^ = l2n(W u), u^ = l2n(v^ W), sigma = v^ W u^T, w_norm = W / sigma."""
    w, u = w.to(D64), u.to(D64)
    v = l2n(w @ u)
    un = l2n(v @ w)
    sigma = (v @ w) @ un
    return dict(v=v, u=un, sigma=sigma.reshape(1), wn=w / sigma)


def sn_bwd_ref(g, wn, u, v, sigma, dw0=None):
    """dW = (G - <G, w_norm> v^T u) / sigma (+ dw0) -> (ref, E)."""
    g, wn, u, v = g.to(D64), wn.to(D64), u.to(D64), v.to(D64)
    s = sigma.to(D64).reshape(())
    n = g.numel()
    d = (g * wn).sum()
    Ad = (g * wn).abs().sum()
    Ed = R.bound(Ad, n) + U32 * Ad                       # the products g w_norm are rounded
    outer = v[:, None] * u[None, :]
    ref = (g - d * outer) / s
    A = (g.abs() + d.abs() * outer.abs()) / s.abs()
    E = SN_BWD_M * U32 * A + Ed * outer.abs() / s.abs()
    if dw0 is not None:
        ref = ref + dw0.to(D64)
        E = E + U32 * (A + dw0.to(D64).abs())
    return ref, E


def pack_ref(wn, taps):
    """[taps][R][cols] and its per-tap transpose of w_norm [taps * R, cols]."""
    rows, cols = wn.shape
    p = wn.reshape(taps, rows // taps, cols)
    return p, p.transpose(1, 2)


def ortho_cosine_ref(A, scale, want_amb=False):
    """The cosine regulariser's rows as the kernel comment states them -> loss terms per row (Fe), dA (Fe)."""
    A = A.to(D64)
    c = A.shape[0]
    a = Fe(A)
    ss = (a * a).sum(1, c, keepdim=True)
    sa = a.sum(1, c, keepdim=True)
    rn, clamped, amb = fe_rsqrt_clamped(ss)
    r = sa * rn
    if c > 1:
        iq = torch.tensor(1.0 / math.sqrt(c - 1), dtype=D64, device=A.device)
        isq = Fe(iq, RSQRT_U * U32 * iq)
    else:
        isq = Fe(torch.zeros((), dtype=D64, device=A.device))
    ah = a * rn
    Rm = (r - ah) * isq
    s2 = (Rm * Rm).sum(1, c, keepdim=True)
    s1 = Rm.sum(1, c, keepdim=True)
    sra = (Rm * ah).sum(1, c, keepdim=True)
    sc = Fe.lift(scale, a)
    terms = (sc.exact(0.5) * s2)
    si = sc * isq
    T = si * (s1 * r - sra)
    dah = si * (s1 - Rm)
    dA = (rn * dah).where(clamped, rn * (dah - ah * T))
    if want_amb:
        return terms, dA, int(amb.sum())
    return terms, dA


def ortho_identity_ref(A, scale):
    """reg = A - I: loss terms scale / 2 reg^2 (Fe, per element), dA = scale reg (ref, E)."""
    A = A.to(D64)
    c = A.shape[0]
    eye = torch.eye(c, dtype=D64, device=A.device)
    r = Fe(A) - Fe(eye)
    terms = (r * r) * Fe.lift(scale, r).exact(0.5)
    dA = scale * r.v
    E = ID_DA_M * U32 * abs(scale) * (A.abs() + eye)
    return terms, dA, E


def loss_sum(loss0, terms, K):
    """loss_accum after the atomicAdds: loss0 + sum of terms, a reduction of K + 1 values in any order -> (ref, E)."""
    ref = loss0.to(D64).sum() + terms.v.sum()
    A = loss0.to(D64).abs().sum() + terms.v.abs().sum()
    return ref.reshape(1), (R.bound(A, K + 1) + terms.e.sum()).reshape(1)


def lowrank_kappa(scale, c):
    """(kappa, k2) = scale (c - 2) / (2 (c - 1)), scale / (2 (c - 1)) as Fe; both 0 for c == 1."""
    if c <= 1:
        return 0.0, 0.0, 0.0, 0.0
    ka = scale * (c - 2) / (2.0 * (c - 1))
    k2 = scale / (2.0 * (c - 1))
    return ka, (1 + DIV_U) * U32 * abs(ka), k2, DIV_U * U32 * abs(k2)       # (scale (c - 2)) (1) / . (DIV_U)


def lowrank_cols_ref(W, P, s, scale, want_amb=False):
    """The low-rank columns: q_i = sum_r W P, t_i = sum_r W s; with qc = max(q, 1e-12) and f = q / qc (1 unless clamped):
       alpha = 2 kappa t / qc,  beta = -kappa t^2 / qc^2 (clamped: k2 / 1e-12, the derivative of k2 q / 1e-12),
       Wb = W diag(beta),  loss terms kappa t^2 / qc + k2 f  - the sum over j of R[i, j]^2 scale / 2 of the dense form.
    -> alpha, beta, Wb, terms (all Fe)."""
    W, P, s = W.to(D64), P.to(D64), s.to(D64)
    rows, c = W.shape
    w = Fe(W)
    q = (w * Fe(P)).sum(0, rows)
    t = (w * Fe(s[:, None])).sum(0, rows)
    ka, eka, k2, ek2 = lowrank_kappa(scale, c)
    z = torch.zeros((), dtype=D64, device=W.device)
    kappa, k2f = Fe(z + ka, z + eka), Fe(z + k2, z + ek2)
    clamped = q.v < EPS
    amb = (q.v - EPS).abs() <= q.e + U32 * EPS
    qc = Fe(torch.clamp(q.v, min=EPS), torch.where(clamped, torch.full_like(q.e, U32 * EPS), q.e))
    alpha = kappa.exact(2.0) * t / qc
    beta = ((kappa * t * t) / (qc * qc)).exact(-1.0).where(~clamped, k2f / Fe(z + EPS, z + U32 * EPS))
    f = Fe(torch.ones_like(q.v)).where(~clamped, q / qc)
    terms = kappa * t * t / qc + k2f * f
    Wb = w * Fe(beta.v[None, :], beta.e[None, :])
    if want_amb:
        return alpha, beta, Wb, terms, int(amb.sum())
    return alpha, beta, Wb, terms


def lowrank_finish_ref(T, P, s, Wa, ab):
    """dW = 2 T + s alpha^T + (W alpha) 1^T + 2 P diag(beta) -> (ref, E)."""
    T, P, s, Wa, ab = (x.to(D64) for x in (T, P, s, Wa, ab))
    c = P.shape[1]
    al, be = ab[:c], ab[c:]
    ref = 2 * T + s[:, None] * al[None, :] + Wa[:, None] + 2 * P * be[None, :]
    A = 2 * T.abs() + s.abs()[:, None] * al.abs()[None, :] + Wa.abs()[:, None] + 2 * P.abs() * be.abs()[None, :]
    return ref, LRF_M * U32 * A


def adam_ref(p, g, m, v, ema, lr, b1, b2, eps, decay, gscale):
    """TF Adam + EMA shadow; every hyper-parameter is the fp32 value the call carries.  -> {name: (ref, E)}; with b1 == 0
    the first moment is g gscale exactly (E = 0) whatever m held."""
    p, g, m, v = (x.to(D64) for x in (p, g, m, v))
    gi = g * gscale
    if b1 == 0.0:
        mn, Em = gi, ADAM_G_M * U32 * gi.abs()                  # (the test requires m == fl(g gscale) bit for bit)
    else:
        om = f32r(1.0 - b1)
        mn = b1 * m + om * gi
        Em = ADAM_M_M * U32 * (abs(b1) * m.abs() + om * gi.abs())
    om2 = f32r(1.0 - b2)
    vn = b2 * v + om2 * gi * gi
    Ev = ADAM_V_M * U32 * vn                                    # every term is non-negative: A = vn
    sq = vn.sqrt()
    den = sq + eps
    Eden = (ADAM_V_M / 2 + SQRT_U) * U32 * sq + U32 * den
    upd = lr * mn / den
    Eupd = abs(lr) * Em / den + upd.abs() * (Eden / den + ADAM_UPD_M * U32)
    pn = p - upd
    Ep = Eupd + U32 * (p.abs() + upd.abs())                     # the subtraction
    out = dict(m=(mn, Em), v=(vn, Ev), p=(pn, Ep))
    if ema is not None:
        e0 = ema.to(D64)
        od = f32r(1.0 - decay)
        en = decay * e0 + od * pn
        out["ema"] = (en, od * Ep + ADAM_EMA_M * U32 * (abs(decay) * e0.abs() + od * pn.abs()))
    return out


# ------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------
OPS = ("sn_fwd", "sn_bwd", "sn_batch_fwd", "sn_batch_phase", "sn_batch_bwd", "symmetrize", "ortho_cosine",
       "ortho_identity", "gemv_rows", "lowrank_cols", "lowrank_finish", "adam")
ENTRY = {"sn_fwd": "bg_spectral_norm_fwd", "sn_bwd": "bg_spectral_norm_bwd", "sn_batch_fwd": "bg_spectral_norm_batch_fwd",
         "sn_batch_phase": "bg_spectral_norm_batch_phase", "sn_batch_bwd": "bg_spectral_norm_batch_bwd",
         "symmetrize": "bg_symmetrize", "ortho_cosine": "bg_ortho_cosine_fwd_bwd",
         "ortho_identity": "bg_ortho_identity_fwd_bwd", "gemv_rows": "bg_gemv_rows",
         "lowrank_cols": "bg_ortho_lowrank_cols", "lowrank_finish": "bg_ortho_lowrank_finish",
         "adam": "bg_adam_tf_ema_step(_dev)"}
# outputs that several blocks add to with fp32 atomicAdd: exempt from the two-runs-equal-bits rule, gated in both runs
LOSS_EXEMPT = ("loss",)

# [rows, cols] of the spectral-norm cases: what each shape is for
SN_SHAPES = ((7, 33, "cols % 4 != 0: the scalar row loop"), (16, 1, "cols = 1"), (216, 3, "cols = 3, 216 rows"),
             (5, 8, "cols % 4 == 0, one pass"), (64, 256, "one full pass of the vector loop; one 64-row unit"),
             (9, 260, "second vector loop only"), (12, 512, "second vector loop only, twice"),
             (20, 516, "eight-load loop + remainder"), (6, 1028, "eight-load loop twice + remainder"),
             (20, 2052, "eight-load loop four times + remainder"),
             (1, 255, "1 row: a wave's extra rows clamp to r0; cols 255"), (2, 256, "2 rows; cols 256"),
             (3, 257, "3 rows; cols 257: two column blocks"), (5, 12, "5 rows"),
             (63, 5, "63 rows: 8-row unroll tail of 7"), (64, 4, "64 rows: one unit"), (65, 7, "65 rows: two units"),
             (130, 516, "130 rows: three units; > 65536 elements: two row-dot units"),
             (72, 136, "> 8192 elements: two normalise units"),
             (1584, 168, "3 x 3 x 176 x 168 > 262144 elements: two dot units"))
SN_COLS = (33, 1, 3, 8, 256, 260, 512, 516, 1028, 2052, 255, 257)
REG_C = (1, 2, 3, 31, 32, 33, 255, 256, 257, 520)
LOWRANK = ((1, 2), (7, 18), (8, 18), (9, 18), (1, 257), (17, 257), (8, 1030), (17, 1030))
ADAM_N = (1, 3, 4, 1023, 1024, 10007)


def case(op, name, why, **kw):
    c = dict(op=op, name=name, why=why, exempt=())
    c.update(kw)
    return c


def item(rows, cols, taps=0, group=None, data="randn"):
    """One BgSnItem: taps > 0 = packed copies of [taps][rows / taps][cols]; group = (gid, column offset, total cols) of a
    shared pack_p / pack_t (the f | g | h layout)."""
    return dict(rows=rows, cols=cols, taps=taps, group=group, data=data)


def _mask_words(bits, n):
    w = [0] * ((n + 63) // 64)
    for b in bits:
        w[b >> 6] |= 1 << (b & 63)
    return w


def _cases():
    out = []
    for rows, cols, why in SN_SHAPES:
        out.append(case("sn_fwd", "%dx%d" % (rows, cols), why, rows=rows, cols=cols, data="randn"))
        out.append(case("sn_bwd", "%dx%d" % (rows, cols), why, rows=rows, cols=cols, data="randn"))
    out.append(case("sn_fwd", "7x33 tiny", "sum of squares < 1e-12: both l2n clamps, sigma tiny but finite", rows=7,
                    cols=33, data="tiny"))
    out.append(case("sn_fwd", "16x8 tiny", "both clamps on the vector path", rows=16, cols=8, data="tiny"))
    out.append(case("sn_bwd", "7x33 tiny", "1 / sigma of a tiny sigma", rows=7, cols=33, data="tiny"))
    # ---- multi-tensor tables
    one = [item(7, 33)]
    fgh = [item(24, 6, 1, (0, 0, 22)), item(24, 6, 1, (0, 6, 22)), item(24, 10, 1, (0, 12, 22))]
    mixed = [item(384, 6, 16), item(20, 516), item(72, 136, 1), fgh[0], item(130, 516), fgh[1], item(1584, 168, 9),
             fgh[2], item(7, 33, data="tiny")]
    many = []
    for k in range(130):
        rows, cols = 1 + (7 * k) % 13, 1 + (5 * k) % 11
        if k % 9 == 4:
            many.append(item(2 * rows, 2 * cols, 1))
        else:
            many.append(item(rows, cols))
    for nm, items in (("1 item", one), ("9 mixed", mixed), ("130 small", many)):
        n = len(items)
        out.append(case("sn_batch_fwd", nm, "BgSnItem table of %d" % n, items=items))
        own = [j for j in range(n) if j % 2 == 0]
        out.append(case("sn_batch_phase", nm, "POWER on the even items, NORMALIZE on all", items=items, own=own))
    out.append(case("sn_batch_bwd", "1 item", "masks NULL: all enabled, none accumulates", items=one, enable=None,
                    accumulate=None))
    out.append(case("sn_batch_bwd", "1 item acc", "accumulate bit 0", items=one, enable=[0], accumulate=[0]))
    out.append(case("sn_batch_bwd", "9 mixed", "item 4 disabled, items 1, 6, 8 accumulate", items=mixed,
                    enable=[0, 1, 2, 3, 5, 6, 7, 8], accumulate=[1, 6, 8]))
    dis = {0, 70, 129}
    out.append(case("sn_batch_bwd", "130 small", "mask words 0, 1, 2: items 0, 70, 129 disabled; bits 63, 64, 128 set",
                    items=many, enable=[j for j in range(130) if j not in dis], accumulate=[1, 63, 64, 100, 128, 129]))
    # ---- regulariser
    for c in REG_C:
        out.append(case("symmetrize", "c%d" % c, "edge tiles of 32 x 32", c=c))
        out.append(case("ortho_cosine", "c%d" % c, "one block per row, %d strides" % ((c + 255) // 256), c=c, data="gram",
                        dA=True, loss0=0.0 if c % 2 else 0.375, exempt=LOSS_EXEMPT))
        out.append(case("ortho_identity", "c%d" % c, "grid-stride over c^2", c=c, data="gram", dA=True,
                        loss0=0.375 if c % 2 else 0.0, exempt=LOSS_EXEMPT))
    for c in (3, 33, 257):
        out.append(case("ortho_cosine", "c%d clamp" % c, "a row with 0 < sum of squares < 1e-12 and an all-zero row", c=c,
                        data="clamp", dA=True, loss0=0.25, exempt=LOSS_EXEMPT))
    for c in (2, 33, 520):
        out.append(case("ortho_cosine", "c%d loss only" % c, "dA == NULL", c=c, data="gram", dA=False, loss0=-0.5,
                        exempt=LOSS_EXEMPT))
        out.append(case("ortho_identity", "c%d loss only" % c, "dA == NULL", c=c, data="gram", dA=False, loss0=-0.5,
                        exempt=LOSS_EXEMPT))
    for cols in SN_COLS:
        for v in (True, False):
            out.append(case("gemv_rows", "5x%d v%d" % (cols, v), "cols %% 4 == %d" % (cols % 4), rows=5, cols=cols, v=v))
    out.append(case("gemv_rows", "17x1030 v1", "the W alpha vector of the widest low-rank case", rows=17, cols=1030, v=True))
    for k, (rows, c) in enumerate(LOWRANK):
        out.append(case("lowrank_cols", "%dx%d" % (rows, c), "rows %% 8 == %d, %d blocks" % (rows % 8, (c + 255) // 256),
                        rows=rows, c=c, data="randn", loss0=0.125 if k % 2 else 0.0, exempt=LOSS_EXEMPT))
        out.append(case("lowrank_finish", "%dx%d" % (rows, c), "grid-stride over rows x c", rows=rows, c=c))
    for rows, c in ((7, 18), (17, 257)):
        out.append(case("lowrank_cols", "%dx%d clamp" % (rows, c), "a column with q in (0, 1e-12) and a column W[:, i] = 0",
                        rows=rows, c=c, data="clamp", loss0=0.125, exempt=LOSS_EXEMPT))
    # ---- Adam
    k = 0
    for n in ADAM_N:
        for b1 in (0.0, 0.5):
            out.append(case("adam", "n%d b1=%g #%d" % (n, b1, k), "n %% 4 == %d" % (n % 4), n=n, b1=b1, align=0,
                            ema=k % 3 != 2, gscale=(1.0, 0.25)[k % 2], decay=(0.999, 0.0)[(k // 2) % 2]))
            k += 1
    for b1 in (0.0, 0.5):
        out.append(case("adam", "n1024 b1=%g +4B" % b1, "aligned n, buffers at +4 bytes: the scalar kernel", n=1024, b1=b1,
                        align=4, ema=True, gscale=0.25, decay=0.999))
    out.append(case("adam", "n1024 b1=0 no ema g1", "ema == NULL on the four-wide kernel", n=1024, b1=0.0, align=0,
                    ema=False, gscale=1.0, decay=0.999))
    out.append(case("adam", "n1024 b1=0.5 decay 0", "decay 0", n=1024, b1=0.5, align=0, ema=True, gscale=0.25, decay=0.0))
    return out


CASES = _cases()


def cases(op=None):
    return [c for c in CASES if op is None or c["op"] == op]


def describe(c):
    return "%s[%s]" % (c["op"], c["name"])


def mask_words(c, key):
    return None if c[key] is None else _mask_words(c[key], len(c["items"]))


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
SCALE = f32r(1e-4)
ADAM = dict(lr=f32r(2e-4 * math.sqrt(1 - 0.999 ** 3)), b2=f32r(0.999), eps=f32r(1e-8))


def _rn(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, device=dev, dtype=D64) * scale).float()


def _sn_inputs(rows, cols, data, gen, dev):
    """One weight with everything both passes read: w, u0; and, from the float64 forward, the backward's inputs."""
    w = _rn((rows, cols), gen, dev, 1e-8 if data == "tiny" else 1.0 / math.sqrt(cols))
    u0 = _rn((cols,), gen, dev)
    r = sn_fwd_ref(w, u0)
    return dict(w=w, u0=u0, g=_rn((rows, cols), gen, dev), dw0=_rn((rows, cols), gen, dev), wn=r["wn"].float(),
                u=r["u"].float(), v=r["v"].float(), sigma=r["sigma"].float())


CLAMP_F = 0.25               # the clamped rows / columns carry sum of squares (q) = CLAMP_F * 1e-12: sum_j Ahat^2 = 0.25


def clamp_column(W, k):
    """Scale column k of the fp32 weight W in place so that q_k = w_k^T (W W^T) w_k is CLAMP_F * 1e-12."""
    Wd = W.double()
    q = ((Wd @ Wd.t() @ Wd) * Wd).sum(0)
    W[:, k] *= math.sqrt(CLAMP_F * EPS / float(q[k]))


def _gram(c, data, gen, dev):
    rows = max(1, c // 2)
    W = torch.randn((rows, c), generator=gen, device=dev, dtype=D64) * (1.0 / math.sqrt(rows))
    if data == "clamp":
        W[:, c - 1] = 0.0          # last row (and column) of A exactly zero
        A = W.t() @ W
        W[:, 1] *= math.sqrt(CLAMP_F * EPS / float((A[1] * A[1]).sum()))      # row 1 of A: sum of squares ~ 1e-12 / 4
    return (W.t() @ W).float()


def make_inputs(c, dev, gen):
    op = c["op"]
    if op in ("sn_fwd", "sn_bwd"):
        return _sn_inputs(c["rows"], c["cols"], c["data"], gen, dev)
    if op.startswith("sn_batch"):
        return dict(items=[_sn_inputs(it["rows"], it["cols"], it["data"], gen, dev) for it in c["items"]])
    if op == "symmetrize":
        return dict(A=_rn((c["c"], c["c"]), gen, dev))
    if op in ("ortho_cosine", "ortho_identity"):
        return dict(A=_gram(c["c"], c["data"], gen, dev), loss0=torch.full((1,), c["loss0"], dtype=F32, device=dev))
    if op == "gemv_rows":
        return dict(w=_rn((c["rows"], c["cols"]), gen, dev), v=_rn((c["cols"],), gen, dev) if c["v"] else None)
    if op in ("lowrank_cols", "lowrank_finish"):
        rows, cc = c["rows"], c["c"]
        W = _rn((rows, cc), gen, dev, 0.3)
        if op == "lowrank_cols" and c["data"] == "clamp":
            W[:, 5] = 0.0
            clamp_column(W, 3)
        Wd = W.double()
        P = ((Wd @ Wd.t()) @ Wd).float()
        s = Wd.sum(1).float()
        if op == "lowrank_cols":
            return dict(W=W, P=P, s=s, loss0=torch.full((1,), c["loss0"], dtype=F32, device=dev))
        return dict(T=_rn((rows, cc), gen, dev), P=P, s=s, Wa=_rn((rows,), gen, dev), ab=_rn((2 * cc,), gen, dev))
    if op == "adam":
        n = c["n"]
        g = _rn((n,), gen, dev)
        v = _rn((n,), gen, dev).square()
        k = torch.arange(n, device=dev)
        v[k % 7 == 0] = 0.0                      # v = 0 with g != 0
        g[k % 14 == 0] = 0.0                     # v = 0, g = 0: 0 / (0 + eps)
        g[k % 14 == 7] *= 1e-5                   # v = 0, g tiny: sqrt(v) of the order of eps
        m = torch.full((n,), POISON, dtype=F32, device=dev) if c["b1"] == 0.0 else _rn((n,), gen, dev, 0.1)
        return dict(p=_rn((n,), gen, dev), g=g, m=m, v=v, ema=_rn((n,), gen, dev) if c["ema"] else None,
                    lr=torch.full((1,), ADAM["lr"], dtype=F32, device=dev))
    raise KeyError(op)


# ------------------------------------------------------------------------------------------
# the check of one call's outputs
# ------------------------------------------------------------------------------------------
def _sn_fwd_check(rec, it, i, out, pre, stages=("v", "u", "sigma", "wn")):
    """The forward chain of one weight, stage by stage; out[pre + name] are the call's tensors.  -> ambiguous clamps."""
    w, u0 = i["w"].double(), i["u0"].double()
    rows, cols = w.shape
    amb = 0
    if "v" in stages:
        A = w.abs() @ u0.abs()
        ref, E, a = l2n_bound(w @ u0, R.bound(A, cols) + U32 * A, SN_V_M)
        amb += a
        rec.gate("v", out[pre + "v"], ref, E)
    if "u" in stages:
        v = out[pre + "v"].double()
        raw = v @ w
        A = v.abs() @ w.abs()
        Eraw = R.bound(A, rows) + 2 * U32 * A + SN_T_M * U32 * raw.abs()      # products v_ w (1), v^'s own rounding (1)
        ref, E, a = l2n_bound(raw, Eraw, sn_u_m(cols))
        amb += a
        rec.gate("u", out[pre + "u"], ref, E)
        if "sigma" in stages:
            ug = out[pre + "u"].double()
            sref = (raw * ug).sum().reshape(1)
            sA = (raw * ug).abs().sum()
            rec.gate("sigma", out[pre + "sigma"], sref, ((ug.abs() * Eraw).sum() + sn_sigma_m(cols) * U32 * sA).reshape(1))
    if "wn" in stages:
        sg = out[pre + "sigma"].double().reshape(())
        if not bool(torch.isfinite(sg)) or float(sg) == 0.0:
            rec.fail("sigma = %r is not finite and non-zero" % float(sg))
            return amb
        q = w / sg
        if pre + "wn" in out:
            rec.gate("w_norm", out[pre + "wn"], q, SN_DIV_M * U32 * q.abs())
        if it is not None and it["taps"]:
            pp, pt = out[pre + "pp"], out[pre + "pt"]
            rp, _ = pack_ref(q, it["taps"])
            rec.gate("pack_p", pp, rp, SN_DIV_M * U32 * rp.abs())
            rec.exact("pack_t", pt, pp.transpose(1, 2))
    return amb


def _sn_bwd_check(rec, i, got, acc):
    ref, E = sn_bwd_ref(i["g"], i["wn"], i["u"], i["v"], i["sigma"], i["dw0"] if acc else None)
    rec.gate("dw", got, ref, E)


def check(c, i, out, rec):
    """Gate the outputs ``out`` (name -> tensor) of case c on inputs i: rec.gate(label, got, ref, E) /
    rec.exact(label, got, want) / rec.fail(message).  -> (elements left out of the gate, outputs)."""
    op = c["op"]
    if op == "sn_fwd":
        return _sn_fwd_check(rec, None, i, out, ""), out["wn"].numel()
    if op == "sn_bwd":
        _sn_bwd_check(rec, i, out["dw"], False)
        return 0, out["dw"].numel()
    if op in ("sn_batch_fwd", "sn_batch_phase"):
        amb = nout = 0
        for j, (it, ij) in enumerate(zip(c["items"], i["items"])):
            amb += _sn_fwd_check(rec, it, ij, out, "%d." % j)
            nout += ij["w"].numel()
        return amb, nout
    if op == "sn_batch_bwd":
        en, acc = c["enable"], c["accumulate"] or []
        nout = 0
        for j, ij in enumerate(i["items"]):
            got = out["%d.dw" % j]
            if en is not None and j not in en:
                rec.exact("dw of a disabled item", got, ij["dw0"])
            else:
                _sn_bwd_check(rec, ij, got, j in acc)
            nout += got.numel()
        return 0, nout
    if op == "symmetrize":
        A = i["A"].double()
        rec.gate("S", out["S"], A + A.t(), torch.zeros_like(A))             # one correctly rounded sum
        return 0, A.numel()
    if op == "ortho_cosine":
        terms, dA, amb = ortho_cosine_ref(i["A"], SCALE, want_amb=True)
        ref, E = loss_sum(i["loss0"], terms, c["c"])
        for k in [k for k in out if k.startswith("loss")]:
            rec.gate("loss", out[k], ref, E)
        if c["dA"]:
            rec.gate("dA", out["dA"], dA.v, dA.e)
        return amb * c["c"], c["c"] * c["c"]
    if op == "ortho_identity":
        terms, dA, E = ortho_identity_ref(i["A"], SCALE)
        ref, El = loss_sum(i["loss0"], terms, c["c"] * c["c"])
        for k in [k for k in out if k.startswith("loss")]:
            rec.gate("loss", out[k], ref, El)
        if c["dA"]:
            rec.gate("dA", out["dA"], dA, E)
        return 0, c["c"] * c["c"]
    if op == "gemv_rows":
        w = i["w"].double()
        if i["v"] is None:
            rec.gate("out", out["out"], w.sum(1), R.bound(w.abs().sum(1), c["cols"]))
        else:
            v = i["v"].double()
            A = w.abs() @ v.abs()
            rec.gate("out", out["out"], w @ v, R.bound(A, c["cols"]) + U32 * A)
        return 0, c["rows"]
    if op == "lowrank_cols":
        alpha, beta, Wb, terms, amb = lowrank_cols_ref(i["W"], i["P"], i["s"], SCALE, want_amb=True)
        ref, E = loss_sum(i["loss0"], terms, c["c"])
        for k in [k for k in out if k.startswith("loss")]:
            rec.gate("loss", out[k], ref, E)
        rec.gate("alpha", out["ab"][:c["c"]], alpha.v, alpha.e)
        rec.gate("beta", out["ab"][c["c"]:], beta.v, beta.e)
        rec.gate("Wb", out["Wb"], Wb.v, Wb.e)
        return amb * c["rows"], c["rows"] * c["c"]
    if op == "lowrank_finish":
        ref, E = lowrank_finish_ref(i["T"], i["P"], i["s"], i["Wa"], i["ab"])
        rec.gate("dW", out["dW"], ref, E)
        return 0, ref.numel()
    if op == "adam":
        r = adam_ref(i["p"], i["g"], i["m"], i["v"], i["ema"], ADAM["lr"], f32r(c["b1"]), ADAM["b2"], ADAM["eps"],
                     f32r(c["decay"]), f32r(c["gscale"]))
        for k, (ref, E) in r.items():
            if k == "m" and c["b1"] == 0.0:
                rec.exact("m (b1 = 0)", out["m"], (i["g"] * f32r(c["gscale"])).float())
            else:
                rec.gate(k, out[k], ref, E)
        return 0, c["n"]
    raise KeyError(op)


# ------------------------------------------------------------------------------------------
# the composed regulariser: OrthoCosineRegFn's two chains on one weight, stage bounds summed to first order
# ------------------------------------------------------------------------------------------
COMPOSED = (9, 18)           # 2 * rows == c: the boundary from which OrthoCosineRegFn takes the low-rank form


def composed_weight(dev):
    rows, c = COMPOSED
    gen = torch.Generator(device=dev).manual_seed(77)
    w = (torch.randn((rows, c), generator=gen, device=dev, dtype=D64) * 0.3).float()
    clamp_column(w, 3)       # q_3 in (0, 1e-12): the clamped column
    return w


def cosine_rows(A, scale):
    """Differentiable float64 form of the dense rows: scale / 2 sum_j R[i, j]^2 per row i."""
    c = A.shape[0]
    Ah = A * torch.clamp((A * A).sum(1, keepdim=True), min=EPS).rsqrt()
    if c == 1:
        return (Ah * 0.0).sum(1)
    Rm = (Ah.sum(1, keepdim=True) - Ah) / math.sqrt(c - 1)
    return scale * 0.5 * (Rm * Rm).sum(1)


def composed_dense(w, scale):
    """gemm A = W^T W (K = rows) -> bg_ortho_cosine_fwd_bwd -> bg_symmetrize -> gemm dW = W S (K = c).  The Gram-side
    kernel's own bound (ortho_cosine_ref) plus its sensitivity to A's error - |d out / d A| E_A by autograd on the float64
    formula, row by row - then one rounding for S and the last GEMM's bound plus |W| E_S."""
    Wd = w.double()
    rows, c = Wd.shape
    A = Wd.t() @ Wd
    EA = R.bound(Wd.abs().t() @ Wd.abs(), rows) + U32 * A.abs()
    terms, dA = ortho_cosine_ref(A, scale)
    leaf = A.clone().requires_grad_(True)
    g = torch.autograd.grad(cosine_rows(leaf, scale).sum(), leaf, create_graph=True)[0]
    Eloss = loss_sum(torch.zeros(1, dtype=D64, device=w.device), terms, c)[1] + (g.detach().abs() * EA).sum()
    EdA = dA.e.clone()
    for i in range(c):
        for j in range(c):
            (gi,) = torch.autograd.grad(g[i, j], leaf, retain_graph=True)
            EdA[i, j] += (gi[i].abs() * EA[i]).sum()                 # row i of dA depends on row i of A alone
    S = dA.v + dA.v.t()
    ES = EdA + EdA.t() + U32 * S.abs()
    return dict(loss=cosine_rows(A, scale).sum().reshape(1), Eloss=Eloss, dA=g.detach(), dW=Wd @ S,
                EdW=R.bound(Wd.abs() @ S.abs(), c) + Wd.abs() @ ES)


def composed_lowrank(w, scale):
    """gemm G = W W^T (K = c), bg_gemv_rows s = W 1, gemm P = G W (K = rows), bg_ortho_lowrank_cols, bg_gemv_rows W alpha,
    gemm H = Wb W^T (K = c), gemm T = H W (K = rows), bg_ortho_lowrank_finish: each stage's own bound, and the errors of its
    inputs times the absolute partial derivatives of the float64 formula."""
    Wd = w.double()
    aW = Wd.abs()
    rows, c = Wd.shape
    G = Wd @ Wd.t()
    EG = R.bound(aW @ aW.t(), c) + U32 * G.abs()
    P = G @ Wd
    EP = R.bound(G.abs() @ aW, rows) + EG @ aW + U32 * P.abs()
    s = Wd.sum(1)
    Es = R.bound(aW.sum(1), c) + U32 * s.abs()
    alpha, beta, Wb, terms = lowrank_cols_ref(Wd, P, s, scale)
    q, t = (Wd * P).sum(0), (Wd * s[:, None]).sum(0)
    Eq, Et = (aW * EP).sum(0), (aW * Es[:, None]).sum(0)
    ka, _, k2, _ = lowrank_kappa(scale, c)
    qc = torch.clamp(q, min=EPS)
    cl = q < EPS
    zero = torch.zeros_like(q)
    dl_dq = torch.where(cl, zero + k2 / EPS, ka * t * t / (qc * qc))
    Eloss = (loss_sum(torch.zeros(1, dtype=D64, device=w.device), terms, c)[1] +
             (dl_dq.abs() * Eq + 2 * abs(ka) * t.abs() / qc * Et).sum())
    Eal = alpha.e + 2 * abs(ka) * (Et / qc + torch.where(cl, zero, t.abs() * Eq / (qc * qc)))
    Ebe = beta.e + torch.where(cl, zero, abs(ka) * (2 * t.abs() * Et / (qc * qc) + 2 * t * t * Eq / qc ** 3))
    Wa = Wd @ alpha.v
    EWa = R.bound(aW @ alpha.v.abs(), c) + aW @ (Eal + U32 * alpha.v.abs()) + U32 * Wa.abs()
    EWb = Wb.e + aW * Ebe[None, :]
    H = Wb.v @ Wd.t()
    EH = R.bound(Wb.v.abs() @ aW.t(), c) + EWb @ aW.t() + U32 * H.abs()
    T = H @ Wd
    ET = R.bound(H.abs() @ aW, rows) + EH @ aW + U32 * T.abs()
    dW, Efin = lowrank_finish_ref(T, P, s, Wa, torch.cat([alpha.v, beta.v]))
    EdW = (Efin + 2 * ET + Es[:, None] * alpha.v.abs()[None, :] + s.abs()[:, None] * Eal[None, :] + EWa[:, None] +
           2 * EP * beta.v.abs()[None, :] + 2 * P.abs() * Ebe[None, :])
    return dict(loss=terms.v.sum().reshape(1), Eloss=Eloss, dW=dW, EdW=EdW)
