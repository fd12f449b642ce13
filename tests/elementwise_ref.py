"""float64 references, error bounds and the case table of the bf16-resident elementwise / reduction kernels.

Test helper, not product code.  Three parts:

* references - plain torch restatements of the "_t" formulas of ``include/biggan_hip.h`` (batch statistics, batch-norm
  apply + PReLU forward / backward, stand-alone PReLU, bias gradient, 2 x 2 max pool, global sum pool, linear
  combination, dot product, cast).  Device-agnostic, evaluated in ``dt`` (float64 for the reference; float32 gives the
  "simulated kernel" of tests/test_elementwise_gate.py), written in the order of operations the header documents.  Next
  to every reference stands the same expression on absolute values, ``A``, and the count of fp32 roundings its bound
  is built from - never anything a kernel returned:
    - elementwise outputs: ``E = m 2^-24 A`` with ``m`` the roundings on the longest path plus one for the
      second-order terms;
    - reductions over K rows: ``launch_replay.bound(A, K)`` plus one unit ``2^-24 A`` for every rounding inside a term
      that is not an exact product of two bf16 values;
    - pure routing (max pool, sum-pool backward, casts that widen) is bit-exact.
  Acceptance is ``launch_replay.gate``.
* sign-ambiguous elements - where the output depends on the sign of a pre-activation computed in fp32 (batch norm with
  PReLU), an element with ``|pre_ref| <= E_pre`` may match either branch; ``check`` counts them, and the share in one
  case must stay <= AMBIGUITY_CAP (continuous data: ~ E_pre / sigma ~ 1e-6).  Exact zeros planted for the alpha / 2
  rule go through the stand-alone PReLU, whose argument is the stored value: never ambiguous.
* CASES - the table both test modules walk: the (N, HW, C) of the batch-norm, PReLU, residual-add, max-pool and
  bias-gradient sites of BASELINE config 3 at batch 256, and small edge shapes for every dispatch fallback (the thin
  slope-gradient path of fp32 tensors with C <= 4 and bg_dot's n % 4 != 0 among them).
"""
import torch

from tests import launch_replay as R

U32 = R.U32
F32, BF16 = R.F32, R.BF16
D64 = torch.float64
AMBIGUITY_CAP = 1e-4
WIDE_MIN = 16 << 20            # elements from which launch_colreduce<.., WIDE> takes the 8-column form
CHUNK = 1 << 24                # elements of one float64 reference chunk


def tdt(code):
    return torch.bfloat16 if code == BF16 else torch.float32


# ------------------------------------------------------------------------------------------
# references.  Activations [n, HW, C] (PReLU / bias gradient: [rows, C]); mean, rstd, alpha, cm halves [C]; ga / be
# broadcast against the activations ([C], [n, 1, C] per sample, or [n, HW, C] per row in the mutation self-test).
# ------------------------------------------------------------------------------------------
def _to(dt, *ts):
    return tuple(None if t is None else t.to(dt) for t in ts)


def slope(v, a):
    """TF gradient of relu(v) + a (v - |v|) / 2: 1 for v > 0, a for v < 0, a / 2 at v == 0."""
    one = torch.ones((), dtype=v.dtype, device=v.device)
    return torch.where(v > 0, one, torch.where(v < 0, a, 0.5 * a))


BN_FWD_M = 5        # inv = rs ga (1); mu inv (2); be - mu inv (3); x inv (2) + sh (4); + 1 second-order
PRE_BWD_M = 5       # x - mu (1); * rs (2); * ga (3); + be (4); + 1 second-order
BN_DX_M = 6         # xh (2) -> xh m2 (3) | g = dy d (1) -> g ga (2) -> - m1 (3); difference (4); * rs (5); + 1
PRELU_M = 1         # a x (the positive branch is a copy)
PRELU_BWD_M = 1     # dy d (d = 1, a, or the exact a / 2)
LINCOMB_M = 3       # s a (1), sb b (1), sum (2); + 1 second-order


def bn_fwd(x, mean, rstd, ga, be, alpha, dt=D64):
    """y = act(x (rs ga) + (be - mu (rs ga))).  -> dict(ref, E [, alt, Ealt, amb]): BN_FWD_M roundings, one more for
    PReLU's a v; alt = the other PReLU branch, amb = |pre| <= E_pre."""
    x, mean, rstd, ga, be, a = _to(dt, x, mean, rstd, ga, be, alpha)
    inv = rstd * ga
    sh = be - mean * inv
    pre = x * inv + sh
    A = x.abs() * inv.abs() + (be.abs() + mean.abs() * inv.abs())
    Epre = BN_FWD_M * U32 * A
    if a is None:
        return dict(ref=pre, E=Epre)
    pos = pre > 0
    neg, Eneg = a * pre, (BN_FWD_M + 1) * U32 * a.abs() * A
    return dict(ref=torch.where(pos, pre, neg), E=torch.where(pos, Epre, Eneg), alt=torch.where(pos, neg, pre),
                Ealt=torch.where(pos, Eneg, Epre), amb=pre.abs() <= Epre)


def _bwd_terms(x, dy, mean, rstd, ga, be, a):
    xh = (x - mean) * rstd
    Axh = (x.abs() + mean.abs()) * rstd.abs()
    pre = xh * ga + be
    Apre = Axh * ga.abs() + be.abs()
    Epre = PRE_BWD_M * U32 * Apre
    if a is None:
        return xh, Axh, pre, Epre, None, None, None
    one = torch.ones((), dtype=x.dtype, device=x.device)
    d = slope(pre, a)
    dalt = torch.where(pre > 0, a, one)
    return xh, Axh, pre, Epre, d, dalt, pre.abs() <= Epre


def bn_bwd_dx(x, dy, mean, rstd, ga, be, alpha, cm, add, dt=D64):
    """dx = rs (g ga - m1 - xh m2) (+ add), g = dy act'(pre), pre = ((x - mu) rs) ga + be recomputed.  BN_DX_M
    roundings, one more for the fused add."""
    x, dy, mean, rstd, ga, be, a, cm, add = _to(dt, x, dy, mean, rstd, ga, be, alpha, cm, add)
    C = x.shape[-1]
    m1, m2 = cm[:C], cm[C:]
    xh, Axh, pre, Epre, d, dalt, amb = _bwd_terms(x, dy, mean, rstd, ga, be, a)
    m = BN_DX_M + (1 if add is not None else 0)

    def form(dd):
        g = dy if dd is None else dy * dd
        out = rstd * (g * ga - m1 - xh * m2)
        A = rstd.abs() * (g.abs() * ga.abs() + m1.abs() + Axh * m2.abs())
        if add is not None:
            out, A = out + add, A + add.abs()
        return out, m * U32 * A
    ref, E = form(d)
    if a is None:
        return dict(ref=ref, E=E)
    alt, Ealt = form(dalt)
    return dict(ref=ref, E=E, alt=alt, Ealt=Ealt, amb=amb)


def bn_bwd_reduce(x, dy, mean, rstd, ga, be, alpha, dt=D64):
    """part[0] = sum_hw g, part[1] = sum_hw g xh, part[2] = sum_hw dy min(pre, 0)   ([3, n, C]).
    Units on top of bound(A, HW): g = dy d is one rounding (d is a generic fp32 slope); g xh: g (1), xh (2), the
    product (1); dy min(pre, 0): pre (4), the product (1).  Without PReLU g = dy: 0 / 3 / the plane is exactly 0.
    An ambiguous element may sit on either branch: |dy| |1 - a| (|xh|) more on planes 0 and 1."""
    x, dy, mean, rstd, ga, be, a = _to(dt, x, dy, mean, rstd, ga, be, alpha)
    HW = x.shape[1]
    xh, Axh, pre, Epre, d, dalt, amb = _bwd_terms(x, dy, mean, rstd, ga, be, a)
    Apre = Epre / (PRE_BWD_M * U32)
    if a is None:
        g, units = dy, (0, 3, 0)
        p2 = torch.zeros_like(x)
        A2 = torch.zeros_like(x)
        X = torch.zeros_like(x)
    else:
        g, units = dy * d, (1, 4, 5)
        p2 = dy * torch.clamp(pre, max=0)
        A2 = dy.abs() * Apre * (pre <= Epre)
        X = amb * dy.abs() * (1 - a).abs()
    ref = torch.stack([g.sum(1), (g * xh).sum(1), p2.sum(1)])
    A = torch.stack([g.abs().sum(1), (g.abs() * Axh).sum(1), A2.sum(1)])
    extra = torch.stack([X.sum(1), (X * Axh).sum(1), torch.zeros_like(A[2])])
    u = torch.tensor(units, dtype=A.dtype, device=A.device)[:, None, None]
    E = R.bound(A, HW, u * U32 * A + extra)
    return dict(ref=ref, E=E, namb=0 if amb is None else int(amb.sum()))


def prelu_fwd(x, alpha, dt=D64):
    x, a = _to(dt, x, alpha)
    ref = torch.where(x > 0, x, a * x)
    return dict(ref=ref, E=PRELU_M * U32 * ref.abs())


def prelu_bwd(x, dy, alpha, add, dt=D64):
    """dx = dy act'(x) (+ add): the argument is the stored value, so the branch is never ambiguous."""
    x, dy, a, add = _to(dt, x, dy, alpha, add)
    ref = dy * slope(x, a)
    A = ref.abs()
    m = PRELU_BWD_M
    if add is not None:
        ref, A, m = ref + add, A + add.abs(), m + 1
    return dict(ref=ref, E=m * U32 * A)


def colsum(t, dt=D64):
    """Column sums of [rows, C] terms that are exact in fp32 (a bf16 value, or a product of two): bound(A, rows)."""
    t = t.to(dt)
    return t.sum(0), t.abs().sum(0)


def _win(x):
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def maxpool_fwd(x):
    a, b, c, d = _win(x)
    return torch.maximum(torch.maximum(a, b), torch.maximum(c, d))


def maxpool_bwd(x, dy, last=False):
    """The whole gradient goes to the first maximum in the order (0,0), (0,1), (1,0), (1,1) (last=True: the mutation)."""
    w = _win(x)
    m = maxpool_fwd(x)
    dx = torch.zeros_like(x)
    taken = torch.zeros_like(m, dtype=torch.bool)
    order = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for k in (reversed(range(4)) if last else range(4)):
        sel = ~taken & (w[k] == m)
        taken = taken | sel
        i, j = order[k]
        dx[:, i::2, j::2] = torch.where(sel, dy, torch.zeros_like(dy))
    return dx


def lincomb(a, s, b, sb, dt=D64):
    a, b = _to(dt, a, b)
    if b is None:
        ref = s * a
        return dict(ref=ref, E=(LINCOMB_M - 1) * U32 * ref.abs())
    ref = s * a + sb * b
    return dict(ref=ref, E=LINCOMB_M * U32 * (abs(s) * a.abs() + abs(sb) * b.abs()))


def select(got, r):
    """(ref, E) against which ``got`` is gated: per ambiguous element, the branch that lies closer to got."""
    if r.get("amb") is None:
        return r["ref"], r["E"]
    g = got.double()
    use = r["amb"] & ((g - r["alt"]).abs() < (g - r["ref"]).abs())
    return torch.where(use, r["alt"], r["ref"]), torch.where(use, r["Ealt"], r["E"])


# ------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------
# ops whose fp32-only entry point ("bg_X" next to "bg_X_t") the GPU test also calls on the fp32 / fp32 rows without dx_add
FP32_ENTRY = ("bn_stats", "bn_fwd", "bn_bwd_reduce", "bn_bwd_dx", "prelu_fwd", "prelu_bwd", "bias_grad", "maxpool_fwd",
              "maxpool_bwd", "sum_pool_fwd", "sum_pool_bwd", "dot")
OPS = ("bn_stats", "bn_fwd", "bn_bwd_reduce", "bn_bwd_dx", "prelu_fwd", "prelu_bwd", "bias_grad", "maxpool_fwd",
       "maxpool_bwd", "sum_pool_fwd", "sum_pool_bwd", "lincomb", "dot", "cast")
TWO_DTYPES = ("bn_fwd", "bn_bwd_reduce", "bn_bwd_dx", "prelu_fwd", "prelu_bwd")
PAIRS = ((BF16, BF16), (F32, BF16), (BF16, F32), (F32, F32))
ADD = ("none", "sep", "alias")


def case(op, name, origin, **kw):
    c = dict(op=op, name=name, origin=origin, N=1, HW=1, C=8, H=0, W=0, n=0, xdt=BF16, ydt=BF16, per_sample=0,
             alpha=True, add="none", align=0, data="randn", small=False, dalpha=True, sa_dev=False, b=True)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def numel(c):
    return c["n"] if c["n"] else c["N"] * (c["H"] * c["W"] if c["H"] else c["HW"]) * c["C"]


# (N, HW, C) of the generator's conditional batch norms of config 3 at batch 256 (model.py _generator_trunk: 4x4x1536,
# then resblock_up_condition's res1 on the block input and res2 behind the up-convolution, channels 1536, 768, 384,
# 192, 96), each with its fork flag: the block input also feeds the skip branch, so its dx takes dx_add
G_BN = ((256, 16, 1536, "alias"),          # resblock_up_16/res1: 6 Mi elements, 4-column reductions, 128 blocks
        (256, 64, 1536, "none"),           # resblock_up_16/res2 = resblock_up_8/res1 input: 24 Mi, 8-column, x8 row step
        (256, 256, 768, "alias"),          #   of 5464 rows > HW; 48 Mi: the 192-block target (> 100 MB as fp32)
        (256, 1024, 384, "sep"),           # resblock_up_4: 96 Mi
        (256, 4096, 192, "alias"),         # resblock_up_2: 192 Mi
        (256, 16384, 96, "none"))          # resblock_up_1/res2: 384 Mi elements, CV = 12


def _production():
    out = []
    for N, HW, C, add in G_BN:
        tag = "g%dx%d" % (HW, C)
        src = "G cond. batch norm, %d px x %d ch @ 256" % (HW, C)
        out.append(case("bn_stats", tag, src, N=N, HW=HW, C=C))
        out.append(case("bn_fwd", tag, src, N=N, HW=HW, C=C, per_sample=1))
        out.append(case("bn_bwd_reduce", tag, src, N=N, HW=HW, C=C, per_sample=1))
        out.append(case("bn_bwd_dx", tag, src, N=N, HW=HW, C=C, per_sample=1, add=add))
    # the generator's last batch norm (model.py: ops._bn_act(x, None) before G_logit): per-channel gamma / beta
    src = "G tail batch norm 128x128x96 @ 256"
    out.append(case("bn_fwd", "gtail", src, N=256, HW=16384, C=96))
    out.append(case("bn_bwd_reduce", "gtail", src, N=256, HW=16384, C=96))
    out.append(case("bn_bwd_dx", "gtail", src, N=256, HW=16384, C=96))
    # the 8x8x1536 site at batch 170: 16 711 680 elements, the largest multiple of one image below 16 Mi - the last
    # shape that still takes the 4-column reductions
    src = "8x8x1536 site at batch 170: just below the 8-column threshold"
    for op in ("bn_stats", "bn_bwd_reduce", "prelu_bwd", "bias_grad"):
        out.append(case(op, "below16Mi", src, N=170, HW=64, C=1536, per_sample=1))
    # D's stand-alone PReLUs (model.py discriminator / ops.resblock_down with strided_conv3: the block input and the
    # strided conv's output, channels 96 .. 1536; then ops.resblock and the last activation at 4x4x1536)
    for HW, C, add in ((4096, 96, "alias"), (1024, 192, "none"), (256, 384, "alias"), (64, 768, "sep"),
                       (16, 1536, "alias")):
        src = "D PReLU %d px x %d ch @ 256" % (HW, C)
        out.append(case("prelu_fwd", "d%dx%d" % (HW, C), src, N=256, HW=HW, C=C))
        out.append(case("prelu_bwd", "d%dx%d" % (HW, C), src, N=256, HW=HW, C=C, add=add))
    # bias gradients of D's convolutions (d_use_bias): dy of the same maps
    for HW, C in ((4096, 96), (1024, 192), (256, 384), (16, 1536)):
        out.append(case("bias_grad", "d%dx%d" % (HW, C), "D conv bias, dy %d px x %d ch @ 256" % (HW, C), N=256, HW=HW,
                        C=C))
    # self-attention's max pools (ops.self_attention_2 at 64x64: G ch 192 -> g 24 / h 96 channels, D ch 96 -> 12 / 48)
    for C in (24, 96, 12, 48):
        src = "self-attention max pool 64x64x%d @ 256" % C
        out.append(case("maxpool_fwd", "sa64x%d" % C, src, N=256, H=64, W=64, C=C))
        out.append(case("maxpool_bwd", "sa64x%d" % C, src, N=256, H=64, W=64, C=C))
    # D's global sum pool (model.py: global_sum_pooling of the 4x4x1536 features)
    out.append(case("sum_pool_fwd", "d16x1536", "D global sum pool 4x4x1536 @ 256", N=256, HW=16, C=1536))
    out.append(case("sum_pool_bwd", "d16x1536", "D global sum pool 4x4x1536 @ 256", N=256, HW=16, C=1536))
    # residual adds / gamma o + x of the attention blocks (device scalar) and the sums of forked gradients
    for n, dev, src in ((256 * 4096 * 192, True, "G attention gamma o + x, 64x64x192 @ 256"),
                        (256 * 4096 * 96, True, "D attention gamma o + x, 64x64x96 @ 256"),
                        (256 * 16 * 1536, False, "D resblock residual add 4x4x1536 @ 256"),
                        (256 * 16384 * 96, False, "forked gradient sum 128x128x96 @ 256")):
        out.append(case("lincomb", "n%d" % n, src, n=n, sa_dev=dev))
    # the attention gamma's gradient <o, dy>
    for n in (256 * 4096 * 192, 256 * 4096 * 96):
        out.append(case("dot", "n%d" % n, "attention gamma gradient <o, dy>, %d elements" % n, n=n))
    # bf16 <-> fp32 at the trunk's ends (ops._resident_out of the 4x4x1536 input; the image layers)
    out.append(case("cast", "f32->bf16", "G trunk input 4x4x1536 @ 256", n=256 * 16 * 1536, xdt=F32, ydt=BF16))
    out.append(case("cast", "bf16->f32", "D features 4x4x1536 @ 256", n=256 * 16 * 1536, xdt=BF16, ydt=F32))
    return out


# small shapes: (N, HW, C, what the shape is for)
EDGE = ((2, 5, 3, "C = 3 (the image: D's first PReLU, G_logit's gradient), 10 rows < one block, one-column kernels"),
        (3, 1, 6, "C = 6 (the split image), HW = 1"),
        (2, 7, 12, "C = 12: C % 4 == 0, C % 8 != 0"),
        (2, 9, 20, "C = 20: C % 4 == 0, C % 8 != 0"),
        (3, 64, 24, "C / 8 = 3 does not divide 256 (the shape of test_typed_elementwise_kernels_match_fp32_kernels)"),
        (2, 33, 8, "C / 8 = 1"),
        (4, 33, 200, "C / 8 = 25: the x8 grid is rounded up to a multiple of 25 blocks"),
        (2, 37, 776, "C / 8 = 97 (prime), more columns than half a block"),
        (256, 16, 24, "HW = 16 with N = 256: a 4x4 map at the production batch"))
EDGE_MAXPOOL = ((2, 2, 6, 3), (1, 4, 2, 6), (2, 6, 4, 12), (3, 8, 8, 24), (2, 4, 4, 200), (1, 2, 2, 776))


def _edge():
    out = []
    k = 0
    for N, HW, C, why in EDGE:
        tag = "%dx%dx%d" % (N, HW, C)
        for xdt, ydt in PAIRS:
            p = "%s/%s" % ("fb"[xdt], "fb"[ydt])
            for per_sample in (0, 1):
                for alpha in (False, True):
                    kw = dict(N=N, HW=HW, C=C, xdt=xdt, ydt=ydt, per_sample=per_sample, alpha=alpha, small=True)
                    nm = "%s %s ps%d a%d" % (tag, p, per_sample, int(alpha))
                    out.append(case("bn_fwd", nm, why, **kw))
                    out.append(case("bn_bwd_reduce", nm, why, **kw))
                    out.append(case("bn_bwd_dx", nm + " add-" + ADD[k % 3], why, add=ADD[k % 3], **kw))
                    k += 1
            kw = dict(N=N, HW=HW, C=C, xdt=xdt, ydt=ydt, small=True)
            out.append(case("prelu_fwd", "%s %s" % (tag, p), why, **kw))
            for add in ADD:
                out.append(case("prelu_bwd", "%s %s add-%s" % (tag, p, add), why, add=add, dalpha=add != "sep", **kw))
            out.append(case("prelu_bwd", "%s %s dalpha only" % (tag, p), why, add="null-dx", **kw))
        for dt in (BF16, F32):
            kw = dict(N=N, HW=HW, C=C, xdt=dt, ydt=dt, small=True)
            for op in ("bn_stats", "bias_grad", "sum_pool_fwd", "sum_pool_bwd"):
                out.append(case(op, "%s %s" % (tag, "fb"[dt]), why, **kw))
    for N, H, W, C in EDGE_MAXPOOL:
        for dt in (BF16, F32):
            for data in ("randn", "ties"):
                kw = dict(N=N, H=H, W=W, C=C, xdt=dt, ydt=dt, data=data, small=True)
                nm = "%dx%dx%dx%d %s %s" % (N, H, W, C, "fb"[dt], data)
                out.append(case("maxpool_fwd", nm, "C = %d, %d x %d map" % (C, H, W), **kw))
                out.append(case("maxpool_bwd", nm, "C = %d, %d x %d map" % (C, H, W), **kw))
    # every bf16 activation pointer 8 bytes off a 16-byte boundary: all-bf16 calls with C % 4 == 0 below 16 Mi
    # elements, for which the header guarantees 8-byte accesses - the x8 forms must fall back to the 4-column kernels
    for N, HW, C in ((3, 64, 24), (4, 33, 200), (2, 7, 12)):
        why = "bf16 pointers at 8 mod 16 bytes, C = %d" % C
        kw = dict(N=N, HW=HW, C=C, align=8, small=True)
        nm = "%dx%dx%d +8B" % (N, HW, C)
        out.append(case("bn_stats", nm, why, **kw))
        out.append(case("bias_grad", nm, why, **kw))
        out.append(case("sum_pool_fwd", nm, why, **kw))
        out.append(case("sum_pool_bwd", nm, why, **kw))
        out.append(case("prelu_fwd", nm, why, **kw))
        for i, add in enumerate(ADD):
            out.append(case("prelu_bwd", nm + " add-" + add, why, add=add, **kw))
            ps, al = (i + 1) // 2, i != 1           # (0, PReLU), (1, none), (1, PReLU)
            out.append(case("bn_fwd", nm + " ps%d a%d" % (ps, al), why, per_sample=ps, alpha=al, **kw))
            out.append(case("bn_bwd_reduce", nm + " ps%d a%d" % (ps, al), why, per_sample=ps, alpha=al, **kw))
            out.append(case("bn_bwd_dx", nm + " add-" + add, why, per_sample=(i + 1) % 2, alpha=i != 0, add=add, **kw))
    out.append(case("maxpool_fwd", "3x8x8x24 +8B", "bf16 pointers at 8 mod 16 bytes", N=3, H=8, W=8, C=24, align=8,
                    data="ties", small=True))
    out.append(case("maxpool_bwd", "3x8x8x24 +8B", "bf16 pointers at 8 mod 16 bytes", N=3, H=8, W=8, C=24, align=8,
                    data="ties", small=True))
    out.append(case("lincomb", "n4608 +8B", "bf16 pointers at 8 mod 16 bytes", n=4608, align=8, small=True))
    out.append(case("dot", "n4608 +8B", "bf16 pointers at 8 mod 16 bytes", n=4608, align=8, small=True))
    # the x8 grid cap: 49152 rows x 25 column groups = 1.2 M items > 4096 blocks x 256 threads, so threads take a second
    # grid-stride step, of 4100 * 256 / 25 = 41984 rows - more than ten samples of 4096 pixels
    why = "x8 grid cap: second grid-stride step, row step 41984 > HW = 4096, C / 8 = 25"
    kw = dict(N=12, HW=4096, C=200, small=True)
    out.append(case("bn_fwd", "12x4096x200 ps1", why, per_sample=1, **kw))
    out.append(case("bn_fwd", "12x4096x200 ps0", why, alpha=False, **kw))
    out.append(case("bn_bwd_dx", "12x4096x200 ps1 add-alias", why, per_sample=1, add="alias", **kw))
    out.append(case("bn_bwd_dx", "12x4096x200 ps0 add-sep", why, add="sep", alpha=False, **kw))
    out.append(case("prelu_fwd", "12x4096x200", why, **kw))
    out.append(case("prelu_bwd", "12x4096x200 add-alias", why, add="alias", **kw))
    # data-driven cases
    out.append(case("bn_stats", "8x64x24 mean 8 +- 0.5", "variance accuracy: |mean| = 16 sigma", N=8, HW=64, C=24,
                    data="mean8", small=True))
    out.append(case("bn_stats", "8x64x20 mean 8 +- 0.5 f32", "variance accuracy: |mean| = 16 sigma", N=8, HW=64, C=20,
                    data="mean8", xdt=F32, ydt=F32, small=True))
    out.append(case("bn_stats", "64x1024x24 mean 8 +- 0.5", "variance accuracy over 65536 rows, 128 blocks", N=64,
                    HW=1024, C=24, data="mean8", small=True))
    for C in (24, 12, 3):
        kw = dict(N=4, HW=256, C=C, data="zeros", small=True)
        why = "exact zeros in ~1 % of the positions: slope alpha / 2"
        out.append(case("prelu_fwd", "4x256x%d zeros" % C, why, **kw))
        out.append(case("prelu_bwd", "4x256x%d zeros" % C, why, **kw))
        out.append(case("prelu_bwd", "4x256x%d zeros add-alias" % C, why, add="alias", **kw))
    # the thin slope-gradient path of an fp32 / fp32 bg_prelu_bwd(_t): C <= 4 and >= 65536 rows (the PReLU of the image) -
    # 256 blocks x 256 threads that own whole pixels, 4 in flight, instead of the column reduction
    for rows, C, both, why in ((65535, 3, False, "one row short of the thin path: the column reduction"),
                               (65536, 1, False, "first thin shape, one grid stride: the tail loop only"),
                               (65536, 3, False, "first thin shape, one grid stride: the tail loop only"),
                               (65536, 4, False, "first thin shape, one grid stride: the tail loop only"),
                               (4 * 65536 + 1000, 3, False, "thin path: the unrolled loop, then the tail"),
                               (65536, 3, True, "thin path: the dx and the dalpha launch of one call")):
        out.append(case("prelu_bwd", "thin %dx%d f/f %s" % (rows, C, "dx + dalpha" if both else "dalpha only"), why,
                        N=1, HW=rows, C=C, xdt=F32, ydt=F32, add="none" if both else "null-dx", small=True))
    # bg_lincomb_t / bg_dot_t / bg_cast: n % 8 == 4, the device scalar (host sa poisoned), b == NULL, fp32, a second
    # grid-stride step of the x8 form (n > 2048 blocks x 256 threads x 8)
    for dt in (BF16, F32):
        for n in (4, 2052, 4608):
            for dev in (False, True):
                for b in (True, False):
                    nm = "n%d %s dev%d b%d" % (n, "fb"[dt], int(dev), int(b))
                    out.append(case("lincomb", nm, "n %% 8 == %d, sa_dev %d, b %d" % (n % 8, dev, b), n=n, xdt=dt, ydt=dt,
                                    sa_dev=dev, b=b, small=True))
            out.append(case("dot", "n%d %s" % (n, "fb"[dt]), "n %% 8 == %d" % (n % 8), n=n, xdt=dt, ydt=dt, small=True))
    for n in (6, 4 * 65536 + 3):        # fp32 through bg_dot alone: bg_dot_t refuses n % 4 != 0
        out.append(case("dot", "n%d f bg_dot" % n, "n %% 4 == %d: the scalar tail (and 2 blocks' worth of groups)" % (n % 4),
                        n=n, xdt=F32, ydt=F32, small=True))
    out.append(case("lincomb", "n5242884 dev1", "second grid-stride step of the x8 form... n % 8 == 4: 4-element form",
                    n=5 * (1 << 20) + 4, sa_dev=True, small=True))
    out.append(case("lincomb", "n5242880 dev1", "second grid-stride step of the x8 form", n=5 * (1 << 20), sa_dev=True,
                    small=True))
    out.append(case("dot", "n5242880", "more than 512 blocks' worth: grid-stride + per-block partials", n=5 * (1 << 20),
                    small=True))
    for xdt, ydt in PAIRS:
        for n in (3, 4099, 65536):
            out.append(case("cast", "n%d %s->%s" % (n, "fb"[xdt], "fb"[ydt]), "n %% 4 == %d" % (n % 4), n=n, xdt=xdt,
                            ydt=ydt, small=True))
    return out


CASES = _production() + _edge()


def cases(op=None, small=None):
    return [c for c in CASES if (op is None or c["op"] == op) and (small is None or c["small"] == small)]


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
POISON = 1.0e30        # the host scalar of a bg_lincomb_t call that passes sa_dev


def _act(shape, gen, dev, dt, data="randn"):
    """bf16-representable activations in the storage type dt."""
    if data == "mean8":
        t = 8.0 + 0.5 * torch.randn(shape, generator=gen, device=dev)
    elif data == "ties":             # multiples of 0.5 in [-2, 2]: most 2 x 2 windows tie (+ 0.0: no negative zero)
        t = torch.round(torch.randn(shape, generator=gen, device=dev).clamp(-1, 1) * 4) / 2 + 0.0
    else:
        t = torch.randn(shape, generator=gen, device=dev)
        if data == "zeros":
            t = t * (torch.rand(shape, generator=gen, device=dev) >= 0.01)
    return t.to(torch.bfloat16).to(dt)


def _par(shape, gen, dev, loc=0.0, scale=1.0, uniform=False):
    """Generic fp32 parameters (not bf16-representable)."""
    r = torch.rand(shape, generator=gen, device=dev) if uniform else torch.randn(shape, generator=gen, device=dev)
    return (loc + scale * r).float()


def make_inputs(c, dev, gen):
    """The call's input tensors in their storage types.  Activations as [N, HW, C] ([N, H, W, C] for the max pool,
    flat for lincomb / dot / cast)."""
    op, N, HW, C = c["op"], c["N"], c["HW"], c["C"]
    xdt, ydt = tdt(c["xdt"]), tdt(c["ydt"])
    i = {}
    if op in ("lincomb", "dot", "cast"):
        n = c["n"]
        if op == "cast":             # fp32 sources are generic: the narrowing cast must round to nearest even
            i["x"] = _par((n,), gen, dev) if xdt == torch.float32 else _act((n,), gen, dev, xdt)
            return i
        i["a"] = _act((n,), gen, dev, xdt)
        i["b"] = _act((n,), gen, dev, xdt) if (c["b"] or op == "dot") else None
        if op == "lincomb":
            i["s"] = _par((1,), gen, dev, 0.7, 0.2)
            i["sb"] = float(_par((1,), gen, dev, -0.4, 0.2))
        else:
            i["out0"] = _par((1,), gen, dev)
        return i
    if op in ("maxpool_fwd", "maxpool_bwd"):
        H, W = c["H"], c["W"]
        i["x"] = _act((N, H, W, C), gen, dev, xdt, c["data"])
        if op == "maxpool_bwd":
            i["dy"] = _act((N, H // 2, W // 2, C), gen, dev, xdt)
        return i
    if op == "sum_pool_bwd":
        i["dy"] = _act((N, C), gen, dev, torch.float32)
        return i
    i["x"] = _act((N, HW, C), gen, dev, xdt, c["data"])
    if op == "bn_stats":
        i["sums0"] = _act((2 * C,), gen, dev, torch.float64)
    if op in ("bn_bwd_reduce", "bn_bwd_dx", "prelu_bwd"):
        i["dy"] = _act((N, HW, C), gen, dev, ydt)
    if op in ("bn_fwd", "bn_bwd_reduce", "bn_bwd_dx"):
        i["mean"] = _par((C,), gen, dev, 0.0, 0.5)
        i["rstd"] = _par((C,), gen, dev, 0.5, 1.0, uniform=True)
        gshape = (N, C) if c["per_sample"] else (C,)
        i["gamma"] = _par(gshape, gen, dev, 1.0, 0.3)
        i["beta"] = _par(gshape, gen, dev, 0.0, 0.5)
    if op in ("bn_fwd", "bn_bwd_reduce", "bn_bwd_dx", "prelu_fwd", "prelu_bwd"):
        i["alpha"] = _par((C,), gen, dev, -0.1, 0.5, uniform=True) if c["alpha"] else None
    if op == "bn_bwd_dx":
        i["cm"] = _par((2 * C,), gen, dev, 0.0, 0.1)
    if op in ("bn_bwd_dx", "prelu_bwd"):
        i["add"] = _act((N, HW, C), gen, dev, xdt) if c["add"] in ("sep", "alias") else None
    if op == "prelu_bwd":
        i["dalpha0"] = _act((C,), gen, dev, torch.float32)
    return i


# ------------------------------------------------------------------------------------------
# the check of one call's outputs
# ------------------------------------------------------------------------------------------
def _img_chunks(N, per_image):
    step = max(1, CHUNK // max(per_image, 1))
    return [slice(a, min(N, a + step)) for a in range(0, N, step)]


def _ps(v, per_sample, sl):
    if v.dim() == 3:
        return v[sl]
    return v[sl][:, None, :] if per_sample else v


def check(c, i, out, rec):
    """Compare the outputs ``out`` (name -> tensor in the storage type) of case c on inputs i with the references, image
    chunk by image chunk: rec.gate(label, got, ref, E) / rec.exact(label, got, want).  -> (ambiguous elements, outputs
    they are counted against)."""
    op, N, HW, C, ps = c["op"], c["N"], c["HW"], c["C"], c["per_sample"]
    namb = 0
    if op == "cast":
        x, y = i["x"], out["y"]
        if y.dtype == torch.float32:                    # widening or copying: bit-exact
            rec.exact("cast", y, x.float())
        else:                                           # narrowing: E = 0, so exactly RNE(x)
            for a in range(0, x.numel(), CHUNK):
                xs = x[a:a + CHUNK].double()
                rec.gate("cast", y[a:a + CHUNK], xs, torch.zeros_like(xs))
        return 0, y.numel()
    if op == "lincomb":
        s = float(i["s"])
        for a in range(0, c["n"], CHUNK):
            sl = slice(a, a + CHUNK)
            r = lincomb(i["a"][sl], s, None if i["b"] is None else i["b"][sl], i["sb"])
            rec.gate("y", out["y"][sl], r["ref"], r["E"])
        return 0, c["n"]
    if op == "dot":
        ref = i["out0"].double().clone()
        A = ref.abs()
        for a in range(0, c["n"], CHUNK):
            p = i["a"][a:a + CHUNK].double() * i["b"][a:a + CHUNK].double()
            ref, A = ref + p.sum(), A + p.abs().sum()
        rec.gate("out", out["out"], ref, R.bound(A, c["n"]))
        return 0, 1
    if op == "maxpool_fwd":
        rec.exact("y", out["y"], maxpool_fwd(i["x"]))
        return 0, out["y"].numel()
    if op == "maxpool_bwd":
        for sl in _img_chunks(N, c["H"] * c["W"] * C):
            rec.exact("dx", out["dx"][sl], maxpool_bwd(i["x"][sl], i["dy"][sl]))
        return 0, out["dx"].numel()
    if op == "sum_pool_bwd":
        want = i["dy"].to(out["dx"].dtype)[:, None, :].expand(N, HW, C)
        rec.exact("dx", out["dx"], want)
        return 0, out["dx"].numel()
    x = i["x"]
    chunks = _img_chunks(N, HW * C)
    if op == "sum_pool_fwd":
        for sl in chunks:
            xs = x[sl].double()
            rec.gate("y", out["y"][sl], xs.sum(1), R.bound(xs.abs().sum(1), HW))
        return 0, N * C
    if op in ("bn_stats", "bias_grad") or (op == "prelu_bwd" and c["dalpha"]):
        # column sums over all N * HW rows of terms that are exact in fp32
        rows = N * HW
        if op == "bn_stats":
            ref, A = i["sums0"].double().clone(), i["sums0"].double().abs()
        elif op == "bias_grad":
            ref = torch.zeros(C, dtype=D64, device=x.device)
            A = torch.zeros_like(ref)
        else:
            ref, A = i["dalpha0"].double().clone(), i["dalpha0"].double().abs()
        for sl in chunks:
            xs = x[sl].double().reshape(-1, C)
            if op == "bn_stats":
                s1, a1 = colsum(xs)
                s2, a2 = colsum(xs * xs)
                ref, A = ref + torch.cat([s1, s2]), A + torch.cat([a1, a2])
            elif op == "bias_grad":
                s1, a1 = colsum(xs)
                ref, A = ref + s1, A + a1
            else:
                s1, a1 = colsum(i["dy"][sl].double().reshape(-1, C) * xs.clamp(max=0))
                ref, A = ref + s1, A + a1
        key = {"bn_stats": "sums", "bias_grad": "db", "prelu_bwd": "dalpha"}[op]
        rec.gate(key, out[key], ref, R.bound(A, rows))
        if op != "prelu_bwd":
            return 0, ref.numel()
    if op == "prelu_fwd":
        for sl in chunks:
            r = prelu_fwd(x[sl], i["alpha"])
            rec.gate("y", out["y"][sl], r["ref"], r["E"])
        return 0, N * HW * C
    if op == "prelu_bwd":
        if c["add"] != "null-dx":
            for sl in chunks:
                r = prelu_bwd(x[sl], i["dy"][sl], i["alpha"], None if i["add"] is None else i["add"][sl])
                rec.gate("dx", out["dx"][sl], r["ref"], r["E"])
        return 0, N * HW * C
    mean, rstd, alpha = i["mean"], i["rstd"], i["alpha"]
    for sl in chunks:
        ga, be = _ps(i["gamma"], ps, sl), _ps(i["beta"], ps, sl)
        if op == "bn_fwd":
            r = bn_fwd(x[sl], mean, rstd, ga, be, alpha)
            key = "y"
        elif op == "bn_bwd_dx":
            r = bn_bwd_dx(x[sl], i["dy"][sl], mean, rstd, ga, be, alpha, i["cm"], None if i["add"] is None
                          else i["add"][sl])
            key = "dx"
        else:
            r = bn_bwd_reduce(x[sl], i["dy"][sl], mean, rstd, ga, be, alpha)
            rec.gate("part", out["part"][:, sl], r["ref"], r["E"])
            namb += r["namb"]
            continue
        got = out[key][sl]
        ref, E = select(got, r)
        rec.gate(key, got, ref, E)
        if r.get("amb") is not None:
            namb += int(r["amb"].sum())
    return namb, N * HW * C


def describe(c):
    return "%s[%s]" % (c["op"], c["name"])


def takes_wide(c):
    """Whether the call's column reduction takes the 8-column form (all-bf16, C % 8 == 0, >= 16 Mi elements)."""
    return c["xdt"] == BF16 and c["ydt"] == BF16 and c["C"] % 8 == 0 and numel(c) >= WIDE_MIN


assert all(not (c["align"] and (takes_wide(c) or c["C"] % 4 or c["xdt"] != BF16 or c["ydt"] != BF16)) for c in CASES)
