"""float64 references, error bounds and the case table of the fp32 "glue" entry points of csrc/elementwise.hip that had no
gate of their own: the batch-norm finalisers (bg_bn_finalize, bg_bn_population, bg_bn_bwd_finalize), batch
renormalisation (bg_renorm_coeffs, bg_renorm_affine_fwd / _bwd), the 2x2 box kernels (bg_box2_down / _up), the small
elementwise family (bg_axpby, bg_add, bg_scale_add, bg_scale_dev, bg_tanh_fwd / _bwd), bg_pad_channels and
bg_weight_pack.

Test helper, not product code.  The pattern of tests/loss_ref.py, whose two arithmetics it reuses:

* references - each formula is written ONCE, in the order of operations ``include/biggan_hip.h`` documents, over an
  arithmetic class: ``Ref`` (float64 values, each carrying an absolute bound on the error of its fp32 counterpart - the
  same expression on absolute values, times the count of roundings) gives the reference and its bound, ``Sim`` (fp32)
  the simulated kernel of tests/test_glue_gate.py.  ``Ref`` is ``weight_ref.Fe`` with the exact scalings, clamps and
  selections these formulas need; rsqrtf, sqrtf and the division take RSQRT_U, SQRT_U and DIV_U of tests/weight_ref.py.
  Never anything a kernel returned.  Acceptance is ``launch_replay.gate``, which adds the final rounding of the stored
  value (2^-24 |ref|) itself.
* the finalisers take the fp64 ``sums`` THE TEST SUPPLIES.  ``sums[C + c] / count - (sums[c] / count)^2`` is evaluated in
  exact rational arithmetic (``fractions.Fraction``), so the reference has no cancellation of its own, whatever the ratio
  |mean| / sigma.  The kernel's fp64 steps enter in units u = 2^-53 of ``S2/n + m^2``: m = S / n carries one
  rounding, m m three (twice m's, one of its own: 3 u m^2), S2 / n one (u S2/n), the difference one (u |var|) -
  u (3 m^2 + S2/n + |var|), at most four units of S2/n + m^2 (a fused multiply-add saves one).  It reaches rstd through
  rsqrt as 0.5 rstd / (var + eps) (evaluated as the exact spread rsqrt(arg - e) - rsqrt(arg), which is that to first
  order and an upper bound beyond).  The clamp of a negative variance is 1-Lipschitz: it adds nothing.
* bg_bn_bwd_finalize accumulates in fp64 (an fp32 x fp32 product is exact in fp64): 2 (N + 4) units of 2^-53 of the
  sum of absolute values - N additions of the kernel, as many of the reference, the division by count - and the final
  cast.
* routing is bit-exact: bg_box2_up with scale 1 or 0.25, the per-sample copies of bg_bn_bwd_finalize, bg_pad_channels
  modes 0 - 2 (the split's residual x - bf16(x) is exactly representable), bg_weight_pack, moving statistics at momentum 1
  and running statistics at update = 0.  bf16 roundings are torch's round-to-nearest-even cast.
* ``tanhf`` takes a measured allowance, TANH_U units of 2^-24 relative error.  Measured on an MI355X with a stand-alone
  program (not part of the repository; compiled with the library's flags, -O3 -std=c++17 for gfx950) against the device's
  float64 tanh, exhaustively over EVERY fp32 argument +-[2^-30, 88] - which covers the library's internal breakpoints -
  and +-0 (returned with their signs): worst 2.4860 units, at x = 0.63521409; below 2^-2 at most 1.08, from 2 on at most
  0.59, from 16 on exact.  Doubled and rounded up.  The simulated kernel uses the
  correctly rounded tanh (float64 tanh rounded to fp32).
* CASES - the table both test modules walk: the smallest shapes at which each kernel can go wrong, and one "second trip"
  case per kernel form (``ew_grid`` caps the grid at 2048 blocks of 256, so the grid-stride loop runs twice from 524 289
  work items on).
* MUTATIONS - one-line variants of the simulated kernel; each fails the gate on at least one row of the table.
"""
import math
import struct
from fractions import Fraction

import torch

from tests import launch_replay as R
from tests.loss_ref import U64, Ref, RefD, Sim, SimD
from tests.weight_ref import DIV_U, RSQRT_U, SQRT_U, f32r          # noqa: F401  (DIV_U, SQRT_U: used through Ref)

U32 = R.U32
D64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
AMBIGUITY_CAP = 0.0          # no output of this table has a discontinuity: clips and clamps are continuous
ERR_ARG = 1
NAN = float("nan")
TANH_U = 5.0                 # tanhf: measured 2.4860 (at x = 0.63521409, just above the library's switch at 0.625)
EXPF_U = 2.9                 # expf (the GLU's sigmoid in the composed BnGluFn case): measured 1.4108 the same way,
                             # exhaustively over +-[2^-30, 87] (normal results on both sides), worst at x = -42.93
GRID_CAP = 2048 * 256        # work items of one trip of a grid-stride loop
SENTINEL_F32 = struct.unpack("<f", bytes([R.SENTINEL] * 4))[0]      # what lies behind a guarded buffer, read as fp32


# ------------------------------------------------------------------------------------------
# helpers over the two arithmetics
# ------------------------------------------------------------------------------------------
def const(ar, x, like):
    return ar(torch.tensor(float(x), dtype=D64 if not ar.sim else F32, device=like.device))


def rsqrt(x):
    """rsqrtf: the argument's error through the exact spread (first order: 0.5 r e / arg), RSQRT_U units of its own."""
    if x.sim:
        return Sim(x.v.rsqrt())
    r = x.v.rsqrt()
    return Ref(r, ((x.v - x.e).clamp_min(1e-300).rsqrt() - r) + RSQRT_U * U32 * r)


def clip(x, lo, hi):
    """fminf(fmaxf(x, lo), hi) with exact fp32 limits: 1-Lipschitz."""
    if x.sim:
        return Sim(torch.minimum(torch.maximum(x.v, torch.tensor(lo, dtype=F32)), torch.tensor(hi, dtype=F32)))
    return Ref(x.v.clamp(lo, hi), x.e)


def maxc(a, b):
    if a.sim:
        return Sim(torch.maximum(a.v, b.v + torch.zeros_like(a.v)))
    return Ref(torch.maximum(a.v, b.v + torch.zeros_like(a.v)), torch.maximum(a.e, b.e + torch.zeros_like(a.e)))


def tanh(x):
    if x.sim:
        return Sim(x.v.double().tanh().float())
    r = x.v.tanh()
    return Ref(r, TANH_U * U32 * r.abs() + x.e)


def scaled(x, s):
    """s * x for an fp32 scalar s: exact for a power of two (1, 0.25), one rounding otherwise."""
    m, _ = math.frexp(abs(s)) if s else (0.5, 0)
    if s == 0.0 or m == 0.5:
        return x.exact(s)
    return x * s


def trunc_bf16(t):
    """The bf16 conversion by truncation (a mutation): the low 16 bits dropped."""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(F32).to(BF16)


def to_bf16(t, mut=None):
    return trunc_bf16(t) if mut == "bf16 conversion by truncation" else t.to(BF16)


# ------------------------------------------------------------------------------------------
# batch-norm finalisers
# ------------------------------------------------------------------------------------------
def exact_stats(sums, count, C):
    """Per channel, in exact rational arithmetic on the fp64 sums: mean, variance (unclamped) and the absolute-value form
    3 m^2 + S2/n + |var| the kernel's fp64 roundings are charged on -> three float64 tensors [C]."""
    s = sums.detach().cpu().tolist()
    n = Fraction(count)
    ms, vs, As = [], [], []
    for c in range(C):
        m = Fraction(s[c]) / n
        q = Fraction(s[C + c]) / n
        v = q - m * m
        ms.append(float(m))
        vs.append(float(v))
        As.append(float(3 * m * m + abs(q) + abs(v)))
    dev = sums.device
    return (torch.tensor(ms, dtype=D64, device=dev), torch.tensor(vs, dtype=D64, device=dev),
            torch.tensor(As, dtype=D64, device=dev))


def _stats_head(ar, i, C, mut):
    """(mean, var) as the kernels form them in double -> (m rounded to fp32, m as stored, var in double (clamped))."""
    s, n = i["sums"], i["count"]
    if i.get("_head") is not None:          # a composed chain: the statistics arrive with the bound of their sums
        return i["_head"]
    if ar.sim:
        m = s[:C] / n
        if mut == "variance subtraction in fp32":
            m32 = m.float()
            var = ((s[C:] / n).float() - m32 * m32).double()
        else:
            var = s[C:] / n - m * m
        if mut != "negative variance left unclamped":
            var = var.clamp_min(0)
        return Sim(m.float()), SimD(var)
    m64, v64, A = exact_stats(s, n, C)
    return Ref(m64, U64 * m64.abs()), Ref(v64.clamp_min(0), U64 * A)


def bn_finalize(ar, c, i, mut=None):
    C = c["C"]
    n = i["count"]
    like = i["sums"]
    m, var = _stats_head(ar, i, C, mut)
    eps, mom = const(ar, i["eps"], like), const(ar, i["momentum"], like)
    mf = m.to32()
    out = {"mean": m, "rstd": rsqrt(var.to32() + eps)}
    one = const(ar, 1.0, like)
    keep, new = (one - mom, mom) if mut == "momentum and 1 - momentum swapped" else (mom, one - mom)
    still = i["momentum"] == 1.0 and not ar.sim                 # the moving statistics must not move by a bit
    if c["mm"]:
        out["moving_mean"] = i["mm0"] if still else ar.of(i["mm0"]) * keep + mf * new
    if c["mv"]:
        unb = bool(c["unbiased"])
        if mut == "Bessel factor on the wrong side":
            unb = not unb
        vv = var
        if unb and n > 1:
            k = n / (n - 1.0)
            vv = SimD(var.v * k) if ar.sim else Ref(var.v * k, var.e * k + 2 * U64 * var.v * k)
        out["moving_var"] = i["mv0"] if still else ar.of(i["mv0"]) * keep + vv.to32() * new
    return out


def bn_population(ar, c, i, mut=None):
    like = i["pop_var"]
    return {"mean": i["pop_mean"], "rstd": rsqrt(ar.of(i["pop_var"]) + const(ar, i["eps"], like))}


def _sum64(t, A, N):
    """A kernel sum of N fp64 terms against the reference's own: 2 (N + 4) units of 2^-53 of the absolute sum."""
    return Ref(t, 2.0 * (N + 4) * U64 * A)


def bn_bwd_finalize(ar, c, i, mut=None):
    """dgamma / dbeta (per sample: copies of planes 1 / 0; shared: sums over N), dalpha = sum of plane 2,
    cm = (sum_n gamma_n part0_n, sum_n gamma_n part1_n) / count."""
    N, C, ps = c["N"], c["C"], c["per_sample"]
    part, gamma, count = i["part"], i["gamma"], i["count"]
    p0, p1, p2 = part[0].double(), part[1].double(), part[2].double()
    if mut == "planes 0 and 1 swapped":
        p0, p1 = p1, p0
    g = gamma.double() if ps else gamma.double()[None, :].expand(N, C)
    if mut == "shared gamma indexed per sample" and not ps:
        ext = torch.cat([gamma.double().reshape(-1), torch.full((N * C,), SENTINEL_F32, dtype=D64, device=gamma.device)])
        g = ext[:N * C].reshape(N, C)
    if mut == "per-sample gamma indexed as shared" and ps:
        g = gamma.double()[0:1].expand(N, C)
    live = N
    if mut == "sample loop dropping the tail past the last multiple of 4":
        live = N // 4 * 4
    if mut == "sample loop dropping the tail past the last multiple of 32":
        live = N // 32 * 32
    sl = slice(0, live)
    div = float(N) if mut == "cm divided by N" else count

    def total(t):
        return t[sl].sum(0), t[sl].abs().sum(0)
    wrap = (lambda v, A: Sim(v.float())) if ar.sim else (lambda v, A: _sum64(v, A, N))
    out = {}
    if ps:
        db, dg = p0.float().clone(), p1.float().clone()
        if ar.sim and live < N:
            db[live:], dg[live:] = NAN, NAN
        out["dbeta"], out["dgamma"] = db, dg
    else:
        out["dbeta"], out["dgamma"] = wrap(*total(p0)), wrap(*total(p1))
    if c["dalpha"]:
        out["dalpha"] = wrap(*total(p1 if mut == "dalpha taken from plane 1" else p2))
    (a0, A0), (a1, A1) = total(g * p0), total(g * p1)
    out["cm"] = wrap(torch.cat([a0, a1]) / div, torch.cat([A0, A1]) / div)
    return out


# ------------------------------------------------------------------------------------------
# batch renormalisation
# ------------------------------------------------------------------------------------------
def renorm_coeffs(ar, c, i, mut=None):
    """The header's formulas, everything after the double-precision mean / variance in fp32.  -> r, d, the running
    statistics and the fade-in weight after the call; "_raw": the unclipped (r, d) of the reference."""
    C, siv, upd = c["C"], c["scale_is_var"], c["update"]
    if mut == "scale_is_var branches swapped":
        siv = 1 - siv
    like = i["sums"]
    m, var = _stats_head(ar, i, C, mut)
    m, var = m.to32(), var.to32()
    K = lambda x: const(ar, x, like)                 # noqa: E731
    eps, one = K(i["eps"]), K(1.0)
    sigma = (var + eps).sqrt()
    rm, rs = ar.of(i["ref_mean0"]), ar.of(i["ref_scale0"])
    w = K(1.0 if i.get("weight0") is None else float(i["weight0"]))
    decay, fade = K(i["decay"]), K(i["fade"])
    new_w = w * fade + one * (one - fade)
    new_rm, new_rs = rm * decay + m * (one - decay), rs * decay + (var if siv else sigma) * (one - decay)
    if mut == "r and d from the updated running statistics" and upd:
        rm, rs = new_rm, new_rs
    w_used = w
    if mut == "*weight updated before it is read" and upd and i.get("weight0") is not None:
        late = (torch.arange(C, device=like.device) >= 256)
        w_used = ar(torch.where(late, new_w.v, w.v + torch.zeros(C, dtype=w.v.dtype, device=like.device)))
    sigma_ref = (rs + eps).sqrt() if siv else maxc(rs, eps.sqrt())
    omw = one - w_used
    sigma_w = w_used * sigma_ref + omw * sigma
    mean_w = w_used * rm + omw * m
    r_raw, d_raw = sigma / sigma_w, (m - mean_w) / sigma_w
    d_lo = 0.0 if mut == "d clipped to [0, dmax]" else -i["dmax"]
    out = {"r": clip(r_raw, i["rmin"], i["rmax"]), "d": clip(d_raw, d_lo, i["dmax"])}
    if upd:
        out["ref_mean"], out["ref_scale"] = new_rm, new_rs
    else:
        out["ref_mean"], out["ref_scale"] = i["ref_mean0"], i["ref_scale0"]
    if i.get("weight0") is not None:
        out["weight"] = new_w.reshape(1) if upd else i["weight0"]
    if not ar.sim:
        out["_raw"] = (r_raw.v, d_raw.v)
    return out


def renorm_affine_fwd(ar, c, i, mut=None):
    g, b, r, d = (ar.of(i[k]) for k in ("gamma", "beta", "r", "d"))
    return {"gamma_eff": r * g, "beta_eff": b + d * g}


def renorm_affine_bwd(ar, c, i, mut=None):
    ge, be, r, d = (ar.of(i[k]) for k in ("dgamma_eff", "dbeta_eff", "r", "d"))
    if mut == "the d dbeta_eff term dropped":
        return {"dgamma": r * ge}
    return {"dgamma": r * ge + d * be}


# ------------------------------------------------------------------------------------------
# 2x2 box kernels
# ------------------------------------------------------------------------------------------
def box2_down(ar, c, i, mut=None):
    """y[n, ho, wo] = scale ((x[2ho, 2wo] + x[2ho, 2wo + 1]) + (x[2ho + 1, 2wo] + x[2ho + 1, 2wo + 1]))."""
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    x = i["x"]
    if mut == "H and W swapped in box2":
        x = x.reshape(N, W, H, C)
    X = ar.of(x)
    a, b = X[:, 0::2, 0::2], X[:, 0::2, 1::2]
    cc, d = X[:, 1::2, 0::2], X[:, 1::2, 1::2]
    if mut == "a box2 tap read twice":
        d = cc
    y = scaled((a + b) + (cc + d), f32r(c["scale"]))
    return {"y": y.reshape(N, H // 2, W // 2, C)}


def box2_up(ar, c, i, mut=None):
    """y[n, 2hi + a, 2wi + b] = scale x[n, hi, wi]; bit-exact for scale 1 and 0.25."""
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    x = i["x"]
    if mut == "H and W swapped in box2":
        x = x.reshape(N, W, H, C)
    rep = lambda t: t.repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(N, 2 * H, 2 * W, C)     # noqa: E731
    s = f32r(c["scale"])
    if s in (1.0, 0.25):
        return {"y": rep(x * s)}
    return {"y": scaled(ar.of(x), s).route(rep)}


# ------------------------------------------------------------------------------------------
# the small elementwise family
# ------------------------------------------------------------------------------------------
def _tail_skipped(o, y0, n, mut):
    """The n % 4 tail left as the output buffer held it (a mutation of the float4 kernels)."""
    if mut != "n % 4 tail skipped" or n % 4 == 0:
        return o
    v = o.v.clone()
    v[n // 4 * 4:] = NAN if y0 is None else y0[n // 4 * 4:].to(v.dtype)
    return type(o)(v)


def axpby(ar, c, i, mut=None):
    """y = a x + b y; y is not read when b == 0.  x_is_y: the in-place form y = a y + b y."""
    a, b = i["a"], i["b"]
    y0 = i.get("y0")
    X = ar.of(y0 if c["alias"] else i["x"])
    if b == 0.0 and mut != "y read when b == 0":
        y = X * a
    else:
        Y = ar.of(y0) if y0 is not None else ar(torch.full_like(X.v, NAN))
        y = X * a + Y * b
    return {"y": _tail_skipped(y, y0, c["n"], mut)}


def add(ar, c, i, mut=None):
    a = ar.of(i["y0"] if c["alias"] else i["a"])
    return {"y": _tail_skipped(a + ar.of(i["b"]), i.get("y0"), c["n"], mut)}


def scale_add(ar, c, i, mut=None):
    g = const(ar, float(i["gamma"]), i["x"])
    return {"y": _tail_skipped(g * ar.of(i["o"]) + ar.of(i["x"]), None, c["n"], mut)}


def scale_dev(ar, c, i, mut=None):
    s = const(ar, float(i["s"]), i["s"])
    return {"y": s * ar.of(i["y0"] if c["alias"] else i["x"])}


def tanh_fwd(ar, c, i, mut=None):
    return {"y": tanh(ar.of(i["x"]))}


def tanh_bwd(ar, c, i, mut=None):
    """dx = dy (1 - y y): three roundings on |dy| (1 + y^2)."""
    y, dy = ar.of(i["y"]), ar.of(i["dy"])
    one = const(ar, 1.0, i["dy"])
    if mut == "1 - y in place of 1 - y^2":
        return {"dx": dy * (one - y)}
    return {"dx": dy * (one - y * y)}


# ------------------------------------------------------------------------------------------
# channel padding, weight packing
# ------------------------------------------------------------------------------------------
def tdt(code):
    return BF16 if code else F32


def pad_channels(ar, c, i, mut=None):
    """[outer, Cs, inner] -> [outer, Cd, inner]: mode 0 zero fill / truncate, 1 split (bf16 value | residual), 2 duplicate,
    3 fold dst[c] = src[c] + src[Cd + c].  Modes 0 - 2 are exact; the fold is one fp32 sum, then the store's rounding."""
    Cs, Cd, mode = c["Cs"], c["Cd"], c["mode"]
    src = i["src"]
    outer, inner = src.shape[0], src.shape[2]
    ddt = tdt(c["ddt"])
    v = src.float()
    cast = (lambda t: t) if ddt == F32 else (lambda t: to_bf16(t, mut))
    if mode == 3:
        if mut == "fold adding c + Cs":
            flat = torch.cat([v.reshape(-1), torch.full((Cs * inner,), SENTINEL_F32, device=v.device)])
            o = torch.arange(outer, device=v.device)[:, None, None] * Cs * inner
            ch = torch.arange(Cd, device=v.device)[None, :, None]
            ix = o + (ch + Cs) * inner + torch.arange(inner, device=v.device)[None, None, :]
            second = flat[ix]
        else:
            second = v[:, Cd:2 * Cd]
        if ar.sim:
            return {"dst": cast(v[:, :Cd] + second)}
        s = v[:, :Cd].double() + second.double()
        return {"dst": Ref(s, torch.zeros_like(s) if ddt == F32 else U32 * s.abs())}
    dst = torch.zeros((outer, Cd, inner), dtype=F32, device=v.device)
    k = min(Cs, Cd)
    if mode == 0:
        dst[:, :k] = v[:, :k]
    elif mode == 2:
        dst[:, :Cs] = v
        dst[:, Cs:2 * Cs] = v
    else:
        hi = to_bf16(v, mut).float()
        dst[:, :Cs] = hi
        dst[:, Cs:2 * Cs] = (hi - to_bf16(hi, mut).float()) if mut == "split residual from the rounded value" else v - hi
    return {"dst": cast(dst)}


def weight_pack(ar, c, i, mut=None):
    """pack_p = bf16(w) [taps][R][Cc], pack_t = its per-tap transpose [taps][Cc][R]: both bit-exact."""
    w = i["w"]
    p = to_bf16(w, mut)
    t = p.transpose(1, 2).contiguous()
    if mut == "pack_t not transposed":
        t = p.reshape(t.shape).clone()
    if mut == "last partial-tile column dropped" and c["Cc"] % 64:
        p, t = p.clone(), t.clone()
        p[:, :, c["Cc"] // 64 * 64 + (c["Cc"] % 64 - 2):] = NAN
        t[:, c["Cc"] // 64 * 64 + (c["Cc"] % 64 - 2):, :] = NAN
    return {"pack_p": p, "pack_t": t}


# ------------------------------------------------------------------------------------------
# the composed chain of functional.BnActFn (tests/test_gpu_glue_kernels.py runs it through the wrapper)
# ------------------------------------------------------------------------------------------
def _nsum(x, N):
    """The fp64 sum over the N samples of bg_bn_bwd_finalize, of terms that carry their own bounds."""
    return Ref(x.v.sum(0), x.e.sum(0) + 2.0 * (N + 4) * U64 * x.v.abs().sum(0))


def composed_bn_act(x, dy, gamma, beta, alpha, eps, mode, st):
    """Bounds of BnActFn forward and backward, stage by stage, each result entering the next with its bound: the column
    sums of bg_bn_stats (fp32 partials over all rows), bg_bn_finalize | bg_bn_population, for ``renorm``
    bg_renorm_coeffs and bg_renorm_affine_fwd, the apply + PReLU pass, the per-sample reductions of the backward,
    bg_bn_bwd_finalize, bg_renorm_affine_bwd and the input gradient (formulas and rounding counts of the apply and
    reduce kernels: tests/elementwise_ref.py).  mode: 'shared' | 'cond' | 'renorm' | 'infer'; st: the state the call
    starts from.  -> name -> Ref, and "_amb": elements within their own bound of the PReLU kink."""
    N, H, W, C = x.shape
    HW, rows = H * W, N * H * W
    n = float(rows)
    dev = x.device
    X, DY = Ref.of(x.reshape(N, HW, C)), Ref.of(dy.reshape(N, HW, C))
    ps = gamma.dim() == 2
    ga, be = Ref.of(gamma), Ref.of(beta)
    A = Ref.of(alpha)
    out = {}
    dummy = torch.zeros(2 * C, dtype=D64, device=dev)
    r = d = None
    if mode != "infer":
        Xr = X.reshape(rows, C)
        m = RefD.of(Xr.sum(0, rows)) / n
        var = (RefD.of((Xr * Xr).sum(0, rows)) / n - m * m).relu()
        head = (Ref(m.v, m.e), Ref(var.v, var.e))
        f = bn_finalize(Ref, dict(C=C, mm=1, mv=1, unbiased=st["unbiased"]),
                        dict(sums=dummy, count=n, eps=eps, momentum=st["momentum"], mm0=st["mm0"], mv0=st["mv0"],
                             _head=head))
        mean, rstd = f["mean"].to32(), f["rstd"]
        out.update(moving_mean=f["moving_mean"], moving_var=f["moving_var"])
        if mode == "renorm":
            rr = renorm_coeffs(Ref, dict(C=C, scale_is_var=st["scale_is_var"], update=1),
                               dict(sums=dummy, count=n, eps=eps, ref_mean0=st["ref_mean0"], ref_scale0=st["ref_scale0"],
                                    weight0=st["weight0"], rmin=st["rmin"], rmax=st["rmax"], dmax=st["dmax"],
                                    decay=st["decay"], fade=st["fade"], _head=head))
            r, d = rr["r"], rr["d"]
            out.update(ref_mean=rr["ref_mean"], ref_scale=rr["ref_scale"], weight=rr["weight"], _raw=rr["_raw"])
            a = renorm_affine_fwd(Ref, None, dict(gamma=ga, beta=be, r=r, d=d))
            ga, be = a["gamma_eff"], a["beta_eff"]
    else:
        p = bn_population(Ref, None, dict(pop_mean=st["mm0"], pop_var=st["mv0"], eps=eps))
        mean, rstd = Ref.of(p["mean"]), p["rstd"]
    gb = ga.reshape(N, 1, C) if ps else ga
    bb = be.reshape(N, 1, C) if ps else be
    # forward: y = act(x (rs ga) + (be - mu (rs ga)))
    inv = rstd * gb
    pre = X * inv + (bb - mean * inv)
    out["y"] = pre.where(pre.v > 0, A * pre).reshape(N, H, W, C)
    amb = int((pre.v.abs() <= pre.e).sum())
    # backward, pass 1: pre recomputed as ((x - mu) rs) ga + be
    xh = (X - mean) * rstd
    pre2 = xh * gb + bb
    amb += int((pre2.v.abs() <= pre2.e).sum())
    one = torch.ones((), dtype=D64, device=dev)
    slope = torch.where(pre2.v > 0, one, torch.where(pre2.v < 0, A.v, 0.5 * A.v))
    g = DY * Ref(slope + torch.zeros_like(DY.v))
    part0, part1 = g.sum(1, HW), (g * xh).sum(1, HW)
    part2 = (DY * pre2.where(pre2.v < 0, 0.0)).sum(1, HW)
    # bg_bn_bwd_finalize
    G = ga if ps else Ref(ga.v[None, :].expand(N, C), ga.e[None, :].expand(N, C))
    dbeta, dgamma = (part0, part1) if ps else (_nsum(part0, N), _nsum(part1, N))
    out["dalpha"] = _nsum(part2, N)
    if mode == "infer":
        zero = torch.zeros(C, dtype=D64, device=dev)
        m1 = m2 = Ref(zero)
    else:
        m1 = (_nsum(RefD.of(G) * RefD.of(part0), N) / n).to32()
        m2 = (_nsum(RefD.of(G) * RefD.of(part1), N) / n).to32()
    out["dbeta"] = dbeta
    if mode == "renorm":
        out["dgamma"] = renorm_affine_bwd(Ref, None, dict(dgamma_eff=dgamma.to32(), dbeta_eff=dbeta.to32(), r=r, d=d))[
            "dgamma"]
    else:
        out["dgamma"] = dgamma
    # pass 2: dx = rs (g ga - m1 - xh m2)
    out["dx"] = (rstd * (g * gb - m1 - xh * m2)).reshape(N, H, W, C)
    out["_amb"] = amb
    return out


def _sigmoid(g):
    """1.f / (1.f + expf(-g)) of csrc/recon.hip: expf's measured allowance, the sum, the division."""
    ev = (-g.v).exp()
    e = Ref(ev, ev * torch.expm1(g.e) + EXPF_U * U32 * ev)
    one = Ref(torch.ones((), dtype=D64, device=g.v.device))
    return one / (one + e)


def composed_bn_glu(x, dy, gamma, beta, eps, st):
    """Bounds of BnGluFn forward and backward (x [N, H, W, 2C], shared gamma / beta [2C]): bg_bn_stats and
    bg_bn_finalize as in composed_bn_act, then the formulas of csrc/recon.hip - pre = x (rs ga) + (be - mu (rs ga)) for
    both halves, y = pre0 sigmoid(pre1); backward g0 = dy s, g1 = dy pre0 s (1 - s), the row sums of g and g xh (fp32
    within a row segment, fp64 across the nseg segments in bg_bn_bwd_finalize: any order and association of an fp32 sum
    over all rows bounds both), cm = gamma (sum g, sum g xh) / count, dx = rs (g ga - m1 - xh m2)."""
    N, H, W, C2 = x.shape
    C, rows = C2 // 2, N * H * W
    n = float(rows)
    X, DY = Ref.of(x.reshape(rows, C2)), Ref.of(dy.reshape(rows, C))
    ga, be = Ref.of(gamma), Ref.of(beta)
    m = RefD.of(X.sum(0, rows)) / n
    var = (RefD.of((X * X).sum(0, rows)) / n - m * m).relu()
    f = bn_finalize(Ref, dict(C=C2, mm=1, mv=1, unbiased=st["unbiased"]),
                    dict(sums=torch.zeros(2 * C2, dtype=D64, device=x.device), count=n, eps=eps, momentum=st["momentum"],
                         mm0=st["mm0"], mv0=st["mv0"], _head=(Ref(m.v, m.e), Ref(var.v, var.e))))
    mean, rstd = f["mean"].to32(), f["rstd"]
    inv = rstd * ga
    pre = X * inv + (be - mean * inv)
    xh = (X - mean) * rstd
    sg = _sigmoid(pre[:, C:])
    one = Ref(torch.ones((), dtype=D64, device=x.device))
    g = Ref.cat([DY * sg, DY * pre[:, :C] * sg * (one - sg)], 1)
    dbeta, dgamma = g.sum(0, rows), (g * xh).sum(0, rows)
    m1 = (RefD.of(ga) * RefD.of(dbeta) / n).to32()
    m2 = (RefD.of(ga) * RefD.of(dgamma) / n).to32()
    return dict(y=(pre[:, :C] * sg).reshape(N, H, W, C), dx=(rstd * (g * ga - m1 - xh * m2)).reshape(N, H, W, C2),
                dgamma=dgamma, dbeta=dbeta, moving_mean=f["moving_mean"], moving_var=f["moving_var"])


FORMULAS = dict(bn_finalize=bn_finalize, bn_population=bn_population, bn_bwd_finalize=bn_bwd_finalize,
                renorm_coeffs=renorm_coeffs, renorm_affine_fwd=renorm_affine_fwd, renorm_affine_bwd=renorm_affine_bwd,
                box2_down=box2_down, box2_up=box2_up, axpby=axpby, add=add, scale_add=scale_add, scale_dev=scale_dev,
                tanh_fwd=tanh_fwd, tanh_bwd=tanh_bwd, pad_channels=pad_channels, weight_pack=weight_pack)
OPS = tuple(FORMULAS)
ENTRY = {op: "bg_" + op for op in OPS}


def formula(c, i, ar, mut=None):
    """The outputs of case c on inputs i over arithmetic ``ar``: name -> Ref / Sim, or a tensor where the result is exact."""
    return FORMULAS[c["op"]](ar, c, i, mut)


def simulate(c, i, mut=None):
    """The simulated fp32 kernel (or one of its mutations) -> name -> tensor, as the entry point would leave its outputs."""
    out = {}
    for k, v in formula(c, i, Sim, mut).items():
        if k.startswith("_"):
            continue
        out[k] = v.v.float() if isinstance(v, Sim) else v
    return out


def check(c, i, out, rec):
    """Gate the outputs ``out`` (name -> tensor) of case c on inputs i: rec.gate(label, got, ref, E) for bounded
    outputs, rec.exact(label, got, want) for routing.  -> (0 sign-ambiguous elements, outputs counted)."""
    r = formula(c, i, Ref)
    r.pop("_raw", None)
    nout = 0
    if set(out) != set(r):
        rec.fail("outputs %s, reference %s" % (sorted(out), sorted(r)))
        return 0, 1
    for k, got in out.items():
        want = r[k]
        nout += got.numel()
        if isinstance(want, Ref):
            rec.gate(k, got, want.v.reshape(got.shape), want.e.reshape(got.shape))
        else:
            rec.exact(k, got, want.reshape(got.shape))
    return 0, nout


class Rec:
    """The callbacks of ``check`` for a test without a Runner: the failures and the worst err / bound."""

    def __init__(self):
        self.bad, self.worst = [], 0.0

    def gate(self, label, got, ref, E):
        ok, ratio, _, _, nbad = R.gate(got, ref, E)
        self.worst = max(self.worst, ratio)
        if not ok:
            self.bad.append("%s: %d outside the bound (worst %.3g)" % (label, nbad, ratio))

    def exact(self, label, got, want):
        want = want.to(got.dtype)
        if not torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)):
            self.bad.append("%s: not bit-exact" % label)

    def fail(self, msg):
        self.bad.append(msg)


# ------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------
BNF_C = (1, 5, 256, 257, 300)
BNF_ROWS = 1024
BWD_N = (1, 3, 4, 5, 31, 32, 33, 37, 256)
BWD_C = (1, 63, 64, 65, 96)
RENORM_C = (1, 255, 256, 257, 600)
RENORM_ROWS = 128
AFFINE_ROWS = (1, 3, 64)
AFFINE_C = (1, 5, 64)
BOX_C = (1, 3, 4, 6, 8, 12)
BOX_NHW = ((1, 2, 2), (2, 2, 6), (3, 6, 4), (1, 4, 2))
BOX_SCALES = (1.0, 0.25, 0.3)
EW_N = (1, 3, 4, 5, 1023, 1024, 1027)
BIG4 = 4 * GRID_CAP + 4099            # float4 kernels: n / 4 > 524 288, n % 4 = 3
BIG1 = GRID_CAP + 5715                # one element per thread, odd
SCALARS = (0.0, 0.37, -1.0)
PAD_PAIRS = {0: ((3, 8), (4, 8), (1, 8), (8, 3), (5, 16)),
             1: ((3, 8), (4, 8), (1, 8), (3, 6), (3, 16)),
             2: ((3, 8), (4, 8), (1, 8), (3, 6), (3, 16)),
             3: ((8, 3), (8, 4), (8, 1), (16, 8), (6, 3))}
PACK_TAPS = (1, 9, 16)
PACK_DIMS = (2, 8, 62, 64, 66, 130)


def case(op, name, origin, **kw):
    c = dict(op=op, name=name, origin=origin, exempt=())
    c.update(kw)
    return c


def pad_fast_form(c):
    """Whether bg_pad_channels takes a one-pixel-per-thread form on 16-byte aligned pointers."""
    if c["inner"] != 1 or c["sdt"] != 0:
        return False
    return (c["ddt"] == 1 and c["Cd"] == 8 and c["Cs"] <= 4 and c["mode"] != 3) or (
        c["mode"] == 3 and c["Cs"] == 8 and c["Cd"] <= 4)


def _cases():
    out = []
    k = 0
    for C in BNF_C:
        for mm in (0, 1):
            for mv in (0, 1):
                for unb in (0, 1):
                    mom = (0.0, 0.98, 1.0)[k % 3]
                    mult = (1, 2)[(k // 3) % 2]
                    out.append(case("bn_finalize", "C%d mm%d mv%d unb%d mom%g x%d" % (C, mm, mv, unb, mom, mult),
                                    "one thread per channel, 256 per block; count = %d rows" % mult, C=C, mm=mm, mv=mv,
                                    unbiased=unb, momentum=mom, mult=mult, rows=BNF_ROWS, off=k % 4,
                                    eps=(1e-5, 1e-3)[k % 2]))
                    k += 1
    out.append(case("bn_finalize", "C5 count 1 unbiased", "count = 1 with unbiased_moving_var: the count > 1 guard", C=5,
                    mm=1, mv=1, unbiased=1, momentum=0.98, mult=1, rows=1, off=0, eps=1e-5))
    for C in BNF_C:
        out.append(case("bn_population", "C%d" % C, "pop_var contains 0", C=C, eps=(1e-5, 1e-3)[C % 2]))
    k = 0
    for N in BWD_N:
        for C in BWD_C:
            out.append(case("bn_bwd_finalize", "N%d C%d ps%d da%d x%d" % (N, C, k % 2, (k // 2) % 2, (1, 3)[(k // 4) % 2]),
                            "sample loop in strides of 32 with 8 clamped loads, 64 channels per block", N=N, C=C,
                            per_sample=k % 2, dalpha=(k // 2) % 2, mult=(1, 3)[(k // 4) % 2], glu=False))
            k += 1
    out.append(case("bn_bwd_finalize", "N16 C24 BnGluFn", "BnGluFn: N = nseg, shared gamma, NULL dalpha, zero plane 2",
                    N=16, C=24, per_sample=0, dalpha=0, mult=1, glu=True))
    k = 0
    for C in RENORM_C:
        for siv in (0, 1):
            for wt in (None, 0.0, 0.3, 1.0):
                for upd in (0, 1):
                    out.append(case("renorm_coeffs", "C%d siv%d w%s upd%d" % (C, siv, wt, upd),
                                    "a single block looping by 256", C=C, scale_is_var=siv, weight=wt, update=upd,
                                    clipset=0, off=k % 6))
                    k += 1
    out.append(case("renorm_coeffs", "C257 dmax 0, rmin = rmax = 1", "degenerate clip ranges: r = 1, d = 0 exactly", C=257,
                    scale_is_var=1, weight=0.3, update=1, clipset=1, off=0))
    out.append(case("renorm_coeffs", "C5 dmax 0, rmin = rmax = 1, Keras", "degenerate clip ranges", C=5, scale_is_var=0,
                    weight=None, update=0, clipset=1, off=2))
    for op in ("renorm_affine_fwd", "renorm_affine_bwd"):
        for rows in AFFINE_ROWS:
            for C in AFFINE_C:
                out.append(case(op, "%dx%d" % (rows, C), "[rows, C] pair against per-channel r, d", rows=rows, C=C))
        out.append(case(op, "4099x129", "528 771 elements: the grid-stride loop's second trip", rows=4099, C=129))
    for op in ("box2_down", "box2_up"):
        for C in BOX_C:
            for N, H, W in BOX_NHW:
                for s in BOX_SCALES:
                    out.append(case(op, "%dx%dx%dx%d s%g" % (N, H, W, C, s), "VEC %d, non-square maps" % (1 if C % 4 else 4),
                                    N=N, H=H, W=W, C=C, scale=s))
        big = ((1, 364, 364, 64), (1, 840, 840, 3)) if op == "box2_down" else ((1, 182, 182, 64), (1, 420, 420, 3))
        for N, H, W, C in big:
            out.append(case(op, "%dx%dx%dx%d s0.3" % (N, H, W, C), "VEC %d: the grid-stride loop's second trip"
                            % (1 if C % 4 else 4), N=N, H=H, W=W, C=C, scale=0.3))
    for n in EW_N + (BIG4,):
        why = "n / 4 float4 items and an n %% 4 = %d tail%s" % (n % 4, ", second trip" if n == BIG4 else "")
        for a in (0.0, 1.0, 0.37):
            for b in (0.0, 1.0, -0.5):
                if n == BIG4 and (a, b) not in ((0.37, -0.5), (0.37, 0.0)):
                    continue
                out.append(case("axpby", "n%d a%g b%g" % (n, a, b), why, n=n, a=a, b=b, alias=False))
        out.append(case("axpby", "n%d in place" % n, "x == y, a = 0, b = 0.25: the averaging / loss-scaling call sites",
                        n=n, a=0.0, b=0.25, alias=True))
        out.append(case("add", "n%d" % n, why, n=n, alias=False))
        out.append(case("add", "n%d in place" % n, "a == y: the accumulation of fan-in gradients", n=n, alias=True))
        for s in SCALARS:
            if n == BIG4 and s != 0.37:
                continue
            out.append(case("scale_add", "n%d g%g" % (n, s), why, n=n, scalar=s))
    for n in EW_N + (BIG1,):
        for s in SCALARS:
            if n == BIG1 and s != 0.37:
                continue
            out.append(case("scale_dev", "n%d s%g" % (n, s), "one element per thread", n=n, scalar=s, alias=False))
        out.append(case("scale_dev", "n%d in place" % n, "y == x: the sigma^2 rescale of the Gram matrix", n=n, scalar=0.37,
                        alias=True))
    for op in ("tanh_fwd", "tanh_bwd"):
        out.append(case(op, "sweep", "+-2^e (1 + m), e in [-30, 4]; +-0; saturation up to +-88; breakpoints; odd n",
                        n=0, data="sweep"))
        out.append(case(op, "n1", "a single element", n=1, data="randn"))
        out.append(case(op, "n%d" % BIG1, "the grid-stride loop's second trip, odd n", n=BIG1, data="randn"))
    for mode in range(4):
        for sdt in (0, 1):
            for ddt in (0, 1):
                for inner in (1, 7):
                    for Cs, Cd in PAD_PAIRS[mode]:
                        c = case("pad_channels", "m%d %s%s %d->%d i%d" % (mode, "fb"[sdt], "fb"[ddt], Cs, Cd, inner), "",
                                 mode=mode, sdt=sdt, ddt=ddt, inner=inner, Cs=Cs, Cd=Cd, outer=300 if inner == 1 else 37,
                                 off4=False)
                        c["origin"] = "one-pixel-per-thread form" if pad_fast_form(c) else "generic kernel"
                        out.append(c)
                        if pad_fast_form(c):
                            out.append(dict(c, name=c["name"] + " +4B", off4=True,
                                            origin="source 4 bytes off: the generic kernel, the same bits"))
    out.append(case("pad_channels", "m1 fb 3->8 i1 big", "530 000 pixels: second trip of the one-pixel-per-thread form",
                    mode=1, sdt=0, ddt=1, inner=1, Cs=3, Cd=8, outer=530000, off4=False))
    out.append(case("pad_channels", "m3 ff 8->3 i1 big", "530 000 pixels: second trip of the fold form",
                    mode=3, sdt=0, ddt=0, inner=1, Cs=8, Cd=3, outer=530000, off4=False))
    out.append(case("pad_channels", "m1 fb 3->8 i7 big", "560 000 elements: second trip of the generic kernel",
                    mode=1, sdt=0, ddt=1, inner=7, Cs=3, Cd=8, outer=10000, off4=False))
    for taps in PACK_TAPS:
        for Rr in PACK_DIMS:
            for Cc in PACK_DIMS:
                out.append(case("weight_pack", "%dx%dx%d" % (taps, Rr, Cc), "64 x 64 tiles of one tap through LDS",
                                taps=taps, R=Rr, Cc=Cc))
    out.append(case("weight_pack", "16x768x768", "2304 tiles > 2048 blocks: a block's second tile", taps=16, R=768, Cc=768))
    return out


CASES = _cases()


def cases(op=None):
    return [c for c in CASES if op is None or c["op"] == op]


def describe(c):
    return "%s[%s]" % (c["op"], c["name"])


def numel(c):
    """Roughly the elements a case's buffers hold (to release the large ones before the next case)."""
    op = c["op"]
    if op in ("box2_down", "box2_up"):
        return 5 * c["N"] * c["H"] * c["W"] * c["C"]
    if op == "weight_pack":
        return 2 * c["taps"] * c["R"] * c["Cc"]
    if op == "pad_channels":
        return c["outer"] * (c["Cs"] + c["Cd"]) * c["inner"]
    if op in ("renorm_affine_fwd", "renorm_affine_bwd"):
        return 4 * c["rows"] * c["C"]
    return 3 * c.get("n", 0)


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
CLIPSETS = ((0.8, 1.25, 0.5), (1.0, 1.0, 0.0))     # (rmin, rmax, dmax)
NEG_VAR = 2                                         # channel pattern of the slightly negative fp64 variance
RATIO_6000 = 1                                      # channel pattern |mean| / sigma = 6000


def _rn(shape, gen, dev, scale=1.0, dtype=F32):
    return torch.randn(shape, generator=gen, device=dev, dtype=dtype) * scale


def _ru(shape, gen, dev):
    return torch.rand(shape, generator=gen, device=dev, dtype=F32)


def bn_sums(rows, C, off, mult, gen, dev):
    """fp64 sums of fp32 data [rows, C] as ``mult`` equal ranks deliver them, channel c of pattern (c + off) % 4:
    0: N(0, 1);  1: mean 300, sigma 0.05 (|mean| / sigma = 6000);  2: S = n v, S2 = n v^2 (1 - 2^-50): the fp64 variance
    comes out slightly negative;  3: mean -3, sigma 2.  -> (sums [2C], count, pattern [C])."""
    pat = (torch.arange(C, device=dev) + off) % 4
    mean = torch.tensor([0.0, 300.0, 0.0, -3.0], device=dev)[pat]
    std = torch.tensor([1.0, 0.05, 1.0, 2.0], device=dev)[pat]
    x = (_rn((rows, C), gen, dev) * std + mean).double()
    n = float(rows * mult)
    S, S2 = x.sum(0) * mult, (x * x).sum(0) * mult
    v = (1000.5 + torch.arange(C, device=dev, dtype=D64) * 0.25)
    neg = pat == NEG_VAR
    S = torch.where(neg, n * v, S)
    S2 = torch.where(neg, n * v * v * (1.0 - 2.0 ** -50), S2)
    return torch.cat([S, S2]), n, pat


def tanh_sweep(dev):
    """+-2^e (1 + m) for e in [-30, 4] and 64 mantissas each (both ends of the binade included), +-0, the saturated range
    up to +-88, and 33 consecutive fp32 values around each of the thresholds a tanhf implementation branches at."""
    m = torch.cat([torch.arange(62, dtype=D64) / 62.0, torch.tensor([2.0 ** -23, 1.0 - 2.0 ** -23], dtype=D64)])
    xs = [(2.0 ** e) * (1.0 + m) for e in range(-30, 5)]
    xs.append(torch.linspace(5.0, 88.0, 257, dtype=D64))
    for t in (2.0 ** -12, 0.25, 0.55, 0.625, 1.0, 8.0, 9.0, 9.0109, 10.0, 19.0625, 22.0):
        b = struct.unpack("<i", struct.pack("<f", t))[0]
        bits = torch.arange(b - 16, b + 17, dtype=torch.int32)
        xs.append(bits.view(F32).double())
    x = torch.cat(xs).float()
    x = torch.cat([x, -x, torch.tensor([0.0, -0.0])])
    if x.numel() % 2 == 0:
        x = torch.cat([x, torch.tensor([0.5])])
    return x.to(dev)


def make_inputs(c, dev, gen):
    op = c["op"]
    if op == "bn_finalize":
        C = c["C"]
        sums, n, pat = bn_sums(c["rows"], C, c["off"], c["mult"], gen, dev)
        i = dict(sums=sums, count=n, eps=f32r(c["eps"]), momentum=f32r(c["momentum"]), pattern=pat)
        if c["mm"]:
            i["mm0"] = _rn((C,), gen, dev)
        if c["mv"]:
            i["mv0"] = _ru((C,), gen, dev) + 0.5
        return i
    if op == "bn_population":
        C = c["C"]
        pv = _ru((C,), gen, dev) * 4.0
        pv[0] = 0.0
        return dict(pop_mean=_rn((C,), gen, dev), pop_var=pv, eps=f32r(c["eps"]))
    if op == "bn_bwd_finalize":
        N, C = c["N"], c["C"]
        part = _rn((3, N, C), gen, dev)
        if c["glu"]:
            part[2] = 0.0
        gamma = _rn((N, C) if c["per_sample"] else (C,), gen, dev) + 1.0
        return dict(part=part, gamma=gamma, count=float(N * c["mult"]))
    if op == "renorm_coeffs":
        C = c["C"]
        pat = (torch.arange(C, device=dev) + c["off"]) % 6
        mean = _rn((C,), gen, dev)
        std = _ru((C,), gen, dev) + 0.5
        x = (_rn((RENORM_ROWS, C), gen, dev) * std + mean).double()
        m, sd = x.mean(0), x.var(0, unbiased=False).sqrt()
        # patterns: 0 inside both ranges, 1 r below rmin, 2 r above rmax, 3 d above dmax, 4 d below -dmax, 5 tiny scale
        ksig = torch.tensor([1.1, 10.0, 0.05, 1.0, 1.0, 0.0], dtype=D64, device=dev)[pat]
        kmu = torch.tensor([0.1, 0.0, 0.0, -20.0, 20.0, 0.0], dtype=D64, device=dev)[pat]
        rsig = torch.where(pat == 5, torch.full_like(sd, 1e-4), ksig * sd)
        rmin, rmax, dmax = CLIPSETS[c["clipset"]]
        i = dict(sums=torch.cat([x.sum(0), (x * x).sum(0)]), count=float(RENORM_ROWS), eps=f32r(1e-5),
                 ref_mean0=(m + kmu * sd).float(), ref_scale0=(rsig * rsig if c["scale_is_var"] else rsig).float(),
                 rmin=f32r(rmin), rmax=f32r(rmax), dmax=f32r(dmax), decay=f32r(0.99), fade=f32r(0.999), pattern=pat)
        if c["weight"] is not None:
            i["weight0"] = torch.tensor([c["weight"]], dtype=F32, device=dev)
        return i
    if op in ("renorm_affine_fwd", "renorm_affine_bwd"):
        rows, C = c["rows"], c["C"]
        i = dict(r=_ru((C,), gen, dev) + 0.5, d=_rn((C,), gen, dev) * 0.3)
        names = ("gamma", "beta") if op == "renorm_affine_fwd" else ("dgamma_eff", "dbeta_eff")
        for k in names:
            i[k] = _rn((rows, C), gen, dev)
        return i
    if op in ("box2_down", "box2_up"):
        return dict(x=_rn((c["N"], c["H"], c["W"], c["C"]), gen, dev))
    if op == "axpby":
        n = c["n"]
        i = dict(a=f32r(c["a"]), b=f32r(c["b"]))
        if not c["alias"]:
            i["x"] = _rn((n,), gen, dev)
        if c["b"] != 0.0:
            i["y0"] = _rn((n,), gen, dev)
        return i
    if op == "add":
        n = c["n"]
        return dict(y0=_rn((n,), gen, dev), b=_rn((n,), gen, dev)) if c["alias"] else dict(a=_rn((n,), gen, dev),
                                                                                          b=_rn((n,), gen, dev))
    if op == "scale_add":
        n = c["n"]
        return dict(o=_rn((n,), gen, dev), x=_rn((n,), gen, dev), gamma=torch.tensor([c["scalar"]], dtype=F32, device=dev))
    if op == "scale_dev":
        n = c["n"]
        i = dict(s=torch.tensor([c["scalar"]], dtype=F32, device=dev))
        i["y0" if c["alias"] else "x"] = _rn((n,), gen, dev)
        return i
    if op == "tanh_fwd":
        return dict(x=tanh_sweep(dev) if c["data"] == "sweep" else _rn((c["n"],), gen, dev, 2.0))
    if op == "tanh_bwd":
        if c["data"] == "sweep":
            edge = torch.tensor([1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 0.0, -0.0], device=dev)
            y = torch.cat([edge.repeat(8), torch.tanh(_rn((975,), gen, dev, 2.0).double()).float()])
        else:
            y = torch.tanh(_rn((c["n"],), gen, dev, 2.0).double()).float()
        return dict(y=y, dy=_rn((y.numel(),), gen, dev))
    if op == "pad_channels":
        src = _rn((c["outer"], c["Cs"], c["inner"]), gen, dev)
        src.reshape(-1)[0] = 1.0 + 2.0 ** -8                      # a tie of the bf16 rounding (to even: 1.0)
        src.reshape(-1)[-1] = 1.0 + 3.0 * 2.0 ** -8               # and one that rounds up to even
        return dict(src=src.to(tdt(c["sdt"])))
    if op == "weight_pack":
        w = _rn((c["taps"], c["R"], c["Cc"]), gen, dev, 0.1)
        w.reshape(-1)[0] = 1.0 + 2.0 ** -8
        w.reshape(-1)[-1] = 1.0 + 3.0 * 2.0 ** -8
        return dict(w=w)
    raise KeyError(op)


# ------------------------------------------------------------------------------------------
# mutations: (what, op, predicate on the case that must expose it)
# ------------------------------------------------------------------------------------------
MUTATIONS = (
    ("variance subtraction in fp32", "bn_finalize", lambda c: c["C"] >= 5),
    ("Bessel factor on the wrong side", "bn_finalize", lambda c: c["mv"] and c["momentum"] != 1.0 and c["rows"] > 1),
    ("momentum and 1 - momentum swapped", "bn_finalize", lambda c: c["mm"] and c["momentum"] == 0.98),
    ("negative variance left unclamped", "bn_finalize", lambda c: c["C"] >= 5),
    ("sample loop dropping the tail past the last multiple of 4", "bn_bwd_finalize", lambda c: c["N"] % 4 != 0),
    ("sample loop dropping the tail past the last multiple of 32", "bn_bwd_finalize", lambda c: c["N"] % 32 != 0),
    ("shared gamma indexed per sample", "bn_bwd_finalize", lambda c: not c["per_sample"] and c["N"] > 1),
    ("per-sample gamma indexed as shared", "bn_bwd_finalize", lambda c: c["per_sample"] and c["N"] > 1),
    ("cm divided by N", "bn_bwd_finalize", lambda c: c["mult"] != 1),
    ("planes 0 and 1 swapped", "bn_bwd_finalize", lambda c: True),
    ("dalpha taken from plane 1", "bn_bwd_finalize", lambda c: c["dalpha"]),
    ("r and d from the updated running statistics", "renorm_coeffs",
     lambda c: c["update"] and c["weight"] in (0.3, 1.0, None) and c["clipset"] == 0 and c["C"] > 1),
    ("*weight updated before it is read", "renorm_coeffs",
     lambda c: c["update"] and c["weight"] == 0.3 and c["C"] > 256 and c["clipset"] == 0),
    ("scale_is_var branches swapped", "renorm_coeffs", lambda c: c["weight"] in (0.3, 1.0, None) and c["clipset"] == 0),
    ("d clipped to [0, dmax]", "renorm_coeffs", lambda c: c["weight"] in (0.3, 1.0, None) and c["C"] >= 255
     and c["clipset"] == 0),
    ("the d dbeta_eff term dropped", "renorm_affine_bwd", lambda c: True),
    ("H and W swapped in box2", "box2_down", lambda c: c["H"] != c["W"] and c["H"] > 2),
    ("H and W swapped in box2", "box2_up", lambda c: c["H"] != c["W"]),
    ("a box2 tap read twice", "box2_down", lambda c: True),
    ("y read when b == 0", "axpby", lambda c: c["b"] == 0.0 and not c["alias"]),
    ("n % 4 tail skipped", "axpby", lambda c: c["n"] % 4 != 0 and not c["alias"] and (c["a"], c["b"]) != (0.0, 1.0)),
    ("n % 4 tail skipped", "add", lambda c: c["n"] % 4 != 0),
    ("n % 4 tail skipped", "scale_add", lambda c: c["n"] % 4 != 0),
    ("split residual from the rounded value", "pad_channels", lambda c: c["mode"] == 1 and c["sdt"] == 0),
    ("fold adding c + Cs", "pad_channels", lambda c: c["mode"] == 3),
    ("bf16 conversion by truncation", "pad_channels", lambda c: c["sdt"] == 0 and (c["ddt"] == 1 or c["mode"] == 1)),
    ("bf16 conversion by truncation", "weight_pack", lambda c: True),
    ("pack_t not transposed", "weight_pack", lambda c: c["R"] != c["Cc"] or c["R"] > 2),
    ("last partial-tile column dropped", "weight_pack", lambda c: c["Cc"] % 64 != 0),
    ("1 - y in place of 1 - y^2", "tanh_bwd", lambda c: True),
)
