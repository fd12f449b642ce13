"""float64 references, error bounds and the case table of the kernels that decide what the networks are trained on:
DiffAugment, the hinge and general GAN losses, the class-label sigmoid cross-entropy (csrc/augment_loss.hip), the gradient
penalty and the second-order (tangent) kernels it needs (csrc/augment_loss.hip, csrc/elementwise.hip).

Test helper, not product code.  The pattern of tests/weight_ref.py:

* references - plain restatements of the formulas documented in ``include/biggan_hip.h`` and above the kernels, written
  ONCE over an arithmetic class and evaluated twice: over ``Ref`` (float64 values, each carrying an absolute bound on the
  error of its fp32 counterpart) for the reference and its bound, and over ``Sim`` (fp32 tensors, the kernel's order of
  operations) for the simulated kernel of tests/test_loss_gate.py.  The coefficient kernels of the batch-norm tangent work
  in double and round once at the end: ``RefD`` / ``SimD``.
* bounds - never anything a kernel returned.  ``Ref`` is the absolute-value expression A and the rounding count m in one:
  every fp32 product, sum, difference and quotient adds ``2^-24`` times the sum of the absolute values of its operands'
  terms (so a bound is m 2^-24 A for an elementwise chain of m roundings), the error of an operand is propagated with
  the absolute value of the partial derivative, and a reduction over K terms adds ``launch_replay.bound(A, K)`` on top of
  the terms' own errors.  Routing (translation, cutout, the max-pool gather, DiffAugment without the colour bit) is exact
  and compared bit for bit.
* the device functions take a measured allowance (units of 2^-24 relative error).  No document installed with ROCm
  states the accuracy of the native exponential, so it was measured once on an MI355X with a stand-alone program (not
  part of the repository) that evaluates ``__expf`` on 2^20 arguments spread over [-104, 0] (half uniform, half
  logarithmically towards 0) against ``exp`` in double, and ``log1pf`` on the results and on 2^20 arguments in (0, 1]:

      e = __expf(x):  |e - exp(x)| <= (2 |x| + C0) 2^-24 exp(x) + 2^-126

    - ``2 |x| 2^-24``: __expf is exp2(x * log2e) with the product formed in fp32.  log2e is rounded to fp32 (relative
      2^-24) and so is the product (2^-24): y = x log2e (1 + d), |d| <= 2 * 2^-24, and exp2(y) = exp(x) exp(x d) differs
      from exp(x) by |x d| <= 2 |x| 2^-24 in relative terms.  Measured: at most 64.3 units at x = -87.3, always below
      2 |x|.
    - ``C0 = 2``: the hardware exponential itself.  Measured worst of (relative error - 2 |x|) over the whole range:
      0.6852 units; worst relative error for |x| <= 1/4, where the first term vanishes: 0.9329 units.  C0 is twice the
      larger, rounded up.
    - ``2^-126`` (the smallest normal fp32): results below it are flushed to zero (all 88975 sampled arguments whose
      exact result is denormal returned 0).  ``Ref`` carries the floor as an absolute error, so it reaches every output
      multiplied by that output's scale factor.
    - ``LOG1P_U = 3``: log1pf, measured 1.0436 units worst; doubled and rounded up.
  sqrtf and the division take SQRT_U and DIV_U of tests/weight_ref.py (measured there: correctly rounded).
* sign-dependent outputs follow the "ambiguous element" rule of ``elementwise_ref.select``: where the deciding quantity
  is computed in fp32 (ra-hinge's ``real - m_f``, ``L - flood``) an element within its own bound of the kink may match
  either branch.  Every case here with such an output has fewer than 10^4 elements, so AMBIGUITY_CAP allows none: the
  inputs are drawn with a margin from every kink, ``check`` only counts, and tests/test_loss_gate.py asserts the count is
  zero.  ``max(e, 0)`` of the penalty's ``lp`` clamp and the hinge VALUES are continuous in their argument: the
  propagated error covers them and they are never ambiguous.  Kinks are planted only where the argument is the stored
  value (real == 1, fake == -1 of the non-relativistic hinge, x == 0 of the PReLU tangent slope, +-0 ties of the gather).
* CASES - the table both test modules walk: the smallest shapes that reach each code path.
"""
import math

import torch

from tests import elementwise_ref as EW
from tests import launch_replay as R
from tests.weight_ref import DIV_U, SQRT_U, f32r

U32 = R.U32
U64 = 2.0 ** -53
TINY = 2.0 ** -126           # smallest normal fp32: the flush-to-zero floor
D64 = torch.float64
F32 = torch.float32
AMBIGUITY_CAP = EW.AMBIGUITY_CAP
C0 = 2.0                     # the native exponential: measured 0.9329 (see above)
LOG1P_U = 3.0                # log1pf: measured 1.0436
ERR_ARG = 1
ERR_UNSUPPORTED = 3
NAN = float("nan")


# ------------------------------------------------------------------------------------------
# the two arithmetics
# ------------------------------------------------------------------------------------------
class Ref:
    """float64 value v with an absolute bound e on the error of its fp32 counterpart (first order, A-form: a sum's own
    rounding is charged on |a| + |b|, not on |a + b|)."""
    U = U32
    DIV = DIV_U
    sim = False

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @classmethod
    def of(cls, t):
        """An input tensor (exact), or an earlier stage's result with its bound (the composed chains)."""
        if isinstance(t, Ref):
            return cls(t.v, t.e)
        return None if t is None else cls(t.double())

    def lift(self, o):
        if isinstance(o, Ref):
            return o
        return type(self)(torch.tensor(float(o), dtype=D64, device=self.v.device))

    def floor(self, r):
        """A product in the denormal range may be flushed to zero (or keeps fewer bits): the smallest normal, absolute."""
        return torch.where(r.abs() < TINY, torch.full_like(r, TINY), torch.zeros_like(r)) * (r != 0)

    def __mul__(self, o):
        o = self.lift(o)
        r = self.v * o.v
        return type(self)(r, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + self.U * r.abs() + self.floor(r))

    __rmul__ = __mul__

    def exact(self, k):
        """Times a power of two or a sign: no rounding."""
        return type(self)(self.v * k, self.e * abs(k))

    def __neg__(self):
        return self.exact(-1.0)

    def _addsub(self, o, sign):
        o = self.lift(o)
        return type(self)(self.v + sign * o.v, self.e + o.e + self.U * (self.v.abs() + o.v.abs()))

    def __add__(self, o):
        return self._addsub(o, 1.0)

    def __sub__(self, o):
        return self._addsub(o, -1.0)

    def __truediv__(self, o):
        o = self.lift(o)
        r = self.v / o.v
        return type(self)(r, (self.e + r.abs() * o.e) / o.v.abs() + self.DIV * self.U * r.abs())

    def sum(self, dim, K, keepdim=False):
        """An fp32 reduction over K terms in any order and association."""
        return type(self)(self.v.sum(dim, keepdim=keepdim),
                          R.bound(self.v.abs().sum(dim, keepdim=keepdim), K) * (self.U / U32)
                          + self.e.sum(dim, keepdim=keepdim))

    def relu(self):
        return type(self)(self.v.clamp_min(0), self.e)

    def abs(self):
        return type(self)(self.v.abs(), self.e)

    def sqrt(self):
        r = self.v.clamp_min(0).sqrt()
        spread = (self.v.clamp_min(0) + self.e).sqrt() - (self.v - self.e).clamp_min(0).sqrt()
        return type(self)(r, spread + SQRT_U * self.U * r)

    def exp(self):
        """__expf of a non-positive argument: (2 |x| + C0) 2^-24 relative, the flush-to-zero floor, the argument's error."""
        r = self.v.exp()
        return type(self)(r, r * torch.expm1(self.e) + (2.0 * self.v.abs() + C0) * U32 * r + TINY)

    def expneg(self):
        """__expf(-fabsf(x))."""
        return type(self)(-self.v.abs(), self.e).exp()

    def log1p(self):
        """log1pf of a value in [0, 1]: |d log1p / dx| <= 1."""
        r = self.v.log1p()
        return type(self)(r, self.e + LOG1P_U * U32 * r)

    def where(self, cond, o):
        o = self.lift(o)
        return type(self)(torch.where(cond, self.v, o.v), torch.where(cond, self.e, o.e + torch.zeros_like(self.e)))

    def masked(self, cond):
        """Exactly +0 where cond is false."""
        z = torch.zeros_like(self.v)
        return type(self)(torch.where(cond, self.v, z), torch.where(cond, self.e, z))

    def div_double(self, k, cast=True):
        """(double) x / k, rounded to fp32 again (cast) or kept in double."""
        r = self.v / k
        return Ref(r, self.e / abs(k) + (U32 * r.abs() if cast else 0.0))

    def to32(self):
        """A double-precision result rounded to fp32."""
        return Ref(self.v, self.e + U32 * self.v.abs())

    def __getitem__(self, ix):
        return type(self)(self.v[ix], self.e[ix])

    def reshape(self, *s):
        return type(self)(self.v.reshape(*s), self.e.reshape(*s))

    def route(self, fn):
        """An exact re-indexing of the elements (values and bounds alike)."""
        return type(self)(fn(self.v), fn(self.e))

    @staticmethod
    def cat(xs, dim=0):
        return type(xs[0])(torch.cat([x.v for x in xs], dim), torch.cat([x.e for x in xs], dim))


class RefD(Ref):
    """Double-precision arithmetic of a kernel: the same bookkeeping in units of 2^-53."""
    U = U64
    DIV = 1.0

    def floor(self, r):
        return torch.zeros_like(r)


class Sim:
    """The fp32 evaluation: what a correct kernel computes, up to the order of its sums."""
    dt = F32
    sim = True
    e = None

    def __init__(self, v):
        self.v = v

    @classmethod
    def of(cls, t):
        if isinstance(t, Sim):
            return cls(t.v.to(cls.dt))
        return None if t is None else cls(t.to(cls.dt))

    def lift(self, o):
        if isinstance(o, Sim):
            return o
        return type(self)(torch.tensor(float(o), dtype=self.dt, device=self.v.device))

    def __mul__(self, o):
        return type(self)(self.v * self.lift(o).v)

    __rmul__ = __mul__

    def exact(self, k):
        return type(self)(self.v * k)

    def __neg__(self):
        return type(self)(-self.v)

    def __add__(self, o):
        return type(self)(self.v + self.lift(o).v)

    def __sub__(self, o):
        return type(self)(self.v - self.lift(o).v)

    def __truediv__(self, o):
        return type(self)(self.v / self.lift(o).v)

    def sum(self, dim, K, keepdim=False):
        return type(self)(self.v.sum(dim, keepdim=keepdim))

    def relu(self):
        return type(self)(self.v.clamp_min(0))

    def abs(self):
        return type(self)(self.v.abs())

    def sqrt(self):
        return type(self)(self.v.sqrt())

    def exp(self):
        return type(self)(self.v.exp())

    def expneg(self):
        return type(self)((-self.v.abs()).exp())

    def log1p(self):
        return type(self)(self.v.log1p())

    def where(self, cond, o):
        return type(self)(torch.where(cond, self.v, self.lift(o).v + torch.zeros_like(self.v)))

    def masked(self, cond):
        return type(self)(torch.where(cond, self.v, torch.zeros_like(self.v)))

    def div_double(self, k, cast=True):
        r = self.v.double() / k
        return Sim(r.float()) if cast else SimD(r)

    def to32(self):
        return Sim(self.v.float())

    def __getitem__(self, ix):
        return type(self)(self.v[ix])

    def reshape(self, *s):
        return type(self)(self.v.reshape(*s))

    def route(self, fn):
        return type(self)(fn(self.v))

    @staticmethod
    def cat(xs, dim=0):
        return type(xs[0])(torch.cat([x.v for x in xs], dim))


class SimD(Sim):
    dt = D64


def double_of(ar):
    return SimD if ar.sim else RefD


def from_double(ar, v64):
    """A quantity the kernel computes in double from exact inputs and rounds to fp32: one rounding."""
    return Sim(v64.float()) if ar.sim else Ref(v64, U32 * v64.abs())


def const(ar, x, dev):
    return ar(torch.tensor(float(x), dtype=D64 if not ar.sim else ar.dt, device=dev))


def seq_sum(x, dim):
    """v0 + v1 + ... along dim in index order, as a thread's register loop adds them (0 + v0 is exact)."""
    n = x.v.shape[dim]
    ix = [slice(None)] * x.v.dim()

    def at(k):
        ix[dim] = slice(k, k + 1)
        return x[tuple(ix)]
    acc = at(0)
    for k in range(1, n):
        acc = acc + at(k)
    return acc


# ------------------------------------------------------------------------------------------
# DiffAugment
# ------------------------------------------------------------------------------------------
def da_params(S):
    """(shift, cutout size, exclusive maximum of the cutout offsets) of image size S (DiffAugment_tf.py:43, 56-58)."""
    shift = int(S * 0.125 + 0.5)
    cs = int(S * 0.5 + 0.5)
    return shift, cs, S + (1 - cs % 2)


def da_cut_mask(S, o_x, o_y, mut=None):
    """[N, S, S] bool, True where the cutout zeroes: rows [max(0, o - cs/2), min(S - 1, o - cs/2 + cs - 1)], columns
    likewise."""
    cs = da_params(S)[1]
    ar = torch.arange(S, device=o_x.device)[None, :]

    def axis(o):
        lo = (o.long() - cs // 2).clamp_min(0)[:, None]
        hi = (o.long() - cs // 2 + cs - 1).clamp_max(S - 1)[:, None]
        if mut == "cutout upper bound off by one":
            return (ar >= lo) & (ar < hi)
        return (ar >= lo) & (ar <= hi)
    return axis(o_x)[:, :, None] & axis(o_y)[:, None, :]


def da_route(t, S, policy, t_x, t_y, o_x, o_y, backward=False, mut=None):
    """-> (routed tensor, live mask [N, S, S]).  Forward: out[n, i, j] = t[n, i + t_x, j + t_y], zero where the source
    lies outside the image or (i, j) is cut out.  Backward, its transpose: out[n, p, q] = t[n, p - t_x, q - t_y], zero
    where (p - t_x, q - t_y) lies outside or is cut out."""
    N = t.shape[0]
    dev = t.device
    ar = torch.arange(S, device=dev)[None, :]
    live = torch.ones((N, S, S), dtype=torch.bool, device=dev)
    out = t
    ii = ar.expand(N, S)
    jj = ar.expand(N, S)
    if policy & 2:
        sg = -1 if backward and mut != "translation sign not flipped in the backward" else 1
        ii = ar + sg * t_x.long()[:, None]
        jj = ar + sg * t_y.long()[:, None]
        live = ((ii >= 0) & (ii < S))[:, :, None] & ((jj >= 0) & (jj < S))[:, None, :]
    ic, jc = ii.clamp(0, S - 1), jj.clamp(0, S - 1)
    b = torch.arange(N, device=dev)[:, None, None]
    if policy & 2:
        out = t[b, ic[:, :, None], jc[:, None, :]]
    if policy & 4:
        cut = da_cut_mask(S, o_x, o_y, mut)
        if backward:
            cut = cut[b, ic[:, :, None], jc[:, None, :]]
        live = live & ~cut
    return torch.where(live[..., None], out, torch.zeros_like(out)), live


def _pi(ar, t):
    return ar.of(t).reshape(-1, 1, 1, 1)


def diffaugment_fwd(ar, i, S, C, policy, mut=None):
    x = i["x"]
    N, px = x.shape[0], S * S
    route = lambda t: da_route(t, S, policy, i["t_x"], i["t_y"], i["o_x"], i["o_y"], False, mut)     # noqa: E731
    if not policy & 1:
        return {"y": route(x)[0]}
    ub, us, uc = _pi(ar, i["u_b"]), _pi(ar, i["u_s"]), _pi(ar, i["u_c"])
    v = ar.of(x) + (ub - 0.5)                                   # brightness
    m = seq_sum(v, 3) / (3.0 if mut == "saturation mean with C fixed at 3" else float(C))
    v = (v - m) * us.exact(2.0) + m                             # saturation
    sums = v.sum((1, 2, 3), px * C, keepdim=True)
    if mut == "per-image partial sums added into the wrong image" and px > 2048:
        sums = sums.route(lambda t: t.roll(1, 0))
    M = sums.div_double(float(px if mut == "contrast mean over px in place of px C" else px * C))
    v = (v - M) * (uc + 0.5) + M                                # contrast
    live = route(x)[1]
    return {"y": v.route(lambda t: route(t)[0]).masked(live[..., None])}


def diffaugment_bwd(ar, i, S, C, policy, mut=None):
    """The adjoint of diffaugment_fwd in dy."""
    dy = i["dy"]
    px = S * S
    route = lambda t: da_route(t, S, policy, i["t_x"], i["t_y"], i["o_x"], i["o_y"], True, mut)      # noqa: E731
    g3 = route(dy)[0]
    if not policy & 1:
        return {"dx": g3}
    us, uc = _pi(ar, i["u_s"]), _pi(ar, i["u_c"])
    g = ar.of(g3)
    sums = g.sum((1, 2, 3), px * C, keepdim=True)
    if mut == "per-image partial sums added into the wrong image" and px > 2048:
        sums = sums.route(lambda t: t.roll(1, 0))
    mg = sums.div_double(float(px if mut == "contrast mean over px in place of px C" else px * C))
    cm = uc + 0.5
    g = cm * g + (const(ar, 1.0, dy.device) - cm) * mg
    mc = seq_sum(g, 3) / (3.0 if mut == "saturation mean with C fixed at 3" else float(C))
    sm = us.exact(2.0)
    return {"dx": sm * g + (const(ar, 1.0, dy.device) - sm) * mc}


# ------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------
STRIDE_MUT = "stride loop stopping after 256 elements"


def _head(x, mut):
    """What a single-block kernel whose stride loop takes one step sees of x."""
    return x[:256] if mut == STRIDE_MUT else x


def _unwritten(o, n, mut):
    """An elementwise output whose tail the mutant never writes."""
    if mut == STRIDE_MUT and n > 256 and o.sim:
        return type(o).cat([o, type(o)(torch.full((n - 256,), NAN, dtype=o.v.dtype, device=o.v.device))])
    return o


def flood_apply(ar, L, flood, exact, mut=None):
    """ops.py:847-848: -> (|L - flood| + flood, sign of L - flood, ambiguous count).  ``exact``: a case built from
    exactly representable values whose loss equals flood: the sign is 0 and the loss is flood, bit for bit."""
    dev = L.v.device
    if flood == 0.0:
        return L, const(ar, 1.0, dev), 0
    if exact and not ar.sim:
        assert float(L.v) == flood
        return torch.tensor([flood], dtype=F32, device=dev), const(ar, 0.0, dev), 0
    d = L - flood
    sg = torch.sign(d.v)
    if mut == "flood sign that is never 0":
        sg = torch.where(d.v >= 0, torch.ones_like(sg), -torch.ones_like(sg))
    amb = 0 if ar.sim else int((d.v.abs() <= L.e).sum())
    return d.abs() + flood, ar(sg), amb


def _step(ar, t, arg, val, mut):
    """val where t > 0, else 0, for t = 1 -+ arg formed in fp32: its sign is that of the exact difference, so only the
    error of arg itself can flip it.  -> (values, ambiguous mask)."""
    cond = t.v >= 0 if mut == "hinge derivative with >= in place of >" else t.v > 0
    der = torch.where(cond, torch.full_like(t.v, val), torch.zeros_like(t.v))
    amb = None if ar.sim else (t.v.abs() <= arg.e) & (arg.e > 0)
    return ar(der), amb


def hinge_d_sums(ar, i, mut=None):
    real, fake = ar.of(_head(i["real"], mut)), ar.of(_head(i["fake"], mut))
    n = i["real"].numel()
    a = (const(ar, 1.0, real.v.device) - real).relu().sum(0, n, keepdim=True)
    b = (const(ar, 1.0, real.v.device) + fake).relu().sum(0, n, keepdim=True)
    s0 = ar.of(i["sums0"])
    return {"sums": ar.cat([s0[0:1] + a, s0[1:2] + b])}


def hinge_g_sums(ar, i, mut=None):
    fake = ar.of(_head(i["fake"], mut))
    return {"sums": ar.of(i["sums0"]) + fake.sum(0, i["fake"].numel(), keepdim=True)}


def hinge_d_grad(ar, i, n_global, flood, exact, loss_out, mut=None):
    real, fake, sums = ar.of(i["real"]), ar.of(i["fake"]), ar.of(i["sums"])
    n, dev = real.v.numel(), real.v.device
    if mut == "local n in place of n_global":
        n_global = n
    inv = from_double(ar, torch.tensor(1.0 / n_global, dtype=D64, device=dev))
    L = sums[0:1] * inv + sums[1:2] * inv
    L, sg, amb = flood_apply(ar, L, flood, exact, mut)
    one = const(ar, 1.0, dev)
    dr, _ = _step(ar, one - real, real, 1.0, mut)
    df, _ = _step(ar, one + fake, fake, 1.0, mut)
    out = {"d_real": dr * (-(sg * inv)), "d_fake": df * (sg * inv)}       # (a grid of blocks: no stride loop of 256)
    if loss_out:
        out["loss"] = L
    out["_amb"] = amb
    return out


def hinge_g_grad(ar, i, n, n_global, flood, exact, loss_out, mut=None):
    sums = ar.of(i["sums"])
    dev = sums.v.device
    if mut == "local n in place of n_global":
        n_global = n
    inv = from_double(ar, torch.tensor(1.0 / n_global, dtype=D64, device=dev))
    L = -(sums[0:1] * inv)
    L, sg, amb = flood_apply(ar, L, flood, exact, mut)
    ones = ar(torch.ones(n, dtype=sg.v.dtype, device=dev))
    out = {"d_fake": ones * (-(sg * inv))}
    if loss_out:
        out["loss"] = L
    out["_amb"] = amb
    return out


KINDS = ("hinge", "lsgan", "gan", "ra-lsgan", "ra-gan", "ra-hinge", "wgan-gp")     # the loss_func names of kinds 0 - 6
RA = (3, 4, 5)


def _softplus(x, mut):
    if mut == "softplus without the max shift":
        return type(x)(x.v.exp()).log1p() if x.sim else x.relu() + x.expneg().log1p()
    return x.relu() + x.expneg().log1p()


def _sigmoid(ar, x):
    e = x.expneg()
    den = const(ar, 1.0, x.v.device) + e
    return (const(ar, 1.0, x.v.device) / den).where(x.v >= 0, e / den)


def gan_phi(ar, kind, gen, real_side, x, mut=None):
    """Value and derivative of the real-side / fake-side term at x -> (val, der, ambiguous mask or None)."""
    dev = x.v.device
    zero = ar(torch.zeros_like(x.v))
    if real_side and gen and kind not in RA:
        return zero, zero, None
    up = real_side != bool(gen)
    one = const(ar, 1.0, dev)
    if kind == 6:
        return (-x if up else x), ar(torch.full_like(x.v, -1.0 if up else 1.0)), None
    if kind in (0, 5):
        if kind == 0 and gen:
            return -x, ar(torch.full_like(x.v, -1.0)), None
        t = one - x if up else one + x
        der, amb = _step(ar, t, x, -1.0 if up else 1.0, mut)
        return t.relu(), der, amb
    if kind in (1, 3):
        tgt = 1.0 if up else (-1.0 if kind == 3 else 0.0)
        d = x - tgt if tgt else x
        return d * d, d.exact(2.0), None
    if up:
        return _softplus(-x, mut), -_sigmoid(ar, -x), None
    return _softplus(x, mut), _sigmoid(ar, x), None


def gan_means(ar, i, mut=None):
    dev = i["fake"].device
    real = i.get("real")
    a = ar.of(_head(real, mut)).sum(0, real.numel(), keepdim=True) if real is not None else const(ar, 0.0, dev).reshape(1)
    b = ar.of(_head(i["fake"], mut)).sum(0, i["fake"].numel(), keepdim=True)
    return {"sums": ar.cat([a, b])}


def _gan_args(ar, kind, i, nrg, nfg, mut):
    """-> (u = real - m_f, v = fake - m_r, m_r, m_f as the kernels form them)."""
    real, fake = i.get("real"), i["fake"]
    nr = 0 if real is None else real.numel()
    if mut == "local n in place of n_global":
        nrg, nfg = float(nr), float(fake.numel())
    ra = kind in RA
    s = ar.of(i["sums"])
    u = ar.of(real)
    v = ar.of(fake)
    if ra:
        if nr:
            u = u - s[1:2].div_double(nfg)                     # m_f = (float) (sums[1] / n_fake_global)
        if nrg > 0:
            v = v - s[0:1].div_double(nrg)
    return u, v, nr, nrg, nfg


def gan_terms(ar, kind, gen, i, nrg, nfg, mut=None):
    u, v, nr, nrg, nfg = _gan_args(ar, kind, i, nrg, nfg, mut)
    dev = i["fake"].device
    nf = i["fake"].numel()
    z = const(ar, 0.0, dev).reshape(1)
    amb = 0
    t = [z, z, z, z]
    if nr:
        val, der, a = gan_phi(ar, kind, gen, True, u, mut)
        t[0], t[2] = _head(val, mut).sum(0, nr, keepdim=True), _head(der, mut).sum(0, nr, keepdim=True)
        amb += 0 if a is None else int(a.sum())
    val, der, a = gan_phi(ar, kind, gen, False, v, mut)
    t[1], t[3] = _head(val, mut).sum(0, nf, keepdim=True), _head(der, mut).sum(0, nf, keepdim=True)
    amb += 0 if a is None else int(a.sum())
    return {"tsums": ar.cat(t), "_amb": amb}


def gan_grad(ar, kind, gen, i, nrg, nfg, flood, exact, loss_out, mut=None):
    u, v, nr, nrg, nfg = _gan_args(ar, kind, i, nrg, nfg, mut)
    dev = i["fake"].device
    nf = i["fake"].numel()
    ra = kind in RA
    use_real = not (gen and not ra) and nrg > 0
    dbl = lambda x: from_double(ar, torch.tensor(x, dtype=D64, device=dev))          # noqa: E731
    inv_r = dbl(1.0 / nrg) if use_real else const(ar, 0.0, dev)
    inv_f = dbl(1.0 / nfg)
    ts = ar.of(i["tsums"])
    L = ts[0:1] * inv_r + ts[1:2] * inv_f
    L, sg, amb = flood_apply(ar, L, flood, exact, mut)
    drop = mut == "the relativistic cross term dropped"
    cross_r = ts[3:4] * inv_f if ra and not drop else const(ar, 0.0, dev)
    cross_f = ts[2:3] * inv_r if ra and not drop else const(ar, 0.0, dev)
    out = {}
    if nr:
        _, der, a = gan_phi(ar, kind, gen, True, u, mut)
        amb += 0 if a is None else int(a.sum())
        out["d_real"] = _unwritten(_head(sg * (der - cross_r) * inv_r, mut), nr, mut)
    _, der, a = gan_phi(ar, kind, gen, False, v, mut)
    amb += 0 if a is None else int(a.sum())
    out["d_fake"] = _unwritten(_head(sg * (der - cross_f) * inv_f, mut), nf, mut)
    if loss_out:
        out["loss"] = L
    out["_amb"] = amb
    return out


def sigmoid_ce(ar, i, scale, mut=None):
    """loss = scale sum ce(x, t) w[j], ce = max(x, 0) - x t + log1p(exp(-|x|));  dx = (sigmoid(x) - t) w[j] scale."""
    x, t = i["logits"], i["truth"]
    B, n = x.shape
    dev = x.device
    X, T = ar.of(x.reshape(-1)), ar.of(t.reshape(-1))
    ix = torch.arange(B * n, device=dev)
    if i.get("weights") is not None:
        wi = (ix // n) % n if mut == "weights[i / n] in place of weights[i % n]" else ix % n
        W = ar.of(i["weights"])[wi]
    else:
        W = ar(torch.ones_like(X.v))
    e = X.expneg()
    ce = (X.relu() - X * T + e.log1p()) * W
    den = const(ar, 1.0, dev) + e
    sig = (const(ar, 1.0, dev) / den).where(X.v >= 0, e / den)
    dx = (sig - T) * W * scale
    loss = _head(ce, mut).sum(0, B * n, keepdim=True) * scale
    return {"loss": loss, "dlogits": _unwritten(_head(dx, mut), B * n, mut).reshape(B, n)}


# ------------------------------------------------------------------------------------------
# gradient penalty
# ------------------------------------------------------------------------------------------
def gp_interpolate(ar, i, count, mut=None):
    real, other = ar.of(i["real"]), ar.of(i["other"])
    N = real.v.shape[0]
    a = ar.of(i["alpha"]).reshape(N, 1)
    if i.get("sums") is None:
        return {"out": real + a * (other - real)}
    D = double_of(ar)
    s = D.of(i["sums"])
    m = s[0:1] / count
    var = (s[1:2] / count - m * m).relu()                      # in double; a negative variance is clamped to 0
    std = var.to32().sqrt()                                     # sqrtf((float) var)
    return {"out": real + a * (std.exact(0.5) * other)}


def gp_penalty(ar, i, count, ld, lp, mut=None):
    """ws[0:N] = ||g_n||^2;  loss = ld sum_n phi(||g_n||) / count;  v = ld phi'(||g_n||) / count * g_n / ||g_n||."""
    g = ar.of(i["g"])
    N, per = g.v.shape
    dev = g.v.device
    nsq = (g * g).sum(1, per)                                                     # fp32 partials, added in double
    nrm = nsq.to32().sqrt()                                                       # sqrtf((float) ws[n])
    e = nrm - 1.0
    if lp and mut != "lp clamp missing":
        e = e.relu()
    acc = (e * e).sum(0, N, keepdim=True)
    loss = (acc * ld).div_double(count)
    safe = nrm.v > 0
    den = nrm.where(safe, 1.0)
    if mut == "penalty coefficient without 1/||g||":
        co = e * (2.0 * ld)
    else:
        co = e * (2.0 * ld) / den                                                 # ld * 2.f is one rounding at most
    if mut == "zero-norm row giving NaN":
        co = type(co)(torch.where(safe, co.v, torch.full_like(co.v, NAN)))
    else:
        co = co.masked(safe)
    cf = co.div_double(count, cast=False).to32()                                  # (float) coeff[n]
    nsq64 = nsq if not ar.sim else SimD(nsq.v.double())
    return {"nsq": nsq64, "loss": loss, "v": cf.reshape(N, 1) * g}


# ------------------------------------------------------------------------------------------
# batch-norm tangent
# ------------------------------------------------------------------------------------------
def chan_dots3(ar, i, mut=None):
    p, q, r = ar.of(i["p"]), ar.of(i["q"]), ar.of(i.get("r"))
    rows, C = p.v.shape
    s = [p.sum(0, rows), (p * q).sum(0, rows),
         (p * r).sum(0, rows) if r is not None else ar(torch.zeros(C, dtype=p.v.dtype, device=p.v.device))]
    out = ar.cat(s)
    return {"sums": SimD(out.v.double()) if ar.sim else out}


def _bn_par(D, i):
    return D.of(i["mean"]), D.of(i["rstd"]), D.of(i["gamma"])


def bn_tangent_fwd_coefs(ar, i, count, rows, mut=None):
    """yd = g r (xd - m1 - xh m2) = cf0 xd + cf1 x + cf2;  m1 = mean(xd), m2 = mean(xd xh) = r (sum xd x - mu sum xd) / n."""
    D = double_of(ar)
    mu, r, g = _bn_par(D, i)
    C = mu.v.numel()
    S = D.of(i["sums"])
    if mut == "count = local rows":
        count = float(rows)
    S1, S2 = S[0:C], S[C:2 * C]
    m1 = S1 / count
    m2 = r * S2 / count if mut == "m2 without the mu sum xd term" else r * (S2 - mu * S1) / count
    cf = [g * r, -(g * r * r * m2), -(g * r * m1) + g * r * r * m2 * mu]
    return {"coefs": D.cat(cf).to32(), "m12": D.cat([m1, m2]).to32()}


def bn_tangent_bwd_coefs(ar, i, count, rows, mut=None):
    """From S = (sum s | sum s x | sum s xd): d_xd = cd0 s + cd1 x + cd2;  d_x = cx0 s + cx1 x + cx2 xd + cx3;  dgamma."""
    D = double_of(ar)
    mu, r, g = _bn_par(D, i)
    C = mu.v.numel()
    S = D.of(i["sums"])
    m12 = D.of(i["m12"])
    if mut == "count = local rows":
        count = float(rows)
    n = count
    m1, m2 = m12[0:C], m12[C:2 * C]
    S1, S2, S3 = S[0:C], S[C:2 * C], S[2 * C:3 * C]
    q = r * S2 / n if mut == "m2 without the mu sum xd term" else r * (S2 - mu * S1) / n
    cd = [g * r, -(g * r * r * q), -(g * r * S1 / n) + g * r * r * q * mu]
    dgamma = r * (S3 - m1 * S1 - m2 * n * q)
    Sw, Swx, Swu = g * r * r * S1, g * r * r * n * q, g * r * r * (S3 - m1 * S1)
    K = (m2.exact(1.0) * 3.0 * Swx - Swu) / n
    cx = [-(m2 * g * r * r), r * K, -(Swx / n), -(r * mu * K) + (Swx / n) * m1 + m2 * Sw / n]
    return {"coefs_dxd": D.cat(cd).to32(), "coefs_dx": D.cat(cx).to32(), "dgamma": dgamma.to32()}


def chan_lincomb3(ar, i, mut=None):
    p, q, r = ar.of(i["p"]), ar.of(i["q"]), ar.of(i.get("r"))
    v = ar.of(i["cp"]) * p + ar.of(i["cq"]) * q + ar.of(i["c0"])
    if r is not None:
        v = v + ar.of(i["cr"]) * r
    return {"out": v}


# ------------------------------------------------------------------------------------------
# gather, PReLU tangent slope gradient
# ------------------------------------------------------------------------------------------
def maxpool2_gather(x, t, last=False):
    """y = t at the first maximum of x's 2x2 window in the order (0,0), (0,1), (1,0), (1,1) (last=True: the mutation)."""
    w, tw = EW._win(x), EW._win(t)
    m = EW.maxpool_fwd(x)
    y = torch.zeros_like(m)
    taken = torch.zeros_like(m, dtype=torch.bool)
    for k in (reversed(range(4)) if last else range(4)):
        sel = ~taken & (w[k] == m)
        taken = taken | sel
        y = torch.where(sel, tw[k], y)
    return y


def prelu_tangent_dalpha(ar, i, mut=None):
    """dalpha[c] = sum_rows dy xdot [x < 0]  (1/2 at x == 0)."""
    x = i["x"]
    rows = x.shape[0]
    at0 = 1.0 if mut == "dalpha without the 1/2 at zero" else 0.5
    w = torch.where(x < 0, 1.0, 0.0) + torch.where(x == 0, at0, 0.0)
    term = (ar.of(i["dy"]) * ar.of(i["xdot"])).route(lambda t: t * w.to(t.dtype))
    return {"dalpha": term.sum(0, rows)}


# ------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------
def softmax_fwd(ar, i, mut=None):
    s = i["s"]
    rows, cols = s.shape
    S = ar.of(s)
    if mut == "softmax including the columns >= cols":
        # the row's registers past cols hold what follows the row in memory (nothing follows the last row)
        width = (cols + 63) // 64 * 64
        flat = torch.cat([s.reshape(-1), torch.full((width,), -1e30, dtype=s.dtype, device=s.device)])
        ix = torch.arange(rows, device=s.device)[:, None] * cols + torch.arange(width, device=s.device)[None, :]
        S = ar.of(flat[ix])
    if mut == "softmax without the max subtraction":
        e = type(S)(S.v.exp()) if ar.sim else S.exp()
    else:
        mx = type(S)(S.v.max(1, keepdim=True).values)
        e = (S - mx).exp()
    inv = const(ar, 1.0, s.device) / e.sum(1, S.v.shape[1], keepdim=True)
    return {"p": (e * inv)[:, :cols]}


def softmax_bwd(ar, i, mut=None):
    p, dp = ar.of(i["p"]), ar.of(i["dp"])
    cols = p.v.shape[1]
    dot = (p * dp).sum(1, cols, keepdim=True)
    return {"ds": p * (dp - dot)}


def softmax_tangent_bwd(ar, i, mut=None):
    """dsdot = p (g - u), dp = g (sdot - t) - u sdot;  t = sum p sdot, u = sum g p."""
    p, sd, g = ar.of(i["p"]), ar.of(i["sdot"]), ar.of(i["g"])
    cols = p.v.shape[1]
    t = (p * sd).sum(1, cols, keepdim=True)
    u = (g * p).sum(1, cols, keepdim=True)
    return {"dsdot": p * (g - u), "dp": g * (sd - t) - u * sd}


# ------------------------------------------------------------------------------------------
# one formula entry for both test modules
# ------------------------------------------------------------------------------------------
def formula(c, i, ar, mut=None):
    """The outputs of case c on inputs i over arithmetic ``ar`` (name -> Ref / Sim, or a tensor where the result is
    exact), and "_amb": the count of sign-ambiguous elements (Ref only)."""
    op = c["op"]
    if op == "da_fwd":
        return diffaugment_fwd(ar, i, c["S"], c["C"], c["policy"], mut)
    if op == "da_bwd":
        return diffaugment_bwd(ar, i, c["S"], c["C"], c["policy"], mut)
    if op == "hinge_d_sums":
        return hinge_d_sums(ar, i, mut)
    if op == "hinge_g_sums":
        return hinge_g_sums(ar, i, mut)
    ex = c.get("flood") == "exact"
    if op == "hinge_d_grad":
        return hinge_d_grad(ar, i, i["n_global"], i["flood"], ex, c["loss_out"], mut)
    if op == "hinge_g_grad":
        return hinge_g_grad(ar, i, c["nf"], i["n_global"], i["flood"], ex, c["loss_out"], mut)
    if op == "gan_means":
        return gan_means(ar, i, mut)
    if op == "gan_terms":
        return gan_terms(ar, c["kind"], c["gen"], i, i["nrg"], i["nfg"], mut)
    if op == "gan_grad":
        return gan_grad(ar, c["kind"], c["gen"], i, i["nrg"], i["nfg"], i["flood"], ex, c["loss_out"], mut)
    if op == "sigmoid_ce":
        return sigmoid_ce(ar, i, i["scale"], mut)
    if op == "gp_interpolate":
        return gp_interpolate(ar, i, i["count"], mut)
    if op == "gp_penalty":
        return gp_penalty(ar, i, i["count"], c["ld"], c["lp"], mut)
    if op == "chan_dots3":
        return chan_dots3(ar, i, mut)
    if op == "bn_fwd_coefs":
        return bn_tangent_fwd_coefs(ar, i, i["count"], c["rows"], mut)
    if op == "bn_bwd_coefs":
        return bn_tangent_bwd_coefs(ar, i, i["count"], c["rows"], mut)
    if op == "chan_lincomb3":
        return chan_lincomb3(ar, i, mut)
    if op == "maxpool_gather":
        return {"y": maxpool2_gather(i["x"], i["t"], last=mut == "gather taking the last maximum")}
    if op == "prelu_dalpha":
        return prelu_tangent_dalpha(ar, i, mut)
    if op == "softmax_fwd":
        return softmax_fwd(ar, i, mut)
    if op == "softmax_bwd":
        return softmax_bwd(ar, i, mut)
    if op == "softmax_tangent_bwd":
        return softmax_tangent_bwd(ar, i, mut)
    raise KeyError(op)


def check(c, i, out, rec):
    """Gate the outputs ``out`` (name -> tensor) of case c on inputs i: rec.gate(label, got, ref, E) /
    rec.exact(label, got, want).  -> (sign-ambiguous elements, outputs they are counted against)."""
    r = formula(c, i, Ref)
    namb = r.pop("_amb", 0)
    nout = 0
    if set(out) != set(r):
        rec.fail("outputs %s, reference %s" % (sorted(out), sorted(r)))
        return namb, 1
    for k, got in out.items():
        want = r[k]
        nout += got.numel()
        if isinstance(want, Ref):
            rec.gate(k, got, want.v.reshape(got.shape), want.e.reshape(got.shape))
        else:
            rec.exact(k, got, want.reshape(got.shape))
    return namb, nout


# ------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------
OPS = ("da_fwd", "da_bwd", "hinge_d_sums", "hinge_d_grad", "hinge_g_sums", "hinge_g_grad", "gan_means", "gan_terms",
       "gan_grad", "sigmoid_ce", "gp_interpolate", "gp_penalty", "chan_dots3", "bn_fwd_coefs", "bn_bwd_coefs",
       "chan_lincomb3", "maxpool_gather", "prelu_dalpha", "softmax_fwd", "softmax_bwd", "softmax_tangent_bwd")
ENTRY = {"da_fwd": "bg_diffaugment_fwd", "da_bwd": "bg_diffaugment_bwd", "hinge_d_sums": "bg_hinge_d_sums",
         "hinge_d_grad": "bg_hinge_d_grad", "hinge_g_sums": "bg_hinge_g_sums", "hinge_g_grad": "bg_hinge_g_grad",
         "gan_means": "bg_gan_loss_means", "gan_terms": "bg_gan_loss_terms", "gan_grad": "bg_gan_loss_grad",
         "sigmoid_ce": "bg_sigmoid_ce", "gp_interpolate": "bg_gp_interpolate", "gp_penalty": "bg_gp_penalty",
         "chan_dots3": "bg_chan_dots3", "bn_fwd_coefs": "bg_bn_tangent_fwd_coefs",
         "bn_bwd_coefs": "bg_bn_tangent_bwd_coefs", "chan_lincomb3": "bg_chan_lincomb3",
         "maxpool_gather": "bg_maxpool2_gather", "prelu_dalpha": "bg_prelu_tangent_dalpha",
         "softmax_fwd": "bg_softmax_fwd", "softmax_bwd": "bg_softmax_bwd",
         "softmax_tangent_bwd": "bg_softmax_tangent_bwd"}

LOGIT_N = (1, 5, 255, 256, 257, 1000)
SCALES = (0.02, 1.5, 30.0)
FLOODS = ("none", "below", "above")
KINK_MARGIN = 1e-3           # distance every ra-hinge argument keeps from its kink (its own error is below 1e-5)
DA_S = (8, 9, 16, 48, 64)
DA_C = (1, 3, 4)
GP_PER = (1, 2047, 2048, 2049, 64 * 2048 + 5)
GP_N = (1, 5, 257)
BN_SHAPES = ((1, 1), (10, 3), (33, 8), (37, 776), (4096, 24))
SM_COLS = (1, 48, 63, 64, 65, 1000, 1024)
SM_ROWS = (1, 7, 4099)
CE_SHAPES = ((1, 1), (5, 51), (1, 257), (16, 1000))


def case(op, name, origin, **kw):
    c = dict(op=op, name=name, origin=origin, exempt=())
    c.update(kw)
    return c


def _da_cases():
    out = []
    k = 0
    for pol in range(1, 8):
        for C in DA_C:
            for S in DA_S:
                for N in ((1, 4) if pol in (1, 7) else (4,)):
                    for op in ("da_fwd", "da_bwd"):
                        out.append(case(op, "p%d C%d S%d N%d" % (pol, C, S, N),
                                        "policy %d; S = %d: %d px, cutout %d, shift %d"
                                        % ((pol, S, S * S) + da_params(S)[1::-1]),
                                        policy=pol, C=C, S=S, N=N, edge=k % 4))
                    k += 1
    for op in ("da_fwd", "da_bwd"):
        out.append(case(op, "p7 C3 S48 N257", "two partial blocks per image, second block of da_sums_finalize_kernel",
                        policy=7, C=3, S=48, N=257, edge=0))
        out.append(case(op, "p7 C3 S256 N17", "17 * 65536 px > 4096 * 256: the grid-stride loop takes a second step",
                        policy=7, C=3, S=256, N=17, edge=1))
        out.append(case(op, "p6 C4 S256 N17", "the same grid without colour: exact routing past the grid cap",
                        policy=6, C=4, S=256, N=17, edge=2))
    return out


def _loss_cases():
    out = []
    k = 0
    for n in LOGIT_N:
        for mult in (1, 4):
            for fl in FLOODS:
                sc = SCALES[k % 3]
                nm = "n%d x%d %s s%g" % (n, mult, fl, sc)
                why = "n = %d (stride loop of 256), n_global = %d n, flood %s, logit scale %g" % (n, mult, fl, sc)
                out.append(case("hinge_d_sums", nm, why, nr=n, nf=n, mult=mult, scale=sc, plant=True))
                out.append(case("hinge_g_sums", nm, why, nr=0, nf=n, mult=mult, scale=sc, plant=False))
                out.append(case("hinge_d_grad", nm, why, nr=n, nf=n, mult=mult, scale=sc, flood=fl, plant=True,
                                loss_out=k % 5 != 4))
                out.append(case("hinge_g_grad", nm, why, nr=0, nf=n, mult=mult, scale=sc, flood=fl, plant=False,
                                loss_out=k % 5 != 3))
                k += 1
    out.append(case("hinge_d_grad", "n256 exact flood", "real = fake = 0: L = 2 = flood exactly, every gradient +-0",
                    nr=256, nf=256, mult=1, scale=0.0, flood="exact", plant=False, loss_out=True))
    out.append(case("hinge_g_grad", "n256 exact flood", "fake = -2: L = 2 = flood exactly, every gradient +-0",
                    nr=0, nf=256, mult=1, scale=0.0, flood="exact", plant=False, loss_out=True))
    pairs = ((1, 1), (5, 257), (255, 5), (256, 1000), (257, 256), (1000, 255), (1000, 1000))
    for j, (nr, nf) in enumerate(pairs):
        for mult in (1, 4):
            out.append(case("gan_means", "nr%d nf%d x%d" % (nr, nf, mult), "nr != nf, the stride loop of 256", nr=nr, nf=nf,
                            mult=mult, scale=SCALES[j % 3], kind=0, gen=0, plant=False))
    out.append(case("gan_means", "nr0 nf257", "real == NULL with nr = 0", nr=0, nf=257, mult=1, scale=1.5, kind=0, gen=1,
                    plant=False))
    for kind in range(7):
        for gen in (0, 1):
            for j, (nr, nf) in enumerate(pairs):
                sc, fl, mult = SCALES[(j + kind) % 3], FLOODS[(j + kind + gen) % 3], (1, 4)[(j + gen) % 2]
                null_real = gen == 1 and kind not in RA and j % 2 == 1
                nm = "%s %s nr%d nf%d x%d %s s%g" % (KINDS[kind], "DG"[gen], 0 if null_real else nr, nf, mult, fl, sc)
                why = "kind %d generator %d%s" % (kind, gen, ", real == NULL with nr = 0" if null_real else "")
                kw = dict(kind=kind, gen=gen, nr=0 if null_real else nr, nf=nf, mult=mult, scale=sc,
                          plant=kind == 0 and gen == 0)
                out.append(case("gan_terms", nm, why, **kw))
                out.append(case("gan_grad", nm, why, flood=fl, loss_out=(j + kind) % 4 != 3, **kw))
    for kind in (2, 4):
        for gen in (0, 1):
            nm = "%s %s planted +-100" % (KINDS[kind], "DG"[gen])
            why = "logits of +-100: the softplus / sigmoid tails, __expf underflow"
            kw = dict(kind=kind, gen=gen, nr=257, nf=300, mult=1, scale=1.5, plant="tails")
            out.append(case("gan_terms", nm, why, **kw))
            out.append(case("gan_grad", nm, why, flood="below", loss_out=True, **kw))
    for kind, why in ((0, "real = fake = 0: L = 2 = flood"), (1, "real = fake = 0: L = 1 = flood"),
                      (6, "real = 1, fake = 2: L = 1 = flood")):
        out.append(case("gan_grad", "%s D exact flood" % KINDS[kind], why + " exactly, every gradient +-0", kind=kind, gen=0,
                        nr=256, nf=256, mult=1, scale=0.0, flood="exact", plant=False, loss_out=True))
    k = 0
    for B, n in CE_SHAPES:
        for wts in (False, True):
            for soft in (False, True):
                out.append(case("sigmoid_ce", "B%d n%d %s %s" % (B, n, "w" if wts else "no-w", "soft" if soft else "hard"),
                                "%d logits to +-100, scale %s" % (B * n, "negative" if k % 2 else "positive"), B=B, n=n,
                                weights=wts, soft=soft, neg=bool(k % 2)))
                k += 1
    return out


def _gp_cases():
    out = []
    for per in (1, 192):
        for N in (1, 5):
            for form in ("lerp", "dragan"):
                out.append(case("gp_interpolate", "%s N%d per%d" % (form, N, per), "alpha contains 0 and 1", N=N, per=per,
                                form=form, data="randn"))
    out.append(case("gp_interpolate", "dragan N5 per192 constant", "constant real: the variance rounds to <= 0, std is 0",
                    N=5, per=192, form="dragan", data="constant"))
    for form in ("lerp", "dragan"):
        out.append(case("gp_interpolate", "%s N5 per209720" % form, "1 048 600 elements > 4096 * 256: the grid-stride step",
                        N=5, per=209720, form=form, data="randn"))
    k = 0
    for per in GP_PER:
        for N in GP_N:
            if per * N > 4 << 20:
                continue                    # (257 rows of 131 077: 135 MB; the 64-block cap is reached at N = 1 and 5)
            for lp in (0, 1):
                for mult in (1, 4):
                    out.append(case("gp_penalty", "N%d per%d lp%d x%d" % (N, per, lp, mult),
                                    "%d gp_sumsq blocks per sample%s" % (min(64, (per + 2047) // 2048),
                                                                         ", N > 256: second step of gp_finish" * (N > 256)),
                                    N=N, per=per, lp=lp, mult=mult, ld=f32r((10.0, 0.3)[k % 2])))
                    k += 1
    return out


def _bn_cases():
    out = []
    for rows, C in BN_SHAPES:
        for data in ("randn", "mean8"):
            for mult in (1, 4):
                nm = "%dx%d %s x%d" % (rows, C, data, mult)
                why = "x ~ %s, count = %d rows" % ("8 +- 0.5 (m2 cancels)" if data == "mean8" else "N(0, 1)", mult)
                out.append(case("bn_fwd_coefs", nm, why, rows=rows, C=C, data=data, mult=mult, r=False))
                out.append(case("bn_bwd_coefs", nm, why, rows=rows, C=C, data=data, mult=mult, r=True))
            for r in (False, True):
                nm = "%dx%d %s %s" % (rows, C, data, "r" if r else "no-r")
                blocks = (rows + 31) // 32 if rows > 32 else 1
                out.append(case("chan_dots3", nm, "%d blocks, VEC %d" % (blocks, 1 if C % 4 else 4),
                                rows=rows, C=C, data=data, mult=1, r=r))
                out.append(case("chan_lincomb3", nm, "coefficients of the tangent pass", rows=rows, C=C, data=data, mult=1,
                                r=r))
    out.append(case("chan_lincomb3", "4099x129 randn r", "528 771 elements > 2048 * 256 (ew_grid): the grid-stride step",
                    rows=4099, C=129, data="randn", mult=1, r=True))
    return out


def _misc_cases():
    out = []
    for N, H, W, C in EW.EDGE_MAXPOOL:
        for data in ("randn", "ties"):
            out.append(case("maxpool_gather", "%dx%dx%dx%d %s" % (N, H, W, C, data), "ties include +0 / -0", N=N, H=H, W=W,
                            C=C, data=data))
    for N, HW, C, why in EW.EDGE:
        rows = N * HW
        out.append(case("prelu_dalpha", "%dx%d" % (rows, C),
                        "launch_colreduce<1> only (no thin dispatch): VEC %d, %s; 1 %% exact zeros"
                        % (1 if C % 4 else 4, "one block" if rows <= 32 else "per-block partials"), rows=rows, C=C))
    out.append(case("prelu_dalpha", "4100x3", "C <= 4 with many rows: still launch_colreduce<1>, 128 blocks of one column",
                    rows=4100, C=3))
    for op in ("softmax_fwd", "softmax_bwd", "softmax_tangent_bwd"):
        for cols in SM_COLS:
            for rows in SM_ROWS:
                if rows == 4099 and cols not in (1, 63, 1024):
                    continue
                for off in (range(4) if rows == 1 else (0,)):
                    out.append(case(op, "%dx%d d%d" % (rows, cols, off),
                                    "row kinds N(0,1) | all equal | one entry 90 above | spread over +-40, from kind %d"
                                    % off,
                                    rows=rows, cols=cols, off=off, inplace=False))
        out.append(case(op, "8193x48 d0",
                        "rows > 2048 * 4 waves (ew_grid; 4099 rows stay below the cap): a wave's second row",
                        rows=8193, cols=48, off=0, inplace=False))
    for cols in (63, 1024):
        out.append(case("softmax_fwd", "7x%d in place" % cols, "p == s", rows=7, cols=cols, off=0, inplace=True))
    return out


CASES = _da_cases() + _loss_cases() + _gp_cases() + _bn_cases() + _misc_cases()


def cases(op=None):
    return [c for c in CASES if op is None or c["op"] == op]


def describe(c):
    return "%s[%s]" % (c["op"], c["name"])


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def _rn(shape, gen, dev, scale=1.0):
    return torch.randn(shape, generator=gen, device=dev, dtype=F32) * scale


def _ru(shape, gen, dev):
    return torch.rand(shape, generator=gen, device=dev, dtype=F32)


def _ri(lo, hi, shape, gen, dev):
    return torch.randint(lo, hi, shape, generator=gen, device=dev, dtype=torch.int32)


def da_draws(c, gen, dev):
    """The seven draws, with the edge values of the case's ``edge`` set planted in image 0 (and the others in the
    following images where there are any)."""
    N, S = c["N"], c["S"]
    shift, _, off_max = da_params(S)
    d = dict(u_b=_ru((N,), gen, dev), u_s=_ru((N,), gen, dev), u_c=_ru((N,), gen, dev),
             t_x=_ri(-shift, shift + 1, (N,), gen, dev), t_y=_ri(-shift, shift + 1, (N,), gen, dev),
             o_x=_ri(0, off_max, (N,), gen, dev), o_y=_ri(0, off_max, (N,), gen, dev))
    below1 = 1.0 - 2.0 ** -24
    edges = (dict(t_x=shift, t_y=-shift, o_x=0, o_y=off_max - 1, u_s=0.0),
             dict(t_x=-shift, t_y=shift, o_x=off_max - 1, o_y=0, u_c=0.0),
             dict(t_x=shift, t_y=shift, o_x=0, o_y=0, u_b=0.0),
             dict(t_x=-shift, t_y=-shift, o_x=off_max - 1, o_y=off_max - 1, u_b=below1, u_s=below1, u_c=below1))
    for n in range(min(N, 4)):
        for k, v in edges[(c["edge"] + n) % 4].items():
            d[k][n] = v
    return d


def _logits(c, gen, dev):
    """real [nr] (None for nr = 0), fake [nf]."""
    nr, nf, sc = c["nr"], c["nf"], c["scale"]
    real = _rn((nr,), gen, dev, sc) + f32r(0.3 * sc) if nr else None
    fake = _rn((nf,), gen, dev, sc) - f32r(0.2 * sc)
    if c.get("plant") is True:               # kinks on stored values: the branch is not ambiguous
        if nr:
            real[::3] = 1.0
            real[-1] = 1.0
        fake[::4] = -1.0
        fake[-1] = -1.0
    if c.get("plant") == "tails":
        for t in (real, fake):
            t[0], t[1], t[-1], t[-2] = 100.0, -100.0, 100.0, -100.0
            t[256] = -100.0
    return real, fake


def _flood_value(L, mode):
    L = float(L)
    if mode == "none":
        return 0.0
    return f32r(L - 0.5 * abs(L) - 0.1) if mode == "below" else f32r(L + 0.5 * abs(L) + 0.1)


def _other_share(own, mult, gen, dev):
    """Global sums: this rank's plus three ranks of about the same (fp32, as the all-reduce delivers them)."""
    if mult == 1:
        return own.float()
    return (own * (4.0 + 0.01 * torch.rand(own.shape, generator=gen, device=dev, dtype=D64))).float()


def _keep_off_kinks(c, real, fake, sums, nrg, nfg):
    """Move every ra-hinge argument u = real - m_f, v = fake - m_r that lies within KINK_MARGIN of +-1 away from it (the
    sums are an input of their own: the means do not move)."""
    if c["kind"] != 5:
        return
    mf = float((sums[1].double() / nfg).float())
    mr = float((sums[0].double() / nrg).float()) if nrg > 0 else 0.0
    for t, m in ((real, mf), (fake, mr)):
        if t is None:
            continue
        u = t.double() - m
        for kink in (1.0, -1.0):
            near = (u - kink).abs() < KINK_MARGIN
            t[near] = (m + kink + 4 * KINK_MARGIN)


def make_inputs(c, dev, gen):
    op = c["op"]
    if op in ("da_fwd", "da_bwd"):
        i = da_draws(c, gen, dev)
        i["x" if op == "da_fwd" else "dy"] = _rn((c["N"], c["S"], c["S"], c["C"]), gen, dev, 0.5)
        return i
    if op in ("hinge_d_sums", "hinge_g_sums", "hinge_d_grad", "hinge_g_grad", "gan_means", "gan_terms", "gan_grad"):
        real, fake = _logits(c, gen, dev)
        nr, nf, mult = c["nr"], c["nf"], c["mult"]
        exact = c.get("flood") == "exact"
        if exact:
            if op == "hinge_g_grad":
                fake = torch.full((nf,), -2.0, device=dev)
            elif c.get("kind") == 6:
                real, fake = torch.ones(nr, device=dev), torch.full((nf,), 2.0, device=dev)
            else:
                real, fake = torch.zeros(nr, device=dev), torch.zeros(nf, device=dev)
        i = dict(fake=fake)
        if real is not None and op not in ("hinge_g_sums", "hinge_g_grad"):
            i["real"] = real
        if op in ("hinge_d_sums", "hinge_g_sums"):
            k = 2 if op == "hinge_d_sums" else 1
            i["sums0"] = (torch.rand(k, generator=gen, device=dev, dtype=F32) * nf * 3 if mult == 4
                          else torch.zeros(k, device=dev))
            return i
        if op == "gan_means":
            return i
        i["n_global"] = float(mult * nf)
        if op in ("hinge_d_grad", "hinge_g_grad"):
            if op == "hinge_d_grad":
                own = torch.stack([(1 - real.double()).clamp_min(0).sum(), (1 + fake.double()).clamp_min(0).sum()])
            else:
                own = fake.double().sum().reshape(1)
            i["sums"] = _other_share(own, mult, gen, dev)
            s = i["sums"].double()
            L = (s.sum() if op == "hinge_d_grad" else -s[0]) / i["n_global"]
            i["flood"] = 2.0 if exact else _flood_value(L, c["flood"])
            return i
        i["nrg"], i["nfg"] = float(mult * nr), float(mult * nf)
        own = torch.stack([real.double().sum() if nr else torch.zeros((), dtype=D64, device=dev), fake.double().sum()])
        i["sums"] = _other_share(own, mult, gen, dev)
        _keep_off_kinks(c, real, fake, i["sums"], i["nrg"], i["nfg"])
        if op == "gan_terms":
            return i
        t = gan_terms(Ref, c["kind"], c["gen"], i, i["nrg"], i["nfg"])["tsums"].v
        i["tsums"] = _other_share(t, mult, gen, dev)
        ts = i["tsums"].double()
        use_real = not (c["gen"] and c["kind"] not in RA) and i["nrg"] > 0
        L = (ts[0] / i["nrg"] if use_real else 0.0) + ts[1] / i["nfg"]
        i["flood"] = {0: 2.0, 1: 1.0, 6: 1.0}[c["kind"]] if exact else _flood_value(L, c["flood"])
        return i
    if op == "sigmoid_ce":
        B, n = c["B"], c["n"]
        x = _rn((B, n), gen, dev, 3.0)
        flat = x.reshape(-1)
        flat[0] = 100.0
        flat[-1] = -100.0
        if B * n > 300:
            flat[299], flat[300] = -100.0, 100.0
        t = _ru((B, n), gen, dev) if c["soft"] else (_ru((B, n), gen, dev) < 0.3).float()
        i = dict(logits=x, truth=t, scale=f32r((-1.0 if c["neg"] else 1.0) * 0.7 / (4 * B * n)))
        if c["weights"]:
            i["weights"] = _ru((n,), gen, dev) * 3.0 + 0.1
        return i
    if op == "gp_interpolate":
        N, per = c["N"], c["per"]
        real = torch.full((N, per), 1.7, device=dev) if c["data"] == "constant" else _rn((N, per), gen, dev)
        i = dict(real=real, alpha=_ru((N,), gen, dev))
        i["alpha"][0] = 0.0
        i["alpha"][-1] = 1.0 if N > 1 else i["alpha"][-1]
        if c["form"] == "dragan":
            i["other"] = _ru((N, per), gen, dev)
            i["sums"] = torch.stack([real.double().sum(), (real.double() ** 2).sum()])
            i["count"] = float(N * per)
        else:
            i["other"] = _rn((N, per), gen, dev)
            i["count"] = 0.0
        if N == 1:
            i["alpha"][0] = (0.0, 1.0)[per % 2]
        return i
    if op == "gp_penalty":
        N, per = c["N"], c["per"]
        g = _rn((N, per), gen, dev)
        nrm = g.double().norm(dim=1, keepdim=True).clamp_min(1e-30)
        target = 0.25 + 1.5 * torch.rand((N, 1), generator=gen, device=dev, dtype=D64)      # norms on both sides of 1
        g = (g.double() / nrm * target).float()
        if N >= 5:
            g[1] = 0.0                                  # an all-zero row: coefficient 0, finite loss
            g[2] = 0.0
            g[2, per // 2] = -1.0                       # norm exactly 1
        return dict(g=g, count=float(c["mult"] * N))
    if op in ("chan_dots3", "bn_fwd_coefs", "bn_bwd_coefs", "chan_lincomb3"):
        rows, C = c["rows"], c["C"]
        x = _rn((rows, C), gen, dev)
        if c["data"] == "mean8":
            x = x * 0.5 + 8.0
        xd, s = _rn((rows, C), gen, dev), _rn((rows, C), gen, dev)
        if op == "chan_dots3":
            i = dict(p=xd, q=x)
            if c["r"]:
                i["r"] = s
            return i
        if op == "chan_lincomb3":
            i = dict(p=xd, q=x, cp=_rn((C,), gen, dev), cq=_rn((C,), gen, dev), c0=_rn((C,), gen, dev))
            if c["r"]:
                i["r"], i["cr"] = s, _rn((C,), gen, dev)
            return i
        x64 = x.double()
        mean = x64.mean(0)
        var = (x64 * x64).mean(0) - mean * mean
        gamma = _rn((C,), gen, dev)
        gamma[0] = 0.0
        if C > 1:
            gamma[1] = -gamma[1].abs() - 0.1
        i = dict(mean=mean.float(), rstd=(var.clamp_min(0) + 1e-5).rsqrt().float(), gamma=gamma,
                 count=float(c["mult"] * rows))
        k = 1.0 if c["mult"] == 1 else 4.0
        if op == "bn_fwd_coefs":
            i["sums"] = torch.cat([xd.double().sum(0), (xd.double() * x64).sum(0)]) * k
            return i
        i["sums"] = torch.cat([s.double().sum(0), (s.double() * x64).sum(0), (s.double() * xd.double()).sum(0)]) * k
        f = dict(i, sums=torch.cat([xd.double().sum(0), (xd.double() * x64).sum(0)]) * k)
        i["m12"] = bn_tangent_fwd_coefs(Ref, f, i["count"], rows)["m12"].v.float()
        return i
    if op == "maxpool_gather":
        shape = (c["N"], c["H"], c["W"], c["C"])
        if c["data"] == "ties":
            x = _ri(-1, 2, shape, gen, dev).float()
            x = torch.where((x == 0) & (_ru(shape, gen, dev) < 0.5), -torch.zeros_like(x), x)
        else:
            x = _rn(shape, gen, dev)
        return dict(x=x, t=_rn(shape, gen, dev))
    if op == "prelu_dalpha":
        rows, C = c["rows"], c["C"]
        x = _rn((rows, C), gen, dev)
        u = _ru((rows, C), gen, dev)
        x = torch.where(u < 0.005, torch.zeros_like(x), torch.where(u < 0.01, -torch.zeros_like(x), x))
        x[0, 0] = 0.0
        return dict(x=x, xdot=_rn((rows, C), gen, dev), dy=_rn((rows, C), gen, dev))
    if op in ("softmax_fwd", "softmax_bwd", "softmax_tangent_bwd"):
        rows, cols = c["rows"], c["cols"]
        s = _rn((rows, cols), gen, dev)
        kind = (torch.arange(rows, device=dev) + c["off"]) % 4
        s[kind == 1] = s[kind == 1][:, :1]
        sp = s[kind == 2]
        sp[:, cols // 2] = sp[:, cols // 2] + 90.0
        s[kind == 2] = sp
        s[kind == 3] = (_ru((rows, cols), gen, dev) * 80.0 - 40.0)[kind == 3]
        if op == "softmax_fwd":
            return dict(s=s)
        p = torch.softmax(s.double(), 1).float()
        p = torch.where(p < TINY, torch.zeros_like(p), p)      # (what the forward stores: it flushes denormal results)
        if op == "softmax_bwd":
            return dict(p=p, dp=_rn((rows, cols), gen, dev))
        return dict(p=p, sdot=_rn((rows, cols), gen, dev), g=_rn((rows, cols), gen, dev))
    raise KeyError(op)


# ------------------------------------------------------------------------------------------
# the composed chains (tests/test_gpu_loss_kernels.py runs them through the wrappers of functional.py)
# ------------------------------------------------------------------------------------------
BN_EPS = 1e-5
COMPOSED_B = 300
COMPOSED_BN = (37, 776)


def rounded_input(v64):
    """An fp32 input that is the rounding of the float64 quantity the oracle uses (batch mean, rstd)."""
    return Ref(v64, U32 * v64.abs())


def bn_tangent_autograd(x, xd, s, gamma):
    """float64 autograd: the JVP yd of training-mode batch norm y = gamma (x - mean) rstd along xd (taken with the
    double-backward construction), and the gradients of <s, yd> in xd, x and gamma."""
    x = x.detach().clone().requires_grad_(True)
    xd = xd.detach().clone().requires_grad_(True)
    gamma = gamma.detach().clone().requires_grad_(True)
    mean = x.mean(0)
    var = (x * x).mean(0) - mean * mean
    y = gamma * (x - mean) * (var + BN_EPS).rsqrt()
    w = torch.zeros_like(y, requires_grad=True)
    vjp, = torch.autograd.grad(y, x, w, create_graph=True)
    yd, = torch.autograd.grad(vjp, w, xd, create_graph=True)
    dxd, dx, dg = torch.autograd.grad((yd * s).sum(), (xd, x, gamma))
    return yd.detach(), dxd, dx, dg


def composed_bn_tangent(x, xd, s, gamma, count):
    """Bounds of functional.BnTangentFn's forward and backward: the stage bounds chained (each stage's result enters the
    next with its bound), mean / rstd as fp32 roundings of the batch statistics."""
    rows, C = x.shape
    x64 = x.double()
    mean = x64.mean(0)
    var = (x64 * x64).mean(0) - mean * mean
    par = dict(mean=rounded_input(mean), rstd=rounded_input((var + BN_EPS).rsqrt()), gamma=gamma)
    s1 = chan_dots3(Ref, dict(p=xd, q=x))["sums"]
    fc = bn_tangent_fwd_coefs(Ref, dict(par, sums=s1), count, rows)
    cf = fc["coefs"]
    y = chan_lincomb3(Ref, dict(p=xd, q=x, cp=cf[0:C], cq=cf[C:2 * C], c0=cf[2 * C:]))["out"]
    s2 = chan_dots3(Ref, dict(p=s, q=x, r=xd))["sums"]
    bc = bn_tangent_bwd_coefs(Ref, dict(par, sums=s2, m12=fc["m12"]), count, rows)
    cd, cx = bc["coefs_dxd"], bc["coefs_dx"]
    dxd = chan_lincomb3(Ref, dict(p=s, q=x, cp=cd[0:C], cq=cd[C:2 * C], c0=cd[2 * C:]))["out"]
    dx = chan_lincomb3(Ref, dict(p=s, q=x, r=xd, cp=cx[0:C], cq=cx[C:2 * C], cr=cx[2 * C:3 * C], c0=cx[3 * C:]))["out"]
    return dict(mean=mean.float(), rstd=(var + BN_EPS).rsqrt().float(), y=y, dxd=dxd, dx=dx, dgamma=bc["dgamma"])


def composed_hinge_d(real, fake, flood):
    n = real.numel()
    s = hinge_d_sums(Ref, dict(real=real, fake=fake, sums0=torch.zeros(2, device=real.device)))["sums"]
    return hinge_d_grad(Ref, dict(real=real, fake=fake, sums=s), float(n), flood, False, True)


def composed_gan(kind, gen, real, fake, flood):
    nr, nf = float(real.numel()), float(fake.numel())
    i = dict(real=real, fake=fake)
    i["sums"] = gan_means(Ref, i)["sums"]
    t = gan_terms(Ref, kind, gen, i, nr, nf)
    i["tsums"] = t["tsums"]
    r = gan_grad(Ref, kind, gen, i, nr, nf, flood, False, True)
    r["_amb"] += t["_amb"]
    return r
