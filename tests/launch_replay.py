"""Record the GEMM-family launches of a training iteration and replay each one against a float64 reference.

Test helper, not product code.  Three parts:

* references - plain float64 restatements of the conv / transposed-conv / attention / GEMM semantics of
  ``include/biggan_hip.h`` (explicit padding + ``F.unfold`` + matmul), device-agnostic so that
  ``tests/test_launch_gate.py`` can check them against ``oracle/kat.py`` and autograd on the CPU;
* ``gate`` - the per-element acceptance test.  Operands are bf16-representable, so every product is exact in fp32 and
  the only errors left are the fp32 accumulation and the output's rounding.  With ``A`` the same reference run on
  absolute values and ``K`` the reduction length, ``E = (8 sqrt(K) + 2) 2^-24 A`` (+ the unit of each extra rounding
  point times its absolute-value term); an fp32 output must satisfy ``|got - ref| <= E + 2^-24 |ref|``, a bf16 output
  ``RNE(ref - E) <= got <= RNE(ref + E)``;
* ``Recorder`` / ``replay`` - a proxy over ``functional.lib`` / ``hip.lib`` keeps the descriptor and flags of every
  conv / deconv / rgbconv / attention16 / attention2 / gram16 / gemm call of an iteration (deduplicated), and ``replay``
  runs each unique
  call again through the same entry point on fresh bf16-exact buffers: NaN-prefilled (or random, when accumulating)
  outputs behind and before which sit guard bands, two runs that must agree bit for bit, and the ``bg_prof`` set of
  (tag, kernel symbol) pairs, which must equal the recorded iteration's.

``tests/geometry_sweep.py`` builds lists of ``Call`` objects for the geometries the entry points accept but no benchmark
model builds; they go through the same ``replay_all``.
"""
import collections
import ctypes
import math
import os
import tempfile

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24            # fp32 unit roundoff
U16 = 2.0 ** -8             # bf16 unit roundoff
PAD_REFLECT, PAD_ZERO = 0, 1
F32, BF16 = 0, 1
GUARD = 256                 # bytes of sentinel before and after every output / workspace
SENTINEL = 0xA5


# ------------------------------------------------------------------------------------------
# float64 references (NHWC; conv kernels [k,k,Cin,Cout], transposed-conv kernels [k,k,Cout,Cin])
# ------------------------------------------------------------------------------------------
def pad_index(n, lo, npad, mode, device=None):
    """Source row of each of the npad rows of a padded axis; index n is an extra zero row (BG_PAD_ZERO)."""
    idx = []
    for u in range(npad):
        j = u - lo
        if mode == PAD_REFLECT:         # tf.pad REFLECT: mirrored without repeating the border
            if j < 0:
                j = -j
            if j >= n:
                j = 2 * (n - 1) - j
            assert 0 <= j < n, (n, lo, npad)
        elif j < 0 or j >= n:
            j = n
        idx.append(j)
    return torch.tensor(idx, dtype=torch.long, device=device)


def pad2d(x, lo, Hp, Wp, mode):
    """x [n,H,W,C] -> the padded grid [n,Hp,Wp,C] whose first row / column is padded row -lo."""
    n, H, W, C = x.shape
    xe = F.pad(x, (0, 0, 0, 1, 0, 1))                        # the zero row / column
    xe = xe.index_select(1, pad_index(H, lo, Hp, mode, x.device))
    return xe.index_select(2, pad_index(W, lo, Wp, mode, x.device))


def fold2d(gp, lo, H, W, mode):
    """Adjoint of pad2d: every padded row / column adds into its source."""
    n, Hp, Wp, C = gp.shape
    t = torch.zeros((n, H + 1, Wp, C), dtype=gp.dtype, device=gp.device).index_add_(
        1, pad_index(H, lo, Hp, mode, gp.device), gp)
    t = torch.zeros((n, H + 1, W + 1, C), dtype=gp.dtype, device=gp.device).index_add_(
        2, pad_index(W, lo, Wp, mode, gp.device), t)
    return t[:, :H, :W]


def _chunk(n, per_item_bytes, budget=1 << 31):
    return max(1, min(n, budget // max(per_item_bytes, 1)))


def corr(xp, w, s):
    """Valid cross-correlation: y[n,i,j,o] = sum_{p,q,c} xp[n, i s + p, j s + q, c] w[p,q,c,o]."""
    n, Hp, Wp, C = xp.shape
    k, O = w.shape[0], w.shape[3]
    Ho, Wo = (Hp - k) // s + 1, (Wp - k) // s + 1
    wf = w.permute(2, 0, 1, 3).reshape(C * k * k, O)
    out = torch.empty((n, Ho, Wo, O), dtype=xp.dtype, device=xp.device)
    step = _chunk(n, C * k * k * Ho * Wo * 8)
    for a in range(0, n, step):
        cols = F.unfold(xp[a:a + step].permute(0, 3, 1, 2), k, stride=s)          # [b, C k k, Ho Wo]
        out[a:a + step] = (cols.transpose(1, 2) @ wf).reshape(-1, Ho, Wo, O)
    return out


def wcorr(xp, dy, k, s):
    """Weight gradient of corr: dw[p,q,c,o] = sum_{n,i,j} xp[n, i s + p, j s + q, c] dy[n,i,j,o]."""
    n, Hp, Wp, C = xp.shape
    _, Ho, Wo, O = dy.shape
    acc = torch.zeros((C * k * k, O), dtype=xp.dtype, device=xp.device)
    step = _chunk(n, C * k * k * Ho * Wo * 8)
    for a in range(0, n, step):
        cols = F.unfold(xp[a:a + step].permute(0, 3, 1, 2), k, stride=s)          # [b, C k k, L]
        b = cols.shape[0]
        acc += cols.permute(1, 0, 2).reshape(C * k * k, b * Ho * Wo) @ dy[a:a + step].reshape(b * Ho * Wo, O)
    return acc.reshape(C, k, k, O).permute(1, 2, 0, 3).contiguous()


def tconv_full(dy, w, s):
    """Transposed correlation onto the whole grid: g[n, i s + p, j s + q, c] += dy[n,i,j,o] w[p,q,c,o];
    the grid is ((Hi-1) s + k) square."""
    n, Hi, Wi, O = dy.shape
    k = w.shape[0]
    dil = torch.zeros((n, (Hi - 1) * s + 1, (Wi - 1) * s + 1, O), dtype=dy.dtype, device=dy.device)
    dil[:, ::s, ::s] = dy
    dil = F.pad(dil, (0, 0, k - 1, k - 1, k - 1, k - 1))
    return corr(dil, w.flip(0, 1).transpose(2, 3), 1)


def conv_fwd(x, w, s, lo, Ho, Wo, mode):
    k = w.shape[0]
    return corr(pad2d(x, lo, (Ho - 1) * s + k, (Wo - 1) * s + k, mode), w, s)


def conv_dgrad(dy, w, s, lo, H, W, mode):
    return fold2d(tconv_full(dy, w, s), lo, H, W, mode)


def conv_wgrad(x, dy, k, s, lo, mode):
    Ho, Wo = dy.shape[1], dy.shape[2]
    return wcorr(pad2d(x, lo, (Ho - 1) * s + k, (Wo - 1) * s + k, mode), dy, k, s)


def deconv_fwd(x, w, s, lo, Ho, Wo):
    """tf.nn.conv2d_transpose(SAME): y[n, a s + p - lo, b s + q - lo, o] += x[n,a,b,c] w[p,q,o,c]."""
    g = tconv_full(x, w, s)
    g = F.pad(g, (0, 0, 0, max(0, lo + Wo - g.shape[2]), 0, max(0, lo + Ho - g.shape[1])))
    return g[:, lo:lo + Ho, lo:lo + Wo]


def deconv_dgrad(dy, w, s, lo, H, W):
    return conv_fwd(dy, w, s, lo, H, W, PAD_ZERO)


def deconv_wgrad(x, dy, k, s, lo):
    H, W = x.shape[1], x.shape[2]
    return wcorr(pad2d(dy, lo, (H - 1) * s + k, (W - 1) * s + k, PAD_ZERO), x, k, s)


def attn_fwd(q, k, v):
    """o = softmax(q k^T) v per batch item (no scale), and lse = the log of each row's normaliser."""
    S = q @ k.transpose(1, 2)
    lse = torch.logsumexp(S, dim=2)
    P = torch.exp(S - lse[..., None])
    return P @ v, lse


def attn_bwd(q, k, v, do, P, delta):
    """Gradients of o = P v, P = softmax(q k^T) given dO and delta_i = sum_c dO_ic o_ic."""
    dP = do @ v.transpose(1, 2)
    dS = P * (dP - delta[..., None])
    return dS @ k, dS.transpose(1, 2) @ q, P.transpose(1, 2) @ do


# ------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------
def bound(A, K, extra=None):
    E = (8.0 * math.sqrt(K) + 2.0) * U32 * A
    return E if extra is None else E + extra


class GateStats:
    """Per kernel symbol: launches, worst |got-ref| / bound, bf16 ambiguous outputs above / below ref."""

    def __init__(self):
        self.rows = collections.OrderedDict()

    def launch(self, key):
        self.rows.setdefault(key, [0, 0.0, 0, 0])[0] += 1

    def add(self, key, ratio, above=0, below=0):
        r = self.rows.setdefault(key, [0, 0.0, 0, 0])
        r[1] = max(r[1], ratio)
        r[2] += above
        r[3] += below

    def table(self):
        lines = ["%-58s %9s %10s %8s %8s" % ("kernel", "launches", "err/bound", "above", "below")]
        for k, (n, w, a, b) in self.rows.items():
            lines.append("%-58s %9d %10.4f %8d %8d" % (k[:58], n, w, a, b))
        return "\n".join(lines)


def gate(got, ref, E):
    """-> (ok, worst err/bound ratio, ambiguous above, ambiguous below, n bad).  got fp32 or bf16; ref, E float64."""
    g = got.double()
    if got.dtype == torch.bfloat16:
        lo = (ref - E).to(torch.bfloat16).double()
        hi = (ref + E).to(torch.bfloat16).double()
        bad = ~((g >= lo) & (g <= hi))
        width = torch.where(g >= ref, hi - ref, ref - lo).clamp_min(1e-300)
        ratio = (g - ref).abs() / width
        amb = lo != hi
        above = int((amb & (g > ref)).sum())
        below = int((amb & (g < ref)).sum())
    else:
        B = E + U32 * ref.abs()
        bad = ~((g - ref).abs() <= B)
        ratio = (g - ref).abs() / B.clamp_min(1e-300)
        above = below = 0
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    nbad = int(bad.sum())
    return nbad == 0, float(ratio.max()) if ratio.numel() else 0.0, above, below, nbad


# ------------------------------------------------------------------------------------------
# recorder
# ------------------------------------------------------------------------------------------
CONV = ("bg_conv2d_fwd", "bg_conv2d_dgrad", "bg_conv2d_wgrad", "bg_deconv2d_fwd", "bg_deconv2d_fwd_stats",
        "bg_deconv2d_dgrad", "bg_deconv2d_wgrad")
RGBCONV = ("bg_rgbconv_fwd", "bg_rgbconv_dgrad", "bg_rgbconv_wgrad")          # (these emit no bg_prof record)
RECORDED = CONV + RGBCONV + ("bg_attention16_fwd", "bg_attention16_bwd", "bg_attention2_fwd", "bg_attention2_bwd",
                             "bg_gram16", "bg_gemm")
# profiled families the replay does not cover (none: every GEMM-family tag is replayed)
UNREPLAYED_TAGS = ()


def _addr(p):
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    return p.value or 0


def _struct(d):
    if isinstance(d, ctypes._Pointer):
        d = d.contents
    elif hasattr(d, "_obj"):                       # ctypes.byref(...)
        d = d._obj
    return tuple(getattr(d, f[0]) for f in d._fields_)


class Call:
    """One unique launch: entry name, descriptor fields, flags, and the pointer alignments (mod 16 bytes) seen."""

    def __init__(self, name, desc, flags, align):
        self.name, self.desc, self.flags, self.align = name, desc, flags, align
        self.count = 1

    def key(self):
        return (self.name, self.desc, tuple(sorted(self.flags.items())), self.align)


def _describe(name, a):
    al = lambda *ps: tuple(_addr(p) % 16 for p in ps)          # noqa: E731
    if name in ("bg_conv2d_fwd", "bg_deconv2d_fwd"):
        d, x, w, bias, alpha, y, acc, ws, nb = a[:9]
        return _struct(d), dict(bias=bool(_addr(bias)), alpha=bool(_addr(alpha)), acc=int(acc), ws=int(nb) if _addr(ws)
                                else 0), al(x, w, y)
    if name == "bg_deconv2d_fwd_stats":
        d, x, w, bias, alpha, y, acc, sums, sws, snb, ws, nb = a[:12]
        return _struct(d), dict(bias=bool(_addr(bias)), alpha=bool(_addr(alpha)), acc=int(acc), stats_ws=int(snb),
                                ws=int(nb) if _addr(ws) else 0), al(x, w, y)
    if name in ("bg_conv2d_dgrad", "bg_deconv2d_dgrad"):
        d, dy, w, alpha, dx, acc, ws, nb = a[:8]
        return _struct(d), dict(alpha=bool(_addr(alpha)), acc=int(acc), ws=int(nb) if _addr(ws) else 0), al(dy, w, dx)
    if name in ("bg_conv2d_wgrad", "bg_deconv2d_wgrad"):
        d, x, dy, dw, ws, nb = a[:6]
        return _struct(d), dict(ws=int(nb) if _addr(ws) else 0), al(x, dy, dw)
    if name == "bg_rgbconv_fwd":
        d, x, w, bias, y, acc = a[:6]
        return _struct(d), dict(bias=bool(_addr(bias)), acc=int(acc)), al(x, w, y)
    if name == "bg_rgbconv_dgrad":
        d, dy, w, dx, acc = a[:5]
        return _struct(d), dict(acc=int(acc)), al(dy, w, dx)
    if name == "bg_rgbconv_wgrad":
        d, x, dy, dw, ws, nb = a[:6]
        return _struct(d), dict(ws=int(nb) if _addr(ws) else 0), al(x, dy, dw)
    if name == "bg_attention2_fwd":
        q, k, v, o, lse = a[:5]
        return tuple(int(t) for t in a[5:10]), {}, al(q, k, v, o)
    if name == "bg_attention2_bwd":
        q, k, v, o, do, lse, dq, dk, dv, delta = a[:10]
        return tuple(int(t) for t in a[10:15]), {}, al(q, k, v, o, do, dq, dk, dv)
    if name == "bg_attention16_fwd":
        D, q, k, v, o, lse = a[:6]
        return _struct(D), {}, al(q, k, v, o)
    if name == "bg_attention16_bwd":
        D, q, k, v, o, do, lse, dq, dk, dv, delta = a[:11]
        flags = dict(dq=bool(_addr(dq)), dk=bool(_addr(dk)), dv=bool(_addr(dv)))
        return _struct(D), flags, al(q, k, v, o, do, dq, dk, dv)
    if name == "bg_gram16":
        a_, rows, cols, ld, out, ws, nb = a[:7]
        return (int(rows), int(cols), int(ld)), dict(ws=int(nb) if _addr(ws) else 0), al(a_, out)
    if name == "bg_gemm":
        d, A, B, bias, alpha, C, acc, ws, nb = a[:9]
        return _struct(d), dict(bias=bool(_addr(bias)), alpha=bool(_addr(alpha)), acc=int(acc),
                                ws=int(nb) if _addr(ws) else 0), al(A, B, C)
    raise KeyError(name)


class _Proxy:
    def __init__(self, L, rec):
        self._L, self._rec = L, rec

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if name not in RECORDED:
            return fn
        rec = self._rec

        def wrapped(*a):
            rec.note(name, a)
            return fn(*a)
        return wrapped


class Recorder:
    """``with Recorder() as rec: <one iteration>`` -> rec.calls (unique launches, first-seen order) and rec.prof (the
    iteration's set of (tag, kernel symbol) pairs from bg_prof_dump)."""

    def __init__(self):
        self.calls = collections.OrderedDict()
        self.prof = set()

    def note(self, name, a):
        desc, flags, align = _describe(name, a)
        c = Call(name, desc, flags, align)
        k = c.key()
        if k in self.calls:
            self.calls[k].count += 1
        else:
            self.calls[k] = c

    def __enter__(self):
        import biggan_tensorflow_amd  # noqa: F401
        from biggan_tensorflow_amd import functional as Fn, hip
        self._mods = (Fn, hip)
        self._saved = (Fn.lib, hip.lib)
        L = hip.lib()
        proxy = _Proxy(L, self)
        Fn.lib = hip.lib = lambda: proxy
        torch.cuda.synchronize()
        L.bg_prof_reset()
        L.bg_prof_enable(1)
        return self

    def __exit__(self, *exc):
        Fn, hip = self._mods
        Fn.lib, hip.lib = self._saved
        torch.cuda.synchronize()
        self.prof = prof_take(hip.lib())
        return False


def prof_take(L):
    """The (tag, kernel) set recorded since the last reset; profiling is switched off and the records cleared."""
    fd, path = tempfile.mkstemp(suffix=".tsv")
    os.close(fd)
    try:
        assert L.bg_prof_dump(path.encode()) == 0
        with open(path) as fh:
            next(fh)
            out = {tuple(line.rstrip("\n").split("\t")[:2]) for line in fh if line.strip()}
    finally:
        os.unlink(path)
        L.bg_prof_reset()
        L.bg_prof_enable(0)
    return out


# ------------------------------------------------------------------------------------------
# replay buffers
# ------------------------------------------------------------------------------------------
class Buf:
    """A tensor of `numel` elements at byte offset `align` (mod 16) inside a raw byte buffer with GUARD sentinel bytes
    on both sides.  ``view`` is what the launch touches: ``shape`` (contiguous) or a (``size``, ``stride``) view, e.g. a
    column slice; every other byte must come back unchanged.  ``y0`` (nullable): the values ``prefill`` puts in the
    view (an accumulating output's initial value, an input that the launch also writes); None = NaN."""

    def __init__(self, numel, dtype, device, align=0, shape=None, size=None, stride=None):
        es = torch.tensor([], dtype=dtype).element_size()
        self.dtype, self.numel, self.nbytes = dtype, numel, numel * es
        self.off = GUARD + align
        self.raw = torch.full((self.off + self.nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        self.flat = self.raw[self.off:self.off + self.nbytes].view(dtype)
        self.size, self.stride = size, stride
        if size is not None:
            self.view = self.flat.as_strided(size, stride)
        else:
            self.view = self.flat.view(shape if shape is not None else (numel,))
        self.y0 = None
        self._mask = None

    def ptr(self):
        return ctypes.c_void_p(self.flat.data_ptr())

    def mask(self):
        if self._mask is None:
            m = torch.zeros(self.numel, dtype=torch.bool, device=self.flat.device)
            m.as_strided(self.size, self.stride).fill_(True)
            self._mask = m
        return self._mask

    def prefill(self):
        """Sentinel everywhere, then y0 or NaN in the launch's view (scratch buffers: sentinel only)."""
        self.raw.fill_(SENTINEL)
        if self.dtype == torch.uint8:
            return
        if self.y0 is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(self.y0.reshape(self.view.shape))

    def guards_ok(self):
        ok = bool((self.raw[:self.off] == SENTINEL).all())
        ok = ok and bool((self.raw[self.off + self.nbytes:] == SENTINEL).all())
        if ok and self.size is not None:
            b = self.raw[self.off:self.off + self.nbytes].view(self.numel, -1)
            ok = bool((b[~self.mask()] == SENTINEL).all())
        return ok


def mirror_mask(d, device):
    """[H, W, 1] float64: 1 on the pixels of a reflect-padded conv input that receive mirrored padded taps."""
    def axis(n, no):
        hp = (no - 1) * d.stride + d.k
        m = torch.bincount(pad_index(n, d.pad_lo, hp, PAD_REFLECT), minlength=n + 1)[:n] > 1
        return m.to(device)
    mh, mw = axis(d.H, d.Ho), axis(d.W, d.Wo)
    return (mh[:, None] | mw[None, :]).double()[..., None]


def dgrad_ring_form(d):
    """Whether the bf16-resident input gradient of reflect-padded conv `d` takes the ring form (plain launch + mirrored-tap
    launches) and not the padded grid + fold: the rule of dgrad_ring_ok (csrc/igemm.hip), BG_DGRAD_RING included."""
    e = os.environ.get("BG_DGRAD_RING")
    if e is not None and e.strip() == "0":
        return False
    forced = e is not None and e.strip() == "1"
    need = 32 if d.H >= 32 else (96 if d.H >= 16 else 160)
    if not forced and d.N < need:
        return False
    return (d.pad_mode == PAD_REFLECT and d.pad_lo == 1 and d.k == 3 and d.stride in (1, 2) and d.H >= 4 and d.W >= 4 and
            d.H % d.stride == 0 and d.W % d.stride == 0 and d.Ho == d.H // d.stride and d.Wo == d.W // d.stride)


def bf16_exact(shape, gen, device, scale=1.0, dtype=torch.float32):
    t = (torch.randn(shape, generator=gen, device=device) * scale).to(torch.bfloat16)
    return t.to(dtype)


def _dt(code):
    return torch.bfloat16 if code == BF16 else torch.float32


def image_subset(n):
    """Images compared for forward / input-gradient outputs when the batch is large: the first, the last, and pairs
    across the image boundaries that 16 .. 256-row M tiles straddle on 4 x 4 and 8 x 8 maps."""
    pick = {0, 1, n - 2, n - 1, n // 2 - 1, n // 2}
    for b in (2, 4, 8, 16, 32, 64):
        pick.update((b - 1, b, 3 * b - 1, 3 * b))
    return sorted(i for i in pick if 0 <= i < n)


# ------------------------------------------------------------------------------------------
# replay
# ------------------------------------------------------------------------------------------
class Failure(AssertionError):
    pass


class Replayer:
    """Replays Calls through the library; ``subset_over`` = batch size above which fwd / dgrad / attention outputs are
    compared on ``image_subset`` only (every output is still checked for unwritten NaN and guard bands in full)."""

    def __init__(self, L, device="cuda", seed=1234, subset_over=16, stats=None):
        self.L, self.dev = L, torch.device(device)
        self.gen = torch.Generator(device=self.dev).manual_seed(seed)
        self.subset_over = subset_over
        self.stats = stats if stats is not None else GateStats()
        self.failures = []
        self.entry = "?"

    def stream(self):
        from biggan_tensorflow_amd import hip
        return hip.stream()

    # -- helpers
    def rnd(self, shape, dtype, align=0, scale=1.0):
        n = math.prod(shape)
        b = Buf(n, dtype, self.dev, align, shape=shape)
        b.view.copy_(bf16_exact(shape, self.gen, self.dev, scale, dtype))
        return b

    def out(self, shape, dtype, align=0, acc=False):
        b = Buf(math.prod(shape), dtype, self.dev, align, shape=shape)
        b.y0 = bf16_exact(shape, self.gen, self.dev, 1.0, dtype) if acc else None
        return b

    def ws(self, nbytes):
        return Buf(max(int(nbytes), 16), torch.uint8, self.dev) if nbytes else None

    def check(self, rc, what):
        if rc != 0:
            raise Failure("%s: %s" % (what, self.L.bg_last_error().decode()))

    def _twice(self, run, outs):
        """Run the launch twice, each time from the same prefill of its outputs (the first run under bg_prof: its
        (tag, kernel) pairs join self.prof).  -> (kernel symbol, error or None): outputs bit-identical, guard bands and
        foreign columns untouched (scratch buffers: guard bands only)."""
        L = self.L
        first = None
        for rep in range(2):
            for o in outs:
                o.prefill()
            torch.cuda.synchronize(self.dev)
            if rep == 0:
                L.bg_prof_reset()
                L.bg_prof_enable(1)
                try:
                    run()
                finally:
                    got = prof_take(L)
                self.prof |= got
                kern = " + ".join(sorted({k for _, k in got})) or self.entry      # (rgbconv: no bg_prof record)
                self.stats.launch(kern)
                first = [o.raw.clone() for o in outs if o.dtype != torch.uint8]
            else:
                run()
        torch.cuda.synchronize(self.dev)
        for o, f in zip([o for o in outs if o.dtype != torch.uint8], first):
            if not torch.equal(o.raw, f):
                return kern, "not bit-reproducible"
        for o in outs:
            if not o.guards_ok():
                return kern, "wrote outside its output (guard band / foreign columns)"
        return kern, None

    def record(self, kernel, what, got, ref, E):
        ok, ratio, above, below, nbad = gate(got, ref, E)
        self.stats.add(kernel, ratio, above, below)
        if not ok:
            g = got.double()
            if got.dtype == torch.bfloat16:
                lo, hi = (ref - E).to(got.dtype).double(), (ref + E).to(got.dtype).double()
            else:
                lo, hi = ref - E - U32 * ref.abs(), ref + E + U32 * ref.abs()
            bad = ~((g >= lo) & (g <= hi))
            where = [tuple(int(i) for i in ix) for ix in bad.nonzero()[:3].tolist()]
            detail = "; ".join("at %s got %.9g ref %.9g E %.3g" % (ix, g[ix].item(), ref[ix].item(), E[ix].item())
                               for ix in where)
            self.failures.append("%s %s: %d of %d elements outside the bound (%s)" % (kernel, what, nbad, got.numel(),
                                                                                     detail))
        return ok

    def fail(self, kernel, msg):
        self.failures.append("%s: %s" % (kernel, msg))

    # -- entry points
    def replay(self, c):
        self.entry = c.name
        fn = getattr(self, "_" + c.name[3:])
        return fn(c)

    def _conv_common(self, c):
        from biggan_tensorflow_amd import hip
        d = hip.BgConvDesc(*c.desc)
        return d

    def _weights(self, c, d, deconv, fwd):
        """fp32 bf16-exact kernel in the variable's layout, and the buffer the call reads (packed when w_packed)."""
        k = d.k
        shape = (k, k, d.Cout, d.Cin) if deconv else (k, k, d.Cin, d.Cout)
        scale = 1.0 / math.sqrt(k * k * (d.Cin if fwd else d.Cout))
        w = bf16_exact(shape, self.gen, self.dev, scale)
        if not d.w_packed:
            b = Buf(w.numel(), torch.float32, self.dev, c.align[1])
            b.flat.copy_(w.reshape(-1))
            return w, b
        pp = torch.empty(w.numel(), dtype=torch.bfloat16, device=self.dev)
        pt = torch.empty(w.numel(), dtype=torch.bfloat16, device=self.dev)
        self.check(self.L.bg_weight_pack(ctypes.c_void_p(w.data_ptr()), k * k, shape[2], shape[3],
                                         ctypes.c_void_p(pp.data_ptr()), ctypes.c_void_p(pt.data_ptr()), self.stream()),
                   "bg_weight_pack")
        # conv: fwd reads [kk][Cout][Cin] = pack_t, dgrad [kk][Cin][Cout] = pack_p; deconv: fwd pack_p, dgrad pack_t
        use = (pp if fwd else pt) if deconv else (pt if fwd else pp)
        b = Buf(w.numel(), torch.bfloat16, self.dev, c.align[1])
        b.flat.copy_(use)
        return w, b

    def _sel(self, n):
        return list(range(n)) if n <= self.subset_over else image_subset(n)

    def _fwd(self, c, deconv):
        L = self.L
        d = self._conv_common(c)
        f = c.flags
        x = self.rnd((d.N, d.H, d.W, d.Cin), _dt(d.x_dtype), c.align[0])
        w, wb = self._weights(c, d, deconv, True)
        bias = bf16_exact((d.Cout,), self.gen, self.dev) if f.get("bias") else None
        alpha = torch.full((1,), 0.5, device=self.dev) if f.get("alpha") else None
        y = self.out((d.N, d.Ho, d.Wo, d.Cout), _dt(d.y_dtype), c.align[2], acc=bool(f["acc"]))
        ws = self.ws(f.get("ws", 0))
        stats = "stats_ws" in f
        sums = Buf(2 * d.Cout, torch.float64, self.dev) if stats else None
        sws = self.ws(f.get("stats_ws", 0))
        P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731

        def run():
            if c.name == "bg_rgbconv_fwd":
                rc = L.bg_rgbconv_fwd(d, x.ptr(), wb.ptr(), P(bias), y.ptr(), f["acc"], self.stream())
            elif stats:
                rc = L.bg_deconv2d_fwd_stats(d, x.ptr(), wb.ptr(), P(bias), P(alpha), y.ptr(), f["acc"], sums.ptr(),
                                             sws.ptr() if sws else None, f["stats_ws"], ws.ptr() if ws else None,
                                             f["ws"], self.stream())
            else:
                ent = L.bg_deconv2d_fwd if deconv else L.bg_conv2d_fwd
                rc = ent(d, x.ptr(), wb.ptr(), P(bias), P(alpha), y.ptr(), f["acc"], ws.ptr() if ws else None, f["ws"],
                         self.stream())
            self.check(rc, c.name)
        outs = [y] + ([sums] if stats else []) + [b for b in (ws, sws) if b is not None]
        return d, x, w, bias, alpha, y, sums, run, outs

    def _conv_or_deconv_fwd(self, c, deconv):
        d, x, w, bias, alpha, y, sums, run, outs = self._fwd(c, deconv)
        kern, err = self._twice(run, outs)
        if err:
            return self.fail(kern, "%s %s" % (c.name, err))
        yv = y.view
        if y.y0 is None and bool(torch.isnan(yv.float()).any()):
            return self.fail(kern, "%s left outputs unwritten" % c.name)
        sel = self._sel(d.N)
        idx = torch.tensor(sel, device=self.dev)
        xs = x.view.index_select(0, idx).double()
        ref_fn = (lambda xx, ww: deconv_fwd(xx, ww, d.stride, d.pad_lo, d.Ho, d.Wo)) if deconv else \
            (lambda xx, ww: conv_fwd(xx, ww, d.stride, d.pad_lo, d.Ho, d.Wo, d.pad_mode))
        a = 0.5 if alpha is not None else 1.0
        ref = a * ref_fn(xs, w.double())
        A = a * ref_fn(xs.abs(), w.double().abs())
        if bias is not None:
            ref = ref + bias.double()
            A = A + bias.double().abs()
        if y.y0 is not None:
            y0 = y.y0.view(yv.shape).index_select(0, idx).double()
            ref, A = ref + y0, A + y0.abs()
        got = yv.index_select(0, idx)
        self.record(kern, c.name, got, ref, bound(A, d.k * d.k * d.Cin))
        if sums is not None:
            ys = yv.double()
            s1, s2 = ys.sum((0, 1, 2)), (ys * ys).sum((0, 1, 2))
            a1 = ys.abs().sum((0, 1, 2))
            n = d.N * d.Ho * d.Wo
            self.record(kern, c.name + " stats", sums.view[:d.Cout].float(), s1, bound(a1, n))
            self.record(kern, c.name + " stats", sums.view[d.Cout:].float(), s2, bound(s2, n))
            # (the fp64 sums are compared as fp32 values against an fp32-accumulation bound: partial rows are fp32)

    def _conv2d_fwd(self, c):
        return self._conv_or_deconv_fwd(c, False)

    def _deconv2d_fwd(self, c):
        return self._conv_or_deconv_fwd(c, True)

    def _deconv2d_fwd_stats(self, c):
        return self._conv_or_deconv_fwd(c, True)

    # bg_rgbconv_*: the same three functions as bg_conv2d_* (fp32 tensors, stride 1, <= 3 output channels) on direct
    # vector-ALU kernels - fp32 FMA chains over the same terms, so the same references and the same bound(A, K)
    def _rgbconv_fwd(self, c):
        return self._conv_or_deconv_fwd(c, False)

    def _rgbconv_dgrad(self, c):
        return self._dgrad(c, False)

    def _rgbconv_wgrad(self, c):
        return self._wgrad(c, False)

    def _dgrad(self, c, deconv):
        L = self.L
        d = self._conv_common(c)
        f = c.flags
        dy = self.rnd((d.N, d.Ho, d.Wo, d.Cout), _dt(d.y_dtype), c.align[0])
        w, wb = self._weights(c, d, deconv, False)
        alpha = torch.full((1,), 0.5, device=self.dev) if f.get("alpha") else None
        dx = self.out((d.N, d.H, d.W, d.Cin), _dt(d.x_dtype), c.align[2], acc=bool(f["acc"]))
        ws = self.ws(f.get("ws", 0))
        ent = L.bg_deconv2d_dgrad if deconv else L.bg_conv2d_dgrad

        def run():
            if c.name == "bg_rgbconv_dgrad":
                return self.check(L.bg_rgbconv_dgrad(d, dy.ptr(), wb.ptr(), dx.ptr(), f["acc"], self.stream()), c.name)
            ap = None if alpha is None else ctypes.c_void_p(alpha.data_ptr())
            self.check(ent(d, dy.ptr(), wb.ptr(), ap, dx.ptr(), f["acc"], ws.ptr() if ws else None, f["ws"],
                           self.stream()), c.name)
        kern, err = self._twice(run, [dx] + ([ws] if ws else []))
        if err:
            return self.fail(kern, "%s %s" % (c.name, err))
        if dx.y0 is None and bool(torch.isnan(dx.view.float()).any()):
            return self.fail(kern, "%s left outputs unwritten" % c.name)
        idx = torch.tensor(self._sel(d.N), device=self.dev)
        dys = dy.view.index_select(0, idx).double()
        if deconv:
            fn = lambda g, ww: deconv_dgrad(g, ww, d.stride, d.pad_lo, d.H, d.W)                 # noqa: E731
            K = d.k * d.k * d.Cout
        else:
            fn = lambda g, ww: conv_dgrad(g, ww, d.stride, d.pad_lo, d.H, d.W, d.pad_mode)       # noqa: E731
            K = d.k * d.k * d.Cout * (4 if d.pad_mode == PAD_REFLECT else 1)
        a = 0.5 if alpha is not None else 1.0
        ref, A = a * fn(dys, w.double()), a * fn(dys.abs(), w.double().abs())
        extra = None
        if not deconv and d.pad_mode == PAD_REFLECT and d.x_dtype == BF16:
            # the bf16 input gradient of a reflect-padded conv is rounded once more where the mirrored taps land: the
            # padded-grid form stores the grid in bf16 before folding it, the ring form adds the mirrored taps to the
            # plain launch's bf16 output.  One bf16 unit of the partial sum on those pixels (rows / columns whose padded
            # source appears twice); every other pixel keeps the single-rounding bracket.  The padded-grid form that
            # ACCUMULATES rounds twice on every pixel: reflect_fold_kernel (csrc/igemm16.hip) reads the bf16 grid, adds the
            # old dx in fp32 and rounds the sum to bf16 - so there the unit of the grid's rounding applies everywhere
            mask = mirror_mask(d, self.dev)
            if dx.y0 is not None and not dgrad_ring_form(d) and (d.pad_lo > 0 or bool(mask.any())):
                mask = torch.ones_like(mask)
            extra = U16 * A * mask
        if dx.y0 is not None:
            y0 = dx.y0.view(dx.view.shape).index_select(0, idx).double()
            ref, A = ref + y0, A + y0.abs()
        self.record(kern, c.name, dx.view.index_select(0, idx), ref, bound(A, K, extra))

    def _conv2d_dgrad(self, c):
        return self._dgrad(c, False)

    def _deconv2d_dgrad(self, c):
        return self._dgrad(c, True)

    def _wgrad(self, c, deconv):
        L = self.L
        d = self._conv_common(c)
        f = c.flags
        x = self.rnd((d.N, d.H, d.W, d.Cin), _dt(d.x_dtype), c.align[0])
        dy = self.rnd((d.N, d.Ho, d.Wo, d.Cout), _dt(d.y_dtype), c.align[1])
        shape = (d.k, d.k, d.Cout, d.Cin) if deconv else (d.k, d.k, d.Cin, d.Cout)
        dw = self.out(shape, torch.float32, c.align[2])
        ws = self.ws(f["ws"])
        ent = L.bg_deconv2d_wgrad if deconv else L.bg_conv2d_wgrad
        if c.name == "bg_rgbconv_wgrad":
            ent = L.bg_rgbconv_wgrad

        def run():
            self.check(ent(d, x.ptr(), dy.ptr(), dw.ptr(), ws.ptr() if ws else None, f["ws"], self.stream()), c.name)
        kern, err = self._twice(run, [dw] + ([ws] if ws else []))
        if err:
            return self.fail(kern, "%s %s" % (c.name, err))
        xd, gd = x.view.double(), dy.view.double()
        if deconv:
            ref, A = deconv_wgrad(xd, gd, d.k, d.stride, d.pad_lo), deconv_wgrad(xd.abs(), gd.abs(), d.k, d.stride,
                                                                                 d.pad_lo)
            K = d.N * d.H * d.W
        else:
            ref = conv_wgrad(xd, gd, d.k, d.stride, d.pad_lo, d.pad_mode)
            A = conv_wgrad(xd.abs(), gd.abs(), d.k, d.stride, d.pad_lo, d.pad_mode)
            K = d.N * d.Ho * d.Wo
        self.record(kern, c.name, dw.view, ref, bound(A, K))

    def _conv2d_wgrad(self, c):
        return self._wgrad(c, False)

    def _deconv2d_wgrad(self, c):
        return self._wgrad(c, True)

    def _gram16(self, c):
        rows, cols, ld = c.desc
        a = self.rnd((rows, ld), torch.bfloat16, c.align[0])
        out = self.out((cols, cols), torch.float32, c.align[1])
        ws = self.ws(c.flags["ws"])

        def run():
            self.check(self.L.bg_gram16(a.ptr(), rows, cols, ld, out.ptr(), ws.ptr() if ws else None, c.flags["ws"],
                                        self.stream()), "bg_gram16")
        kern, err = self._twice(run, [out] + ([ws] if ws else []))
        if err:
            return self.fail(kern, "bg_gram16 " + err)
        m = a.view[:, :cols].double()
        self.record(kern, "bg_gram16", out.view, m.t() @ m, bound(m.abs().t() @ m.abs(), rows))

    def _gemm(self, c):
        from biggan_tensorflow_amd import hip
        d = hip.BgGemmDesc(*c.desc)
        f = c.flags
        ra, ca = (d.K, d.M) if d.transA else (d.M, d.K)
        rb, cb = (d.N, d.K) if d.transB else (d.K, d.N)
        na = (d.batch - 1) * d.strideA + (ra - 1) * d.lda + ca
        nb_ = (d.batch - 1) * d.strideB + (rb - 1) * d.ldb + cb
        nc = (d.batch - 1) * d.strideC + (d.M - 1) * d.ldc + d.N
        A = Buf(na, torch.float32, self.dev, c.align[0])
        A.flat.copy_(bf16_exact((na,), self.gen, self.dev))
        B = Buf(nb_, torch.float32, self.dev, c.align[1])
        B.flat.copy_(bf16_exact((nb_,), self.gen, self.dev))
        Cb = Buf(nc, torch.float32, self.dev, c.align[2], size=(d.batch, d.M, d.N), stride=(d.strideC, d.ldc, 1))
        Cb.y0 = bf16_exact((d.batch, d.M, d.N), self.gen, self.dev) if f["acc"] else None
        bias = bf16_exact((d.N,), self.gen, self.dev) if f["bias"] else None
        alpha = torch.full((1,), 0.5, device=self.dev) if f["alpha"] else None
        ws = self.ws(f["ws"])
        P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731

        def run():
            self.check(self.L.bg_gemm(d, A.ptr(), B.ptr(), P(bias), P(alpha), Cb.ptr(), f["acc"],
                                      ws.ptr() if ws else None, f["ws"], self.stream()), "bg_gemm")
        kern, err = self._twice(run, [Cb] + ([ws] if ws else []))
        if err:
            return self.fail(kern, "bg_gemm " + err)
        Av = A.flat.double().as_strided((d.batch, ra, ca), (d.strideA, d.lda, 1))
        Bv = B.flat.double().as_strided((d.batch, rb, cb), (d.strideB, d.ldb, 1))
        opA = Av.transpose(1, 2) if d.transA else Av
        opB = Bv.transpose(1, 2) if d.transB else Bv
        a = 0.5 if alpha is not None else 1.0
        ref, Aabs = a * (opA @ opB), a * (opA.abs() @ opB.abs())
        if bias is not None:
            ref, Aabs = ref + bias.double(), Aabs + bias.double().abs()
        if Cb.y0 is not None:
            ref, Aabs = ref + Cb.y0.double(), Aabs + Cb.y0.double().abs()
        self.record(kern, "bg_gemm", Cb.view, ref, bound(Aabs, d.K))

    # -- attention
    def _attn_desc(self, c):
        """-> (D, element type, unit roundoff of P / dS / the outputs).  bg_attention16_*: the recorded BgAttn16Desc, bf16;
        bg_attention2_*: (B, N, Nk, d, dv) as the same fields with the strides of contiguous fp32 tensors."""
        if c.name.startswith("bg_attention16"):
            from biggan_tensorflow_amd import hip
            return hip.BgAttn16Desc(*c.desc), torch.bfloat16, U16
        B, N, Nk, d, dv = c.desc
        D = collections.namedtuple("Attn2Desc", "B N Nk d dv ldq sq ldk sk ldv sv ldo so ldg sg lddq sdq lddk sdk lddv sdv")(
            B, N, Nk, d, dv, d, N * d, d, Nk * d, dv, Nk * dv, dv, N * dv, dv, N * dv, d, N * d, d, Nk * d, dv, Nk * dv)
        return D, torch.float32, U32

    def _attn_bufs(self, D, c, dtype=torch.bfloat16):
        """q, k, v, o as column slices of [B, rows, ld] buffers with the recorded strides."""
        def sl(rows, width, ld, s, align):
            n = (D.B - 1) * s + (rows - 1) * ld + width
            return Buf(n, dtype, self.dev, align, size=(D.B, rows, width), stride=(s, ld, 1))
        return sl

    def _attn_inputs(self, D, c, dtype=torch.bfloat16):
        sl = self._attn_bufs(D, c, dtype)
        q = sl(D.N, D.d, D.ldq, D.sq, c.align[0])
        k = sl(D.Nk, D.d, D.ldk, D.sk, c.align[1])
        v = sl(D.Nk, D.dv, D.ldv, D.sv, c.align[2])
        for b, scale in ((q, 0.5), (k, 0.5), (v, 1.0)):
            b.y0 = bf16_exact(b.size, self.gen, self.dev, scale, dtype)
            b.prefill()
        return sl, q, k, v

    def _attn16_fwd_ref(self, q, k, v, sel):
        """float64 o, lse, P, and the per-row relative error coefficient of P (S error, bf16 P, exp argument)."""
        qd, kd, vd = (t.view.index_select(0, sel).double() for t in (q, k, v))
        S = qd @ kd.transpose(1, 2)
        lse = torch.logsumexp(S, dim=2)
        P = torch.exp(S - lse[..., None])
        eS = (8.0 * math.sqrt(qd.shape[2]) + 2.0) * U32 * (qd.abs() @ kd.abs().transpose(1, 2))
        rel = 2.0 * eS.amax(2) + 4.0 * U32 * (S.abs().amax(2) + lse.abs() + 2.0)
        return qd, kd, vd, S, lse, P, rel

    def _attn_fwd(self, c):
        """bg_attention16_fwd and bg_attention2_fwd.  The bound's rounding points: the fp32 accumulation of P v over Nk keys
        (online-softmax rescaling included), P's own rounding U before the product (bf16 in attention16.hip; in
        attention.hip P stays fp32, so U = U32 stands for the rounding of exp's result), the output's division by the row
        sum, and `rel` (the S error through exp, the exponent's argument).  attention.hip has no rounding point beyond
        these: its S, P v and dP are fp32 MFMA chains, exp / log are the same v_exp_f32 / v_log_f32 forms."""
        D, dtype, U = self._attn_desc(c)
        sl, q, k, v = self._attn_inputs(D, c, dtype)
        o = sl(D.N, D.dv, D.ldo, D.so, c.align[3])
        lse = Buf(D.B * D.N, torch.float32, self.dev)

        def run():
            if dtype == torch.bfloat16:
                rc = self.L.bg_attention16_fwd(D, q.ptr(), k.ptr(), v.ptr(), o.ptr(), lse.ptr(), self.stream())
            else:
                rc = self.L.bg_attention2_fwd(q.ptr(), k.ptr(), v.ptr(), o.ptr(), lse.ptr(), D.B, D.N, D.Nk, D.d, D.dv,
                                              self.stream())
            self.check(rc, c.name)
        kern, err = self._twice(run, [o, lse])
        if err:
            return self.fail(kern, c.name + " " + err)
        if bool(torch.isnan(o.view.float()).any()) or bool(torch.isnan(lse.view).any()):
            return self.fail(kern, c.name + " left outputs unwritten")
        sel = torch.tensor(self._sel(D.B), device=self.dev)
        for part in torch.split(sel, max(1, (1 << 28) // (D.N * D.Nk))):
            qd, kd, vd, S, _, P, rel = self._attn16_fwd_ref(q, k, v, part)
            ref, lref = attn_fwd(qd, kd, vd)
            Pv = P @ vd.abs()
            E = bound(Pv, D.Nk, (U + rel)[..., None] * Pv)
            self.record(kern, c.name + " o", o.view.index_select(0, part), ref, E)
            lg = lse.view.view(D.B, D.N).index_select(0, part)
            self.record(kern, c.name + " lse", lg, lref, rel + 8.0 * U32 * (lref.abs() + 1.0))

    _attention16_fwd = _attention2_fwd = _attn_fwd

    def _attn_bwd(self, c):
        """bg_attention16_bwd (dq and / or dk + dv, per the recorded flags) and bg_attention2_bwd (always all three, delta
        computed by the call).  U = the rounding of P and of dS before their products: bf16 in attention16.hip, fp32 in
        attention.hip (U32: exp's result, the dS product)."""
        D, dtype, U = self._attn_desc(c)
        f = c.flags if dtype == torch.bfloat16 else dict(dq=True, dk=True, dv=True)
        sl, q, k, v = self._attn_inputs(D, c, dtype)
        o = sl(D.N, D.dv, D.ldo, D.so, c.align[3])
        do = sl(D.N, D.dv, D.ldg, D.sg, c.align[4])
        o.y0 = bf16_exact(o.size, self.gen, self.dev, 0.5, dtype)
        do.y0 = bf16_exact(do.size, self.gen, self.dev, 1.0, dtype)
        o.prefill()
        do.prefill()
        # lse from float64 (the forward's output, as fp32); delta = rowsum(dO o) for a dq-only call that reuses it
        qd, kd = q.view.double(), k.view.double()
        lse32 = torch.empty((D.B, D.N), dtype=torch.float32, device=self.dev)
        for part in torch.split(torch.arange(D.B, device=self.dev), max(1, (1 << 28) // (D.N * D.Nk))):
            lse32[part] = torch.logsumexp(qd[part] @ kd[part].transpose(1, 2), dim=2).float()
        del qd, kd
        lse = Buf(D.B * D.N, torch.float32, self.dev)
        lse.flat.copy_(lse32.reshape(-1))
        delta64 = (do.view.double() * o.view.double()).sum(2)
        delta = Buf(D.B * D.N, torch.float32, self.dev)
        dq_only = f["dq"] and not f["dk"]
        if dq_only:               # the dq-only call reads delta as the dk / dv call left it
            delta.y0 = delta64.float().reshape(-1)
            delta64 = delta.y0.view(D.B, D.N).double()
        outs = []
        dq = dk = dv = None
        if f["dq"]:
            dq = sl(D.N, D.d, D.lddq, D.sdq, c.align[5])
            outs.append(dq)
        if f["dk"]:
            dk = sl(D.Nk, D.d, D.lddk, D.sdk, c.align[6])
            outs.append(dk)
        if f["dv"]:
            dv = sl(D.Nk, D.dv, D.lddv, D.sdv, c.align[7])
            outs.append(dv)

        def run():
            if dtype == torch.bfloat16:
                rc = self.L.bg_attention16_bwd(D, q.ptr(), k.ptr(), v.ptr(), o.ptr(), do.ptr(), lse.ptr(),
                                               dq.ptr() if dq else None, dk.ptr() if dk else None,
                                               dv.ptr() if dv else None, delta.ptr(), self.stream())
            else:
                rc = self.L.bg_attention2_bwd(q.ptr(), k.ptr(), v.ptr(), o.ptr(), do.ptr(), lse.ptr(), dq.ptr(), dk.ptr(),
                                              dv.ptr(), delta.ptr(), D.B, D.N, D.Nk, D.d, D.dv, self.stream())
            self.check(rc, c.name)
        kern, err = self._twice(run, outs + [delta])
        if err:
            return self.fail(kern, c.name + " " + err)
        for b in outs:
            if bool(torch.isnan(b.view.float()).any()):
                return self.fail(kern, c.name + " left outputs unwritten")
        sel = torch.tensor(self._sel(D.B), device=self.dev)
        for part in torch.split(sel, max(1, (1 << 27) // (D.N * D.Nk))):
            qd, kd, vd, S, _, _, rel = self._attn16_fwd_ref(q, k, v, part)
            lsep = lse32.index_select(0, part).double()
            P = torch.exp(S - lsep[..., None])
            od, dod = o.view.index_select(0, part).double(), do.view.index_select(0, part).double()
            dlt = delta64.index_select(0, part)
            rdq, rdk, rdv = attn_bwd(qd, kd, vd, dod, P, dlt)
            # |.| term of dS: P (|dO| |v|^T + sum |dO| |o|); relative coefficient: bf16 dS, bf16 P, S error, dP sums
            T = P * (dod.abs() @ vd.abs().transpose(1, 2) + (dod.abs() * od.abs()).sum(2)[..., None])
            relb = (2.0 * U + rel + (8.0 * math.sqrt(D.dv) + 2.0) * U32)[..., None]
            if dq is not None:
                A = T @ kd.abs()
                self.record(kern, c.name + " dq", dq.view.index_select(0, part), rdq,
                            bound(A, D.Nk, (relb * T) @ kd.abs()))
            if dk is not None:
                A = T.transpose(1, 2) @ qd.abs()
                self.record(kern, c.name + " dk", dk.view.index_select(0, part), rdk,
                            bound(A, D.N, (relb * T).transpose(1, 2) @ qd.abs()))
            if dv is not None:
                A = P.transpose(1, 2) @ dod.abs()
                relp = (U + rel)[..., None]
                self.record(kern, c.name + " dv", dv.view.index_select(0, part), rdv,
                            bound(A, D.N, (relp * P).transpose(1, 2) @ dod.abs()))

    _attention16_bwd = _attention2_bwd = _attn_bwd


def replay_all(calls, L, subset_over=16, stats=None):
    """Replay every unique call; -> (GateStats, failures, replay prof set)."""
    r = Replayer(L, subset_over=subset_over, stats=stats)
    r.prof = set()
    for c in calls:
        try:
            r.replay(c)
        except Failure as e:
            r.failures.append(str(e))
    torch.cuda.synchronize()
    return r.stats, r.failures, r.prof


def comparable(prof):
    return {p for p in prof if not p[0].startswith(UNREPLAYED_TAGS)}
