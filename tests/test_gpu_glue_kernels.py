"""The batch-norm finalisers and the fp32 glue kernels of csrc/elementwise.hip - bg_bn_finalize, bg_bn_population,
bg_bn_bwd_finalize, bg_renorm_coeffs, bg_renorm_affine_fwd / _bwd, bg_box2_down / _up, bg_axpby, bg_add, bg_scale_add,
bg_scale_dev, bg_tanh_fwd / _bwd, bg_pad_channels, bg_weight_pack - against float64.

Every row of the case table of tests/glue_ref.py calls its entry point raw through ``hip.lib()`` under the rules of
tests/test_gpu_elementwise16.Runner: guarded buffers (launch_replay.Buf) for every input and output, outputs prefilled
with NaN - or with their initial value where the call updates in place: the moving and running statistics, ``*weight``,
``y`` of bg_axpby, the aliased outputs of the in-place forms - two runs that must agree bit for bit, inputs left
unchanged, and the per-element gate of launch_replay against the float64 reference with the bounds of glue_ref (routing
rows bit for bit).  One GateStats row per entry point records how much of each bound is used.

One composed case per family runs the wrappers of functional.py (BnActFn shared / conditional / renorm / inference,
BnGluFn, AvgPool2Fn, UpSample2Fn, ScaleAddFn, TanhFn) against float64 autograd through oracle/ref_ops.py under the chained stage
bounds."""
import ctypes
import time

import pytest
import torch

from tests import glue_ref as G
from tests import launch_replay as R
from tests.test_gpu_elementwise16 import Runner, _lib

pytestmark = pytest.mark.gpu

BIG = 1 << 20
F32 = torch.float32


class GlueRunner(Runner):
    ref = G

    def key_of(self, c):
        return G.ENTRY[c["op"]]

    alt_label = "aligned source"

    def wants_alt(self, c):
        """A bg_pad_channels row with the source 4 bytes off (the generic kernel) also runs the one-pixel-per-thread
        form on an aligned copy, into the same output: the bits must be the same."""
        return bool(c.get("off4"))

    def gate(self, label, got, ref, Eb):
        entry = self.key
        self.key = "%s: %s" % (entry, label)
        try:
            super().gate(label, got, ref, Eb)
            self.stats.add(entry, self.stats.rows[self.key][1])
        finally:
            self.key = entry

    def exact(self, label, got, want):
        entry = self.key
        self.key = "%s: %s (exact)" % (entry, label)
        try:
            super().exact(label, got, want)
            self.stats.add(entry, self.stats.rows[self.key][1])
        finally:
            self.key = entry

    def inb_at(self, t, align):
        """A guarded copy of t at byte offset ``align`` (mod 16), whatever its element type."""
        b = R.Buf(t.numel(), t.dtype, self.dev, align, shape=tuple(t.shape))
        b.view.copy_(t)
        b.src = t
        self.ins.append(b)
        return b

    def launcher(self, c, i):
        lib, st = self.L, self.hip.stream
        op = c["op"]
        P = lambda b: None if b is None else b.ptr()                # noqa: E731
        inb, outb = self.inb, self.outb
        if op == "bn_finalize":
            C = c["C"]
            s = inb(i["sums"])
            out = {"mean": outb((C,), F32), "rstd": outb((C,), F32)}
            if c["mm"]:
                out["moving_mean"] = outb((C,), F32, y0=i["mm0"])
            if c["mv"]:
                out["moving_var"] = outb((C,), F32, y0=i["mv0"])
            return (lambda: lib.bg_bn_finalize(P(s), i["count"], i["eps"], i["momentum"], c["unbiased"], P(out["mean"]),
                                               P(out["rstd"]), P(out.get("moving_mean")), P(out.get("moving_var")), C,
                                               st())), out
        if op == "bn_population":
            C = c["C"]
            pm, pv = inb(i["pop_mean"]), inb(i["pop_var"])
            out = {"mean": outb((C,), F32), "rstd": outb((C,), F32)}
            return (lambda: lib.bg_bn_population(P(pm), P(pv), i["eps"], P(out["mean"]), P(out["rstd"]), C, st())), out
        if op == "bn_bwd_finalize":
            N, C, ps = c["N"], c["C"], c["per_sample"]
            part, gamma = inb(i["part"]), inb(i["gamma"])
            shape = (N, C) if ps else (C,)                      # sized for their form: a shared call must not write [N, C]
            out = {"dgamma": outb(shape, F32), "dbeta": outb(shape, F32)}
            if c["dalpha"]:
                out["dalpha"] = outb((C,), F32)
            out["cm"] = outb((2 * C,), F32)
            return (lambda: lib.bg_bn_bwd_finalize(P(part), P(gamma), ps, i["count"], P(out["dgamma"]), P(out["dbeta"]),
                                                   P(out.get("dalpha")), P(out["cm"]), N, C, st())), out
        if op == "renorm_coeffs":
            C = c["C"]
            s = inb(i["sums"])
            out = {"r": outb((C,), F32), "d": outb((C,), F32), "ref_mean": outb((C,), F32, y0=i["ref_mean0"]),
                   "ref_scale": outb((C,), F32, y0=i["ref_scale0"])}
            if i.get("weight0") is not None:
                out["weight"] = outb((1,), F32, y0=i["weight0"])
            return (lambda: lib.bg_renorm_coeffs(P(s), i["count"], P(out["ref_mean"]), P(out["ref_scale"]),
                                                 c["scale_is_var"], P(out.get("weight")), i["eps"], i["rmin"], i["rmax"],
                                                 i["dmax"], i["decay"], i["fade"], c["update"], P(out["r"]), P(out["d"]), C,
                                                 st())), out
        if op == "renorm_affine_fwd":
            rows, C = c["rows"], c["C"]
            g, b, r, d = (inb(i[k]) for k in ("gamma", "beta", "r", "d"))
            out = {"gamma_eff": outb((rows, C), F32), "beta_eff": outb((rows, C), F32)}
            return (lambda: lib.bg_renorm_affine_fwd(P(g), P(b), P(r), P(d), P(out["gamma_eff"]), P(out["beta_eff"]), rows,
                                                     C, st())), out
        if op == "renorm_affine_bwd":
            rows, C = c["rows"], c["C"]
            g, b, r, d = (inb(i[k]) for k in ("dgamma_eff", "dbeta_eff", "r", "d"))
            out = {"dgamma": outb((rows, C), F32)}
            return (lambda: lib.bg_renorm_affine_bwd(P(g), P(b), P(r), P(d), P(out["dgamma"]), rows, C, st())), out
        if op in ("box2_down", "box2_up"):
            N, H, W, C = c["N"], c["H"], c["W"], c["C"]
            x = inb(i["x"])
            s = G.f32r(c["scale"])
            if op == "box2_down":
                y = outb((N, H // 2, W // 2, C), F32)
                return (lambda: lib.bg_box2_down(P(x), P(y), N, H, W, C, s, st())), {"y": y}
            y = outb((N, 2 * H, 2 * W, C), F32)
            return (lambda: lib.bg_box2_up(P(x), P(y), N, H, W, C, s, st())), {"y": y}
        if op == "axpby":
            n = c["n"]
            y = outb((n,), F32, y0=i.get("y0"))
            x = y if c["alias"] else inb(i["x"])
            return (lambda: lib.bg_axpby(P(x), i["a"], P(y), i["b"], n, st())), {"y": y}
        if op == "add":
            n = c["n"]
            b = inb(i["b"])
            y = outb((n,), F32, y0=i.get("y0"))
            a = y if c["alias"] else inb(i["a"])
            return (lambda: lib.bg_add(P(a), P(b), P(y), n, st())), {"y": y}
        if op == "scale_add":
            n = c["n"]
            o, g, x = inb(i["o"]), inb(i["gamma"]), inb(i["x"])
            y = outb((n,), F32)
            return (lambda: lib.bg_scale_add(P(o), P(g), P(x), P(y), n, st())), {"y": y}
        if op == "scale_dev":
            n = c["n"]
            s = inb(i["s"])
            y = outb((n,), F32, y0=i.get("y0"))
            x = y if c["alias"] else inb(i["x"])
            return (lambda: lib.bg_scale_dev(P(x), P(s), P(y), n, st())), {"y": y}
        if op == "tanh_fwd":
            x = inb(i["x"])
            y = outb(tuple(i["x"].shape), F32)
            return (lambda: lib.bg_tanh_fwd(P(x), P(y), i["x"].numel(), st())), {"y": y}
        if op == "tanh_bwd":
            y, dy = inb(i["y"]), inb(i["dy"])
            dx = outb(tuple(i["y"].shape), F32)
            return (lambda: lib.bg_tanh_bwd(P(y), P(dy), P(dx), i["y"].numel(), st())), {"dx": dx}
        if op == "pad_channels":
            outer, Cs, Cd, inner = c["outer"], c["Cs"], c["Cd"], c["inner"]
            src = self.inb_at(i["src"], 4 if c["off4"] else 0)
            dst = outb((outer, Cd, inner), G.tdt(c["ddt"]))
            if c["off4"]:
                fast = self.inb_at(i["src"], 0)
                self.call32 = lambda: lib.bg_pad_channels(P(fast), c["sdt"], P(dst), c["ddt"], outer, Cs, Cd, inner,
                                                          c["mode"], st())
            return (lambda: lib.bg_pad_channels(P(src), c["sdt"], P(dst), c["ddt"], outer, Cs, Cd, inner, c["mode"],
                                                st())), {"dst": dst}
        if op == "weight_pack":
            taps, Rr, Cc = c["taps"], c["R"], c["Cc"]
            w = inb(i["w"])
            pp, pt = outb((taps, Rr, Cc), torch.bfloat16), outb((taps, Cc, Rr), torch.bfloat16)
            return (lambda: lib.bg_weight_pack(P(w), taps, Rr, Cc, P(pp), P(pt), st())), {"pack_p": pp, "pack_t": pt}
        raise KeyError(op)


@pytest.mark.parametrize("op", G.OPS)
def test_entry_point_matches_float64(op):
    hip, lib = _lib()
    r = GlueRunner(hip, lib)
    t0 = time.time()
    todo = G.cases(op)
    for k, c in enumerate(todo):
        r.run(c, 7000 + k)
        big = G.numel(c) >= BIG
        r.ins, r.outs = [], []
        if big:
            torch.cuda.empty_cache()
    print("\n[%s] %d cases in %.1f s" % (G.ENTRY[op], len(todo), time.time() - t0))
    print(r.stats.table())
    assert not r.failures, "%d failures:\n%s" % (len(r.failures), "\n".join(r.failures[:20]))
    assert G.ENTRY[op] in r.stats.rows and r.stats.rows[G.ENTRY[op]][0] == len(todo)
    assert all(row[1] <= 1.0 for row in r.stats.rows.values())


def test_bad_arguments_are_rejected_and_launch_nothing():
    """BG_ERR_ARG with a message in bg_last_error, and no byte of any buffer involved changes: odd inner dimensions of
    bg_weight_pack, a mode that does not fit Cs -> Cd, bad clip ranges, pointers of bg_axpby / bg_add / bg_scale_add and -
    at C % 4 == 0 - of bg_box2_down / _up that are not 16-byte aligned, odd H or W of bg_box2_down, zero sizes."""
    hip, L = _lib()
    st = hip.stream
    dev = torch.device("cuda")
    bufs = [R.Buf(4096, F32, dev) for _ in range(6)]
    for b in bufs:
        b.y0 = torch.full((4096,), 3.0, device=dev)
        b.prefill()
    d64 = R.Buf(64, torch.float64, dev)
    d64.y0 = torch.ones(64, dtype=torch.float64, device=dev)
    d64.prefill()
    torch.cuda.synchronize()
    before = [b.raw.clone() for b in bufs + [d64]]
    a, b, c, d, e, f = (x.ptr() for x in bufs)
    off = lambda p, k=4: ctypes.c_void_p(p.value + k)                            # noqa: E731
    s = d64.ptr()

    def refused(rc, name):
        assert rc == G.ERR_ARG, (name, rc)
        assert name.encode() in L.bg_last_error(), (name, L.bg_last_error())

    refused(L.bg_weight_pack(a, 1, 3, 8, b, c, st()), "bg_weight_pack")
    refused(L.bg_weight_pack(a, 1, 8, 5, b, c, st()), "bg_weight_pack")
    refused(L.bg_weight_pack(a, 0, 8, 8, b, c, st()), "bg_weight_pack")
    refused(L.bg_pad_channels(a, hip.F32, b, hip.F32, 4, 3, 5, 1, 1, st()), "bg_pad_channels")
    refused(L.bg_pad_channels(a, hip.F32, b, hip.F32, 4, 3, 5, 1, 2, st()), "bg_pad_channels")
    refused(L.bg_pad_channels(a, hip.F32, b, hip.F32, 4, 8, 5, 1, 3, st()), "bg_pad_channels")
    refused(L.bg_pad_channels(a, hip.F32, b, hip.F32, 4, 3, 8, 1, 4, st()), "bg_pad_channels")
    refused(L.bg_pad_channels(a, hip.F32, b, hip.F32, 0, 3, 8, 1, 0, st()), "bg_pad_channels")
    refused(L.bg_pad_channels(a, hip.F32, b, hip.F32, 4, 3, 8, 0, 0, st()), "bg_pad_channels")
    for rmin, rmax, dmax in ((0.0, 1.0, 1.0), (2.0, 1.0, 1.0), (0.5, 2.0, -1.0)):
        refused(L.bg_renorm_coeffs(s, 8.0, a, b, 1, c, 1e-5, rmin, rmax, dmax, 0.99, 0.999, 1, d, e, 8, st()),
                "bg_renorm_coeffs")
    refused(L.bg_renorm_coeffs(s, 0.0, a, b, 1, c, 1e-5, 0.5, 2.0, 1.0, 0.99, 0.999, 1, d, e, 8, st()), "bg_renorm_coeffs")
    refused(L.bg_renorm_coeffs(s, 8.0, a, b, 1, c, 1e-5, 0.5, 2.0, 1.0, 0.99, 0.999, 1, d, e, 0, st()), "bg_renorm_coeffs")
    refused(L.bg_axpby(off(a), 1.0, b, 1.0, 64, st()), "bg_axpby")
    refused(L.bg_axpby(a, 1.0, off(b, 8), 1.0, 64, st()), "bg_axpby")
    refused(L.bg_axpby(a, 1.0, b, 1.0, 0, st()), "bg_axpby")
    refused(L.bg_add(off(a), b, c, 64, st()), "bg_add")
    refused(L.bg_add(a, off(b), c, 64, st()), "bg_add")
    refused(L.bg_add(a, b, off(c, 12), 64, st()), "bg_add")
    refused(L.bg_add(a, b, c, 0, st()), "bg_add")
    refused(L.bg_scale_add(off(a), d, b, c, 64, st()), "bg_scale_add")
    refused(L.bg_scale_add(a, d, off(b), c, 64, st()), "bg_scale_add")
    refused(L.bg_scale_add(a, d, b, off(c), 64, st()), "bg_scale_add")
    refused(L.bg_scale_add(a, d, b, c, 0, st()), "bg_scale_add")
    refused(L.bg_scale_dev(a, d, b, 0, st()), "bg_scale_dev")
    refused(L.bg_tanh_fwd(a, b, 0, st()), "bg_tanh_fwd")
    refused(L.bg_tanh_bwd(a, b, c, 0, st()), "bg_tanh_bwd")
    refused(L.bg_box2_down(a, b, 1, 3, 4, 8, 0.25, st()), "bg_box2_down")
    refused(L.bg_box2_down(a, b, 1, 4, 3, 8, 0.25, st()), "bg_box2_down")
    refused(L.bg_box2_down(a, b, 0, 4, 4, 8, 0.25, st()), "bg_box2_down")
    refused(L.bg_box2_down(off(a), b, 1, 4, 4, 8, 0.25, st()), "bg_box2_down")
    refused(L.bg_box2_down(a, off(b, 8), 1, 4, 4, 8, 0.25, st()), "bg_box2_down")
    refused(L.bg_box2_up(off(a), b, 1, 4, 4, 8, 1.0, st()), "bg_box2_up")
    refused(L.bg_box2_up(a, off(b), 1, 4, 4, 8, 1.0, st()), "bg_box2_up")
    refused(L.bg_box2_up(a, b, 1, 4, 0, 8, 1.0, st()), "bg_box2_up")
    refused(L.bg_bn_finalize(s, 0.0, 1e-5, 0.9, 0, a, b, c, d, 8, st()), "bg_bn_finalize")
    refused(L.bg_bn_finalize(s, 8.0, 1e-5, 0.9, 0, a, b, c, d, 0, st()), "bg_bn_finalize")
    refused(L.bg_bn_population(a, b, 1e-5, c, d, 0, st()), "bg_bn_population")
    refused(L.bg_bn_bwd_finalize(a, b, 0, 8.0, c, d, e, f, 0, 8, st()), "bg_bn_bwd_finalize")
    refused(L.bg_bn_bwd_finalize(a, b, 0, 0.0, c, d, e, f, 4, 8, st()), "bg_bn_bwd_finalize")
    refused(L.bg_renorm_affine_fwd(a, b, c, d, e, f, 0, 8, st()), "bg_renorm_affine_fwd")
    refused(L.bg_renorm_affine_bwd(a, b, c, d, e, 4, 0, st()), "bg_renorm_affine_bwd")
    torch.cuda.synchronize()
    for x, was in zip(bufs + [d64], before):
        assert torch.equal(x.raw, was)
    # C % 4 != 0 takes 4-byte accesses: the same offset is accepted there, and an aligned call goes through
    assert L.bg_box2_down(off(a), off(b), 1, 4, 4, 3, 0.25, st()) == 0
    assert L.bg_box2_down(a, b, 1, 4, 4, 8, 0.25, st()) == 0
    torch.cuda.synchronize()
    assert all(x.guards_ok() for x in bufs)


# ------------------------------------------------------------------------------------------
# composed: the wrappers of functional.py against the oracle
# ------------------------------------------------------------------------------------------
def _gate_all(stats, bad, family, items):
    for what, got, ref, Eb in items:
        ok, ratio, _, _, nbad = R.gate(got, ref.reshape(got.shape), Eb.reshape(got.shape))
        key = "%s %s" % (family, what)
        stats.launch(key)
        stats.add(key, ratio)
        if not ok:
            bad.append((key, nbad, ratio))


def test_composed_pooling_agrees_with_the_oracle():
    """AvgPool2Fn and UpSample2Fn forward and backward on the non-square map x[3, 6, 10, 12] / x[3, 3, 5, 12] against
    ref_ops.avg_pooling / up_sample and their float64 autograd gradients: the forward of one is the backward of the
    other, under the bounds of bg_box2_down (three sums; the scale 0.25 and 1 are exact) and bit for bit for bg_box2_up."""
    from oracle import ref_ops
    hip, lib = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(41)
    stats, bad = R.GateStats(), []
    x = torch.randn(3, 6, 10, 12, generator=gen, device=dev)
    dy = torch.randn(3, 3, 5, 12, generator=gen, device=dev)
    x64 = x.double().cpu().requires_grad_(True)
    yref = ref_ops.avg_pooling(x64)
    yref.backward(dy.double().cpu())
    xl = x.clone().requires_grad_(True)
    y = Fn.AvgPool2Fn.apply(xl)
    y.backward(dy)
    torch.cuda.synchronize()
    cd = dict(N=3, H=6, W=10, C=12, scale=0.25)
    b = G.box2_down(G.Ref, cd, dict(x=x))["y"]
    assert torch.equal(xl.grad.cpu().double(), x64.grad)                       # routing: exact
    _gate_all(stats, bad, "AvgPool2Fn", (("y", y.detach(), yref.detach().to(dev), b.e),))
    u = torch.randn(3, 3, 5, 12, generator=gen, device=dev)
    du = torch.randn(3, 6, 10, 12, generator=gen, device=dev)
    u64 = u.double().cpu().requires_grad_(True)
    uref = ref_ops.up_sample(u64)
    uref.backward(du.double().cpu())
    ul = u.clone().requires_grad_(True)
    up = Fn.UpSample2Fn.apply(ul)
    up.backward(du)
    torch.cuda.synchronize()
    assert torch.equal(up.detach().cpu().double(), uref.detach())
    bb = G.box2_down(G.Ref, dict(cd, scale=1.0), dict(x=du))["y"]
    _gate_all(stats, bad, "UpSample2Fn", (("dx", ul.grad, u64.grad.to(dev), bb.e),))
    print("\n" + stats.table())
    assert not bad, bad


def test_composed_scale_add_and_tanh_agree_with_autograd():
    """ScaleAddFn (gamma o + x: bg_scale_add forward, bg_scale_dev and a dot product backward) and TanhFn (bg_tanh_fwd /
    _bwd, the backward on the STORED fp32 output) at 3 x 5 x 7 x 9 = 945 elements against float64 autograd.  The bound of
    TanhFn's gradient chains the forward's: dx = dy (1 - y^2) with y carrying TANH_U units."""
    hip, lib = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(43)
    stats, bad = R.GateStats(), []
    shape = (3, 5, 7, 9)
    n = 945
    o, x, dy = (torch.randn(shape, generator=gen, device=dev) for _ in range(3))
    gamma = torch.tensor([0.37], device=dev)
    o64, x64, g64 = (t.double().requires_grad_(True) for t in (o, x, gamma))
    yref = g64 * o64 + x64
    yref.backward(dy.double())
    ol, xl, gl = (t.clone().requires_grad_(True) for t in (o, x, gamma))
    y = Fn.ScaleAddFn.apply(ol, gl, xl)
    y.backward(dy)
    torch.cuda.synchronize()
    c = dict(n=n)
    by = G.scale_add(G.Ref, c, dict(o=o.reshape(-1), x=x.reshape(-1), gamma=gamma))["y"]
    bo = G.scale_dev(G.Ref, dict(alias=False), dict(x=dy.reshape(-1), s=gamma))["y"]
    dot = (G.Ref.of(dy.reshape(-1)) * G.Ref.of(o.reshape(-1))).sum(0, n, keepdim=True)
    assert torch.equal(xl.grad, dy)
    _gate_all(stats, bad, "ScaleAddFn", (("y", y.detach(), yref.detach(), by.e), ("d_o", ol.grad, o64.grad, bo.e),
                                          ("d_gamma", gl.grad.reshape(1), g64.grad.reshape(1), dot.e)))
    t = torch.randn(shape, generator=gen, device=dev) * 2.0
    t64 = t.double().requires_grad_(True)
    zref = torch.tanh(t64)
    zref.backward(dy.double())
    tl = t.clone().requires_grad_(True)
    z = Fn.TanhFn.apply(tl)
    z.backward(dy)
    torch.cuda.synchronize()
    bz = G.tanh_fwd(G.Ref, c, dict(x=t.reshape(-1)))["y"]
    bd = G.tanh_bwd(G.Ref, c, dict(y=bz, dy=dy.reshape(-1)))["dx"]
    _gate_all(stats, bad, "TanhFn", (("y", z.detach(), zref.detach(), bz.e), ("dx", tl.grad, t64.grad, bd.e)))
    print("\n" + stats.table())
    assert not bad, bad


BN_SHAPE = (5, 3, 3, 72)


def _bn_setup(mode):
    """Inputs of one composed batch-norm case, drawn on the CPU (the same on every machine)."""
    gen = torch.Generator().manual_seed(51 + len(mode))
    N, H, W, C = BN_SHAPE
    rn = lambda *sh: torch.randn(*sh, generator=gen)                            # noqa: E731
    ru = lambda *sh: torch.rand(*sh, generator=gen)                             # noqa: E731
    x = rn(N, H, W, C) * 1.5 + 0.3
    gs = (N, C) if mode in ("cond", "renorm") else (C,)
    st = dict(unbiased=int(mode == "shared"), momentum=G.f32r(0.98), mm0=rn(C) * 0.5, mv0=ru(C) + 0.5,
              scale_is_var=1, ref_mean0=rn(C) * 0.6 + 0.3, ref_scale0=ru(C) * 5.7 + 0.3, weight0=torch.tensor([0.3]),
              rmin=G.f32r(1 / 1.1), rmax=G.f32r(1.1), dmax=G.f32r(0.1), decay=G.f32r(0.9), fade=G.f32r(0.9999))
    return dict(x=x, dy=rn(N, H, W, C), gamma=rn(*gs), beta=rn(*gs), alpha=ru(C) * 0.35 + 0.05, st=st)


def _bn_oracle(mode, t, eps):
    """float64 autograd of tf.nn.batch_normalization + PReLU as oracle/ref_ops.py states them (batch_norm,
    condition_batch_norm, condition_batch_renorm, prelu) -> y, and the gradients in x, gamma, beta, alpha."""
    st = t["st"]
    C = BN_SHAPE[3]
    xt, gt, bt, at = (t[k].double().requires_grad_(True) for k in ("x", "gamma", "beta", "alpha"))
    gb = gt.reshape(-1, 1, 1, C) if gt.dim() == 2 else gt
    bb = bt.reshape(-1, 1, 1, C) if bt.dim() == 2 else bt
    if mode == "infer":
        mean, var = st["mm0"].double(), st["mv0"].double()
    else:
        mean = xt.mean(dim=(0, 1, 2))
        var = ((xt - mean) ** 2).mean(dim=(0, 1, 2))
    if mode == "renorm":
        w = float(st["weight0"])
        sigma = torch.sqrt(var + eps)
        sw = w * torch.sqrt(st["ref_scale0"].double() + eps) + (1 - w) * sigma
        mw = w * st["ref_mean0"].double() + (1 - w) * mean
        r = torch.clamp(sigma / sw, st["rmin"], st["rmax"]).detach()
        d = torch.clamp((mean - mw) / sw, -st["dmax"], st["dmax"]).detach()
        gb, bb = r * gb, bb + d * gb
    inv = torch.rsqrt(var + eps) * gb
    pre = xt * inv + (bb - mean * inv)
    y = torch.relu(pre) + at * (pre - pre.abs()) * 0.5
    y.backward(t["dy"].double())
    return dict(y=y.detach(), dx=xt.grad, dgamma=gt.grad, dbeta=bt.grad, dalpha=at.grad, mean=mean.detach(),
                var=var.detach())


@pytest.mark.parametrize("mode", ["shared", "cond", "renorm", "infer"])
def test_composed_bn_act_agrees_with_the_oracle(mode):
    """BnActFn with PReLU on x[5, 3, 3, 72]: shared (tf.layers: Bessel-corrected moving variance), conditional
    ([N, C] gamma / beta), conditional renorm (fade-in weight 0.3, update = 1) and inference, forward and backward,
    against float64 autograd under the chained bounds of glue_ref.composed_bn_act; the moving and running statistics and
    the fade-in weight against the same chain.  Shared and inference are also tied to ref_ops.batch_norm + prelu."""
    from oracle import ref_ops
    hip, lib = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    eps = G.f32r(1e-5)
    t = _bn_setup(mode)
    st = t["st"]
    o = _bn_oracle(mode, t, eps)
    if mode in ("shared", "infer"):
        vs = ref_ops.VarStore()
        vs.load({"s/batch_norm/gamma": t["gamma"].double().numpy(), "s/batch_norm/beta": t["beta"].double().numpy(),
                 "s/batch_norm/moving_mean": st["mm0"].double().numpy(),
                 "s/batch_norm/moving_variance": st["mv0"].double().numpy(), "s/alpha": t["alpha"].double().numpy()})
        yo = ref_ops.prelu(vs, "s", ref_ops.batch_norm(vs, "s/batch_norm", t["x"].double(), {"bn_momentum": st["momentum"]},
                                                        mode == "shared"))
        assert float((yo.detach() - o["y"]).abs().max()) < 1e-10
    b = G.composed_bn_act(t["x"], t["dy"], t["gamma"], t["beta"], t["alpha"], eps, mode, st)
    assert b["_amb"] == 0
    for k in ("y", "dx", "dgamma", "dbeta", "dalpha"):          # the chain's values ARE the oracle's
        assert float((b[k].v.reshape(o[k].shape) - o[k]).abs().max()) <= 1e-10 * max(1.0, float(o[k].abs().max())), k
    if mode == "renorm":
        r_raw, d_raw = b["_raw"]
        assert bool((r_raw < st["rmin"]).any()) and bool((r_raw > st["rmax"]).any()) and bool((d_raw > st["dmax"]).any())
        assert bool((d_raw < -st["dmax"]).any()) and bool(((r_raw > st["rmin"]) & (r_raw < st["rmax"])).any())
    cu = lambda v, g=False: v.to(dev).clone().requires_grad_(g)                 # noqa: E731
    xc, gc, bc, ac = (cu(t[k], True) for k in ("x", "gamma", "beta", "alpha"))
    mm, mv, rm, rs = cu(st["mm0"]), cu(st["mv0"]), cu(st["ref_mean0"]), cu(st["ref_scale0"])
    wt = torch.full((), 0.3, dtype=torch.float32, device=dev)
    renorm = None
    if mode == "renorm":
        renorm = dict(ref_mean=rm, ref_scale=rs, scale_is_var=1, weight=wt, update=1, rmin=st["rmin"], rmax=st["rmax"],
                      dmax=st["dmax"], decay=st["decay"], fadein_decay=st["fade"])
    y = Fn.BnActFn.apply(xc, gc, bc, ac, mm, mv, 0.98, 1e-5, bool(st["unbiased"]), mode != "infer", None, 1, renorm)
    y.backward(t["dy"].to(dev))
    torch.cuda.synchronize()
    D = lambda v: v.to(dev)                                                     # noqa: E731
    items = [(k, got, D(o[k]), D(b[k].e)) for k, got in (("y", y.detach()), ("dx", xc.grad), ("dgamma", gc.grad),
                                                         ("dbeta", bc.grad), ("dalpha", ac.grad))]
    if mode == "infer":
        assert torch.equal(mm.cpu(), st["mm0"]) and torch.equal(mv.cpu(), st["mv0"])
    else:
        items += [("moving_mean", mm, D(b["moving_mean"].v), D(b["moving_mean"].e)),
                  ("moving_var", mv, D(b["moving_var"].v), D(b["moving_var"].e))]
        keep = st["momentum"]
        bessel = 45.0 / 44.0 if st["unbiased"] else 1.0
        assert float((b["moving_var"].v - (st["mv0"].double() * keep + o["var"] * bessel * (1 - keep))).abs().max()) < 1e-12
    if mode == "renorm":
        items += [("ref_mean", rm, D(b["ref_mean"].v), D(b["ref_mean"].e)),
                  ("ref_scale", rs, D(b["ref_scale"].v), D(b["ref_scale"].e)),
                  ("weight", wt.reshape(1), D(b["weight"].v.reshape(1)), D(b["weight"].e.reshape(1)))]
        assert float((b["ref_scale"].v - (st["ref_scale0"].double() * st["decay"] + o["var"] * (1 - st["decay"]))).abs().max()
                     ) < 1e-12
    stats, bad = R.GateStats(), []
    _gate_all(stats, bad, "BnActFn " + mode, items)
    print("\n" + stats.table())
    assert not bad, bad


def test_composed_bn_glu_agrees_with_the_oracle():
    """BnGluFn on x[5, 8, 8, 48] (320 rows: bg_bn_bwd_finalize sums N = nseg = 5 row segments, shared gamma, NULL dalpha,
    zero plane 2) forward and backward against float64 autograd of ref_ops.batch_norm followed by the GLU, under the
    chained bounds of glue_ref.composed_bn_glu."""
    from oracle import ref_ops
    hip, lib = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(61)
    N, H, W, C2 = 5, 8, 8, 48
    C = C2 // 2
    x = torch.randn(N, H, W, C2, generator=gen) * 1.5 + 0.3
    dy = torch.randn(N, H, W, C, generator=gen)
    gamma, beta = torch.randn(C2, generator=gen), torch.randn(C2, generator=gen)
    st = dict(unbiased=1, momentum=G.f32r(0.98), mm0=torch.randn(C2, generator=gen) * 0.5, mv0=torch.rand(C2, generator=gen) + 0.5)
    eps = G.f32r(1e-5)
    vs = ref_ops.VarStore()
    vs.load({"s/gamma": gamma.double().numpy(), "s/beta": beta.double().numpy(), "s/moving_mean": st["mm0"].double().numpy(),
             "s/moving_variance": st["mv0"].double().numpy()})
    x64 = x.double().requires_grad_(True)
    bn = ref_ops.batch_norm(vs, "s", x64, {"bn_momentum": st["momentum"]}, True)
    yref = bn[..., :C] * torch.sigmoid(bn[..., C:])
    yref.backward(dy.double())
    b = G.composed_bn_glu(x, dy, gamma, beta, eps, st)
    want = dict(y=yref.detach(), dx=x64.grad, dgamma=vs.vars["s/gamma"].grad, dbeta=vs.vars["s/beta"].grad,
                moving_mean=vs.state_updates["s/moving_mean"], moving_var=vs.state_updates["s/moving_variance"])
    for k, w in want.items():                                   # the chain's values ARE the oracle's
        assert float((b[k].v.reshape(w.shape) - w).abs().max()) <= 1e-9 * max(1.0, float(w.abs().max())), k
    cu = lambda v, g=False: v.to(dev).clone().requires_grad_(g)                 # noqa: E731
    xc, gc, bc, mm, mv = cu(x, True), cu(gamma, True), cu(beta, True), cu(st["mm0"]), cu(st["mv0"])
    y = Fn.BnGluFn.apply(xc, gc, bc, mm, mv, 0.98, 1e-5, True, None, 1)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    got = dict(y=y.detach(), dx=xc.grad, dgamma=gc.grad, dbeta=bc.grad, moving_mean=mm, moving_var=mv)
    stats, bad = R.GateStats(), []
    _gate_all(stats, bad, "BnGluFn", [(k, got[k], want[k].to(dev), b[k].e.to(dev)) for k in want])
    print("\n" + stats.table())
    assert not bad, bad
