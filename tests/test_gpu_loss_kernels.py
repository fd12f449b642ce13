"""The kernels that decide what the networks are trained on - DiffAugment, the hinge and general GAN losses, the class-label
sigmoid cross-entropy, the gradient penalty and its second-order (tangent) kernels, the softmax trio - against float64.

Every row of the case table of tests/loss_ref.py calls its entry point raw through ``hip.lib()`` under the rules of
tests/test_gpu_elementwise16.Runner: guarded buffers (launch_replay.Buf) for every input, output and workspace, outputs
prefilled with NaN (or their initial value where the call accumulates or works in place: the hinge sums, the in-place
softmax), two runs that must agree bit for bit, inputs left unchanged, and the per-element gate of launch_replay against
the float64 reference with the bounds of loss_ref.  One GateStats table per entry point records how much of each bound is
used.

One composed case per family runs the wrappers of functional.py (HingeDLossFn, GanLossFn, DiffAugmentFn, BnTangentFn)
against float64 autograd through oracle/ref_ops.py, under the chained stage bounds."""
import time

import pytest
import torch

from tests import launch_replay as R
from tests import loss_ref as L
from tests.test_gpu_elementwise16 import Runner, _lib

pytestmark = pytest.mark.gpu

BIG = 1 << 20


class View:
    """An output that is a slice of a buffer another entry of ``outs`` guards."""

    def __init__(self, view):
        self.view = view


class LossRunner(Runner):
    ref = L

    def key_of(self, c):
        return L.ENTRY[c["op"]]

    def wants_alt(self, c):
        return False

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
        finally:
            self.key = entry

    def scratch(self, nbytes):
        b = R.Buf(max(int(nbytes), 16), torch.uint8, self.dev)
        self.outs.append(b)
        return b

    def launcher(self, c, i):
        lib, st = self.L, self.hip.stream
        op = c["op"]
        P = lambda b: None if b is None else b.ptr()                # noqa: E731
        f32 = torch.float32
        b = {k: self.inb(v) for k, v in i.items() if torch.is_tensor(v) and k != "sums0"}
        g = b.get
        if op in ("da_fwd", "da_bwd"):
            N, S, C, pol = c["N"], c["S"], c["C"], c["policy"]
            o = self.outb((N, S, S, C), f32)
            ws = self.scratch(8 * N)
            if op == "da_fwd":
                return (lambda: lib.bg_diffaugment_fwd(P(b["x"]), P(o), P(b["u_b"]), P(b["u_s"]), P(b["u_c"]), P(b["t_x"]),
                                                       P(b["t_y"]), P(b["o_x"]), P(b["o_y"]), N, S, C, pol, P(ws),
                                                       st())), {"y": o}
            return (lambda: lib.bg_diffaugment_bwd(P(b["dy"]), P(o), P(b["u_s"]), P(b["u_c"]), P(b["t_x"]), P(b["t_y"]),
                                                   P(b["o_x"]), P(b["o_y"]), N, S, C, pol, P(ws), st())), {"dx": o}
        if op == "hinge_d_sums":
            o = self.outb((2,), f32, y0=i["sums0"])
            return (lambda: lib.bg_hinge_d_sums(P(b["real"]), P(b["fake"]), P(o), c["nf"], st())), {"sums": o}
        if op == "hinge_g_sums":
            o = self.outb((1,), f32, y0=i["sums0"])
            return (lambda: lib.bg_hinge_g_sums(P(b["fake"]), P(o), c["nf"], st())), {"sums": o}
        if op in ("hinge_d_grad", "hinge_g_grad", "gan_grad"):
            nr, nf = c["nr"], c["nf"]
            out = {}
            if nr:
                out["d_real"] = self.outb((nr,), f32)
            out["d_fake"] = self.outb((nf,), f32)
            if c["loss_out"]:
                out["loss"] = self.outb((1,), f32)
            lo = out.get("loss")
            if op == "hinge_d_grad":
                return (lambda: lib.bg_hinge_d_grad(P(b["real"]), P(b["fake"]), P(b["sums"]), i["n_global"], i["flood"],
                                                    P(out["d_real"]), P(out["d_fake"]), P(lo), nf, st())), out
            if op == "hinge_g_grad":
                return (lambda: lib.bg_hinge_g_grad(P(b["sums"]), i["n_global"], i["flood"], P(out["d_fake"]), P(lo), nf,
                                                    st())), out
            return (lambda: lib.bg_gan_loss_grad(c["kind"], c["gen"], P(g("real")), P(b["fake"]), P(b["sums"]),
                                                 P(b["tsums"]), i["nrg"], i["nfg"], i["flood"], P(out.get("d_real")),
                                                 P(out["d_fake"]), P(lo), nr, nf, st())), out
        if op == "gan_means":                # overwrites: the seeded values must not survive
            o = self.outb((2,), f32, y0=torch.tensor([7.0, -3.0], device=self.dev))
            return (lambda: lib.bg_gan_loss_means(P(g("real")), P(b["fake"]), P(o), c["nr"], c["nf"], st())), {"sums": o}
        if op == "gan_terms":
            o = self.outb((4,), f32)
            return (lambda: lib.bg_gan_loss_terms(c["kind"], c["gen"], P(g("real")), P(b["fake"]), P(b["sums"]), i["nrg"],
                                                  i["nfg"], P(o), c["nr"], c["nf"], st())), {"tsums": o}
        if op == "sigmoid_ce":
            B, n = c["B"], c["n"]
            lo, dl = self.outb((1,), f32), self.outb((B, n), f32)
            return (lambda: lib.bg_sigmoid_ce(P(b["logits"]), P(b["truth"]), P(g("weights")), i["scale"], P(lo), P(dl), B,
                                              n, st())), {"loss": lo, "dlogits": dl}
        if op == "gp_interpolate":
            N, per = c["N"], c["per"]
            o = self.outb((N, per), f32)
            return (lambda: lib.bg_gp_interpolate(P(b["real"]), P(b["other"]), P(b["alpha"]), P(g("sums")), i["count"],
                                                  P(o), N, per, st())), {"out": o}
        if op == "gp_penalty":
            N, per = c["N"], c["per"]
            ws = self.outb((2 * N,), torch.float64)
            lo, v = self.outb((1,), f32), self.outb((N, per), f32)
            return (lambda: lib.bg_gp_penalty(P(b["g"]), N, per, i["count"], c["ld"], c["lp"], P(ws), P(lo), P(v),
                                              st())), {"nsq": View(ws.view[:N]), "loss": lo, "v": v}
        if op == "chan_dots3":
            o = self.outb((3 * c["C"],), torch.float64)
            return (lambda: lib.bg_chan_dots3(P(b["p"]), P(b["q"]), P(g("r")), P(o), c["rows"], c["C"], st())), {"sums": o}
        if op == "bn_fwd_coefs":
            C = c["C"]
            cf, m12 = self.outb((3 * C,), f32), self.outb((2 * C,), f32)
            return (lambda: lib.bg_bn_tangent_fwd_coefs(P(b["sums"]), i["count"], P(b["mean"]), P(b["rstd"]), P(b["gamma"]),
                                                        P(cf), P(m12), C, st())), {"coefs": cf, "m12": m12}
        if op == "bn_bwd_coefs":
            C = c["C"]
            cd, cx, dg = self.outb((3 * C,), f32), self.outb((4 * C,), f32), self.outb((C,), f32)
            return (lambda: lib.bg_bn_tangent_bwd_coefs(P(b["sums"]), i["count"], P(b["mean"]), P(b["rstd"]), P(b["gamma"]),
                                                        P(b["m12"]), P(cd), P(cx), P(dg), C,
                                                        st())), {"coefs_dxd": cd, "coefs_dx": cx, "dgamma": dg}
        if op == "chan_lincomb3":
            o = self.outb((c["rows"], c["C"]), f32)
            return (lambda: lib.bg_chan_lincomb3(P(b["p"]), P(b["cp"]), P(b["q"]), P(b["cq"]), P(g("r")), P(g("cr")),
                                                 P(b["c0"]), P(o), c["rows"], c["C"], st())), {"out": o}
        if op == "maxpool_gather":
            N, H, W, C = c["N"], c["H"], c["W"], c["C"]
            o = self.outb((N, H // 2, W // 2, C), f32)
            return (lambda: lib.bg_maxpool2_gather(P(b["x"]), P(b["t"]), P(o), N, H, W, C, st())), {"y": o}
        if op == "prelu_dalpha":
            o = self.outb((c["C"],), f32)
            return (lambda: lib.bg_prelu_tangent_dalpha(P(b["x"]), P(b["xdot"]), P(b["dy"]), P(o), c["rows"], c["C"],
                                                        st())), {"dalpha": o}
        rows, cols = c["rows"], c["cols"]
        if op == "softmax_fwd":
            if c["inplace"]:                 # p == s: the buffer starts as the logits
                self.ins.remove(b["s"])
                o = self.outb((rows, cols), f32, y0=i["s"])
                return (lambda: lib.bg_softmax_fwd(P(o), P(o), rows, cols, st())), {"p": o}
            o = self.outb((rows, cols), f32)
            return (lambda: lib.bg_softmax_fwd(P(b["s"]), P(o), rows, cols, st())), {"p": o}
        if op == "softmax_bwd":
            o = self.outb((rows, cols), f32)
            return (lambda: lib.bg_softmax_bwd(P(b["p"]), P(b["dp"]), P(o), rows, cols, st())), {"ds": o}
        if op == "softmax_tangent_bwd":
            dp, ds = self.outb((rows, cols), f32), self.outb((rows, cols), f32)
            return (lambda: lib.bg_softmax_tangent_bwd(P(b["p"]), P(b["sdot"]), P(b["g"]), P(dp), P(ds), rows, cols,
                                                       st())), {"dp": dp, "dsdot": ds}
        raise KeyError(op)


@pytest.mark.parametrize("op", L.OPS)
def test_entry_point_matches_float64(op):
    hip, lib = _lib()
    r = LossRunner(hip, lib)
    t0 = time.time()
    todo = L.cases(op)
    namb = 0
    for k, c in enumerate(todo):
        namb += r.run(c, 3000 + k) or 0
        big = sum(bf.numel for bf in r.ins + r.outs) >= BIG
        r.ins, r.outs = [], []
        if big:
            torch.cuda.empty_cache()
    print("\n[%s] %d cases in %.1f s, %d sign-ambiguous elements" % (L.ENTRY[op], len(todo), time.time() - t0, namb))
    print(r.stats.table())
    assert not r.failures, "%d failures:\n%s" % (len(r.failures), "\n".join(r.failures[:20]))
    assert namb == 0
    assert all(row[1] <= 1.0 for row in r.stats.rows.values())


def test_softmax_refuses_more_than_1024_columns_and_launches_nothing():
    """cols = 1025: an error code from all three entry points, and no byte of any buffer involved changes."""
    hip, lib = _lib()
    r = LossRunner(hip, lib)
    r.ins, r.outs = [], []
    rows, cols = 3, 1025
    bufs = [r.outb((rows, cols), torch.float32, y0=torch.ones(rows, cols, device=r.dev)) for _ in range(5)]
    for o in bufs:
        o.prefill()
    torch.cuda.synchronize()
    before = [o.raw.clone() for o in bufs]
    s, p, a, d1, d2 = (o.ptr() for o in bufs)
    st = hip.stream
    assert lib.bg_softmax_fwd(s, p, rows, cols, st()) == L.ERR_UNSUPPORTED
    assert b"1025" in lib.bg_last_error()
    assert lib.bg_softmax_bwd(s, p, d1, rows, cols, st()) == L.ERR_UNSUPPORTED
    assert lib.bg_softmax_tangent_bwd(s, p, a, d1, d2, rows, cols, st()) == L.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for o, bb in zip(bufs, before):
        assert torch.equal(o.raw, bb)
    assert lib.bg_softmax_fwd(s, p, rows, 1024, st()) == 0
    torch.cuda.synchronize()


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


def _logits(seed, dev, shift):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(L.COMPOSED_B, 1, generator=gen, device=dev) * 1.5 + shift


def test_composed_losses_agree_with_the_oracle():
    """HingeDLossFn and GanLossFn ('ra-gan', discriminator) at B = 300 with flood below the loss: loss and both logit
    gradients against ref_ops.discriminator_loss and its float64 autograd gradient, under the chained bounds of the two /
    three kernels of each (loss_ref.composed_*); the backward's scaling by g = 1 is exact.  The chained bound is the worst
    case over two or three 300-term sums, so a correct chain uses 0.03 - 10 % of it: the stage gates above are the sharp
    ones, this test holds the glue between them (argument order, world size, what is zeroed before which call)."""
    from oracle import ref_ops
    hip, lib = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    real, fake = _logits(11, dev, 0.4), _logits(12, dev, -0.3)
    stats, bad = R.GateStats(), []
    for name, kind in (("hinge", 0), ("ra-gan", 4)):
        r64, f64 = real.double().requires_grad_(True), fake.double().requires_grad_(True)
        flood = L.f32r(0.5 * float(ref_ops.discriminator_loss(name, r64, f64, 0).detach()))
        lref = ref_ops.discriminator_loss(name, r64, f64, flood)
        lref.backward()
        b = (L.composed_hinge_d(real.reshape(-1), fake.reshape(-1), flood) if kind == 0
             else L.composed_gan(kind, 0, real.reshape(-1), fake.reshape(-1), flood))
        assert b["_amb"] == 0
        lval = float(lref.detach())
        assert abs(float(b["loss"].v) - lval) <= 1e-12 * abs(lval)                       # the reference IS the oracle
        rl, fl = real.clone().requires_grad_(True), fake.clone().requires_grad_(True)
        loss = (Fn.HingeDLossFn.apply(rl, fl, flood, None, 1) if kind == 0
                else Fn.GanLossFn.apply(rl, fl, kind, 0, flood, None, 1))
        loss.backward()
        torch.cuda.synchronize()
        _gate_all(stats, bad, name, (("loss", loss.detach().reshape(1), lref.detach().reshape(1), b["loss"].e),
                                     ("d_real", rl.grad, r64.grad, b["d_real"].e),
                                     ("d_fake", fl.grad, f64.grad, b["d_fake"].e)))
    print("\n" + stats.table())
    assert not bad, bad


def test_composed_diffaugment_agrees_with_the_oracle():
    """DiffAugmentFn forward and backward at B = 300, S = 16, C = 3, all three policies, against ref_ops.diffaugment and
    its float64 autograd gradient."""
    import numpy as np
    from oracle import ref_ops
    hip, lib = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    c = dict(op="da_fwd", N=L.COMPOSED_B, S=16, C=3, policy=7, edge=0)
    gen = torch.Generator(device=dev).manual_seed(21)
    i = L.make_inputs(c, dev, gen)
    dy = torch.randn(i["x"].shape, generator=gen, device=dev)
    draws = {k: np.asarray(v.cpu()) for k, v in i.items() if k != "x"}
    x64 = i["x"].double().cpu().requires_grad_(True)
    yref = ref_ops.diffaugment(x64, draws)
    yref.backward(dy.double().cpu())
    xl = i["x"].clone().requires_grad_(True)
    y = Fn.DiffAugmentFn.apply(xl, i["u_b"], i["u_s"], i["u_c"], i["t_x"], i["t_y"], i["o_x"], i["o_y"], 7)
    y.backward(dy)
    torch.cuda.synchronize()
    bf = L.diffaugment_fwd(L.Ref, i, 16, 3, 7)["y"]
    bb = L.diffaugment_bwd(L.Ref, dict(i, dy=dy), 16, 3, 7)["dx"]
    stats, bad = R.GateStats(), []
    _gate_all(stats, bad, "DiffAugmentFn", (("y", y.detach(), yref.detach().to(dev), bf.e),
                                            ("dx", xl.grad, x64.grad.to(dev), bb.e)))
    print("\n" + stats.table())
    assert not bad, bad
    assert bool(((y.detach() == 0) == (yref.detach().to(dev) == 0)).all())             # the zero pattern


@pytest.mark.parametrize("data", ["randn", "mean8"])
def test_composed_bn_tangent_chain_agrees_with_autograd(data):
    """functional.BnTangentFn forward and backward at (37, 776), x ~ N(0, 1) and x ~ 8 +- 0.5 - where
    m2 = r (sum xd x - mu sum xd) / n cancels - against the float64 autograd JVP of training-mode batch norm and its
    gradients.  The bound chains the stage bounds (column sums, coefficients, linear combination), so the cancellation is
    paid for by the absolute-value expression of m2 and not by a tolerance: at mean 8 that worst case over three stages is
    (8 / 0.5)^2 times wider and a correct chain uses under 1 % of it; the stage gates above are the sharp ones."""
    hip, lib = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    rows, C = L.COMPOSED_BN
    gen = torch.Generator(device=dev).manual_seed(31)
    x = torch.randn(rows, C, generator=gen, device=dev)
    if data == "mean8":
        x = x * 0.5 + 8.0
    xd, s = torch.randn(rows, C, generator=gen, device=dev), torch.randn(rows, C, generator=gen, device=dev)
    gamma = torch.randn(C, generator=gen, device=dev)
    gamma[0] = 0.0
    b = L.composed_bn_tangent(x, xd, s, gamma, float(rows))
    yd, dxd, dx, dg = (t.to(dev) for t in L.bn_tangent_autograd(x.double().cpu(), xd.double().cpu(), s.double().cpu(),
                                                                 gamma.double().cpu()))
    xl, xdl, gl = (t.clone().requires_grad_(True) for t in (x, xd, gamma))
    y = Fn.BnTangentFn.apply(xdl, xl, gl, b["mean"], b["rstd"], float(rows), None)
    y.backward(s)
    torch.cuda.synchronize()
    stats, bad = R.GateStats(), []
    _gate_all(stats, bad, "BnTangentFn " + data, (("yd", y.detach(), yd, b["y"].e), ("d_xd", xdl.grad, dxd, b["dxd"].e),
                                          ("d_x", xl.grad, dx, b["dx"].e), ("dgamma", gl.grad, dg, b["dgamma"].e)))
    print("\n" + stats.table())
    assert not bad, bad
