"""CPU checks of tests/loss_ref.py: its float64 references against float64 autograd through oracle/ref_ops.py
(discriminator_loss, generator_loss, diffaugment, cls_loss_logistic), a written-out gradient penalty, a training-mode
batch-norm JVP differentiated once more, torch.softmax and its JVP, and literal Python loops for the routing; and a mutation
self-test of its case table in the pattern of tests/test_weight_gate.py - the simulated correct kernel (the same formulas
evaluated in fp32) passes the gate on every case, on the reference alone no case has a sign-ambiguous element, and each
simulated kernel bug is rejected on at least one case."""
import numpy as np
import pytest
import torch

from oracle import ref_ops
from tests import elementwise_ref as EW
from tests import launch_replay as R
from tests import loss_ref as L

D64 = torch.float64
F32 = torch.float32


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_g(seed), dtype=D64) * scale


def _close(a, b, tol=1e-12):
    return bool(((a - b).abs() <= tol * (1.0 + b.abs())).all())


# ------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [0, 1])
@pytest.mark.parametrize("kind", range(7))
def test_loss_references_match_the_oracle(kind, gen):
    """means -> terms -> grad, chained, against ref_ops.discriminator_loss / generator_loss and their autograd gradients:
    nr != nf, flood off / below / above the loss, logits to +-30; the dedicated hinge pair as well."""
    name = L.KINDS[kind]
    tol = 5e-9 if kind in (2, 4) else 1e-12         # (F.softplus is linear above 20: the oracle itself is off by e^-20)
    for nr, nf, flood_mode in ((5, 7, "none"), (300, 257, "below"), (1, 256, "above")):
        real, fake = (_rand((nr,), 10 * kind + gen) * 3 + 0.3).float(), (_rand((nf,), 50 + kind) * 3 - 0.2).float()
        real[0], fake[0] = 30.0, -30.0
        r64, f64 = real.double().requires_grad_(True), fake.double().requires_grad_(True)
        fn = (lambda fl: ref_ops.generator_loss(name, f64, r64, fl)) if gen else \
            (lambda fl: ref_ops.discriminator_loss(name, r64, f64, fl))
        flood = L._flood_value(fn(0).detach(), flood_mode)
        loss = fn(flood)
        gr, gf = torch.autograd.grad(loss, (r64, f64), allow_unused=True)
        b = L.composed_gan(kind, gen, real, fake, flood)
        assert b["_amb"] == 0
        assert _close(b["loss"].v, loss.detach(), tol)
        assert _close(b["d_fake"].v, gf, tol)
        assert _close(b["d_real"].v, torch.zeros_like(r64) if gr is None else gr, tol)
        assert float(b["loss"].e) > 0 and bool((b["d_fake"].e >= 0).all())
        if kind == 0 and gen == 0 and nr == nf:
            h = L.composed_hinge_d(real, fake, flood)
            assert _close(h["loss"].v, loss.detach(), tol) and _close(h["d_real"].v, gr) and _close(h["d_fake"].v, gf)
        if kind == 0 and gen == 1:
            s = L.hinge_g_sums(L.Ref, dict(fake=fake, sums0=torch.zeros(1)))["sums"]
            h = L.hinge_g_grad(L.Ref, dict(sums=s), nf, float(nf), flood, False, True)
            assert _close(h["loss"].v, loss.detach(), tol) and _close(h["d_fake"].v, gf)
    # real == NULL with nr = 0 is the non-relativistic generator loss
    if gen and kind not in L.RA:
        i = dict(fake=fake)
        i["sums"] = L.gan_means(L.Ref, i)["sums"]
        i["tsums"] = L.gan_terms(L.Ref, kind, 1, i, 0.0, float(nf))["tsums"]
        r = L.gan_grad(L.Ref, kind, 1, i, 0.0, float(nf), flood, False, True)
        assert _close(r["loss"].v, loss.detach(), tol) and _close(r["d_fake"].v, gf, tol) and "d_real" not in r


def test_n_global_scales_the_share_of_this_rank():
    """With n_global = 4 n and the other ranks' sums added in, the loss is the global mean and the gradients are this
    rank's rows of the global gradient."""
    real, fake = _rand((12,), 1).float(), _rand((12,), 2).float()
    r64, f64 = real.double().requires_grad_(True), fake.double().requires_grad_(True)
    loss = ref_ops.discriminator_loss("hinge", r64, f64, 0)
    loss.backward()
    own = slice(3, 6)
    i = dict(real=real[own], fake=fake[own])
    s = torch.stack([(1 - real.double()).clamp_min(0).sum(), (1 + fake.double()).clamp_min(0).sum()])
    r = L.hinge_d_grad(L.Ref, dict(i, sums=s), 12.0, 0.0, False, True)
    assert _close(r["loss"].v, loss.detach())
    assert _close(r["d_real"].v, r64.grad[own]) and _close(r["d_fake"].v, f64.grad[own])


def test_sigmoid_ce_reference_matches_the_oracle():
    B, n = 5, 9
    x, t, w = _rand((B, n), 3, 4.0).float(), torch.rand((B, n), generator=_g(4)), torch.rand((n,), generator=_g(5)) + 0.1
    x[0, 0], x[1, 1] = 100.0, -100.0
    x64 = x.double().requires_grad_(True)
    loss = ref_ops.cls_loss_logistic(t.double(), x64, w.double())
    loss.backward()
    scale = L.f32r(1.0 / (B * n))
    r = L.sigmoid_ce(L.Ref, dict(logits=x, truth=t, weights=w), scale)
    k = scale * B * n
    assert _close(r["loss"].v, loss.detach() * k) and _close(r["dlogits"].v, x64.grad * k)
    r1 = L.sigmoid_ce(L.Ref, dict(logits=x, truth=t), scale)
    l1 = ref_ops.cls_loss_logistic(t.double(), x.double(), torch.ones(n, dtype=D64))
    assert _close(r1["loss"].v, l1 * k)


@pytest.mark.parametrize("S,C", [(8, 1), (9, 3), (16, 4)])
def test_diffaugment_references_match_the_oracle_and_literal_loops(S, C):
    names = {1: "color", 2: "translation", 4: "cutout"}
    N = 4
    for pol in range(1, 8):
        c = dict(N=N, S=S, C=C, policy=pol, edge=pol % 4)
        d = L.da_draws(c, _g(100 + pol), "cpu")
        x = _rand((N, S, S, C), pol).float()
        dy = _rand((N, S, S, C), 20 + pol).float()
        x64 = x.double().requires_grad_(True)
        draws = {k: np.asarray(v) for k, v in d.items()}
        y = ref_ops.diffaugment(x64, draws, ",".join(names[b] for b in (1, 2, 4) if pol & b))
        y.backward(dy.double())
        f = L.diffaugment_fwd(L.Ref, dict(d, x=x), S, C, pol)["y"]
        bw = L.diffaugment_bwd(L.Ref, dict(d, dy=dy), S, C, pol)["dx"]
        fv, bv = (f.v if isinstance(f, L.Ref) else f.double()), (bw.v if isinstance(bw, L.Ref) else bw.double())
        assert _close(fv, y.detach()) and _close(bv, x64.grad)
        assert isinstance(f, L.Ref) == bool(pol & 1)                                     # no colour: exact routing
        assert bool(((fv == 0) == (y.detach() == 0)).all())
    # the routing against the literal emulations of the TF graph and a Python loop for the transpose
    xs = x.numpy()
    t_x, t_y, o_x, o_y = (draws[k] for k in ("t_x", "t_y", "o_x", "o_y"))
    lit = ref_ops.cutout_literal(ref_ops.translation_literal(xs, t_x, t_y), o_x, o_y)
    got, _ = L.da_route(x, S, 6, d["t_x"], d["t_y"], d["o_x"], d["o_y"])
    assert np.array_equal(got.numpy(), lit)
    back, _ = L.da_route(dy, S, 6, d["t_x"], d["t_y"], d["o_x"], d["o_y"], backward=True)
    cs = L.da_params(S)[1]
    want = np.zeros_like(xs)
    for n in range(N):
        for i in range(S):
            for j in range(S):                                   # out[i, j] reads x[i + t_x, j + t_y] unless cut or outside
                si, sj = i + int(t_x[n]), j + int(t_y[n])
                r0, r1 = max(0, int(o_x[n]) - cs // 2), min(S - 1, int(o_x[n]) - cs // 2 + cs - 1)
                c0, c1 = max(0, int(o_y[n]) - cs // 2), min(S - 1, int(o_y[n]) - cs // 2 + cs - 1)
                if 0 <= si < S and 0 <= sj < S and not (r0 <= i <= r1 and c0 <= j <= c1):
                    want[n, si, sj] += dy.numpy()[n, i, j]
    assert np.array_equal(back.numpy(), want)
    if S == 9:
        assert L.da_params(9) == (1, 5, 9) and int(L.da_cut_mask(9, torch.tensor([4]), torch.tensor([4])).sum()) == 25


def test_gradient_penalty_references_match_a_written_out_penalty():
    N, per, ld = 6, 11, 10.0
    g = _rand((N, per), 7).float()
    g[1] = 0.0
    g[2] = 0.0
    g[2, 3] = 1.0
    g[3] *= 0.1
    for lp in (0, 1):
        for count in (float(N), 4.0 * N):
            g64 = g.double().requires_grad_(True)
            nrm = (g64 * g64).sum(1).clamp_min(1e-300).sqrt() * (g64.abs().sum(1) > 0)
            e = nrm - 1.0
            pen = ld * ((e.clamp_min(0) if lp else e) ** 2).sum() / count
            pen.backward()
            r = L.gp_penalty(L.Ref, dict(g=g), count, ld, lp)
            assert _close(r["loss"].v, pen.detach()) and _close(r["nsq"].v, (g.double() ** 2).sum(1))
            want = g64.grad.clone()
            want[1] = 0.0                                        # the zero row: coefficient 0, by definition
            assert _close(r["v"].v, want)
            assert bool(torch.isfinite(r["v"].e).all()) and float(r["v"].v[2].abs().max()) == 0.0
    real, other, a = _rand((3, 5), 8).float(), _rand((3, 5), 9).float(), torch.tensor([0.0, 1.0, 0.3])
    r = L.gp_interpolate(L.Ref, dict(real=real, other=other, alpha=a), 0.0)["out"]
    assert _close(r.v, real.double() + a.double()[:, None] * (other.double() - real.double()))
    sums = torch.stack([real.double().sum(), (real.double() ** 2).sum()])
    r = L.gp_interpolate(L.Ref, dict(real=real, other=other, alpha=a, sums=sums), 15.0)["out"]
    std = real.double().std(unbiased=False)
    assert _close(r.v, real.double() + a.double()[:, None] * 0.5 * std * other.double())
    const = torch.full((3, 5), 1.7)
    sums = torch.stack([const.double().sum(), (const.double() ** 2).sum()])
    r = L.gp_interpolate(L.Ref, dict(real=const, other=other, alpha=a, sums=sums), 15.0)["out"]
    assert bool(torch.isfinite(r.v).all()) and bool((r.v - 1.7).abs().max() < 1e-6) and bool((r.e < 1e-5).all())


@pytest.mark.parametrize("data", ["randn", "mean8"])
def test_bn_tangent_references_match_a_jvp_differentiated_once_more(data):
    rows, C = 10, 3
    x = _rand((rows, C), 11).float() * (0.5 if data == "mean8" else 1.0) + (8.0 if data == "mean8" else 0.0)
    xd, s, gamma = _rand((rows, C), 12).float(), _rand((rows, C), 13).float(), torch.tensor([0.0, -1.3, 0.7])
    yd, dxd, dx, dg = L.bn_tangent_autograd(x.double(), xd.double(), s.double(), gamma.double())
    b = L.composed_bn_tangent(x, xd, s, gamma, float(rows))
    tol = 1e-9
    assert _close(b["y"].v, yd, tol) and _close(b["dxd"].v, dxd, tol) and _close(b["dx"].v, dx, tol)
    assert _close(b["dgamma"].v, dg, tol)
    # count = 4 rows with four equal shares is the same batch four times over: the same coefficients
    x64 = x.double()
    i = dict(mean=b["mean"], rstd=b["rstd"], gamma=gamma, sums=torch.cat([xd.double().sum(0), (xd.double() * x64).sum(0)]))
    one = L.bn_tangent_fwd_coefs(L.Ref, i, float(rows), rows)
    four = L.bn_tangent_fwd_coefs(L.Ref, dict(i, sums=i["sums"] * 4), 4.0 * rows, rows)
    assert _close(one["coefs"].v, four["coefs"].v) and _close(one["m12"].v, four["m12"].v)
    # chan_dots3 with r == NULL leaves the third block zero
    d = L.chan_dots3(L.Ref, dict(p=xd, q=x))["sums"]
    assert float(d.v[2 * C:].abs().max()) == 0.0 and _close(d.v[C:2 * C], (xd.double() * x64).sum(0))


def test_softmax_references_match_torch_softmax_and_its_jvp():
    rows, cols = 4, 9
    s = _rand((rows, cols), 14, 3.0).float()
    s[1] = s[1, 0]
    s[2, 4] += 90.0
    p = L.softmax_fwd(L.Ref, dict(s=s))["p"]
    assert _close(p.v, torch.softmax(s.double(), 1)) and bool((p.e > 0).all())
    pf = torch.softmax(s.double(), 1).float()
    sdot, g = _rand((rows, cols), 15).float(), _rand((rows, cols), 16).float()
    _, jvp = torch.autograd.functional.jvp(lambda t: torch.softmax(t, 1), s.double(), sdot.double())
    # (as a function of the stored p: pdot = p (sdot - sum p sdot))
    ds = L.softmax_bwd(L.Ref, dict(p=pf, dp=sdot))["ds"]
    p64 = pf.double()
    assert _close(ds.v, p64 * (sdot.double() - (p64 * sdot.double()).sum(1, keepdim=True)))
    assert bool((ds.v - jvp).abs().max() < 1e-6)
    pl, sl = p64.clone().requires_grad_(True), sdot.double().requires_grad_(True)
    pdot = pl * (sl - (pl * sl).sum(1, keepdim=True))
    (pdot * g.double()).sum().backward()
    r = L.softmax_tangent_bwd(L.Ref, dict(p=pf, sdot=sdot, g=g))
    assert _close(r["dp"].v, pl.grad) and _close(r["dsdot"].v, sl.grad)


def test_gather_and_slope_gradient_match_literal_loops():
    x = torch.tensor([[0.0, -0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 2.0], [3.0, 3.0, -1.0, -1.0], [3.0, 3.0, -1.0, -1.0]])
    x = x.reshape(1, 4, 4, 1)
    t = torch.arange(16.0).reshape(1, 4, 4, 1)
    for last in (False, True):
        y = L.maxpool2_gather(x, t, last)
        for ho in range(2):
            for wo in range(2):
                win = [(2 * ho + a, 2 * wo + b) for a in (0, 1) for b in (0, 1)]
                m = max(float(x[0, i, j, 0]) for i, j in win)
                hits = [(i, j) for i, j in win if float(x[0, i, j, 0]) == m]
                i, j = hits[-1] if last else hits[0]
                assert float(y[0, ho, wo, 0]) == float(t[0, i, j, 0])
    xs = _rand((7, 3), 17).float()
    xs[0, 0], xs[1, 1] = 0.0, -0.0
    xdot, dy = _rand((7, 3), 18).float(), _rand((7, 3), 19).float()
    a = torch.tensor([0.2, -0.5, 1.5], dtype=D64, requires_grad=True)
    (dy.double() * xdot.double() * EW.slope(xs.double(), a)).sum().backward()
    r = L.prelu_tangent_dalpha(L.Ref, dict(x=xs, xdot=xdot, dy=dy))["dalpha"]
    assert _close(r.v, a.grad)


# ------------------------------------------------------------------------------------------
# the simulated kernels and their mutations
# ------------------------------------------------------------------------------------------
LOSS_OPS = ("hinge_d_grad", "hinge_g_grad", "gan_terms", "gan_grad")
DA = ("da_fwd", "da_bwd")
MUTATIONS = {
    # name: (ops it applies to, the cases among them on which it shows)
    "hinge derivative with >= in place of >": (("hinge_d_grad", "gan_terms", "gan_grad"), lambda c: c["plant"] is True),
    "flood sign that is never 0": (("hinge_d_grad", "hinge_g_grad", "gan_grad"), lambda c: c["flood"] == "exact"),
    "local n in place of n_global": (LOSS_OPS, lambda c: c["mult"] == 4),
    "the relativistic cross term dropped": (("gan_grad",), lambda c: c["kind"] in L.RA),
    "softplus without the max shift": (("gan_terms",), lambda c: c["plant"] == "tails"),
    "weights[i / n] in place of weights[i % n]": (("sigmoid_ce",), lambda c: c["weights"] and c["B"] > 1),
    L.STRIDE_MUT: (("hinge_d_sums", "hinge_g_sums", "gan_means", "gan_terms", "gan_grad", "sigmoid_ce"),
                   lambda c: c.get("nf", 0) > 256 or c.get("B", 0) * c.get("n", 0) > 256),
    "cutout upper bound off by one": (DA, lambda c: c["policy"] & 4 and c["S"] <= 64),
    "translation sign not flipped in the backward": (("da_bwd",), lambda c: c["policy"] & 2 and c["S"] <= 64),
    "contrast mean over px in place of px C": (DA, lambda c: c["policy"] & 1 and c["C"] > 1 and c["S"] <= 64),
    "saturation mean with C fixed at 3": (DA, lambda c: c["policy"] & 1 and c["C"] != 3),
    "per-image partial sums added into the wrong image": (DA, lambda c: (c["policy"] & 1 and c["S"] in (48, 64)
                                                                          and c["N"] == 4)),
    "penalty coefficient without 1/||g||": (("gp_penalty",), lambda c: c["per"] < 4096),
    "lp clamp missing": (("gp_penalty",), lambda c: c["lp"] == 1 and c["per"] < 4096),
    "zero-norm row giving NaN": (("gp_penalty",), lambda c: c["N"] >= 5 and c["per"] < 4096),
    "m2 without the mu sum xd term": (("bn_fwd_coefs", "bn_bwd_coefs"), lambda c: True),
    "count = local rows": (("bn_fwd_coefs", "bn_bwd_coefs"), lambda c: c["mult"] == 4),
    "gather taking the last maximum": (("maxpool_gather",), lambda c: True),
    "dalpha without the 1/2 at zero": (("prelu_dalpha",), lambda c: True),
    "softmax including the columns >= cols": (("softmax_fwd",), lambda c: c["cols"] % 64 != 0 and 1 < c["rows"] < 100),
    "softmax without the max subtraction": (("softmax_fwd",), lambda c: c["rows"] < 100),
}
M = list(MUTATIONS)


def applies(mut, c):
    ops, where = MUTATIONS[mut]
    return c["op"] in ops and bool(where(c))


def sim(c, i, mut=None):
    """The outputs of 'kernels' that evaluate the documented formulas in fp32; ``mut`` names the bug they have."""
    out = L.formula(c, i, L.Sim, mut)
    out.pop("_amb", None)
    return {k: (v.v if isinstance(v, L.Sim) else v) for k, v in out.items()}


class Rec:
    def __init__(self):
        self.ok, self.worst, self.nbad = True, 0.0, 0

    def gate(self, label, got, ref, Eb):
        ok, ratio, _, _, nbad = R.gate(got, ref, Eb)
        self.ok, self.worst, self.nbad = self.ok and ok, max(self.worst, ratio), self.nbad + nbad
        if ok:
            assert ratio <= 1.0, (label, ratio)

    def exact(self, label, got, want):
        same = torch.equal(got.contiguous().view(torch.uint8), want.to(got.dtype).contiguous().view(torch.uint8))
        self.ok = self.ok and same
        self.nbad += 0 if same else 1

    def fail(self, msg):
        self.ok = False
        self.nbad += 1


def _run(c, mut=None):
    i = L.make_inputs(c, "cpu", _g(1234))
    rec = Rec()
    namb, nout = L.check(c, i, sim(c, i, mut), rec)
    return rec, namb, nout


@pytest.mark.parametrize("op", L.OPS)
def test_gate_accepts_a_correct_kernel_and_no_element_is_ambiguous(op):
    """Every case of the table: the simulated correct kernel passes, and on the reference alone no element lies within
    its own bound of a kink (every case with a sign-dependent output has fewer than 10^4 elements: none is allowed)."""
    worst, n = 0.0, 0
    for c in L.cases(op):
        rec, namb, nout = _run(c)
        assert rec.ok, (L.describe(c), rec.worst, rec.nbad)
        assert namb == 0 and nout > 0, (L.describe(c), namb, nout)
        worst, n = max(worst, rec.worst), n + 1
    assert n > 0
    print("%-22s %3d cases accepted (worst err/bound %.3f), 0 elements outside the gate, 0 ambiguous" % (op, n, worst))


@pytest.mark.parametrize("mut", M)
def test_gate_rejects(mut):
    """Each simulated bug is rejected on at least one case of the table."""
    tried = 0
    for c in (c for c in L.CASES if applies(mut, c)):
        tried += 1
        rec, _, _ = _run(c, mut)
        if not rec.ok:
            print("mutation %-52s rejected on %s: %d outputs outside the bound (case %d it applies to)"
                  % (mut, L.describe(c), rec.nbad, tried))
            return
    raise AssertionError("no case of the table rejects: %s (%d cases tried)" % (mut, tried))


def test_every_mutation_is_rejected_where_it_matters_most():
    """The cases built for a bug reject it."""
    by_name = {L.describe(c): c for c in L.CASES}
    for mut, name in (("flood sign that is never 0", "hinge_d_grad[n256 exact flood]"),
                      ("flood sign that is never 0", "gan_grad[wgan-gp D exact flood]"),
                      ("hinge derivative with >= in place of >", "hinge_d_grad[n1000 x1 none s0.02]"),
                      (L.STRIDE_MUT, "sigmoid_ce[B16 n1000 w soft]"), (L.STRIDE_MUT, "gan_means[nr257 nf256 x1]"),
                      ("softplus without the max shift", "gan_terms[ra-gan G planted +-100]"),
                      ("per-image partial sums added into the wrong image", "da_fwd[p7 C3 S48 N257]"),
                      ("per-image partial sums added into the wrong image", "da_bwd[p7 C3 S48 N257]"),
                      ("cutout upper bound off by one", "da_fwd[p4 C1 S9 N4]"),
                      ("zero-norm row giving NaN", "gp_penalty[N257 per1 lp0 x1]"),
                      ("m2 without the mu sum xd term", "bn_fwd_coefs[37x776 mean8 x1]"),
                      ("gather taking the last maximum", "maxpool_gather[2x2x6x3 ties]"),
                      ("softmax without the max subtraction", "softmax_fwd[1x48 d2]"),
                      ("softmax including the columns >= cols", "softmax_fwd[7x65 d0]")):
        c = by_name[name]
        rec, _, _ = _run(c, mut)
        assert not rec.ok, (mut, name)


def test_table_covers_what_the_issue_lists():
    cs = L.CASES
    assert len({L.describe(c) for c in cs}) == len(cs)
    assert set(L.ENTRY) == set(L.OPS) and all(L.cases(op) for op in L.OPS)
    da = [c for c in cs if c["op"] == "da_fwd"]
    assert {(c["policy"], c["C"], c["S"]) for c in da} >= {(p, C, S) for p in range(1, 8) for C in (1, 3, 4)
                                                           for S in (8, 9, 16, 48, 64)}
    assert {1, 4, 257, 17} <= {c["N"] for c in da} and any(c["N"] * c["S"] ** 2 > 4096 * 256 for c in da)
    assert L.da_params(9)[1] == 5 and 48 * 48 > 2048 >= 32 * 32
    assert {(c["policy"], c["C"], c["S"], c["N"]) for c in da} == {(c["policy"], c["C"], c["S"], c["N"])
                                                                   for c in cs if c["op"] == "da_bwd"}
    for op in ("hinge_d_sums", "hinge_d_grad", "hinge_g_sums", "hinge_g_grad"):
        h = [c for c in cs if c["op"] == op]
        assert set(L.LOGIT_N) <= {c["nf"] for c in h} and {1, 4} == {c["mult"] for c in h}
        assert set(L.SCALES) <= {c["scale"] for c in h}
    for op in ("hinge_d_grad", "hinge_g_grad", "gan_grad"):
        h = [c for c in cs if c["op"] == op]
        assert {"none", "below", "above", "exact"} == {c["flood"] for c in h} and {True, False} == {c["loss_out"] for c in h}
    gt = [c for c in cs if c["op"] == "gan_terms"]
    assert {(c["kind"], c["gen"]) for c in gt} == {(k, g) for k in range(7) for g in (0, 1)}
    assert any(c["nr"] == 0 for c in gt) and any(c["nr"] not in (0, c["nf"]) for c in gt)
    assert set(L.LOGIT_N) <= {c["nr"] for c in gt} | {c["nf"] for c in gt}
    assert {2, 4} == {c["kind"] for c in gt if c["plant"] == "tails"}
    ce = [c for c in cs if c["op"] == "sigmoid_ce"]
    assert {(c["B"], c["n"]) for c in ce} == set(L.CE_SHAPES) and {True, False} == {c["neg"] for c in ce}
    gi = [c for c in cs if c["op"] == "gp_interpolate"]
    assert any(c["N"] * c["per"] > 1048576 for c in gi) and any(c["data"] == "constant" for c in gi)
    gp = [c for c in cs if c["op"] == "gp_penalty"]
    assert set(L.GP_PER) == {c["per"] for c in gp} and set(L.GP_N) == {c["N"] for c in gp}
    assert {0, 1} == {c["lp"] for c in gp} and {1, 4} == {c["mult"] for c in gp}
    for op in ("chan_dots3", "bn_fwd_coefs", "bn_bwd_coefs", "chan_lincomb3"):
        assert set(L.BN_SHAPES) <= {(c["rows"], c["C"]) for c in cs if c["op"] == op}
        assert {"randn", "mean8"} == {c["data"] for c in cs if c["op"] == op}
    assert any(c["rows"] * c["C"] > 2048 * 256 for c in cs if c["op"] == "chan_lincomb3")
    assert {(c["N"], c["H"], c["W"], c["C"]) for c in cs if c["op"] == "maxpool_gather"} == set(EW.EDGE_MAXPOOL)
    assert {(n * hw, C) for n, hw, C, _ in EW.EDGE} <= {(c["rows"], c["C"]) for c in cs if c["op"] == "prelu_dalpha"}
    for op in ("softmax_fwd", "softmax_bwd", "softmax_tangent_bwd"):
        sm = [c for c in cs if c["op"] == op]
        assert set(L.SM_COLS) == {c["cols"] for c in sm} and set(L.SM_ROWS) <= {c["rows"] for c in sm}
    assert any(c["inplace"] for c in cs if c["op"] == "softmax_fwd")
    # inputs carry what the table promises
    i = L.make_inputs(next(c for c in gp if c["N"] == 5 and c["per"] == 2049), "cpu", _g(1))
    nrm = i["g"].double().norm(dim=1)
    assert float(nrm[1]) == 0.0 and float(nrm[2]) == 1.0 and bool((nrm > 1).any()) and bool(((nrm < 1) & (nrm > 0)).any())
    i = L.make_inputs(next(c for c in cs if c["op"] == "prelu_dalpha" and c["rows"] == 4096), "cpu", _g(1))
    share = float((i["x"] == 0).float().mean())
    assert 0.005 < share < 0.02 and bool(torch.signbit(i["x"][i["x"] == 0]).any())
    i = L.make_inputs(next(c for c in cs if c["op"] == "maxpool_gather" and c["data"] == "ties"), "cpu", _g(1))
    z = i["x"][i["x"] == 0]
    assert bool(torch.signbit(z).any()) and bool((~torch.signbit(z)).any())
    i = L.make_inputs(next(c for c in cs if c["op"] == "hinge_d_grad" and c["nf"] == 1000), "cpu", _g(1))
    assert bool((i["real"] == 1.0).any()) and bool((i["fake"] == -1.0).any())
