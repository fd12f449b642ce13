"""CPU checks of tests/elementwise_ref.py: its float64 references against float64 autograd and direct Python loops at small
shapes, and a mutation self-test of its case table in the pattern of tests/test_launch_gate.py - a simulated correct
kernel (the reference evaluated in fp32 and rounded once to the output type) passes the gate on every small case, each
simulated kernel bug is rejected on at least one of them, and no small case has more sign-ambiguous elements than the
cap on the reference alone."""
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_ref as E
from tests import launch_replay as R

D64 = torch.float64
F32 = torch.float32


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=D64) * scale


# ------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------
def _finalize_loop(part, gamma, per_sample, count):
    """bg_bn_bwd_finalize as a direct loop: dgamma / dbeta (per sample: copies; per channel: sums over N), dalpha, cm."""
    _, N, C = part.shape
    dbeta = torch.zeros((N, C) if per_sample else (C,), dtype=D64)
    dgamma = torch.zeros_like(dbeta)
    dalpha = torch.zeros(C, dtype=D64)
    cm = torch.zeros(2 * C, dtype=D64)
    for c in range(C):
        for n in range(N):
            ga = gamma[n, c] if per_sample else gamma[c]
            if per_sample:
                dbeta[n, c] = part[0, n, c]
                dgamma[n, c] = part[1, n, c]
            else:
                dbeta[c] += part[0, n, c]
                dgamma[c] += part[1, n, c]
            dalpha[c] += part[2, n, c]
            cm[c] += ga * part[0, n, c] / count
            cm[C + c] += ga * part[1, n, c] / count
    return dgamma, dbeta, dalpha, cm


@pytest.mark.parametrize("per_sample", [0, 1])
@pytest.mark.parametrize("with_alpha", [False, True])
def test_bn_prelu_references_match_autograd(per_sample, with_alpha):
    """Forward, and reduce -> finalize -> dx composed, against autograd through the batch statistics."""
    N, HW, C, eps = 3, 5, 4, 1e-5
    x = _rand((N, HW, C), 1).requires_grad_(True)
    gamma = (1 + 0.3 * _rand((N, C) if per_sample else (C,), 2)).requires_grad_(True)
    beta = _rand((N, C) if per_sample else (C,), 3, 0.5).requires_grad_(True)
    alpha = (_rand((C,), 4, 0.3)).requires_grad_(True) if with_alpha else None
    w = _rand((N, HW, C), 5)
    mu = x.mean((0, 1))
    var = ((x - mu) ** 2).mean((0, 1))
    rstd = 1 / torch.sqrt(var + eps)
    ga = gamma[:, None, :] if per_sample else gamma
    be = beta[:, None, :] if per_sample else beta
    pre = (x - mu) * rstd * ga + be
    y = F.relu(pre) + alpha * (pre - pre.abs()) / 2 if with_alpha else pre
    (y * w).sum().backward()
    d = lambda t: None if t is None else t.detach()           # noqa: E731
    r = E.bn_fwd(d(x), d(mu), d(rstd), d(ga), d(be), d(alpha))
    assert torch.allclose(r["ref"], d(y), rtol=0, atol=1e-12)
    part = E.bn_bwd_reduce(d(x), w, d(mu), d(rstd), d(ga), d(be), d(alpha))["ref"]
    dgamma, dbeta, dalpha, cm = _finalize_loop(part, d(gamma), per_sample, N * HW)
    assert torch.allclose(dgamma, gamma.grad, rtol=0, atol=1e-12)
    assert torch.allclose(dbeta, beta.grad, rtol=0, atol=1e-12)
    if with_alpha:
        assert torch.allclose(dalpha, alpha.grad, rtol=0, atol=1e-12)
    else:
        assert float(part[2].abs().max()) == 0.0
    dx = E.bn_bwd_dx(d(x), w, d(mu), d(rstd), d(ga), d(be), d(alpha), cm, None)["ref"]
    assert torch.allclose(dx, x.grad, rtol=0, atol=1e-12)
    add = _rand((N, HW, C), 6)
    dx2 = E.bn_bwd_dx(d(x), w, d(mu), d(rstd), d(ga), d(be), d(alpha), cm, add)["ref"]
    assert torch.allclose(dx2, x.grad + add, rtol=0, atol=1e-12)


def test_bwd_reduce_reference_matches_direct_loop():
    N, HW, C = 2, 3, 2
    x, dy = _rand((N, HW, C), 11), _rand((N, HW, C), 12)
    mean, rstd = _rand((C,), 13, 0.5), _rand((C,), 14).abs() + 0.5
    gamma, beta, alpha = 1 + 0.3 * _rand((N, C), 15), _rand((N, C), 16, 0.5), _rand((C,), 17, 0.3)
    x[1, 2, 1] = mean[1] - beta[1, 1] / (rstd[1] * gamma[1, 1])            # a pre-activation of (nearly) zero
    part = E.bn_bwd_reduce(x, dy, mean, rstd, gamma[:, None, :], beta[:, None, :], alpha)["ref"]
    for n in range(N):
        for c in range(C):
            p = [0.0, 0.0, 0.0]
            for r in range(HW):
                xh = (x[n, r, c].item() - mean[c].item()) * rstd[c].item()
                pre = xh * gamma[n, c].item() + beta[n, c].item()
                a = alpha[c].item()
                g = dy[n, r, c].item() * (1.0 if pre > 0 else (a if pre < 0 else 0.5 * a))
                p[0] += g
                p[1] += g * xh
                p[2] += dy[n, r, c].item() * min(pre, 0.0)
            for q in range(3):
                assert abs(part[q, n, c].item() - p[q]) < 1e-12


def test_prelu_references_match_autograd():
    x = _rand((7, 5), 21).requires_grad_(True)
    with torch.no_grad():
        x[2, 3] = 0.0                                       # the alpha / 2 rule: TF's (and torch's) d|x|/dx = 0 at 0
        x[5, 0] = 0.0
    alpha = _rand((5,), 22, 0.3).requires_grad_(True)
    dy = _rand((7, 5), 23)
    y = F.relu(x) + alpha * (x - x.abs()) / 2
    y.backward(dy)
    xd, ad = x.detach(), alpha.detach()
    assert torch.allclose(E.prelu_fwd(xd, ad)["ref"], y.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(E.prelu_bwd(xd, dy, ad, None)["ref"], x.grad, rtol=0, atol=1e-12)
    assert torch.allclose(E.prelu_bwd(xd, dy, ad, dy)["ref"], x.grad + dy, rtol=0, atol=1e-12)
    assert torch.allclose(E.colsum(dy * xd.clamp(max=0))[0], alpha.grad, rtol=0, atol=1e-12)
    assert torch.equal(E.slope(torch.zeros(5, dtype=D64), ad), 0.5 * ad)


def test_maxpool_references_match_autograd_and_first_maximum_loop():
    x = _rand((2, 4, 6, 3), 31).requires_grad_(True)        # continuous data: no ties
    y = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    dy = _rand(tuple(y.shape), 32)
    y.backward(dy)
    assert torch.equal(E.maxpool_fwd(x.detach()), y.detach())
    assert torch.equal(E.maxpool_bwd(x.detach(), dy), x.grad)
    # ties: the first maximum in the order (0,0), (0,1), (1,0), (1,1), by a direct loop
    xt = torch.round(_rand((2, 4, 4, 3), 33).clamp(-1, 1) * 2) / 2 + 0.0
    dyt = _rand((2, 2, 2, 3), 34)
    want = torch.zeros_like(xt)
    ties = 0
    for n in range(2):
        for i in range(2):
            for j in range(2):
                for c in range(3):
                    w = [xt[n, 2 * i + p, 2 * j + q, c].item() for p, q in ((0, 0), (0, 1), (1, 0), (1, 1))]
                    k = w.index(max(w))
                    ties += w.count(max(w)) > 1
                    want[n, 2 * i + k // 2, 2 * j + k % 2, c] = dyt[n, i, j, c]
    assert ties >= 5                                       # of 24 windows
    assert torch.equal(E.maxpool_bwd(xt, dyt), want)
    assert not torch.equal(E.maxpool_bwd(xt, dyt, last=True), want)


def test_sum_pool_and_linear_references():
    x = _rand((3, 5, 4), 41).requires_grad_(True)
    dy = _rand((3, 4), 42)
    y = x.sum(1)
    y.backward(dy)
    assert torch.allclose(E.colsum(x.detach()[1])[0], y.detach()[1], rtol=0, atol=1e-12)
    assert torch.equal(dy[:, None, :].expand(3, 5, 4), x.grad)
    a, b = _rand((16,), 43), _rand((16,), 44)
    assert torch.allclose(E.lincomb(a, 0.7, b, -0.3)["ref"], 0.7 * a - 0.3 * b, rtol=0, atol=1e-12)
    assert torch.allclose(E.lincomb(a, 0.7, None, 5.0)["ref"], 0.7 * a, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------
# the simulated kernel and its mutations
# ------------------------------------------------------------------------------------------
def _rtz_bf16(x32):
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _rows(v, per_sample):
    return v[:, None, :] if per_sample else v


def first_step_elems(c):
    """Elements the kernel's first grid-stride step covers (None: the generic forms, not modelled here)."""
    if c["xdt"] != E.BF16 or c["ydt"] != E.BF16 or c["align"]:
        return None
    if c["op"] == "lincomb" and c["n"] % 8 == 0:
        return 2048 * 256 * 8
    if c["op"] in ("bn_fwd", "bn_bwd_dx", "prelu_fwd", "prelu_bwd") and c["C"] % 8 == 0:
        CV, rows = c["C"] // 8, c["N"] * c["HW"]
        a, b = CV, 256
        while b:
            a, b = b, a % b
        unit = CV // a
        want = min(max((rows * CV + 255) // 256, 1), 4096)
        grid = (want + unit - 1) // unit * unit
        return grid * 256 // CV * c["C"]
    return None


MUTATIONS = {
    # name: ops it applies to
    "previous sample's gamma / beta on a sample's first row": ("bn_fwd", "bn_bwd_dx"),
    "last group of 8 channels skipped": ("bn_fwd", "bn_bwd_dx", "prelu_fwd", "prelu_bwd", "bn_stats", "bias_grad"),
    "rows after the first grid-stride step skipped": ("bn_fwd", "bn_bwd_dx", "prelu_fwd", "prelu_bwd", "lincomb"),
    "last maximum instead of first": ("maxpool_bwd",),
    "slope alpha instead of alpha / 2 at 0": ("prelu_bwd",),
    "dx_add dropped": ("bn_bwd_dx", "prelu_bwd"),
    "dx_add added twice when it aliases dx": ("bn_bwd_dx", "prelu_bwd"),
    "sa used where sa_dev is given": ("lincomb",),
    "output truncated instead of RNE": ("bn_fwd", "prelu_fwd", "lincomb", "cast"),
    "sum x^2 from squares rounded to bf16": ("bn_stats",),
}
M = list(MUTATIONS)


def applies(mut, c):
    if c["op"] not in MUTATIONS[mut]:
        return False
    allbf = c["xdt"] == E.BF16 and c["ydt"] == E.BF16
    if mut == M[0]:
        return c["per_sample"] == 1 and c["N"] > 1
    if mut == M[1]:
        return allbf and c["C"] % 8 == 0
    if mut == M[2]:
        fs = first_step_elems(c)
        return fs is not None and fs < E.numel(c)
    if mut == M[5]:
        return c["add"] in ("sep", "alias")
    if mut == M[6]:
        return c["add"] == "alias"
    if mut == M[7]:
        return c["sa_dev"]
    if mut == M[8]:
        return c["ydt"] == E.BF16
    return True


def simulate(c, i, mut=None):
    """The outputs of a 'kernel' that evaluates the documented formula in fp32 and rounds once to the output type;
    ``mut`` names the bug it has."""
    op, N, HW, C, ps = c["op"], c["N"], c["HW"], c["C"], c["per_sample"]
    xdt, ydt = E.tdt(c["xdt"]), E.tdt(c["ydt"])
    rnd = (lambda t, dt: _rtz_bf16(t) if dt == torch.bfloat16 else t) if mut == M[8] else (lambda t, dt: t.to(dt))
    add = i.get("add")
    if mut == M[5]:
        add = None
    out = {}
    if op in ("bn_fwd", "bn_bwd_reduce", "bn_bwd_dx"):
        ga, be = _rows(i["gamma"], ps), _rows(i["beta"], ps)
        if mut == M[0]:
            ga, be = ga.expand(N, HW, C).clone(), be.expand(N, HW, C).clone()
            ga[1:, 0], be[1:, 0] = i["gamma"][:-1], i["beta"][:-1]
        if op == "bn_fwd":
            out["y"] = rnd(E.bn_fwd(i["x"], i["mean"], i["rstd"], ga, be, i["alpha"], F32)["ref"], ydt)
        elif op == "bn_bwd_reduce":
            out["part"] = E.bn_bwd_reduce(i["x"], i["dy"], i["mean"], i["rstd"], ga, be, i["alpha"], F32)["ref"]
        else:
            v = E.bn_bwd_dx(i["x"], i["dy"], i["mean"], i["rstd"], ga, be, i["alpha"], i["cm"], add, F32)["ref"]
            if mut == M[6]:
                v = v + i["add"].float()
            out["dx"] = rnd(v, xdt)
    elif op == "prelu_fwd":
        out["y"] = rnd(E.prelu_fwd(i["x"], i["alpha"], F32)["ref"], ydt)
    elif op == "prelu_bwd":
        if c["add"] != "null-dx":
            if mut == M[4]:
                x, a = i["x"].float(), i["alpha"]
                v = i["dy"].float() * torch.where(x > 0, torch.ones(()), a)
                v = v if add is None else v + add.float()
            else:
                v = E.prelu_bwd(i["x"], i["dy"], i["alpha"], add, F32)["ref"]
            if mut == M[6]:
                v = v + i["add"].float()
            out["dx"] = rnd(v, xdt)
        if c["dalpha"]:
            t = (i["dy"].float() * i["x"].float().clamp(max=0)).reshape(-1, C)
            out["dalpha"] = (i["dalpha0"].double() + t.sum(0).double()).float()
    elif op == "bn_stats":
        x = i["x"].float().reshape(-1, C)
        sq = x * x
        if mut == M[9]:
            sq = sq.to(torch.bfloat16).float()
        out["sums"] = i["sums0"] + torch.cat([x.sum(0), sq.sum(0)]).double()
    elif op == "bias_grad":
        out["db"] = i["x"].float().reshape(-1, C).sum(0)
    elif op == "sum_pool_fwd":
        out["y"] = i["x"].float().sum(1)
    elif op == "sum_pool_bwd":
        out["dx"] = i["dy"].to(xdt)[:, None, :].expand(N, HW, C).contiguous()
    elif op == "maxpool_fwd":
        out["y"] = E.maxpool_fwd(i["x"])
    elif op == "maxpool_bwd":
        out["dx"] = E.maxpool_bwd(i["x"], i["dy"], last=mut == M[3])
    elif op == "lincomb":
        s = E.POISON if mut == M[7] else float(i["s"])
        out["y"] = rnd(E.lincomb(i["a"], s, i["b"], i["sb"], F32)["ref"], ydt)
    elif op == "dot":
        out["out"] = (i["out0"].double() + (i["a"].float() * i["b"].float()).sum().double()).float()
    elif op == "cast":
        out["y"] = rnd(i["x"].float(), ydt)
    # the bugs that leave prefilled NaNs behind
    for k, v in out.items():
        if mut == M[1] and k in ("y", "dx"):
            v = v.clone()
            v[..., C - 8:] = float("nan")
        elif mut == M[1]:                                   # sums / db: the last 8 columns keep their initial value
            v = v.clone()
            v[..., C - 8:] = i["sums0"][..., C - 8:] if op == "bn_stats" else 0.0
        elif mut == M[2] and k in ("y", "dx"):
            v = v.clone()
            v.view(-1)[first_step_elems(c):] = float("nan")
        out[k] = v
    return out


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
        self.nbad += 0 if same else int((got != want.to(got.dtype)).sum())


def _run(c, mut=None):
    gen = torch.Generator().manual_seed(1234)
    i = E.make_inputs(c, "cpu", gen)
    rec = Rec()
    namb, nout = E.check(c, i, simulate(c, i, mut), rec)
    return rec, namb, nout


@pytest.mark.parametrize("op", E.OPS)
def test_gate_accepts_a_correct_kernel_and_ambiguity_is_within_the_cap(op):
    """Every small case of the table: the simulated correct kernel passes, and the reference alone marks no more than
    AMBIGUITY_CAP of the elements as sign-ambiguous."""
    worst, n, tamb = 0.0, 0, 0
    for c in E.cases(op, small=True):
        rec, namb, nout = _run(c)
        assert rec.ok, (E.describe(c), rec.worst, rec.nbad)
        assert namb <= E.AMBIGUITY_CAP * nout, (E.describe(c), namb, nout)
        worst, n, tamb = max(worst, rec.worst), n + 1, tamb + namb
    assert n > 0
    print("%-14s %3d small cases accepted (worst err/bound %.3f, %d ambiguous elements)" % (op, n, worst, tamb))


@pytest.mark.parametrize("mut", M)
def test_gate_rejects(mut):
    """Each simulated bug is rejected on at least one small case of the table (the smallest that it applies to first)."""
    tried = 0
    for c in sorted((c for c in E.cases(small=True) if applies(mut, c)), key=E.numel):
        tried += 1
        rec, _, _ = _run(c, mut)
        if not rec.ok:
            print("mutation %-55s rejected on %s: %d outputs outside the bound (case %d it applies to)"
                  % (mut, E.describe(c), rec.nbad, tried))
            return
    raise AssertionError("no small case of the table rejects: %s (%d cases tried)" % (mut, tried))


def test_every_mutation_is_rejected_where_it_matters_most():
    """The cases built for a bug reject it: the second grid-stride step, the tie-heavy max pool, the planted zeros, the
    poisoned host scalar, the aliased dx_add and the large-mean statistics."""
    by_name = {E.describe(c): c for c in E.CASES}
    for mut, name in ((M[2], "bn_fwd[12x4096x200 ps1]"), (M[0], "bn_bwd_dx[12x4096x200 ps1 add-alias]"),
                      (M[3], "maxpool_bwd[3x8x8x24 f ties]"), (M[3], "maxpool_bwd[3x8x8x24 b ties]"),
                      (M[4], "prelu_bwd[4x256x24 zeros]"), (M[4], "prelu_bwd[4x256x3 zeros]"),
                      (M[7], "lincomb[n4608 b dev1 b1]"), (M[7], "lincomb[n2052 f dev1 b0]"),
                      (M[6], "prelu_bwd[4x256x12 zeros add-alias]"), (M[9], "bn_stats[8x64x24 mean 8 +- 0.5]"),
                      (M[9], "bn_stats[8x64x20 mean 8 +- 0.5 f32]"), (M[2], "lincomb[n5242880 dev1]")):
        c = by_name[name]
        assert applies(mut, c), (mut, name)
        rec, _, _ = _run(c, mut)
        assert not rec.ok, (mut, name)


def test_table_covers_what_the_issue_lists():
    cs = E.CASES
    big = [c for c in cs if not c["small"]]
    for op in ("bn_stats", "bn_bwd_reduce", "prelu_bwd", "bias_grad"):          # the four colreduce functors
        n = [E.numel(c) for c in big if c["op"] == op]
        assert any(v >= E.WIDE_MIN for v in n) and any(E.WIDE_MIN - 2 * 64 * 1536 < v < E.WIDE_MIN for v in n), op
        assert any(v * 4 >= 100 << 20 for v in n), op
    edge = [c for c in cs if c["small"]]
    assert {3, 6, 12, 20, 24, 200, 776} <= {c["C"] for c in edge if c["op"] == "bn_fwd"}
    assert {1, 3, 25, 97} <= {c["C"] // 8 for c in edge if c["op"] == "bn_bwd_dx" and c["C"] % 8 == 0}
    for op in E.TWO_DTYPES:
        assert {(c["xdt"], c["ydt"]) for c in edge if c["op"] == op} == set(E.PAIRS)
        assert any(c["HW"] == 1 for c in edge if c["op"] == op)
        assert any(c["HW"] == 16 and c["N"] == 256 for c in edge if c["op"] == op)
        assert any(c["align"] == 8 for c in edge if c["op"] == op)
    for op in ("bn_bwd_dx", "prelu_bwd"):
        assert {"none", "sep", "alias"} <= {c["add"] for c in edge if c["op"] == op}
    assert {(c["per_sample"], c["alpha"]) for c in edge if c["op"] == "bn_bwd_reduce"} == {(0, False), (0, True),
                                                                                           (1, False), (1, True)}
    lc = [c for c in edge if c["op"] == "lincomb"]
    assert any(c["n"] % 8 == 4 for c in lc) and any(c["sa_dev"] for c in lc) and any(not c["b"] for c in lc)
    assert len({E.describe(c) for c in cs}) == len(cs)
