"""CPU checks of tests/glue_ref.py, the gate of the batch-norm finalisers and the fp32 glue kernels: the float64 references
against torch autograd and direct Python loops, the simulated fp32 kernel inside the bound on EVERY row of the case table,
every mutation rejected, the preconditions of the constructed inputs, the gap of the whole-tensor criterion written down,
and the case table itself."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_ref as G
from tests.loss_ref import Ref

D64 = torch.float64
CPU = torch.device("cpu")
SMALL = 1 << 20              # mutations and preconditions are searched on the rows below this size


def _inputs(c, seed=0):
    return G.make_inputs(c, CPU, torch.Generator().manual_seed(1000 + seed))


def _ref(c, i):
    return {k: (v.v if isinstance(v, Ref) else v) for k, v in G.formula(c, i, Ref).items() if not k.startswith("_")}


def _verdict(c, i, outs):
    rec = G.Rec()
    G.check(c, i, outs, rec)
    return rec


def _find(op, **kw):
    for c in G.cases(op):
        if all(c[k] == v for k, v in kw.items()):
            return c
    raise KeyError((op, kw))


def _rel_err(a, b):
    """tests/common.rel_err: the relative L2 norm of a whole tensor."""
    a, b = a.double().numpy().ravel(), b.double().numpy().ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------------
# references against autograd and direct loops
# ------------------------------------------------------------------------------------------
def test_exact_statistics_against_numpy_and_the_issue_figures():
    """Mean 300, sigma 0.05, n = 4096: the rational reference agrees with numpy's two-pass variance of the same float64
    samples to the fp64 form's own error (3.4e-7 relative in the issue's run; here asserted below 1e-5, thirty times the
    figure), and the same subtraction in fp32 is off by more than 40 % in every channel."""
    gen = torch.Generator().manual_seed(7)
    x = (torch.randn(4096, 8, generator=gen) * 0.05 + 300.0).double()
    sums = torch.cat([x.sum(0), (x * x).sum(0)])
    m, v, A = G.exact_stats(sums, 4096.0, 8)
    want = torch.tensor(np.var(x.numpy(), axis=0))
    assert float(((v - want).abs() / want).max()) < 1e-5
    assert float((m - x.mean(0)).abs().max()) < 1e-10
    assert float((G.U64 * A / v).max()) < 1e-5                   # what the bound charges the kernel's fp64 steps
    v32 = (sums[8:] / 4096.0).float() - (sums[:8] / 4096.0).float() ** 2
    assert float(((v32.double() - want).abs() / want).min()) > 0.4


def test_bwd_finalize_reference_against_direct_loops():
    for c in (_find("bn_bwd_finalize", N=3, C=1), _find("bn_bwd_finalize", N=5, C=63),
              _find("bn_bwd_finalize", N=16, C=24)):
        i = _inputs(c)
        r = _ref(c, i)
        N, C, ps = c["N"], c["C"], c["per_sample"]
        p, g = i["part"].double(), i["gamma"].double()
        for ch in range(C):
            s0 = sum(float(p[0, n, ch]) for n in range(N))
            s1 = sum(float(p[1, n, ch]) for n in range(N))
            g0 = sum(float(g[n, ch] if ps else g[ch]) * float(p[0, n, ch]) for n in range(N)) / i["count"]
            g1 = sum(float(g[n, ch] if ps else g[ch]) * float(p[1, n, ch]) for n in range(N)) / i["count"]
            assert abs(float(r["cm"][ch]) - g0) < 1e-12 and abs(float(r["cm"][C + ch]) - g1) < 1e-12
            if not ps:
                assert abs(float(r["dbeta"][ch]) - s0) < 1e-12 and abs(float(r["dgamma"][ch]) - s1) < 1e-12
            if c["dalpha"]:
                assert abs(float(r["dalpha"][ch]) - sum(float(p[2, n, ch]) for n in range(N))) < 1e-12
        if ps:
            assert torch.equal(r["dbeta"], i["part"][0]) and torch.equal(r["dgamma"], i["part"][1])
        assert ("dalpha" in r) == bool(c["dalpha"])


def test_renorm_references_against_a_scalar_restatement_and_autograd():
    c = _find("renorm_coeffs", C=255, scale_is_var=1, weight=0.3, update=1)
    i = _inputs(c)
    r = _ref(c, i)
    m, v, _ = G.exact_stats(i["sums"], i["count"], c["C"])
    for ch in (0, 1, 2, 3, 4, 5, 254):
        eps, w = i["eps"], 0.3
        w = float(i["weight0"])
        sigma = (max(float(v[ch]), 0.0) + eps) ** 0.5
        sref = (float(i["ref_scale0"][ch]) + eps) ** 0.5
        sw = w * sref + (1 - w) * sigma
        mw = w * float(i["ref_mean0"][ch]) + (1 - w) * float(m[ch])
        assert abs(float(r["r"][ch]) - min(max(sigma / sw, i["rmin"]), i["rmax"])) < 1e-12
        assert abs(float(r["d"][ch]) - min(max((float(m[ch]) - mw) / sw, -i["dmax"]), i["dmax"])) < 1e-12
        assert abs(float(r["ref_scale"][ch]) - (float(i["ref_scale0"][ch]) * i["decay"]
                                                + max(float(v[ch]), 0.0) * (1 - i["decay"]))) < 1e-12
    assert abs(float(r["weight"]) - (w * i["fade"] + 1 - i["fade"])) < 1e-15
    # the affine pair: dgamma of bg_renorm_affine_bwd is the autograd gradient of the forward in gamma
    cf = _find("renorm_affine_fwd", rows=3, C=5)
    i = _inputs(cf)
    g = i["gamma"].double().requires_grad_(True)
    ge, be = i["r"].double() * g, i["beta"].double() + i["d"].double() * g
    rf = _ref(cf, i)
    assert torch.allclose(rf["gamma_eff"], ge.detach(), rtol=0, atol=1e-14)
    assert torch.allclose(rf["beta_eff"], be.detach(), rtol=0, atol=1e-14)
    cb = _find("renorm_affine_bwd", rows=3, C=5)
    ib = dict(_inputs(cb), r=i["r"], d=i["d"])
    want, = torch.autograd.grad([ge, be], [g], [ib["dgamma_eff"].double(), ib["dbeta_eff"].double()])
    assert torch.allclose(_ref(cb, ib)["dgamma"], want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("C", G.BOX_C)
def test_box_references_against_torch_and_the_adjoint_identity(C):
    for N, H, W in G.BOX_NHW:
        for s in G.BOX_SCALES:
            cd = _find("box2_down", N=N, H=H, W=W, C=C, scale=s)
            cu = _find("box2_up", N=N, H=H // 2, W=W // 2, C=C, scale=s) if (N, H // 2, W // 2) in G.BOX_NHW else dict(
                cd, op="box2_up", H=H // 2, W=W // 2)
            x = _inputs(cd)["x"]
            y = torch.randn(N, H // 2, W // 2, C, generator=torch.Generator().manual_seed(3))
            down = _ref(cd, dict(x=x))["y"]
            up = _ref(cu, dict(x=y))["y"].double()
            x64 = x.double().requires_grad_(True)
            pooled = F.avg_pool2d(x64.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * 4.0 * G.f32r(s)
            assert torch.allclose(down, pooled.detach(), rtol=0, atol=1e-13)
            near = F.interpolate(y.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
            assert torch.allclose(up, near * G.f32r(s), rtol=0, atol=1e-13)
            grad, = torch.autograd.grad(pooled, x64, y.double())        # up is the adjoint of down
            assert torch.allclose(up, grad, rtol=0, atol=1e-13)
            lhs, rhs = float((down * y.double()).sum()), float((x.double() * up).sum())
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_elementwise_and_tanh_references():
    c = _find("axpby", n=1027, a=0.37, b=-0.5)
    i = _inputs(c)
    assert torch.equal(_ref(c, i)["y"], i["a"] * i["x"].double() + i["b"] * i["y0"].double())
    c = _find("axpby", n=5, alias=True)
    i = _inputs(c)
    assert torch.equal(_ref(c, i)["y"], 0.25 * i["y0"].double())
    c = _find("scale_add", n=1027, scalar=0.37)
    i = _inputs(c)
    assert torch.equal(_ref(c, i)["y"], float(i["gamma"]) * i["o"].double() + i["x"].double())
    c = _find("tanh_bwd", data="sweep")
    i = _inputs(c)
    x = torch.randn(64, dtype=D64, generator=torch.Generator().manual_seed(5)).requires_grad_(True)
    y = torch.tanh(x)
    dy = torch.randn(64, dtype=D64, generator=torch.Generator().manual_seed(6))
    want, = torch.autograd.grad(y, x, dy)
    got = G.tanh_bwd(Ref, c, dict(y=y.detach(), dy=dy))["dx"].v
    assert torch.allclose(got, want, rtol=0, atol=1e-14)
    assert i["y"].numel() % 2 == 1 and _inputs(_find("tanh_fwd", data="sweep"))["x"].numel() % 2 == 1
    for edge in (1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 0.0):
        assert bool((i["y"] == edge).any())


def test_pad_and_pack_references():
    """Split: hi + lo is the source exactly and lo is the exact residual; fold is the adjoint of duplicate; zero fill and
    truncation by direct loops; pack_t is the per-tap transpose."""
    c = _find("pad_channels", mode=1, sdt=0, ddt=0, Cs=3, Cd=8, inner=7)
    i = _inputs(c)
    d = _ref(c, i)["dst"]
    assert torch.equal(d[:, :3].double() + d[:, 3:6].double(), i["src"].double()) and bool((d[:, 6:] == 0).all())
    assert torch.equal(d[:, :3], i["src"].to(torch.bfloat16).float())
    c2 = _find("pad_channels", mode=2, sdt=0, ddt=0, Cs=3, Cd=6, inner=7)
    c3 = _find("pad_channels", mode=3, sdt=0, ddt=0, Cs=6, Cd=3, inner=7)
    i2, i3 = _inputs(c2), _inputs(c3)
    dup, fold = _ref(c2, i2)["dst"].double(), _ref(c3, i3)["dst"]
    lhs, rhs = float((dup * i3["src"].double()).sum()), float((i2["src"].double() * fold).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    for Cs, Cd in ((8, 3), (5, 16)):
        c0 = _find("pad_channels", mode=0, sdt=0, ddt=0, Cs=Cs, Cd=Cd, inner=7)
        i0 = _inputs(c0)
        d0 = _ref(c0, i0)["dst"]
        for ch in range(Cd):
            want = i0["src"][:, ch] if ch < Cs else torch.zeros_like(d0[:, ch])
            assert torch.equal(d0[:, ch], want)
    cw = _find("weight_pack", taps=9, R=8, Cc=62)
    iw = _inputs(cw)
    r = _ref(cw, iw)
    for t in range(9):
        assert torch.equal(r["pack_t"][t], iw["w"][t].to(torch.bfloat16).t())
    assert r["pack_p"].dtype == torch.bfloat16 and float(r["pack_p"].reshape(-1)[0]) == 1.0      # the tie goes to even
    assert float(r["pack_p"].reshape(-1)[-1]) == 1.0 + 2.0 ** -6


# ------------------------------------------------------------------------------------------
# the simulated kernel on every row; the preconditions of the constructed inputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", G.OPS)
def test_simulated_kernel_passes_every_row(op):
    """Honest fp32 (one rounding per operation, the kernel's order) lies inside every bound, so none is tighter than the
    arithmetic allows; routing rows are reproduced bit for bit."""
    worst = 0.0
    for k, c in enumerate(G.cases(op)):
        i = _inputs(c, k)
        rec = _verdict(c, i, G.simulate(c, i))
        assert not rec.bad, (G.describe(c), rec.bad)
        worst = max(worst, rec.worst)
    assert worst <= 1.0
    print("\n[%s] %d rows, worst err / bound of the simulated kernel %.4f" % (op, len(G.cases(op)), worst))


def test_constructed_inputs_meet_their_preconditions():
    seen = dict(neg=0, ratio=0, below=0, inside=0, above=0, dhi=0, dlo=0, tiny=0)
    for k, c in enumerate(G.cases("bn_finalize")):
        i = _inputs(c, k)
        C = c["C"]
        if c["rows"] == 1:
            continue
        neg = i["pattern"] == G.NEG_VAR
        m = i["sums"][:C] / i["count"]
        var64 = i["sums"][C:] / i["count"] - m * m               # as the kernel forms it
        _, vex, _ = G.exact_stats(i["sums"], i["count"], C)
        assert bool((var64[neg] < 0).all()) and bool((vex[neg] < 0).all()), G.describe(c)
        assert bool((var64[~neg] > 0).all())
        r = _ref(c, i)
        assert bool(((r["rstd"][neg] * i["eps"] ** 0.5 - 1.0).abs() < 1e-15).all())     # the clamp yields rsqrt(eps)
        seen["neg"] += int(neg.sum())
        hard = i["pattern"] == G.RATIO_6000
        if bool(hard.any()):
            ratio = m[hard].abs() / vex[hard].sqrt()
            assert 5000 < float(ratio.min()) and float(ratio.max()) < 7000
            seen["ratio"] += int(hard.sum())
    for k, c in enumerate(G.cases("renorm_coeffs")):
        if c["clipset"] != 0 or c["weight"] == 0.0:
            continue                                             # (w = 0: r = 1 and d = 0 whatever the running statistics)
        i = _inputs(c, k)
        r_raw, d_raw = G.formula(c, i, Ref)["_raw"]
        p = i["pattern"]
        for name, pat, ok in (("inside", 0, (r_raw > i["rmin"]) & (r_raw < i["rmax"]) & (d_raw.abs() < i["dmax"])),
                              ("below", 1, r_raw < i["rmin"]), ("above", 2, r_raw > i["rmax"]),
                              ("dhi", 3, d_raw > i["dmax"]), ("dlo", 4, d_raw < -i["dmax"])):
            assert bool(ok[p == pat].all()), (G.describe(c), name)
            seen[name] += int((p == pat).sum())
        if not c["scale_is_var"]:
            tiny = p == 5
            assert bool((i["ref_scale0"][tiny].double() < i["eps"] ** 0.5).all())
            seen["tiny"] += int(tiny.sum())
    assert all(v > 0 for v in seen.values()), seen


def test_update_free_and_momentum_one_rows_are_exact_outputs():
    """update = 0 leaves ref_mean, ref_scale and *weight bit-unchanged; momentum 1 leaves the moving statistics; C = 600
    moves *weight exactly once (a single value) and every channel uses the old one."""
    c = _find("renorm_coeffs", C=600, weight=0.3, update=0, scale_is_var=0)
    i = _inputs(c)
    r = G.formula(c, i, Ref)
    assert r["ref_mean"] is i["ref_mean0"] and r["ref_scale"] is i["ref_scale0"] and r["weight"] is i["weight0"]
    c = _find("renorm_coeffs", C=600, weight=0.3, update=1, scale_is_var=0)
    i = _inputs(c)
    r = G.formula(c, i, Ref)
    assert r["weight"].v.numel() == 1 and abs(float(r["weight"].v) - (0.3 * 0.999 + 0.001)) < 1e-7
    late = G.simulate(c, i, "*weight updated before it is read")
    good = G.simulate(c, i)
    assert torch.equal(late["r"][:256], good["r"][:256]) and not torch.equal(late["r"][256:], good["r"][256:])
    done = 0
    for c in G.cases("bn_finalize"):
        if c["momentum"] == 1.0 and (c["mm"] or c["mv"]):
            i = _inputs(c)
            r = G.formula(c, i, Ref)
            assert all(r[k] is i[k0] for k, k0 in (("moving_mean", "mm0"), ("moving_var", "mv0")) if k in r)
            done += 1
    assert done >= 4


# ------------------------------------------------------------------------------------------
# mutations
# ------------------------------------------------------------------------------------------
def _exposing(what, op, pred):
    """The rows of the table (below SMALL) on which the gate rejects the mutant, with the mutant's worst whole-tensor
    relative error on each."""
    out = []
    for k, c in enumerate(G.cases(op)):
        if G.numel(c) >= SMALL or not pred(c):
            continue
        i = _inputs(c, k)
        bad = G.simulate(c, i, what)
        if _verdict(c, i, bad).bad:
            ref = _ref(c, i)
            with np.errstate(all="ignore"):
                worst = max(_rel_err(bad[n], ref[n]) for n in ref)
            out.append((c, worst))
    return out


_EXPOSED = {}


@pytest.mark.parametrize("what,op", [(m[0], m[1]) for m in G.MUTATIONS], ids=["%s [%s]" % (m[0], m[1]) for m in G.MUTATIONS])
def test_mutation_is_rejected(what, op):
    pred = [m[2] for m in G.MUTATIONS if (m[0], m[1]) == (what, op)][0]
    rows = _exposing(what, op, pred)
    _EXPOSED[(what, op)] = rows
    assert rows, "'%s' passed the gate on every row of %s" % (what, op)


# What ``rel_err < 1e-5`` of the whole tensor - the criterion these entry points were held to inside the wrappers - makes of
# the mutants, on the rows where the gate rejects them.  The unclamped negative variance stays below it on three rows
# (3.8e-7 at the least: a few channels of 256 - 300 moved by 4e-6).  Every other mutant is above 1e-5 on each row that
# exposes it - the Bessel factor by as little as 1.7e-5 - so what let them through was not the criterion's width but
# that no test ran these rows: N off the multiples of 4 and 32, count != N, C > 256 with the fade-in weight, a clip on
# each side, non-square maps, |mean| / sigma = 6000.
LET_THROUGH_BY_REL_ERR = {("negative variance left unclamped", "bn_finalize")}


def test_whole_tensor_criterion_accepts_what_the_gate_rejects():
    got = set()
    least = {}
    for what, op, pred in G.MUTATIONS:
        rows = _EXPOSED.get((what, op)) or _exposing(what, op, pred)
        errs = [e for _, e in rows]
        least[(what, op)] = min([e for e in errs if e == e] or [float("inf")])
        if any(e < 1e-5 for e in errs):
            got.add((what, op))
    print("\nleast whole-tensor rel_err on a rejected row:\n" + "\n".join("%-62s %-18s %.3g" % (k + (v,))
                                                                          for k, v in least.items()))
    assert got == LET_THROUGH_BY_REL_ERR
    assert 1e-5 < least[("Bessel factor on the wrong side", "bn_finalize")] < 1e-4


# ------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------
def test_case_table():
    assert G._cases() == G.CASES
    names = [G.describe(c) for c in G.CASES]
    assert len(set(names)) == len(names)
    by = {op: G.cases(op) for op in G.OPS}
    assert all(by[op] for op in G.OPS)
    assert set(G.ENTRY.values()) == {
        "bg_bn_finalize", "bg_bn_population", "bg_bn_bwd_finalize", "bg_renorm_coeffs", "bg_renorm_affine_fwd",
        "bg_renorm_affine_bwd", "bg_box2_down", "bg_box2_up", "bg_axpby", "bg_add", "bg_scale_add", "bg_scale_dev",
        "bg_tanh_fwd", "bg_tanh_bwd", "bg_pad_channels", "bg_weight_pack"}
    f = by["bn_finalize"]
    assert {c["C"] for c in f} == set(G.BNF_C) and {c["momentum"] for c in f} == {0.0, 0.98, 1.0}
    assert {(c["mm"], c["mv"]) for c in f} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c["mult"] for c in f} == {1, 2}
    assert {(c["unbiased"], c["mv"]) for c in f} >= {(0, 1), (1, 1)} and any(c["rows"] == 1 and c["unbiased"] for c in f)
    assert any(c["momentum"] == 1.0 and c["mm"] and c["mv"] for c in f)
    b = by["bn_bwd_finalize"]
    assert {c["N"] for c in b} >= set(G.BWD_N) and {c["C"] for c in b} >= set(G.BWD_C)
    for N in (5, 33, 37):                                         # the tails: both forms of gamma, dalpha NULL and not
        assert {c["per_sample"] for c in b if c["N"] == N} == {0, 1} and {c["dalpha"] for c in b if c["N"] == N} == {0, 1}
    assert {c["mult"] for c in b} == {1, 3} and sum(c["glu"] for c in b) == 1
    r = by["renorm_coeffs"]
    assert {(c["C"], c["scale_is_var"], c["weight"], c["update"]) for c in r if c["clipset"] == 0} == {
        (C, s, w, u) for C in G.RENORM_C for s in (0, 1) for w in (None, 0.0, 0.3, 1.0) for u in (0, 1)}
    assert G.CLIPSETS[1] == (1.0, 1.0, 0.0) and sum(c["clipset"] == 1 for c in r) == 2
    for op in ("renorm_affine_fwd", "renorm_affine_bwd"):
        assert {(c["rows"], c["C"]) for c in by[op]} >= {(a, b_) for a in G.AFFINE_ROWS for b_ in G.AFFINE_C}
        assert any(c["rows"] * c["C"] > G.GRID_CAP for c in by[op])
    for op in ("box2_down", "box2_up"):
        small = [c for c in by[op] if G.numel(c) < SMALL]
        assert {(c["C"], (c["N"], c["H"], c["W"]), c["scale"]) for c in small} == {
            (C, s, k) for C in G.BOX_C for s in G.BOX_NHW for k in G.BOX_SCALES}
        work = lambda c: c["N"] * c["H"] * c["W"] * c["C"] // (4 if op == "box2_down" else 1)        # noqa: E731
        assert any(c["C"] % 4 == 0 and work(c) // 4 > G.GRID_CAP for c in by[op])
        assert any(c["C"] % 4 != 0 and work(c) > G.GRID_CAP for c in by[op])
    for op in ("axpby", "add", "scale_add"):
        assert {c["n"] for c in by[op]} == set(G.EW_N) | {G.BIG4}
    assert G.BIG4 % 4 != 0 and G.BIG4 // 4 > G.GRID_CAP and G.BIG1 % 2 == 1 and G.BIG1 > G.GRID_CAP
    assert {(c["a"], c["b"]) for c in by["axpby"] if not c["alias"]} == {(a, b_) for a in (0.0, 1.0, 0.37)
                                                                         for b_ in (0.0, 1.0, -0.5)}
    assert any(c["alias"] for c in by["axpby"]) and any(c["alias"] for c in by["add"])
    assert {c["scalar"] for c in by["scale_add"]} == set(G.SCALARS) == {c["scalar"] for c in by["scale_dev"]}
    assert {c["n"] for c in by["scale_dev"]} == set(G.EW_N) | {G.BIG1}
    assert any(c["alias"] and c["n"] == G.BIG1 for c in by["scale_dev"])
    p = by["pad_channels"]
    for mode in range(4):
        for sdt in (0, 1):
            for ddt in (0, 1):
                for inner in (1, 7):
                    assert {(c["Cs"], c["Cd"]) for c in p if (c["mode"], c["sdt"], c["ddt"], c["inner"]) ==
                            (mode, sdt, ddt, inner)} >= set(G.PAD_PAIRS[mode])
    fast = [c for c in p if G.pad_fast_form(c) and not c["off4"] and c["outer"] == 300]
    assert fast and all(any(d["off4"] and d["name"] == c["name"] + " +4B" for d in p) for c in fast)
    assert not any(G.pad_fast_form(c) and c["sdt"] for c in p)
    assert sum(c["outer"] * (c["Cd"] * c["inner"] if not G.pad_fast_form(c) else 1) > G.GRID_CAP for c in p) == 3
    w = by["weight_pack"]
    assert {(c["taps"], c["R"], c["Cc"]) for c in w} >= {(t, a, b_) for t in G.PACK_TAPS for a in G.PACK_DIMS
                                                         for b_ in G.PACK_DIMS}
    assert any(c["taps"] * ((c["R"] + 63) // 64) * ((c["Cc"] + 63) // 64) > 2048 for c in w)
    # every aliasing form a call site uses is a row: x == y of bg_axpby (model.py, functional.py: the averaging of
    # multi-scale outputs, the loss scalings), a == y of bg_add (the fan-in of gradients), y == x of bg_scale_dev
    assert {c["op"] for c in G.CASES if c.get("alias")} == {"axpby", "add", "scale_dev"}
