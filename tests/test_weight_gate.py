"""CPU checks of tests/weight_ref.py: its float64 references against float64 autograd through oracle/ref_ops.py and against
direct Python loops (mask bits, packed layouts, a written-out TF Adam), and a mutation self-test of its case table in the
pattern of tests/test_elementwise_gate.py - a simulated correct kernel (the documented formula evaluated in fp32 in the
kernel's order, rounded once to the output type) passes the gate on every case, each simulated kernel bug is rejected on
at least one of them, and on the reference alone no case leaves an element out of the gate."""
import math

import pytest
import torch

from oracle import ref_ops
from tests import launch_replay as R
from tests import weight_ref as W

D64 = torch.float64
F32 = torch.float32
NAN = float("nan")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=D64) * scale


# ------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e-9])
def test_l2n_and_spectral_norm_references_match_autograd(scale):
    """l2n against ref_ops.l2_normalize, value and gradient - clamped (scale 1e-9), the gradient has no projection term;
    the power iteration and dW = (G - <G, w_norm> v^T u) / sigma against autograd through ref_ops' formula with u^, v^
    stop-gradient."""
    t = (_rand((7,), 1) * scale).requires_grad_(True)
    g = _rand((7,), 2)
    y = ref_ops.l2_normalize(t)
    y.backward(g)
    assert torch.allclose(W.l2n(t.detach()), y.detach(), rtol=1e-14, atol=0)
    if scale < 1e-6:
        assert torch.allclose(t.grad, g * 1e6, rtol=1e-12, atol=0)               # rs = 1e6, a constant
    else:
        rs = 1 / t.detach().norm()
        yh = y.detach()
        assert torch.allclose(t.grad, rs * (g - yh * (g * yh).sum()), rtol=1e-12, atol=1e-15)
    w = (_rand((5, 9), 3) * scale).requires_grad_(True)
    u0 = _rand((1, 9), 4)
    with torch.no_grad():
        v_hat = ref_ops.l2_normalize(u0 @ w.t())
        u_hat = ref_ops.l2_normalize(v_hat @ w)
    sigma = (v_hat @ w) @ u_hat.t()
    wn = w / sigma
    G = _rand((5, 9), 5)
    wn.backward(G)
    r = W.sn_fwd_ref(w.detach(), u0[0])
    assert torch.allclose(r["v"], v_hat[0], rtol=1e-13, atol=0)
    assert torch.allclose(r["u"], u_hat[0], rtol=1e-13, atol=0)
    assert torch.allclose(r["sigma"], sigma.detach().reshape(1), rtol=1e-13, atol=0)
    assert torch.allclose(r["wn"], wn.detach(), rtol=1e-13, atol=0)
    dw, E = W.sn_bwd_ref(G, r["wn"], r["u"], r["v"], r["sigma"])
    assert torch.allclose(dw, w.grad, rtol=1e-11, atol=1e-12 * float(w.grad.abs().max()))
    dw2, E2 = W.sn_bwd_ref(G, r["wn"], r["u"], r["v"], r["sigma"], dw0=G)
    assert torch.allclose(dw2, w.grad + G, rtol=1e-11, atol=1e-12 * float(w.grad.abs().max()))
    assert bool((E2 >= E).all())


@pytest.mark.parametrize("c,data", [(1, "gram"), (2, "gram"), (3, "gram"), (6, "gram"), (3, "clamp"), (6, "clamp")])
def test_gram_side_references_match_autograd(c, data):
    """ortho_cosine_ref / ortho_identity_ref / cosine_rows as functions of A against autograd of ref_ops' formula in A."""
    A = W._gram(c, data, torch.Generator().manual_seed(10 + c), "cpu").double()
    scale = W.SCALE
    leaf = A.clone().requires_grad_(True)
    eye = torch.eye(c, dtype=D64)
    nb = ref_ops.l2_normalize(torch.ones_like(eye) - eye, 1)
    reg = ref_ops.l2_normalize(leaf, 1) @ nb.t()
    loss = scale * 0.5 * (reg * reg).sum()
    loss.backward()
    loss = loss.detach()
    terms, dA = W.ortho_cosine_ref(A, scale)
    tol = 1e-12 * max(float(loss), 1e-30)
    assert abs(float(terms.v.sum()) - float(loss)) <= tol
    # (c == 2: the loss is constant and the gradient cancels to zero; its terms are of the order of scale * rn)
    mag = scale * float(torch.clamp((A * A).sum(1), min=W.EPS).rsqrt().max())
    assert torch.allclose(dA.v, leaf.grad, rtol=1e-10, atol=1e-12 * mag)
    assert abs(float(W.cosine_rows(A, scale).sum()) - float(loss)) <= tol
    assert bool(torch.isfinite(dA.v).all()) and bool(torch.isfinite(dA.e).all())
    if c == 1:
        assert float(loss) == 0.0 and float(dA.v.abs().max()) == 0.0
    leaf = A.clone().requires_grad_(True)
    li = scale * 0.5 * ((leaf - eye) ** 2).sum()
    li.backward()
    li = li.detach()
    terms, dI, _ = W.ortho_identity_ref(A, scale)
    assert abs(float(terms.v.sum()) - float(li)) <= 1e-12 * max(float(li), 1e-30)
    assert torch.allclose(dI, leaf.grad, rtol=1e-13, atol=0)
    S = A + A.t()
    assert torch.equal(S, S.t())


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("kind", ["ortho_cosine", "ortho"])
def test_composed_references_match_the_oracle(kind, clamp):
    """Both chains of OrthoCosineRegFn, stated in float64 (dense: A, rows, S, W S; low rank: G, s, P, the columns, W alpha,
    H, H W, finish), against ref_ops.ortho_reg_loss and its autograd gradient - on a weight with a column whose q lies in
    (0, 1e-12) and one that is exactly zero when ``clamp``: the low-rank form must carry q / 1e-12 there."""
    rows, c = 4, 9
    w = _rand((rows, c), 21, 0.3)
    if clamp:
        w[:, 5] = 0.0
        W.clamp_column(w, 3)
    leaf = w.clone().requires_grad_(True)
    loss = ref_ops.ortho_reg_loss(leaf, W.SCALE, kind)
    loss.backward()
    loss = loss.detach()
    if kind == "ortho":
        A = w.t() @ w
        terms, dA, _ = W.ortho_identity_ref(A, W.SCALE)
        assert abs(float(terms.v.sum()) - float(loss)) <= 1e-12 * float(loss)
        assert torch.allclose(w @ (dA + dA.t()), leaf.grad, rtol=1e-11, atol=1e-18)
        return
    d, lr = W.composed_dense(w.float(), W.SCALE), W.composed_lowrank(w.float(), W.SCALE)
    leaf = w.float().double().requires_grad_(True)
    loss = ref_ops.ortho_reg_loss(leaf, W.SCALE, kind)
    loss.backward()
    gmax = float(leaf.grad.abs().max())
    for form in (d, lr):
        assert abs(float(form["loss"]) - float(loss.detach())) <= 1e-11 * float(loss.detach())
        assert torch.allclose(form["dW"], leaf.grad, rtol=1e-9, atol=1e-11 * gmax)
        assert bool((form["EdW"] > 0).all()) and float(form["Eloss"]) > 0
    # the autograd gradient in A that composed_dense propagates with is ortho_cosine_ref's dA
    A = leaf.detach().t() @ leaf.detach()
    assert torch.allclose(d["dA"], W.ortho_cosine_ref(A, W.SCALE)[1].v, rtol=1e-9, atol=1e-12 * float(d["dA"].abs().max()))
    if clamp:
        q = ((leaf.detach() @ leaf.detach().t() @ leaf.detach()) * leaf.detach()).sum(0)
        assert 0 < float(q[3]) < W.EPS and float(q[5]) == 0.0


def test_adam_reference_matches_a_written_out_tf_adam():
    n = 40
    p, g, m, v, ema = (_rand((n,), 30 + k).float() for k in range(5))
    v = v.square()
    v[::7] = 0.0
    g[::14] = 0.0
    a = W.ADAM
    for b1, decay, gs in ((0.5, 0.999, 0.25), (0.0, 0.0, 1.0)):
        r = W.adam_ref(p, g, m, v, ema, a["lr"], W.f32r(b1), a["b2"], a["eps"], W.f32r(decay), W.f32r(gs))
        for k in range(n):
            gi = float(g[k]) * gs
            mk = b1 * float(m[k]) + (1 - b1) * gi
            vk = a["b2"] * float(v[k]) + (1 - a["b2"]) * gi * gi
            pk = float(p[k]) - a["lr"] * mk / (math.sqrt(vk) + a["eps"])
            ek = W.f32r(decay) * float(ema[k]) + (1 - W.f32r(decay)) * pk
            for name, want in (("m", mk), ("v", vk), ("p", pk), ("ema", ek)):
                assert abs(float(r[name][0][k]) - want) <= 1e-13 * max(1.0, abs(want)), (name, k)
        assert bool(torch.isfinite(r["p"][0]).all()) and bool(torch.isfinite(r["p"][1]).all())
        if b1 == 0.0:
            assert float(r["p"][0][0]) == float(p[0])                   # v = 0, g = 0, m = g: 0 / (0 + eps)
    assert "ema" not in W.adam_ref(p, g, m, v, None, a["lr"], 0.5, a["b2"], a["eps"], 0.999, 1.0)


def test_mask_and_pack_semantics_match_direct_loops():
    bits = [0, 5, 63, 64, 100, 128, 129]
    words = W._mask_words(bits, 130)
    assert len(words) == 3
    for j in range(130):
        assert ((words[j >> 6] >> (j & 63)) & 1) == (1 if j in bits else 0)
    assert W._mask_words([], 64) == [0] and len(W._mask_words([64], 65)) == 2
    taps, Rr, cols = 3, 4, 6
    wn = _rand((taps * Rr, cols), 41)
    pp, pt = W.pack_ref(wn, taps)
    for tp in range(taps):
        for r in range(Rr):
            for cc in range(cols):
                assert pp[tp, r, cc] == wn[tp * Rr + r, cc] and pt[tp, cc, r] == wn[tp * Rr + r, cc]
    w = _rand((3, 5), 42)
    v = _rand((5,), 43)
    for r in range(3):
        assert abs(float((w @ v)[r]) - sum(float(w[r, k]) * float(v[k]) for k in range(5))) < 1e-14
    T, P, s, Wa, ab = _rand((3, 5), 44), _rand((3, 5), 45), _rand((3,), 46), _rand((3,), 47), _rand((10,), 48)
    ref, _ = W.lowrank_finish_ref(T, P, s, Wa, ab)
    for r in range(3):
        for k in range(5):
            want = 2 * T[r, k] + s[r] * ab[k] + Wa[r] + 2 * P[r, k] * ab[5 + k]
            assert abs(float(ref[r, k]) - float(want)) < 1e-14


# ------------------------------------------------------------------------------------------
# the simulated kernels and their mutations
# ------------------------------------------------------------------------------------------
MUTATIONS = {
    # name: ops it applies to
    "w_norm: last row left unwritten": ("sn_fwd", "sn_batch_fwd"),
    "dw: last column computed from the neighbour's u": ("sn_bwd", "sn_batch_bwd"),
    "n % 4 tail left unwritten": ("adam", "sn_fwd"),
    "u and v exchanged in the backward outer product": ("sn_bwd", "sn_batch_bwd"),
    "1 / sigma applied twice": ("sn_bwd", "sn_batch_bwd"),
    "1 / sigma not applied": ("sn_bwd", "sn_batch_bwd"),
    "accumulate bit ignored": ("sn_batch_bwd",),
    "enable bit ignored": ("sn_batch_bwd",),
    "item 64's mask bit read from word 0": ("sn_batch_bwd",),
    "rs_v of item j used for item j + 1": ("sn_batch_fwd",),
    "clamp branch of ortho_cosine keeps the projection term": ("ortho_cosine",),
    "dA not symmetrised on one 32 x 32 edge tile": ("symmetrize",),
    "isq computed from c instead of c - 1": ("ortho_cosine",),
    "kappa with c - 1 in place of c - 2": ("lowrank_cols",),
    "low-rank clamp: 0 / 1 factor instead of q / max(q, 1e-12)": ("lowrank_cols",),
    "finish misses the factor 2 on P diag(beta)": ("lowrank_finish",),
    "Adam: g instead of g gscale in v": ("adam",),
    "EMA computed from the old p": ("adam",),
    "sqrt(v + eps) in place of sqrt(v) + eps": ("adam",),
    "pack_t written with pack_p's leading dimension": ("sn_batch_fwd",),
    "gemv: last row computed from the neighbour": ("gemv_rows",),
    "ortho_identity: the diagonal's 1 dropped": ("ortho_identity",),
}
M = list(MUTATIONS)


def applies(mut, c):
    op = c["op"]
    if op not in MUTATIONS[mut]:
        return False
    if mut == M[2]:
        return (c["n"] % 4 != 0) if op == "adam" else (c["rows"] * c["cols"]) % 4 != 0
    if mut == M[6]:
        return bool(c["accumulate"])
    if mut == M[7]:
        return c["enable"] is not None and len(c["enable"]) < len(c["items"])
    if mut == M[8]:
        return len(c["items"]) > 64
    if mut == M[9]:
        return len(c["items"]) > 1
    if mut == M[10]:
        return c["data"] == "clamp" and c["dA"]
    if mut == M[12]:
        return c["c"] > 1
    if mut == M[14]:
        return c["data"] == "clamp"
    if mut == M[16]:
        return c["gscale"] != 1.0
    if mut == M[17]:
        return c["ema"]
    if mut == M[19]:
        return any(it["group"] is not None for it in c["items"])
    if mut == M[11]:
        return c["c"] > 1
    return True


def _rs(ss):
    return torch.clamp(ss, min=torch.tensor(1e-12, dtype=F32)).rsqrt()


def sim_sn_fwd(w, u0, mut=None, rs_v_other=None):
    """bg_spectral_norm_fwd in fp32, in the kernels' order.  -> dict(v, u, sigma, wn), and rs_v."""
    vraw = w @ u0
    ss = (vraw.double() * vraw.double()).sum().float()
    rs_v = _rs(ss)
    use = rs_v_other if rs_v_other is not None else rs_v
    uraw = (vraw.double() @ w.double()).float()
    t = uraw * use
    ssu = (t * t).sum()
    rs_u = _rs(ssu)
    sigma = ssu * rs_u
    wn = w / sigma
    if mut == M[0]:
        wn = wn.clone()
        wn[-1] = NAN
    if mut == M[2] and wn.numel() % 4:
        wn = wn.clone()
        wn.view(-1)[wn.numel() // 4 * 4:] = NAN
    return dict(v=vraw * use, u=t * rs_u, sigma=sigma.reshape(1), wn=wn), rs_v


def sim_sn_bwd(i, acc, mut=None):
    g, wn, u, v, sigma = i["g"], i["wn"], i["u"], i["v"], i["sigma"]
    rows, cols = g.shape
    d = (g * wn).sum()
    inv = 1.0 / sigma.reshape(())
    uu, vv = u, v
    if mut == M[3]:                                   # v indexed by the column, u by the row (wrapped into range)
        vv = u[torch.arange(rows) % cols]
        uu = v[torch.arange(cols) % rows]
    outer_u = uu.clone()
    if mut == M[1] and cols > 1:
        outer_u[-1] = uu[-2]
    o = (g - d * vv[:, None] * outer_u[None, :])
    if mut == M[4]:
        o = o * inv * inv
    elif mut != M[5]:
        o = o * inv
    return o + i["dw0"] if acc else o


def sim(c, i, mut=None):
    """The outputs of 'kernels' that evaluate the documented formulas in fp32; ``mut`` names the bug they have."""
    op = c["op"]
    if op == "sn_fwd":
        return sim_sn_fwd(i["w"], i["u0"], mut)[0]
    if op == "sn_bwd":
        return {"dw": sim_sn_bwd(i, False, mut)}
    if op in ("sn_batch_fwd", "sn_batch_phase"):
        out, groups, prev = {}, {}, None
        for j, (it, ij) in enumerate(zip(c["items"], i["items"])):
            o, rs_v = sim_sn_fwd(ij["w"], ij["u0"], mut if mut == M[0] else None, prev if mut == M[9] else None)
            prev = rs_v
            if it["taps"]:
                taps, Rr, cols = it["taps"], it["rows"] // it["taps"], it["cols"]
                wn = torch.nan_to_num(o["wn"], nan=0.0) if mut == M[0] else o["wn"]
                pp, pt = W.pack_ref(wn.to(torch.bfloat16), taps)
                if it["group"] is None:
                    o["pp"], o["pt"] = pp, pt.contiguous()
                else:
                    gid, co, ct = it["group"]
                    if gid not in groups:
                        groups[gid] = (torch.full((1, Rr, ct), NAN, dtype=torch.bfloat16),
                                       torch.full((ct * Rr,), NAN, dtype=torch.bfloat16))
                    gp, gt = groups[gid]
                    gp[:, :, co:co + cols] = pp
                    ld = ct if mut == M[19] else Rr
                    idx = (co * Rr + torch.arange(cols)[:, None] * ld + torch.arange(Rr)[None, :]).reshape(-1)
                    keep = idx < gt.numel()
                    gt[idx[keep]] = pt[0].reshape(-1)[keep]
                    o["pp"] = gp[:, :, co:co + cols]
                    o["pt"] = gt.view(1, ct, Rr)[:, co:co + cols, :]
            for k, v in o.items():
                out["%d.%s" % (j, k)] = v
        return out
    if op == "sn_batch_bwd":
        n = len(c["items"])
        en = set(range(n)) if c["enable"] is None else set(c["enable"])
        acc = set(c["accumulate"] or [])
        if mut == M[8] and n > 64:
            en = (en - {64}) | ({64} if 0 in en else set())
            acc = (acc - {64}) | ({64} if 0 in acc else set())
        out = {}
        for j, ij in enumerate(i["items"]):
            if j not in en and mut != M[7]:
                out["%d.dw" % j] = ij["dw0"]
                continue
            out["%d.dw" % j] = sim_sn_bwd(ij, j in acc and mut != M[6], mut)
        return out
    if op == "symmetrize":
        A = i["A"]
        S = A + A.t()
        if mut == M[11]:
            k = (A.shape[0] - 1) // 32 * 32
            S = S.clone()
            S[k:, :32] = A[k:, :32]
        return {"S": S}
    if op == "ortho_cosine":
        A, cc = i["A"], c["c"]
        scale = torch.tensor(W.SCALE, dtype=F32)
        ss, sa = (A * A).sum(1, keepdim=True), A.sum(1, keepdim=True)
        clamped = ss < 1e-12
        rn = _rs(ss)
        r = sa * rn
        isq = torch.tensor(0.0 if cc == 1 else 1.0 / math.sqrt(cc if mut == M[12] else cc - 1), dtype=F32)
        ah = A * rn
        Rm = (r - ah) * isq
        s2, s1, sra = (Rm * Rm).sum(1, keepdim=True), Rm.sum(1, keepdim=True), (Rm * ah).sum(1, keepdim=True)
        loss = i["loss0"] + (0.5 * scale * s2).sum()
        T = scale * isq * (s1 * r - sra)
        dah = scale * isq * (s1 - Rm)
        full = rn * (dah - ah * T)
        dA = full if mut == M[10] else torch.where(clamped, rn * dah, full)
        return {"loss": loss.reshape(1), "dA": dA} if c["dA"] else {"loss": loss.reshape(1)}
    if op == "ortho_identity":
        A = i["A"]
        scale = torch.tensor(W.SCALE, dtype=F32)
        r = A if mut == M[21] else A - torch.eye(c["c"], dtype=F32)
        out = {"loss": (i["loss0"] + 0.5 * scale * (r * r).sum()).reshape(1)}
        if c["dA"]:
            out["dA"] = scale * r
        return out
    if op == "gemv_rows":
        o = i["w"].sum(1) if i["v"] is None else i["w"] @ i["v"]
        if mut == M[20]:
            o = o.clone()
            o[-1] = o[-2]
        return {"out": o}
    if op == "lowrank_cols":
        Wt, P, s, cc = i["W"], i["P"], i["s"], c["c"]
        scale = torch.tensor(W.SCALE, dtype=F32)
        q, t = (Wt * P).sum(0), (Wt * s[:, None]).sum(0)
        f = lambda x: torch.tensor(float(x), dtype=F32)                # noqa: E731
        kappa = scale * f(cc - 1 if mut == M[13] else cc - 2) / (f(2.0) * f(cc - 1)) if cc > 1 else f(0.0)
        k2 = scale / (f(2.0) * f(cc - 1)) if cc > 1 else f(0.0)
        clamped = q < 1e-12
        qc = torch.clamp(q, min=f(1e-12))
        a = 2.0 * kappa * t / qc
        b = -kappa * t * t / (qc * qc)
        if mut == M[14]:
            b = torch.where(clamped, torch.zeros_like(b), b)
            contrib = kappa * t * t / qc + k2 * torch.where(clamped, torch.zeros_like(q), torch.ones_like(q))
        else:
            b = torch.where(clamped, k2 / f(1e-12), b)
            contrib = kappa * t * t / qc + k2 * torch.where(clamped, q / qc, torch.ones_like(q))
        return {"loss": (i["loss0"] + contrib.sum()).reshape(1), "ab": torch.cat([a, b]), "Wb": Wt * b[None, :]}
    if op == "lowrank_finish":
        cc = c["c"]
        ab = i["ab"]
        k = 1.0 if mut == M[15] else 2.0
        return {"dW": 2.0 * i["T"] + i["s"][:, None] * ab[None, :cc] + i["Wa"][:, None] + k * i["P"] * ab[None, cc:]}
    if op == "adam":
        a = W.ADAM
        f = lambda x: torch.tensor(float(x), dtype=F32)                # noqa: E731
        b1, b2, eps, dec, gs, lr = f(c["b1"]), f(a["b2"]), f(a["eps"]), f(c["decay"]), f(c["gscale"]), f(a["lr"])
        gi = i["g"] * gs
        mn = gi if c["b1"] == 0.0 else b1 * i["m"] + (1 - b1) * gi
        gv = i["g"] if mut == M[16] else gi
        vn = b2 * i["v"] + (1 - b2) * gv * gv
        den = (vn + eps).sqrt() if mut == M[18] else vn.sqrt() + eps
        pn = i["p"] - lr * mn / den
        out = dict(m=mn, v=vn, p=pn)
        if c["ema"]:
            out["ema"] = dec * i["ema"] + (1 - dec) * (i["p"] if mut == M[17] else pn)
        if mut == M[2]:
            n4 = c["n"] // 4 * 4
            for k in out:
                out[k] = torch.cat([out[k][:n4], i[k][n4:]])
        return out
    raise KeyError(op)


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
    gen = torch.Generator().manual_seed(1234)
    i = W.make_inputs(c, "cpu", gen)
    rec = Rec()
    left_out, nout = W.check(c, i, sim(c, i, mut), rec)
    return rec, left_out, nout


@pytest.mark.parametrize("op", W.OPS)
def test_gate_accepts_a_correct_kernel_and_leaves_nothing_out(op):
    """Every case of the table: the simulated correct kernel passes, and the reference alone leaves no element out of the
    gate (no sum of squares within its own error of the 1e-12 clamp): well inside the 1e-4 cap."""
    worst, n = 0.0, 0
    for c in W.cases(op):
        rec, left_out, nout = _run(c)
        assert rec.ok, (W.describe(c), rec.worst, rec.nbad)
        assert left_out <= W.AMBIGUITY_CAP * nout and left_out == 0, (W.describe(c), left_out, nout)
        worst, n = max(worst, rec.worst), n + 1
    assert n > 0
    print("%-16s %3d cases accepted (worst err/bound %.3f)" % (op, n, worst))


@pytest.mark.parametrize("mut", M)
def test_gate_rejects(mut):
    """Each simulated bug is rejected on at least one case of the table."""
    tried = 0
    for c in (c for c in W.CASES if applies(mut, c)):
        tried += 1
        rec, _, _ = _run(c, mut)
        if not rec.ok:
            print("mutation %-60s rejected on %s: %d outputs outside the bound (case %d it applies to)"
                  % (mut, W.describe(c), rec.nbad, tried))
            return
    raise AssertionError("no case of the table rejects: %s (%d cases tried)" % (mut, tried))


def test_every_mutation_is_rejected_where_it_matters_most():
    """The cases built for a bug reject it."""
    by_name = {W.describe(c): c for c in W.CASES}
    for mut, name in ((M[8], "sn_batch_bwd[130 small]"), (M[6], "sn_batch_bwd[130 small]"), (M[7], "sn_batch_bwd[9 mixed]"),
                      (M[9], "sn_batch_fwd[9 mixed]"), (M[19], "sn_batch_fwd[9 mixed]"), (M[10], "ortho_cosine[c33 clamp]"),
                      (M[14], "lowrank_cols[7x18 clamp]"), (M[14], "lowrank_cols[17x257 clamp]"),
                      (M[11], "symmetrize[c33]"), (M[11], "symmetrize[c520]"), (M[18], "adam[n1024 b1=0 no ema g1]"),
                      (M[2], "adam[n10007 b1=0 #10]"), (M[3], "sn_bwd[64x256]"), (M[13], "lowrank_cols[8x1030]")):
        c = by_name[name]
        assert applies(mut, c), (mut, name)
        rec, _, _ = _run(c, mut)
        assert not rec.ok, (mut, name)


def test_table_covers_what_the_issue_lists():
    cs = W.CASES
    sn = {(c["rows"], c["cols"]) for c in cs if c["op"] == "sn_fwd"}
    assert {(7, 33), (16, 1), (216, 3), (5, 8), (64, 256), (9, 260), (12, 512), (20, 516), (6, 1028), (20, 2052)} <= sn
    assert {1, 2, 3, 5, 63, 64, 65, 130} <= {r for r, _ in sn} and {255, 256, 257} <= {k for _, k in sn}
    n = sorted(r * k for r, k in sn)
    assert any(8192 < v <= 16384 for v in n) and any(65536 < v <= 131072 for v in n) and any(v > 262144 for v in n)
    assert any(c["data"] == "tiny" for c in cs if c["op"] == "sn_fwd")
    tables = [c["items"] for c in cs if c["op"] == "sn_batch_fwd"]
    assert {1, 9, 130} == {len(t) for t in tables}
    mixed = next(t for t in tables if len(t) == 9)
    assert {1, 9, 16} <= {it["taps"] for it in mixed} and any(it["taps"] == 0 for it in mixed)
    assert {(24, 6), (72, 136)} <= {(it["rows"] // it["taps"], it["cols"]) for it in mixed if it["taps"]}
    grp = [it for it in mixed if it["group"] is not None]
    assert len(grp) == 3 and sum(it["cols"] for it in grp) == grp[0]["group"][2]
    assert any(it["rows"] * it["cols"] > 262144 for it in mixed) and any(it["data"] == "tiny" for it in mixed)
    big = next(c for c in cs if c["op"] == "sn_batch_bwd" and len(c["items"]) == 130)
    assert {63, 64, 128} <= set(big["enable"]) and {63, 64, 128} <= set(big["accumulate"])
    assert 0 not in big["enable"] and 0 not in big["accumulate"]                  # bit 64 differs from bit 0
    assert {w != 0 for w in W.mask_words(big, "accumulate")} == {True} and len(W.mask_words(big, "enable")) == 3
    assert any(c["enable"] is None for c in cs if c["op"] == "sn_batch_bwd")
    for op in ("symmetrize", "ortho_cosine", "ortho_identity"):
        assert set(W.REG_C) <= {c["c"] for c in cs if c["op"] == op}
    assert set(W.REG_C) == {1, 2, 3, 31, 32, 33, 255, 256, 257, 520}
    for op in ("ortho_cosine", "ortho_identity", "lowrank_cols"):
        assert any(c["loss0"] != 0.0 for c in cs if c["op"] == op)
        assert all(c["exempt"] == W.LOSS_EXEMPT for c in cs if c["op"] == op)
    assert all(c["exempt"] == () for c in cs if c["op"] not in ("ortho_cosine", "ortho_identity", "lowrank_cols"))
    for op in ("ortho_cosine", "ortho_identity"):
        assert {True, False} == {c["dA"] for c in cs if c["op"] == op}
    lr = {(c["rows"], c["c"]) for c in cs if c["op"] == "lowrank_cols"}
    assert {1, 7, 8, 9, 17} == {r for r, _ in lr} and {2, 18, 257, 1030} == {k for _, k in lr}
    assert all(2 * r <= k for r, k in lr) and 2 * W.COMPOSED[0] == W.COMPOSED[1]
    assert any(c["data"] == "clamp" for c in cs if c["op"] == "lowrank_cols")
    gv = [c for c in cs if c["op"] == "gemv_rows"]
    assert set(W.SN_COLS) <= {c["cols"] for c in gv if c["v"]} and set(W.SN_COLS) <= {c["cols"] for c in gv if not c["v"]}
    ad = [c for c in cs if c["op"] == "adam"]
    assert {1, 3, 4, 1023, 1024, 10007} == {c["n"] for c in ad}
    assert any(c["align"] == 4 and c["n"] % 4 == 0 for c in ad) and {0.0, 0.5} == {c["b1"] for c in ad}
    assert {True, False} == {c["ema"] for c in ad} and {1.0, 0.25} == {c["gscale"] for c in ad}
    assert {0.0, 0.999} == {c["decay"] for c in ad}
    assert len({W.describe(c) for c in cs}) == len(cs)
