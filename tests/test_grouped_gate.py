"""CPU checks of tests/grouped_ref.py, the gate of the multi-branch convolution, grouped dense and latent routing
kernels: the float64 references against autograd, the simulated correct kernels inside every bound, the mutations a
subtly wrong kernel would show rejected, the gap of the whole-tensor criterion written down, and the case tables."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import grouped_ref as G
from tests.launch_replay import GateStats

D64 = torch.float64
MIX_NAMES = [c["name"] for c in G.MIX_CASES]


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _rel_err(a, b):
    """tests/common.rel_err: the relative L2 norm of a whole tensor."""
    a, b = a.double().numpy().ravel(), b.double().numpy().ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


_CACHE = {}


def _mix(name):
    """(case, inputs, expectations), computed once per case and left unchanged."""
    if name not in _CACHE:
        c = G.gap_case() if name == "GAP" else G.MIX[name]
        inp = G.mix_inputs(c)
        _CACHE[name] = (c, inp, G.mix_expect(c, inp))
    return _CACHE[name]


def _rejected(c, exp, outs):
    return bool(G.mix_check(c, exp, outs))


# ------------------------------------------------------------------------------------------
# references against autograd
# ------------------------------------------------------------------------------------------
def _autograd_branch(x, w, b):
    """F.pad + F.conv2d(dilation=): the transposed branch as the correlation with the flipped kernel."""
    hi = (b["k"] - 1) * b["dil"] - b["lo"]
    xin = F.pad(x.permute(0, 3, 1, 2), (b["lo"], hi, b["lo"], hi), mode="reflect" if b["mode"] == G.REFLECT else "constant")
    wt = (w.permute(2, 3, 0, 1).flip(2, 3) if b["tr"] else w.permute(3, 2, 0, 1)).contiguous()
    return F.conv2d(xin, wt, dilation=b["dil"]).permute(0, 2, 3, 1)


@pytest.mark.parametrize("name", MIX_NAMES)
def test_mixconv_references_against_autograd(name):
    c, inp, _ = _mix(name)
    x = inp["x"].double().requires_grad_(True)
    ws = [w.double().requires_grad_(True) for w in inp["w"]]
    lo, hi = G.mix_cols(c)
    dy = inp["dy"].double()
    y = torch.cat([_autograd_branch(x, w, b) for w, b in zip(ws, c["table"])], -1)
    grads = torch.autograd.grad(y, [x] + ws, dy[..., lo:hi])
    dx = 0.0
    for j, (b, w) in enumerate(zip(c["table"], ws)):
        sl = slice(b["c_off"], b["c_off"] + b["cb"])
        assert _close(G.fwd_branch(x.detach(), w.detach(), b), y[..., sl.start - lo:sl.stop - lo].detach()), (name, j)
        assert _close(G.wgrad_branch(x.detach(), dy[..., sl], b), grads[1 + j]), (name, j)
        # summed slab by slab the weight gradient is the same sum
        parts = sum(G.wgrad_branch(x.detach(), dy[..., sl], b, p0, p1) for p0, p1 in G.slab_ranges(c))
        assert _close(parts, grads[1 + j]), (name, j)
        dx = dx + G.dgrad_branch(dy[..., sl], w.detach(), b)
    assert _close(dx, grads[0]), name
    # the adjoint identity <fwd(x), dy> = <x, dgrad(dy)>
    lhs = float((y.detach() * dy[..., lo:hi]).sum())
    rhs = float((x.detach() * dx).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0), (lhs, rhs)


@pytest.mark.parametrize("name", [c["name"] for c in G.DENSE_CASES])
def test_dense_references_against_autograd(name):
    c = G.DENSE[name]
    for i in G.dense_inputs(c):
        x, w = i["x"].double().requires_grad_(True), i["w"].double().requires_grad_(True)
        b = torch.zeros(w.shape[1], dtype=D64, requires_grad=True)
        y = x @ w + b
        gx, gw, gb = torch.autograd.grad(y, [x, w, b], i["dy"].double())
        assert _close(G.dense_fwd(x.detach(), w.detach()), y.detach())
        dw, db = G.dense_wgrad(x.detach(), i["dy"].double())
        assert _close(dw, gw) and _close(db, gb)
        assert _close(G.dense_dgrad([i["dy"].double()], [w.detach()]), gx)
        lhs, rhs = float((y.detach() * i["dy"].double()).sum()), float((x.detach() * gx).sum())
        assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0)


@pytest.mark.parametrize("name", [c["name"] for c in G.DENSE_DGRAD_CASES])
def test_dense_group_input_gradient_against_autograd(name):
    c = G.DENSE[name]
    inp = G.dense_dgrad_inputs(c)
    x = torch.zeros((c["B"], c["K"]), dtype=D64, requires_grad=True)
    ys = [x @ w.double() for w in inp["ws"]]
    gx, = torch.autograd.grad(ys, [x], [d.double() for d in inp["dys"]])
    assert _close(G.dense_dgrad([d.double() for d in inp["dys"]], [w.double() for w in inp["ws"]]), gx)


def test_latent_routing_against_direct_loops_and_autograd():
    for c in G.LATENT_CASES:
        inp = G.latent_inputs(c)
        got = G.latent_route(c["targets"], c["segs"], inp["srcs"], inp["priors"], c["B"])
        for t, tg in enumerate(c["targets"]):
            want = torch.zeros((c["B"], tg["width"]), dtype=D64)
            for b in range(c["B"]):
                for col in range(tg["width"]):
                    s = 0.0
                    for sg in c["segs"]:
                        if sg["target"] == t and sg["dst_col"] <= col < sg["dst_col"] + sg["width"]:
                            s += float(inp["srcs"][sg["src"]][b, sg["src_col"] + col - sg["dst_col"]])
                    want[b, col] = s + (float(inp["priors"][t][b, col]) if tg["accumulate"] else 0.0)
            assert _close(got[t], want), (c["name"], t)
    # fan-out is a concatenation; the fan-in of its transposed segments is its autograd gradient
    c = G.LATENT["L1"]
    inp = G.latent_inputs(c)
    z, e, s = [t.double().requires_grad_(True) for t in inp["srcs"]]
    packed = torch.cat([z[:, :10], e, s, z[:, 10:40], e, s, e], 1)
    out = G.latent_route(c["targets"], c["segs"], inp["srcs"], inp["priors"], c["B"])[0]
    assert torch.equal(out, packed.detach())
    g = torch.randn(packed.shape, dtype=D64, generator=torch.Generator().manual_seed(1))
    grads = torch.autograd.grad(packed, [z, e, s], g)
    back = [dict(src=0, src_col=sg["dst_col"], target=sg["src"], dst_col=sg["src_col"], width=sg["width"])
            for sg in c["segs"]]
    tg = [dict(width=w, ldd=w, accumulate=0) for w in c["src_widths"]]
    for a, b in zip(G.latent_route(tg, back, [g], None, c["B"]), grads):
        assert _close(a, b)


# ------------------------------------------------------------------------------------------
# simulated kernels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MIX_NAMES)
def test_simulated_mixconv_kernels_pass_the_gate(name):
    """fp32 accumulation and the bf16 store, the weight gradient in one sum and slab by slab: inside every bound."""
    c, inp, exp = _mix(name)
    stats = GateStats()
    assert G.mix_check(c, exp, G.mix_sim(c, inp), stats) == []
    assert G.mix_check(c, exp, G.mix_sim(c, inp, slabwise=True), stats) == []
    # (a correct kernel uses a small share of the fp32 bounds - at most 0.053, M3's weight gradient - and a bf16 store
    # lies at most at the edge of its interval)
    assert all(row[1] <= 1.0 for row in stats.rows.values())
    foreign = torch.ones(c["ldy"], dtype=torch.bool)
    for b in c["table"]:
        foreign[b["c_off"]:b["c_off"] + b["cb"]] = False
    assert bool(G.mix_sim(c, inp)["y"][..., foreign].isnan().all())


def test_simulated_dense_and_latent_kernels_pass_the_gate():
    for c in G.DENSE_CASES:
        inp = G.dense_inputs(c)
        assert G.flat_check(c, G.dense_expect(c, inp), G.dense_sim(c, inp)) == []
    for c in G.DENSE_DGRAD_CASES:
        inp = G.dense_dgrad_inputs(c)
        assert G.flat_check(c, G.dense_dgrad_expect(c, inp), G.dense_dgrad_sim(c, inp)) == []
    for c in G.LATENT_CASES:
        inp = G.latent_inputs(c)
        assert G.flat_check(c, G.latent_expect(c, inp), G.latent_sim(c, inp)) == []


# ------------------------------------------------------------------------------------------
# mutations
# ------------------------------------------------------------------------------------------
def _median_product(a, b):
    """The product of median magnitude among the non-zero products a * b of one reduction (fp32, exact)."""
    p = (a.float() * b.float()).flatten()
    p = p[p != 0]
    return p[p.abs().argsort()[p.numel() // 2]]


def _drop(outs, key, index, prod):
    outs = dict(outs)
    t = outs[key].clone()
    t[index] = (t[index].float() - prod).to(t.dtype)
    outs[key] = t
    return outs


def test_a_single_dropped_product_is_rejected_in_every_pass():
    """The condition on the tightness of the bounds: the longest reduction of each pass with one product of median
    magnitude missing falls outside its bound (fp32 outputs; the bf16 store is tested with the other mutations)."""
    # forward: D2, fp32 y, the 5 x 5 branch (K = 800), an interior pixel
    c, inp, exp = _mix("D2")
    b, w = c["table"][1], inp["w"][1]
    outs = G.mix_sim(c, inp)
    prod = _median_product(inp["x"][0, 1:6, 1:6, :], w[:, :, :, 0])
    assert _rejected(c, exp, _drop(outs, "y", (0, 3, 3, b["c_off"]), prod)), "forward D2"
    # input gradient: D3, fp32 dx (accumulating), pixel (3, 3): the outputs (3 + 2 - i, 3 + 2 - j) of the 5 x 5 branch
    c, inp, exp = _mix("D3")
    b, w = c["table"][1], inp["w"][1]
    outs = G.mix_sim(c, inp)
    dyw = inp["dy"][0, 1:6, 1:6, b["c_off"]:b["c_off"] + b["cb"]].flip(0, 1)
    prod = _median_product(dyw, w[:, :, 0, :])
    assert _rejected(c, exp, _drop(outs, "dx", (0, 3, 3, 0), prod)), "input gradient D3"
    # weight gradient: M5, the centre tap of conv5 (every one of the 1280 pixels contributes, none padded), 5 slabs
    c, inp, exp = _mix("M5")
    b = c["table"][3]
    assert b["k"] == 5 and b["dw"] and G.mix_slabs(c) == 5
    outs = G.mix_sim(c, inp, slabwise=True)
    prod = _median_product(inp["x"][..., 0], inp["dy"][..., b["c_off"]])
    assert _rejected(c, exp, _drop(outs, "dw3", (2, 2, 0, 0), prod)), "weight gradient M5"
    # dense group: G8 item 0 (K = 37, B = 130), DG3 (sum of N = 429)
    c = G.DENSE["G8"]
    inp = G.dense_inputs(c)
    exp, outs = G.dense_expect(c, inp), G.dense_sim(c, inp)
    i0 = inp[0]
    assert G.flat_check(c, exp, _drop(outs, "y0", (0, 0), _median_product(i0["x"][0], i0["w"][:, 0]))), "dense forward G8"
    assert G.flat_check(c, exp, _drop(outs, "dw0", (0, 0), _median_product(i0["x"][:, 0], i0["dy"][:, 0]))), "dense dw G8"
    assert G.flat_check(c, exp, _drop(outs, "db0", (0,), _median_product(i0["dy"][:, 0], torch.ones(130)))), "dense db G8"
    c = G.DENSE["DG3"]
    inp = G.dense_dgrad_inputs(c)
    outs = G.dense_dgrad_sim(c, inp)
    prod = _median_product(inp["dys"][0][0], inp["ws"][0][0])
    assert G.flat_check(c, G.dense_dgrad_expect(c, inp), _drop(outs, "dx", (0, 0), prod)), "dense input gradient DG3"
    # latent fan-in: L4, one of the covering segments of a column missing
    c = G.LATENT["L4"]
    inp = G.latent_inputs(c)
    outs = G.latent_sim(c, inp)
    sg = c["segs"][0]
    prod = inp["srcs"][sg["src"]][0, sg["src_col"]]
    assert G.flat_check(c, G.latent_expect(c, inp), _drop(outs, "t0", (0, sg["dst_col"]), prod)), "fan-in L4"


MUTATIONS = [
    ("the reflect fold dropped at the mirrored pixel (1, 1) of conv3", "M1", ("nofold", 3, 1, 1)),
    ("the reflect fold dropped at (1, 1) of the dilated branch at lo = H - 1", "M4", ("nofold", 0, 1, 1)),
    ("edge replication in place of reflection in conv3", "M1", ("edge", 3)),
    ("edge replication in place of reflection, fp32 output", "D2", ("edge", 0)),
    ("the transposed branch left unflipped", "M3", ("noflip", 1)),
    ("one branch written one channel to the right", "M3", ("shift", 1)),
    ("the last partial tile left unwritten", "M1", ("tile",)),
    ("accumulate ignored (MFMA form)", "M2", ("no_acc",)),
    ("accumulate ignored (direct form, fp32 dx)", "D3", ("no_acc",)),
    ("acc_w ignored", "M1", ("no_acc_w",)),
    ("operands unrounded under BG_COMPUTE_BF16", "D4b", ("unrounded",)),
    ("the last pixel before the slab boundary 292 dropped", "M1", ("slab_drop",)),
    ("the last pixel before a slab boundary dropped, 5 aligned slabs", "M5", ("slab_drop",)),
]


@pytest.mark.parametrize("what,name,mut", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mixconv_mutation_is_rejected(what, name, mut):
    c, inp, exp = _mix(name)
    assert _rejected(c, exp, G.mix_sim(c, inp, mut)), "%s passed the gate on %s" % (what, name)


def test_dense_and_latent_mutations_are_rejected():
    c = G.DENSE["G4"]
    inp = G.dense_inputs(c)
    exp = G.dense_expect(c, inp)
    assert G.flat_check(c, exp, G.dense_sim(c, inp, ("db_rows",))), "a bias gradient over B - 1 rows passed on G4"
    assert G.flat_check(c, exp, G.dense_sim(c, inp, ("no_acc_w",))), "acc_w ignored passed on G4"
    c = G.DENSE["DG2"]
    inp = G.dense_dgrad_inputs(c)
    assert G.flat_check(c, G.dense_dgrad_expect(c, inp), G.dense_dgrad_sim(c, inp, ("no_acc",))), "accumulate ignored: DG2"
    c = G.LATENT["L3"]
    inp = G.latent_inputs(c)
    bad = G.latent_sim(c, inp, ("wrong_target", 2, 0))
    assert G.flat_check(c, G.latent_expect(c, inp), bad), "fan-in segment 2 summed onto target 0 passed on L3"


# ------------------------------------------------------------------------------------------
# the gap of the whole-tensor criterion
# ------------------------------------------------------------------------------------------
def test_whole_tensor_criterion_accepts_what_the_gate_rejects():
    """At N 2, 32 x 32, Cin 96, inner 48 - the largest map of test_bf16_mfma_path_against_float64 - a reflect fold
    dropped at one mirrored pixel of one branch, and a single output element short of one product, both stay below
    rel_err < 1e-2 of the whole tensor and both fail the gate.  The figures: the simulated correct kernel 1.66e-3 (its
    bf16 store), the dropped fold at (1, 1) of conv3 in image 0 5.5e-3, the missing product 1.72e-3."""
    c, inp, exp = _mix("GAP")
    good = G.mix_sim(c, inp)
    assert G.mix_check(c, exp, good) == []
    dx_ref = [e for e in exp if e[2] == "dx"][0][4]
    y_ref = torch.cat([e[4] for e in exp if e[2] == "y"], -1)
    base = _rel_err(good["dx"], dx_ref)
    assert base < 3e-3, base
    folded = G.mix_sim(c, inp, ("nofold", 3, 1, 1))
    assert base <= _rel_err(folded["dx"], dx_ref) < 1e-2
    assert _rejected(c, exp, folded)
    b = c["table"][4]
    prod = (inp["x"][0, 14:19, 14:19, :].float() * inp["w"][4][:, :, :, 0]).abs().max()
    short = _drop(good, "y", (0, 16, 16, b["c_off"]), prod)
    assert _rel_err(short["y"], y_ref) < 1e-2
    assert _rejected(c, exp, short)


# ------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------
def test_case_tables():
    again = G._mix_cases()
    assert again == G.MIX_CASES and G._latent_cases() == G.LATENT_CASES
    for c in G.MIX_CASES:
        a, b = G.mix_inputs(c), G.mix_inputs(copy.deepcopy(c))
        assert torch.equal(a["x"], b["x"]) and all(torch.equal(u, v) for u, v in zip(a["w"], b["w"]))
        assert G.mix_prepare_ok(c), c["name"]
        assert G.mfma_shape(c) == (c["name"][0] == "M" or c["name"] == "D5"), c["name"]
        assert G.mfma_ok(c) == (c["name"][0] == "M"), c["name"]
        assert sum(1 for br in c["table"] if not br["dw"]) == 1
        assert c["accumulate"] == c["idx"] % 2
        if not c["unrounded"]:          # bf16-representable operands: every product is exact in fp32
            for t in [a["x"], a["dy"][..., slice(*G.mix_cols(c))]] + a["w"]:
                assert torch.equal(t.float(), t.to(torch.bfloat16).float())
        else:
            assert not torch.equal(a["x"], a["x"].to(torch.bfloat16).float())
    M = G.MIX
    assert [b["cb"] for b in M["M1"]["table"]] == [2, 2, 1, 1, 1, 1] and M["M1"]["N"] * M["M1"]["H"] * M["M1"]["W"] == 585
    assert G.slab_ranges(M["M1"]) == [(0, 292), (292, 585)] and 292 % 8 != 0
    assert [b["cb"] for b in M["M2"]["table"]] == [34, 34, 17, 17, 17, 17] and M["M2"]["Cin"] % 64 != 0
    assert [(b["c_off"], b["cb"]) for b in M["M3"]["table"]] == [(3, 72), (75, 80)] and M["M3"]["ldy"] == 160
    assert M["M4"]["table"][0]["lo"] == M["M4"]["H"] - 1 == 4
    assert len(M["M5"]["table"]) == 5 and sum(b["cb"] for b in M["M5"]["table"]) == 16
    assert G.slab_ranges(M["M5"]) == [(256 * i, 256 * (i + 1)) for i in range(5)]
    assert G.mix_slabs(M["D5"]) == 2 and G.mix_slabs(M["D1"]) == 45
    assert max(c["N"] * c["H"] * c["W"] * c["Cin"] for c in G.MIX_CASES) == 1280 * 32
    # dense: the group sizes, batch sizes, K and N of the issue, a column slice, NULL bias / db, both acc values
    items = [it for c in G.DENSE_CASES for it in c["items"]]
    assert sorted(len(c["items"]) for c in G.DENSE_CASES) == [1, 4, G.DENSE_GROUP_MAX]
    assert {c["B"] for c in G.DENSE_CASES} == {3, 13, 130}
    assert {it["K"] for it in items} == {1, 20, 37} and {it["N"] for it in items} == {1, 17, 300}
    assert any(it["ldx"] > it["K"] for it in items) and any(not it["bias"] for it in items)
    assert any(not it["db"] for it in items)
    assert {it["acc_w"] for it in items} == {0, 1} and {it["acc_b"] for it in items if it["db"]} == {0, 1}
    dg = G.DENSE_DGRAD_CASES
    assert {c["K"] for c in dg} == {1, 37, 65} and {n for c in dg for n in c["Ns"]} == {1, 64, 65, 300}
    assert {c["acc"] for c in dg} == {0, 1}
    L4 = G.LATENT["L4"]
    assert len(L4["segs"]) == G.LATENT_MAX_SEGS and len(L4["targets"]) == G.LATENT_MAX_TARGETS
    for c in G.LATENT_CASES:                     # latent_prepare's preconditions
        for sg in c["segs"]:
            tg = c["targets"][sg["target"]]
            assert sg["width"] >= 1 and sg["dst_col"] + sg["width"] <= tg["width"] <= tg["ldd"]
            assert sg["src_col"] + sg["width"] <= c["src_widths"][sg["src"]]
    assert any(tg["ldd"] > tg["width"] for c in G.LATENT_CASES for tg in c["targets"])
