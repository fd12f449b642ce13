"""CPU checks of the launch-replay gate (tests/launch_replay.py): its float64 references against oracle/kat.py, float64
autograd and a direct softmax loop at small shapes, and a mutation self-test - a simulated correct kernel passes the
gate, and each simulated kernel bug is rejected."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import kat
from tests import launch_replay as R

D64 = torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=D64) * scale


# ------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.PAD_REFLECT, R.PAD_ZERO])
@pytest.mark.parametrize("H,k,s,lo,Ho", [(8, 3, 1, 1, 8), (8, 3, 2, 1, 4), (7, 3, 2, 1, 4), (6, 1, 1, 0, 6),
                                         (4, 3, 1, 1, 4)])
def test_conv_reference_matches_kat(mode, H, k, s, lo, Ho):
    x, w = _rand((2, H, H, 5), 1), _rand((k, k, 5, 4), 2)
    hi = (Ho - 1) * s + k - H - lo
    if mode == R.PAD_REFLECT:
        xp = kat.reflect_pad(x.numpy(), lo, hi)
    else:
        xp = np.pad(x.numpy(), ((0, 0), (lo, hi), (lo, hi), (0, 0)))
    want = kat.conv2d_valid(xp, w.numpy(), s)
    got = R.conv_fwd(x, w, s, lo, Ho, Ho, mode)
    assert got.shape == want.shape
    assert torch.allclose(got, _t(want), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("H,k,s", [(4, 4, 2), (5, 4, 2), (6, 3, 1), (4, 3, 1)])
def test_deconv_reference_matches_kat(H, k, s):
    x, w = _rand((2, H, H, 5), 3), _rand((k, k, 4, 5), 4)
    _, lo, _ = kat.same_padding(s * H, k, s)
    want = kat.conv2d_transpose_same(x.numpy(), w.numpy(), s)
    got = R.deconv_fwd(x, w, s, lo, s * H, s * H)
    assert torch.allclose(got, _t(want), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mode", [R.PAD_REFLECT, R.PAD_ZERO])
@pytest.mark.parametrize("H,k,s,lo,Ho", [(8, 3, 1, 1, 8), (8, 3, 2, 1, 4), (4, 3, 1, 1, 4), (6, 1, 1, 0, 6)])
def test_conv_gradients_match_autograd(mode, H, k, s, lo, Ho):
    """dgrad (the reflect fold included) and wgrad against float64 autograd of tf.pad + VALID conv in torch."""
    x = _rand((2, H, H, 6), 5).requires_grad_(True)
    w = _rand((k, k, 6, 3), 6).requires_grad_(True)
    hi = (Ho - 1) * s + k - H - lo
    xn = x.permute(0, 3, 1, 2)
    xp = F.pad(xn, (lo, hi, lo, hi), mode="reflect" if mode == R.PAD_REFLECT else "constant")
    y = F.conv2d(xp, w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
    g = _rand(tuple(y.shape), 7)
    y.backward(g)
    assert torch.allclose(R.conv_fwd(x.detach(), w.detach(), s, lo, Ho, Ho, mode), y.detach(), atol=1e-12)
    assert torch.allclose(R.conv_dgrad(g, w.detach(), s, lo, H, H, mode), x.grad, atol=1e-12)
    assert torch.allclose(R.conv_wgrad(x.detach(), g, k, s, lo, mode), w.grad, atol=1e-11)


@pytest.mark.parametrize("H,k,s", [(4, 4, 2), (5, 4, 2), (6, 3, 1)])
def test_deconv_gradients_match_autograd(H, k, s):
    x = _rand((2, H, H, 5), 8).requires_grad_(True)
    w = _rand((k, k, 3, 5), 9).requires_grad_(True)
    _, lo, _ = kat.same_padding(s * H, k, s)
    y = R.deconv_fwd(x, w, s, lo, s * H, s * H)
    g = _rand(tuple(y.shape), 10)
    y.backward(g)
    assert torch.allclose(R.deconv_dgrad(g, w.detach(), s, lo, H, H), x.grad, atol=1e-12)
    assert torch.allclose(R.deconv_wgrad(x.detach(), g, k, s, lo), w.grad, atol=1e-11)


def test_attention_reference_matches_direct_loop():
    B, N, Nk, d, dv = 2, 6, 5, 3, 4
    q, k, v = _rand((B, N, d), 11), _rand((B, Nk, d), 12), _rand((B, Nk, dv), 13)
    do = _rand((B, N, dv), 14)
    o, lse = R.attn_fwd(q, k, v)
    P = torch.exp(q @ k.transpose(1, 2) - lse[..., None])
    delta = (do * o).sum(2)
    dq, dk, dv_ = R.attn_bwd(q, k, v, do, P, delta)
    for b in range(B):
        for i in range(N):
            s = [sum(q[b, i, c].item() * k[b, j, c].item() for c in range(d)) for j in range(Nk)]
            m = max(s)
            e = [math.exp(t - m) for t in s]
            z = sum(e)
            p = [t / z for t in e]
            assert abs(lse[b, i].item() - (m + math.log(z))) < 1e-12
            for c in range(dv):
                assert abs(o[b, i, c].item() - sum(p[j] * v[b, j, c].item() for j in range(Nk))) < 1e-12
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    oo = torch.softmax(qq @ kk.transpose(1, 2), dim=2) @ vv
    oo.backward(do)
    for got, want in ((dq, qq.grad), (dk, kk.grad), (dv_, vv.grad)):
        assert torch.allclose(got, want, atol=1e-12)


# ------------------------------------------------------------------------------------------
# mutation self-test of the gate
# ------------------------------------------------------------------------------------------
def _bf16_exact(shape, seed, scale=1.0):
    return _rand(shape, seed, scale).to(torch.bfloat16).double()


def _rtz_bf16(x32):
    return (x32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _sim_conv(x, w, s, lo, Ho, mode, seed=0, rnd=lambda t: t.to(torch.bfloat16), sym=False):
    """A 'kernel': exact fp32 products summed in fp32 in a shuffled order, then rounded (RNE by default)."""
    k, C, O = w.shape[0], w.shape[2], w.shape[3]
    Hp = (Ho - 1) * s + k
    if sym:                                  # the bug: a reflect that repeats the border pixel (symmetric padding)
        idx = torch.tensor([min(max(u - lo if u - lo >= 0 else -(u - lo) - 1, 0), x.shape[1] - 1) for u in range(Hp)])
        xp = x.index_select(1, idx).index_select(2, idx)
    else:
        xp = R.pad2d(x, lo, Hp, Hp, mode)
    cols = F.unfold(xp.permute(0, 3, 1, 2), k, stride=s).transpose(1, 2)          # [n, L, C k k]
    wf = w.permute(2, 0, 1, 3).reshape(C * k * k, O)
    prod = (cols[..., None] * wf).float()                                          # exact in fp32
    perm = torch.randperm(prod.shape[2], generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(prod.shape[:2] + (O,), dtype=torch.float32)
    for j in perm.tolist():
        acc += prod[:, :, j]
    return rnd(acc).reshape(x.shape[0], Ho, Ho, O)


def _gate_conv(got, x, w, s, lo, Ho, mode):
    ref = R.conv_fwd(x, w, s, lo, Ho, Ho, mode)
    A = R.conv_fwd(x.abs(), w.abs(), s, lo, Ho, Ho, mode)
    return R.gate(got, ref, R.bound(A, w.shape[0] ** 2 * w.shape[2]))


def _case():
    x = _bf16_exact((3, 7, 7, 32), 21)
    w = _bf16_exact((3, 3, 32, 24), 22, 1 / math.sqrt(288))
    return x, w, 1, 1, 7, R.PAD_REFLECT          # M = 3 * 49 = 147 output rows: the last 16-row tile is ragged


def test_gate_accepts_a_correct_kernel():
    x, w, s, lo, Ho, mode = _case()
    for seed in range(3):
        ok, ratio, above, below, nbad = _gate_conv(_sim_conv(x, w, s, lo, Ho, mode, seed), x, w, s, lo, Ho, mode)
        assert ok and ratio <= 1.0, (ratio, nbad)
    print("correct kernel: accepted (worst err/bound %.3f, ambiguous above %d / below %d)" % (ratio, above, below))


def _rejected(name, got, x, w, s, lo, Ho, mode):
    ok, ratio, _, _, nbad = _gate_conv(got, x, w, s, lo, Ho, mode)
    assert not ok, name
    print("mutation %-34s rejected: %d outputs outside the bound" % (name, nbad))


def test_gate_rejects_round_toward_zero():
    x, w, s, lo, Ho, mode = _case()
    _rejected("round-toward-zero bf16 output", _sim_conv(x, w, s, lo, Ho, mode, rnd=_rtz_bf16), x, w, s, lo, Ho, mode)


def test_gate_rejects_one_scaled_tile():
    x, w, s, lo, Ho, mode = _case()
    y = _sim_conv(x, w, s, lo, Ho, mode).float().reshape(-1, 24)
    y[32:48, 0:16] *= 1 + 2 ** -6
    _rejected("one 16x16 tile scaled by 1+2^-6", y.to(torch.bfloat16).reshape(3, Ho, Ho, 24), x, w, s, lo, Ho, mode)


def test_gate_rejects_unwritten_ragged_tile():
    x, w, s, lo, Ho, mode = _case()
    y = _sim_conv(x, w, s, lo, Ho, mode).float().reshape(-1, 24)
    y[144:, :] = float("nan")                      # rows 144..146: the ragged last tile, left as prefilled
    _rejected("last ragged tile unwritten", y.to(torch.bfloat16).reshape(3, Ho, Ho, 24), x, w, s, lo, Ho, mode)


def test_gate_rejects_channel_swap():
    x, w, s, lo, Ho, mode = _case()
    y = _sim_conv(x, w, s, lo, Ho, mode)
    y = y[..., [1, 0] + list(range(2, 24))]
    _rejected("output channels 0 and 1 swapped", y, x, w, s, lo, Ho, mode)


def test_gate_rejects_reflect_repeating_the_border():
    x, w, s, lo, Ho, mode = _case()
    _rejected("reflect repeating the border", _sim_conv(x, w, s, lo, Ho, mode, sym=True), x, w, s, lo, Ho, mode)


def test_gate_rejects_a_dropped_wgrad_term():
    """fp32 weight gradient elements with K = 9 * 1536 terms (a 3x3 conv over 1536 pixels): one term missing."""
    K = 9 * 1536
    a, b = _bf16_exact((K, 8), 31), _bf16_exact((K, 8), 32)
    prod = (a[:, :, None] * b[:, None, :]).float()                 # [K, 8, 8], exact
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3))
    acc = prod[perm].sum(0)                                        # fp32 accumulation
    ref, A = a.t() @ b, a.abs().t() @ b.abs()
    E = R.bound(A, K)
    ok, ratio, _, _, _ = R.gate(acc, ref, E)
    assert ok, ratio
    j = int(prod[:, 2, 5].abs().argmax())
    bad = acc.clone()
    bad[2, 5] -= prod[j, 2, 5]
    ok, ratio, _, _, nbad = R.gate(bad, ref, E)
    assert not ok and nbad == 1
    print("mutation %-34s rejected: err/bound %.2f" % ("one term dropped (fp32, K=9*1536)", ratio))


def test_gate_rejects_a_write_past_the_output():
    b = R.Buf(100, torch.bfloat16, "cpu", align=2, shape=(10, 10))
    b.prefill()
    b.view.fill_(1.0)
    assert b.guards_ok()
    b.raw[b.off + b.nbytes] = 0                                    # one byte of the element past the end
    assert not b.guards_ok()
    s = R.Buf(40, torch.float32, "cpu", size=(2, 3, 4), stride=(20, 6, 1))     # column slices of [2, 3, 6] rows
    s.prefill()
    s.view.fill_(1.0)
    assert s.guards_ok()
    s.flat[4] = 2.0                                                # column 4 of row 0 lies outside the slice
    assert not s.guards_ok()
    print("mutation %-34s rejected: guard band changed" % "write one element past the output")


# ------------------------------------------------------------------------------------------
# the geometry sweep (tests/geometry_sweep.py): its references, its mutation checks, the generator itself
# ------------------------------------------------------------------------------------------
from tests import geometry_sweep as G                                              # noqa: E402

_REFLECT_GEOMS = G.conv_geometries(R.PAD_REFLECT)


def _geom_id(g):
    return "%dx%d-k%d-s%d-pad%d+%d" % (g.H, g.W, g.k, g.stride, g.pad_lo, g.pad_hi)


def test_sweep_has_the_geometries_where_the_kernels_were_wrong():
    have = {(g.H, g.W, g.k, g.stride, g.pad_lo, g.pad_hi) for g in _REFLECT_GEOMS}
    assert (3, 3, 3, 1, 1, 1) in have                               # a row that mirrors both borders
    assert (4, 4, 5, 1, 2, 2) in have
    assert (4, 4, 4, 1, 1, 2) in have and (8, 8, 4, 1, 1, 2) in have                # even k at stride 1: unequal pads
    assert (4, 4, 5, 2, 1, 2) in have and (4, 4, 5, 2, 2, 1) in have                # k = 5 at stride 2, both splits
    assert (3, 5, 3, 1, 1, 1) in have and (5, 4, 7, 1, 3, 3) in have                # non-square maps


@pytest.mark.parametrize("mode", [R.PAD_REFLECT, R.PAD_ZERO])
def test_conv_references_match_autograd_at_every_sweep_geometry(mode):
    """conv_fwd / conv_dgrad / conv_wgrad against float64 autograd of F.pad + conv2d at EVERY geometry of the sweep: the
    reference must be right exactly where the kernels were wrong (doubly mirrored rows, unequal pads, both splits)."""
    for g in G.conv_geometries(mode):
        x = _rand((2, g.H, g.W, 3), 41).requires_grad_(True)
        w = _rand((g.k, g.k, 3, 2), 42).requires_grad_(True)
        xp = F.pad(x.permute(0, 3, 1, 2), (g.pad_lo, g.pad_hi, g.pad_lo, g.pad_hi),
                   mode="reflect" if mode == R.PAD_REFLECT and g.pad_lo + g.pad_hi else "constant")
        y = F.conv2d(xp, w.permute(3, 2, 0, 1), stride=g.stride).permute(0, 2, 3, 1)
        assert tuple(y.shape) == (2, g.Ho, g.Wo, 2), _geom_id(g)
        dy = _rand(tuple(y.shape), 43)
        y.backward(dy)
        xd, wd = x.detach(), w.detach()
        assert torch.allclose(R.conv_fwd(xd, wd, g.stride, g.pad_lo, g.Ho, g.Wo, mode), y.detach(), atol=1e-12), _geom_id(g)
        assert torch.allclose(R.conv_dgrad(dy, wd, g.stride, g.pad_lo, g.H, g.W, mode), x.grad, atol=1e-12), _geom_id(g)
        assert torch.allclose(R.conv_wgrad(xd, dy, g.k, g.stride, g.pad_lo, mode), w.grad, atol=1e-11), _geom_id(g)


def _mirror_rows(n, n_pad, lo, hi, variant):
    """Padded positions that fold onto each row of an n-row map, as an input-gradient kernel enumerates them: the row
    itself, its mirror below the map (1 <= o <= lo) and above it (n - 1 - hi <= o <= n - 2).  variant "truth", or one of the
    two defects: "else_if" drops the second mirror of a row that has both, "lo_for_hi" takes the high range with lo."""
    rows = []
    for o in range(n):
        pos = [o + lo]
        low = 1 <= o <= lo
        high = n - 1 - (lo if variant == "lo_for_hi" else hi) <= o <= n - 2
        if low:
            pos.append(lo - o)
        if high and not (low and variant == "else_if"):
            pos.append(2 * (n - 1) - o + lo)
        rows.append([u for u in pos if 0 <= u < n_pad])
    return rows


def _variant_dgrad(dy, w, g, variant):
    gp = R.tconv_full(dy, w, g.stride)                                # the gradient on the padded grid
    for axis, n in ((1, g.H), (2, g.W)):
        rows = _mirror_rows(n, gp.shape[axis], g.pad_lo, g.pad_hi, variant)
        gp = torch.stack([gp.index_select(axis, torch.tensor(r, dtype=torch.long)).sum(axis) for r in rows], axis)
    return gp


@pytest.mark.parametrize("variant", ["else_if", "lo_for_hi"])
def test_gate_rejects_a_wrong_mirror_at_every_geometry_where_it_matters(variant):
    """An input gradient built from a fold that drops the second mirror of a doubly mirrored row, or that takes the high
    border's range with pad_lo: the gate flags it at every sweep geometry where it differs from the truth, accepts it
    where it does not (and the truth everywhere)."""
    flagged = []
    for g in _REFLECT_GEOMS:
        dy = _bf16_exact((2, g.Ho, g.Wo, 5), 51)
        w = _bf16_exact((g.k, g.k, 6, 5), 52, 1.0 / (g.k * math.sqrt(5.0)))
        ref = R.conv_dgrad(dy, w, g.stride, g.pad_lo, g.H, g.W, R.PAD_REFLECT)
        A = R.conv_dgrad(dy.abs(), w.abs(), g.stride, g.pad_lo, g.H, g.W, R.PAD_REFLECT)
        E = R.bound(A, g.k * g.k * 5 * 4)
        truth = _variant_dgrad(dy, w, g, "truth")
        assert torch.allclose(truth, ref, atol=1e-12), _geom_id(g)
        assert R.gate(truth.float(), ref, E)[0], _geom_id(g)
        got = _variant_dgrad(dy, w, g, variant)
        differs = bool((got != truth).any())
        ok = R.gate(got.float(), ref, E)[0]
        assert ok != differs, (_geom_id(g), differs, ok)
        if differs:
            flagged.append((g.H, g.W, g.k, g.stride, g.pad_lo))
    print("mutation %-34s rejected at %d of %d geometries" % (variant, len(flagged), len(_REFLECT_GEOMS)))
    if variant == "else_if":
        assert (3, 3, 3, 1, 1) in flagged and (4, 4, 5, 1, 2) in flagged and (5, 4, 5, 1, 2) in flagged
        assert (4, 4, 3, 1, 1) not in flagged and (8, 8, 5, 1, 2) not in flagged
    else:
        assert (8, 8, 4, 1, 1) in flagged and (6, 6, 4, 1, 1) in flagged             # every even k at stride 1
        assert (8, 8, 3, 1, 1) not in flagged


def test_gate_rejects_unwritten_attention_columns():
    """d = 16, dv = 256 on a kernel instance that stores columns < 128 only: columns 128 .. 255 keep the NaN prefill."""
    q, k, v = _bf16_exact((1, 128, 16), 61, 0.5), _bf16_exact((1, 128, 16), 62, 0.5), _bf16_exact((1, 128, 256), 63)
    ref, _ = R.attn_fwd(q, k, v)
    P = torch.softmax(q @ k.transpose(1, 2), dim=2)
    Pv = P @ v.abs()
    E = R.bound(Pv, 128, R.U16 * Pv)
    good = ref.to(torch.bfloat16)
    assert R.gate(good, ref, E)[0]
    bad = good.clone()
    bad[:, :, 128:] = float("nan")
    ok, _, _, _, nbad = R.gate(bad, ref, E)
    assert not ok and nbad == 128 * 128
    print("mutation %-34s rejected: %d outputs outside the bound" % ("attention columns 128.. unwritten", nbad))


def test_sweep_generator_meets_the_entry_points_preconditions():
    for mode in (R.PAD_REFLECT, R.PAD_ZERO):
        geoms = G.conv_geometries(mode)
        assert len(set(geoms)) == len(geoms)
        for g in geoms:
            assert g.H % g.stride == 0 and g.W % g.stride == 0 and 0 <= g.pad_lo < g.k and g.pad_lo < min(g.H, g.W)
            assert g.pad_hi == (g.Ho - 1) * g.stride + g.k - 1 - g.pad_lo - (g.H - 1) or g.pad_hi == 0
            for n, no in ((g.H, g.Ho), (g.W, g.Wo)):                # single reflection: pad_index asserts otherwise
                idx = R.pad_index(n, g.pad_lo, (no - 1) * g.stride + g.k, mode)
                assert len(idx) >= n or g.stride > 1
    # every k, both strides and every map survive the preconditions
    assert {g.k for g in _REFLECT_GEOMS} == set(G.CONV_K) and {g.stride for g in _REFLECT_GEOMS} == {1, 2}
    assert {(g.H, g.W) for g in _REFLECT_GEOMS} == set(G.CONV_MAPS)


def test_sweep_attention_lists_hit_both_sides_of_every_rung():
    for edge in (16, 32):                                  # DQT rungs of A16_DISPATCH (d <= 16 | 32 | 64)
        assert edge in G.A16_D and edge + 4 in G.A16_D
    for edge in (32, 64, 96, 128, 192):                    # DVT rungs 1 | 2 | 3 | 4 | 6 | 8
        assert edge in G.A16_DV and edge + 4 in G.A16_DV
    assert min(G.A16_D) == 4 and max(G.A16_D) == 64 and min(G.A16_DV) == 4 and max(G.A16_DV) == 256
    assert len({G.a16_instance(d, dv) for d in G.A16_D for dv in G.A16_DV}) == 10
    assert G.a16_instance(16, 256) == (2, 8) and G.a16_instance(16, 128) == (1, 4)
    assert 16 in G.A2_D and 20 in G.A2_D and max(G.A2_D) == 32 and max(G.A2_DV) == 128
    for edge in (32, 64, 96):
        assert edge in G.A2_DV and edge + 4 in G.A2_DV
    assert len({G.a2_instance(d, dv) for d in G.A2_D for dv in G.A2_DV}) == 8
    for kind in ("fwd", "dkv", "dq"):
        calls = G.attention16_calls(kind, 128, 256)
        assert len(calls) == len(G.A16_D) * len(G.A16_DV)
        for c in calls:                                    # column slices: every row stride is 4 wider than the row
            B, N, Nk, d, dv = c.desc[:5]
            assert (B, N, Nk) == (1, 128, 256) and c.desc[6] == d + 4 and c.desc[10] == dv + 4 and c.desc[12] == dv + 4


def test_sweep_lists_are_deterministic_and_bounded():
    a, b = G.cases(), G.cases()
    assert list(a) == list(b)
    for cid in a:
        assert [c.key() for c in a[cid][1]] == [c.key() for c in b[cid][1]], cid
        assert 0 < len(a[cid][1]) <= 150, (cid, len(a[cid][1]))
    fwd = a["conv_fwd_gemm/fp32/reflect"][1]
    assert 0.4 <= sum(c.flags["bias"] for c in fwd) / len(fwd) <= 0.6
    assert 0.2 <= sum(c.flags["acc"] for c in fwd) / len(fwd) <= 0.3


def test_narrowed_rows_are_documented_and_few():
    import os
    header = " ".join(open(os.path.join(os.path.dirname(__file__), "..", "include", "biggan_hip.h")).read()
                      .replace(" * ", " ").split())
    for rule, sentence, pred in G.NARROWED:
        assert " ".join(sentence.split()) in header, rule
    per_family = {}
    for cid, (_, calls) in G.cases().items():
        n, r = per_family.get(G.family(cid), (0, 0))
        per_family[G.family(cid)] = (n + len(calls), r + sum(G.narrowed(c) is not None for c in calls))
    assert set(per_family) == {"conv", "deconv", "attention16", "attention2"}
    for fam, (n, r) in per_family.items():
        print("%-12s %5d calls, %4d narrowed (%.1f %%)" % (fam, n, r, 100.0 * r / n))
        assert r <= G.MAX_REJECTED * n, fam
