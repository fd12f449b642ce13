"""The discriminator's reconstruction heads on the GPU (--d_reconstruction, --d_reconstruction_halfres,
--d_reconstruction_texture): every kernel of csrc/recon.hip against float64 on BASELINE config 3's shapes and on edge
shapes, whole-D-step parity against the float64 restatement (tests/recon_ref.py installed over the oracle), graph replay
with fresh offsets, virtual batches, a bf16-resident step at config 3's topology, the training loop's sample grids and a
2-rank step against the 1-rank step at the global batch.

Bounds.  fp32 whole-step gates are the project's (tests/test_gpu_step.py: losses 1e-4, gradients 1e-3 relative L2), bf16
the ones of tests/test_gpu_bf16.py (losses 2e-2).  Per-element kernel outputs are held to ``launch_replay.gate`` with
E = m 2^-24 A, m counted from the roundings of the formula as tests/elementwise_ref.py does - never from an output."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import ref_model as RM
from tests import launch_replay as G
from tests import recon_ref as RR
from tests.common import hip_model_like, dev_draws, rel_err, t2n, make_args
from tests.test_gpu_step import _run_parity, _loss_close, cu, GRAD_TOL

pytestmark = pytest.mark.gpu

U32 = G.U32
D64 = torch.float64


def _hip():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip
    return Fn, hip


def _gate(label, got, ref, E):
    ok, ratio, above, below, nbad = G.gate(got, ref, E)
    print("%-28s %s worst err/bound %.3f (bf16 ambiguous +%d -%d)" % (label, tuple(got.shape), ratio, above, below))
    assert ok, (label, nbad, ratio)


def _rand(shape, seed, dtype, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


# BASELINE config 3 (128^2, d_ch 96): the glu inputs [N, H, W, 2C] of the full coarse head (8 x 8 x 768 map -> 128), of the
# halfres head and of the texture head (4 x 4 x 384 crop -> 32), at batch 8; and edge shapes: odd sizes, channel counts
# that are no multiple of the 16-byte piece, one pixel
GLU_CONFIG3 = [(8, 16, 16, 512), (8, 32, 32, 256), (8, 64, 64, 128), (8, 128, 128, 64), (8, 8, 8, 384), (8, 32, 32, 96)]
GLU_EDGE = [(3, 5, 7, 8), (2, 3, 3, 5), (1, 1, 1, 1), (1, 1, 1, 8), (2, 7, 5, 12), (5, 1, 9, 3)]

S_M = 4            # roundings in s = 1 / (1 + exp(-g)): exp (2 ulp), the sum, the division


def _glu_refs(x, dy):
    C = x.shape[-1] // 2
    a, g = x.double()[..., :C], x.double()[..., C:]
    s = torch.sigmoid(g)
    y = a * s
    Ey = (S_M + 2) * U32 * y.abs()                                   # + the product + 1 second-order
    d = dy.double()
    da = d * s
    Eda = (S_M + 2) * U32 * da.abs()
    dg = d * a * s * (1 - s)
    # s (1 - s): the error of s enters with |1 - 2 s|; 1 - s (1), three products (3), + 1 second-order
    Edg = U32 * (d * a).abs() * s * (S_M * (1 - 2 * s).abs() + 5 * (1 - s))
    return y, Ey, torch.cat([da, dg], dim=-1), torch.cat([Eda, Edg], dim=-1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", GLU_CONFIG3 + GLU_EDGE)
def test_glu_against_float64(shape, dtype):
    Fn, _ = _hip()
    N, H, W, C = shape
    x = _rand((N, H, W, 2 * C), 1 + C + H, dtype, 1.5).requires_grad_(True)
    y = Fn.GluFn.apply(x)
    assert y.dtype == dtype and tuple(y.shape) == (N, H, W, C)
    dy = _rand((N, H, W, C), 2 + C, dtype)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert dx.dtype == dtype and dx.shape == x.shape
    yr, Ey, dxr, Edx = _glu_refs(x.detach(), dy)
    _gate("glu fwd %s" % dtype, y.detach(), yr, Ey)
    _gate("glu bwd %s" % dtype, dx, dxr, Edx)


# ---------------------------------------------------------------- batch norm + GLU in one kernel
BN_FWD_M = 5       # tests/elementwise_ref.py: inv = rs ga (1); mu inv (2); be - mu inv (3); x inv (2) + shift (4); + 1
XH_M = 4           # the rounded mean, the difference, the rounded rstd, the product
BN_EPS = 1e-5


def _bn_glu_refs(x, dy, gamma, beta):
    """Training-mode batch norm on [rows, 2C] then glu, and the gradients for dL/dy = dy, in float64 from the stored
    inputs, with the error bounds built from the formula's roundings (E = m 2^-24 A; column sums over K rows:
    launch_replay.bound plus every term's own error)."""
    C = x.shape[-1] // 2
    xd = x.double().reshape(-1, 2 * C)
    d = dy.double().reshape(-1, C)
    K = xd.shape[0]
    ga, be = gamma.double(), beta.double()
    mu = xd.mean(0)
    rs = torch.rsqrt(((xd - mu) ** 2).mean(0) + BN_EPS)
    inv = rs * ga
    pre = xd * inv + (be - mu * inv)
    E_pre = BN_FWD_M * U32 * ((xd * inv).abs() + be.abs() + (mu * inv).abs())
    xh = (xd - mu) * rs
    E_xh = XH_M * U32 * (xd.abs() + mu.abs()) * rs
    pm, pg = pre[:, :C], pre[:, C:]
    s = torch.sigmoid(pg)
    E_s = S_M * U32 * s + s * (1 - s) * E_pre[:, C:]
    y = pm * s
    E_y = E_pre[:, :C] * s + pm.abs() * E_s + 2 * U32 * y.abs()
    gm = d * s
    E_gm = d.abs() * E_s + 2 * U32 * gm.abs()
    gg = d * pm * s * (1 - s)
    E_gg = d.abs() * (E_pre[:, :C] * s * (1 - s) + pm.abs() * (1 - 2 * s).abs() * E_s + 5 * U32 * pm.abs() * s * (1 - s))
    g = torch.cat([gm, gg], dim=1)
    E_g = torch.cat([E_gm, E_gg], dim=1)
    dbeta = g.sum(0)
    E_dbeta = G.bound(g.abs().sum(0), K) + E_g.sum(0)
    dgamma = (g * xh).sum(0)
    E_dgamma = G.bound((g * xh).abs().sum(0), K) + (E_g * xh.abs() + g.abs() * E_xh).sum(0)
    m1, m2 = ga * dbeta / K, ga * dgamma / K
    E_m1 = ga.abs() * E_dbeta / K + U32 * m1.abs()
    E_m2 = ga.abs() * E_dgamma / K + U32 * m2.abs()
    dx = rs * (g * ga - m1 - xh * m2)
    E_dx = rs * (ga.abs() * E_g + E_m1 + xh.abs() * E_m2 + m2.abs() * E_xh) \
        + 4 * U32 * rs * ((g * ga).abs() + m1.abs() + (xh * m2).abs())
    return (y, E_y), (dx, E_dx), (dgamma, E_dgamma), (dbeta, E_dbeta)


BN_GLU_SHAPES = [(8, 16, 16, 512), (8, 64, 64, 128), (4, 128, 128, 64), (8, 32, 32, 96), (3, 5, 7, 8), (2, 3, 3, 5),
                 (4, 1, 1, 1), (2, 7, 5, 12), (2, 9, 9, 260)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", BN_GLU_SHAPES)
def test_bn_glu_against_float64(shape, dtype):
    Fn, _ = _hip()
    N, H, W, C = shape
    x = (_rand((N, H, W, 2 * C), 11 + C, torch.float32, 1.3) + 0.3).to(dtype).requires_grad_(True)
    gamma = (torch.rand(2 * C, generator=torch.Generator().manual_seed(C)) + 0.5).cuda().requires_grad_(True)
    beta = (torch.randn(2 * C, generator=torch.Generator().manual_seed(C + 1)) * 0.3).cuda().requires_grad_(True)
    mm, mv = torch.zeros(2 * C, device="cuda"), torch.ones(2 * C, device="cuda")
    y = Fn.BnGluFn.apply(x, gamma, beta, mm, mv, 0.9, BN_EPS, True, None, 1)
    assert y.dtype == dtype and tuple(y.shape) == (N, H, W, C)
    dy = _rand((N, H, W, C), 12 + C, dtype)
    dx, dg, db = torch.autograd.grad(y, [x, gamma, beta], dy)
    (yr, Ey), (dxr, Edx), (dgr, Edg), (dbr, Edb) = _bn_glu_refs(x.detach(), dy, gamma.detach(), beta.detach())
    _gate("bn+glu fwd %s" % dtype, y.detach().reshape(-1, C), yr, Ey)
    _gate("bn+glu dx %s" % dtype, dx.reshape(-1, 2 * C), dxr, Edx)
    _gate("bn+glu dgamma", dg, dgr, Edg)
    _gate("bn+glu dbeta", db, dbr, Edb)
    # the moving statistics moved as tf.layers.batch_normalization moves them (momentum 0.9, Bessel-corrected variance)
    xd = x.detach().double().reshape(-1, 2 * C)
    K = xd.shape[0]
    assert rel_err(t2n(mm), (0.1 * xd.mean(0)).cpu().numpy()) < 1e-5
    assert rel_err(t2n(mv), (0.9 + 0.1 * xd.var(0, unbiased=False) * K / max(K - 1, 1)).cpu().numpy()) < 1e-5


def test_fused_bn_glu_is_the_unfused_pair_in_fp32():
    """BG_FUSE_BNGLU: the same arithmetic element by element - the forward is bit-identical to bn then glu on fp32 tensors,
    the gradients differ by the order of the column sums only."""
    from biggan_tensorflow_amd import ops, scope as S
    x0 = _rand((4, 16, 16, 64), 5, torch.float32, 1.2)
    dy = _rand((4, 16, 16, 32), 6, torch.float32)
    outs = []
    for flag in ("1", "0"):
        prev = os.environ.get("BG_FUSE_BNGLU")
        os.environ["BG_FUSE_BNGLU"] = flag
        try:
            store = S.VariableStore("cuda", seed=1)
            S.set_default_store(store)
            ops.begin_run()
            x = x0.clone().requires_grad_(True)
            with S.variable_scope("discriminator"):
                y = ops.bn_glu(x, opt={"is_training": True, "bn": {"type": "batch_norm", "momentum": 0.98}})
            (dx,) = torch.autograd.grad(y, x, dy)
            outs.append((y.detach(), dx, {k: t2n(v).copy() for k, v in store.vars.items()}))
        finally:
            if prev is None:
                os.environ.pop("BG_FUSE_BNGLU", None)
            else:
                os.environ["BG_FUSE_BNGLU"] = prev
    (y1, dx1, v1), (y0, dx0, v0) = outs
    assert torch.equal(y1, y0)
    assert rel_err(t2n(dx1), t2n(dx0)) < 1e-5
    assert set(v1) == set(v0) == {"discriminator/batch_norm/" + k for k in ("gamma", "beta", "moving_mean",
                                                                             "moving_variance")}
    for k in v1:
        assert np.array_equal(v1[k], v0[k]), k


UP_SHAPES = [(8, 8, 8, 768), (8, 64, 64, 128), (8, 4, 4, 384), (3, 5, 7, 8), (2, 3, 3, 5), (1, 1, 1, 1), (2, 1, 9, 24)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_up_sample_is_the_indexing_and_its_backward_the_box_sum(shape, dtype):
    Fn, hip = _hip()
    N, H, W, C = shape
    x = _rand(shape, 3 + C, dtype).requires_grad_(True)
    y = Fn.UpSample2Fn.apply(x)
    assert y.dtype == dtype
    assert torch.equal(y.detach(), x.detach().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
    dy = _rand((N, 2 * H, 2 * W, C), 4 + C, dtype)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert dx.dtype == dtype
    win = dy.double().reshape(N, H, 2, W, 2, C)
    ref = win.sum(dim=(2, 4))
    _gate("up_sample bwd %s" % dtype, dx, ref, 3 * U32 * win.abs().sum(dim=(2, 4)))       # three fp32 additions
    if dtype == torch.bfloat16:
        # the raw typed entry points serve fp32 tensors as well
        xf = x.detach().float()
        yf = torch.empty(N, 2 * H, 2 * W, C, device="cuda")
        hip.check(hip.lib().bg_upsample2_fwd_t(hip.act(xf), hip.act(yf), hip.F32, N, H, W, C, hip.stream()))
        assert torch.equal(yf, y.detach().float())
    # ops.up_sample keeps the type: no fp32 round trip for a bf16 map
    from biggan_tensorflow_amd import ops
    assert ops.up_sample(x.detach()).dtype == dtype


CROP_CASES = [(8, 16, 16, 384, 4, 12, 0), (8, 16, 16, 384, 4, 0, 12), (8, 16, 16, 384, 4, 5, 9), (2, 7, 5, 5, 3, 4, 2),
              (3, 6, 6, 8, 6, 0, 0), (1, 1, 1, 1, 1, 0, 0), (2, 9, 9, 12, 2, 7, 0)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", CROP_CASES)
def test_crop_at_a_device_offset_is_the_indexing(case, dtype):
    Fn, _ = _hip()
    N, H, W, C, p, oy, ox = case
    x = _rand((N, H, W, C), 5 + C, dtype).requires_grad_(True)
    ro_x = torch.full((N,), oy, dtype=torch.int32, device="cuda")          # (the first offset is the height offset)
    ro_y = torch.full((N,), ox, dtype=torch.int32, device="cuda")
    ro_x[1:] = 99                                                          # only element [0] is used
    y = Fn.CropAtFn.apply(x, ro_x, ro_y, p)
    assert torch.equal(y.detach(), x.detach()[:, oy:oy + p, ox:ox + p, :])
    dy = _rand((N, p, p, C), 6 + C, dtype)
    (dx,) = torch.autograd.grad(y, x, dy)
    want = torch.zeros_like(x.detach())
    want[:, oy:oy + p, ox:ox + p, :] = dy
    assert torch.equal(dx, want)
    # the offsets are read when the kernel runs: the same launch arguments with new contents
    ro_x[0], ro_y[0] = H - p, 0
    assert torch.equal(Fn.CropAtFn.apply(x.detach(), ro_x, ro_y, p), x.detach()[:, H - p:, :p, :])
    # out-of-range draws are clamped on the device: nothing outside the tensor is addressed
    ro_x[0], ro_y[0] = -3, 10 ** 6
    assert torch.equal(Fn.CropAtFn.apply(x.detach(), ro_x, ro_y, p), x.detach()[:, :p, W - p:, :])


# (N, h, S, C, mode, f, (oy, ox)): config 3's three heads (full coarse 128, halfres 64 of 128, texture 32 of 128 with
# f = 8 at both offset extremes) and edge shapes (c_dim 1 / 4, one pixel, odd sizes)
LOSS_CASES = [(8, 128, 128, 3, 0, 1, (0, 0)), (8, 64, 128, 3, 1, 1, (0, 0)), (8, 32, 128, 3, 2, 8, (12, 0)),
              (8, 32, 128, 3, 2, 8, (0, 12)), (4, 16, 64, 4, 2, 4, (5, 9)), (3, 5, 5, 1, 0, 1, (0, 0)),
              (2, 3, 6, 4, 1, 1, (0, 0)), (1, 1, 1, 3, 0, 1, (0, 0)), (2, 3, 7, 3, 2, 2, (2, 1))]
TANH_M = 2         # tanhf


def _loss_refs(y, t, mode, f, off, ld, dloss):
    N, h, _, C = y.shape
    v = torch.tanh(y.double())
    td = t.double()
    if mode == 0:
        tgt, At, mt = td, td.abs(), 0
    elif mode == 1:
        S = t.shape[1]
        win = td.reshape(N, S // 2, 2, S // 2, 2, C)
        tgt, At, mt = win.mean(dim=(2, 4)), win.abs().mean(dim=(2, 4)), 4           # three additions and the 0.25
    else:
        oy, ox = off
        tgt = td[:, oy * f:oy * f + h, ox * f:ox * f + h, :]
        At, mt = tgt.abs(), 0
    d = v - tgt
    Ed = U32 * (TANH_M * v.abs() + mt * At + d.abs())                              # tanh, the target, the difference
    ssq = (d * d).sum()
    K = d.numel()
    E_ssq = G.bound((d * d).sum(), K) + (2 * d.abs() * Ed + 2 * U32 * d * d).sum()  # the reduction + every term's own error
    scale = 1000.0 * ld / K
    loss = torch.sqrt(ssq) * scale
    E_loss = scale * E_ssq / (2 * torch.sqrt(ssq)) + 2 * U32 * loss                # sqrt halves the relative error; the cast
    k = scale / torch.sqrt(ssq) * dloss
    rel_k = E_ssq / (2 * ssq) + 2 * U32                                            # cast to fp32, times dloss
    one_m = 1 - v * v
    dy = k * d * one_m
    E_dy = k.abs() * (Ed * one_m + d.abs() * U32 * (5 * v * v + one_m)) + dy.abs() * (rel_k + 3 * U32)
    return v, TANH_M * U32 * v.abs(), loss, E_loss, dy, E_dy


@pytest.mark.parametrize("case", LOSS_CASES)
def test_recon_loss_against_float64(case):
    Fn, _ = _hip()
    N, h, S, C, mode, f, (oy, ox) = case
    y = _rand((N, h, h, C), 7 + h, torch.float32, 0.7).requires_grad_(True)
    t = (torch.rand(N, S, S, C, generator=torch.Generator().manual_seed(S + C)) * 2 - 1).cuda()
    ro_x = torch.full((N,), oy, dtype=torch.int32, device="cuda")
    ro_y = torch.full((N,), ox, dtype=torch.int32, device="cuda")
    ld = 0.5
    loss, img = Fn.ReconLossFn.apply(y, t, ro_x, ro_y, mode, f, ld, None, 1)
    assert tuple(loss.shape) == (1,) and not img.requires_grad
    dl = torch.tensor([0.75], device="cuda")
    (dy,) = torch.autograd.grad(loss, y, dl)
    v, Ev, lr, El, dyr, Edy = _loss_refs(y.detach(), t, mode, f, (oy, ox), ld, 0.75)
    print("loss %.7f reference %.7f bound %.2e" % (loss.item(), lr.item(), El.item()))
    _gate("tanh image", img, v, Ev)
    _gate("loss", loss, lr.reshape(1), El.reshape(1))
    _gate("dy", dy, dyr, Edy)
    assert float(dy.abs().max()) > 0


def test_recon_loss_is_zero_gradient_at_the_singular_point():
    Fn, _ = _hip()
    y = torch.zeros(2, 4, 4, 3, device="cuda", requires_grad=True)
    t = torch.zeros(2, 4, 4, 3, device="cuda")
    loss, _ = Fn.ReconLossFn.apply(y, t, None, None, 0, 1, 1.0, None, 1)
    (dy,) = torch.autograd.grad(loss, y)
    assert loss.item() == 0.0 and torch.equal(dy, torch.zeros_like(dy))


def test_abi_rejects_bad_arguments():
    _, hip = _hip()
    L = hip.lib()
    s = hip.stream()
    x = torch.zeros(2, 4, 4, 16, device="cuda", dtype=torch.bfloat16)
    y = torch.zeros(2, 8, 8, 16, device="cuda", dtype=torch.bfloat16)
    o = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()      # noqa: E731
    assert L.bg_glu_fwd(p(x), p(y), hip.BF16, 32, 8, s) == 0
    assert L.bg_glu_fwd(None, p(y), hip.BF16, 32, 8, s) == 1
    assert L.bg_glu_fwd(p(x), p(y), 7, 32, 8, s) == 1
    assert L.bg_glu_fwd(p(x), p(y), hip.BF16, 0, 8, s) == 1
    assert L.bg_glu_bwd(p(x), None, p(y), hip.BF16, 32, 8, s) == 1
    f = torch.ones(32, device="cuda")
    assert L.bg_bn_glu_fwd(p(y), p(f), p(f), p(f), p(f), p(x), hip.BF16, 64, 8, s) == 0        # [64, 16] -> [64, 8]
    assert L.bg_bn_glu_fwd(p(y), None, p(f), p(f), p(f), p(x), hip.BF16, 128, 8, s) == 1
    assert L.bg_bn_glu_bwd_reduce(p(y), p(x), p(f), p(f), p(f), p(f), p(f), hip.BF16, 128, 8, 0, s) == 1     # nseg >= 1
    assert L.bg_bn_glu_bwd_dx(p(y), p(x), p(f), p(f), p(f), p(f), None, p(y), hip.BF16, 128, 8, s) == 1
    assert L.bg_upsample2_fwd_t(p(x), p(y), hip.BF16, 2, 4, 4, 16, s) == 0
    assert L.bg_upsample2_fwd_t(p(x), p(y), hip.BF16, 2, 0, 4, 16, s) == 1
    assert L.bg_upsample2_bwd_t(p(y), None, hip.BF16, 2, 4, 4, 16, s) == 1
    assert L.bg_crop_at_fwd(p(y), p(x), hip.BF16, p(o), p(o), 2, 8, 8, 4, 16, s) == 0
    assert L.bg_crop_at_fwd(p(y), p(x), hip.BF16, None, p(o), 2, 8, 8, 4, 16, s) == 1      # offsets live on the device
    assert L.bg_crop_at_fwd(p(y), p(x), hip.BF16, p(o), p(o), 2, 8, 8, 9, 16, s) == 1      # window larger than the map
    assert L.bg_crop_at_bwd(p(x), p(y), hip.BF16, p(o), p(o), 2, 8, 8, 0, 16, s) == 1
    yf = torch.zeros(2, 4, 4, 3, device="cuda")
    tf = torch.zeros(2, 8, 8, 3, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    assert L.bg_recon_loss_sums(p(yf), p(tf), None, None, None, 1, 1, p(acc), 2, 4, 4, 8, 3, s) == 0
    assert L.bg_recon_loss_sums(p(yf), p(tf), None, None, None, 0, 1, p(acc), 2, 4, 4, 8, 3, s) == 1     # identity: S == h
    assert L.bg_recon_loss_sums(p(yf), p(tf), None, None, None, 2, 2, p(acc), 2, 4, 4, 8, 3, s) == 1     # crop: offsets
    assert L.bg_recon_loss_sums(p(yf), p(tf), None, None, None, 3, 1, p(acc), 2, 4, 4, 8, 3, s) == 1
    assert L.bg_recon_loss_finalize(None, 1.0, p(yf), s) == 1
    assert L.bg_recon_loss_bwd(p(yf), p(tf), None, None, 1, 1, p(acc), 1.0, None, None, 2, 4, 4, 8, 3, s) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- whole D step
def _offsets(off, B):
    return (torch.full((B,), off[0], dtype=torch.int32, device="cuda"),
            torch.full((B,), off[1], dtype=torch.int32, device="cuda"))


def _pair(monkeypatch, case):
    name, flags, off = RR.PARITY_CASES[case]
    RR.install(monkeypatch)
    tr = RR.trainer(**dict(RR.PARITY_SHAPE, **flags))
    gan = hip_model_like(tr, **flags)
    assert set(gan.store.vars) == set(tr.vs.vars)
    B = RR.PARITY_SHAPE["batch_size"]
    tr.recon_offsets = off                                             # explicit offsets on both sides
    gan.d_step = functools.partial(gan.d_step, recon_offsets=_offsets(off, B))
    return name, tr, gan, RM.synthetic_batch(tr.cfg, 70 + case, B)


@pytest.mark.parametrize("case", range(len(RR.PARITY_CASES)))
def test_d_step_parity(monkeypatch, case):
    """Losses (d_recon and d_tex_recon included), every D gradient, the post-step weights and state - and the G step, which
    the heads must leave alone - against the installed restatement, with the gates of tests/test_gpu_step.py."""
    name, tr, gan, batch = _pair(monkeypatch, case)
    hip0 = gan.store.export_arrays()
    okw, hkw = {}, {}
    if "gp" in batch:
        okw = dict(gp=batch["gp"])
        hkw = dict(gp_draws={"alpha": cu(batch["gp"]["alpha"]), "aug": dev_draws(batch["gp"]["aug"])})
    ro = tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"], apply=False, **okw)
    ho = gan.d_step(cu(batch["real"]), cu(batch["z_d"]), dev_draws(batch["aug_real"]), dev_draws(batch["aug_fake_d"]),
                    apply=False, **hkw)
    for key, imgkey in (("d_recon", "coarse_upscaled"), ("d_tex_recon", "texture_upscaled")):
        assert (key in ro) == (key in ho)
        if key in ro:
            print("%s %s: product %.7f restatement %.7f" % (name, key, ho[key].item(), ro[key].item()))
            assert _loss_close(ho[key].item(), ro[key].item()), (key, ho[key].item(), ro[key].item())
            assert rel_err(t2n(ho[imgkey]), ro[imgkey].detach().numpy()) < GRAD_TOL
    assert _loss_close(ho["d_loss"].item(), ro["d_loss"].item())
    assert ("d_recon" in ro) or ("d_tex_recon" in ro)
    tr.vs.state_updates.clear()
    gan.store.load_arrays(hip0, reset_ema=False)
    _run_parity(tr, gan, batch)


def test_heads_leave_the_g_step_and_the_flagless_model_alone(monkeypatch):
    """The G step of a model with the heads is the G step of the model without them (the heads run in the real call of the
    D step only), and it leaves every variable of the heads untouched."""
    _, flags, off = RR.PARITY_CASES[3]
    RR.install(monkeypatch)
    tr = RR.trainer(**dict(RR.PARITY_SHAPE, **flags))
    plain = RR.trainer(**RR.PARITY_SHAPE)
    gan = hip_model_like(tr, **flags)
    ref = hip_model_like(plain)
    shared = {k: v for k, v in gan.store.export_arrays().items() if k in ref.store.vars}
    ref.store.load_arrays(shared)
    batch = RM.synthetic_batch(tr.cfg, 9, 4)
    outs = []
    for g in (gan, ref):
        o = g.g_step(4, cu(batch["z_g"]), dev_draws(batch["aug_fake_g"]), apply=False)
        outs.append((o["g_loss"].item(), t2n(g.g_arena.grads).copy()))
    # (same launches on the same data: the forward pass is bit-reproducible, backward reductions up to their atomics)
    assert outs[0][0] == outs[1][0] and rel_err(outs[0][1], outs[1][1]) < 1e-6
    u0 = {k: t2n(v).copy() for k, v in gan.store.vars.items() if "upscaler" in k}
    gan.g_step(4, cu(batch["z_g"]), dev_draws(batch["aug_fake_g"]))
    for k, v in u0.items():                                    # u, moving statistics and weights of the heads: untouched
        assert np.array_equal(t2n(gan.store.vars[k]), v), k


def test_virtual_batches_take_offsets_and_norm_per_virtual_batch(monkeypatch):
    _, flags, _ = RR.PARITY_CASES[3]
    RR.install(monkeypatch)
    tr = RR.trainer(**dict(RR.PARITY_SHAPE, **flags))
    one = hip_model_like(tr, **flags)
    two = hip_model_like(tr, virtual_batches=2, **flags)
    batches = [RM.synthetic_batch(tr.cfg, 21 + i, 4) for i in range(2)]
    offs = [_offsets((12, 3), 4), _offsets((0, 7), 4)]

    def args(b):
        return cu(b["real"]), cu(b["z_d"]), dev_draws(b["aug_real"]), dev_draws(b["aug_fake_d"])
    singles, grads = [], 0.0
    for b, o in zip(batches, offs):                            # (u and the moving statistics advance from run to run)
        out = one.d_step(*args(b), apply=False, recon_offsets=o)
        singles.append({k: out[k].item() for k in ("d_loss", "d_recon", "d_tex_recon")})
        grads = grads + t2n(one.d_arena.grads).astype(np.float64)
    cols = list(zip(*[args(b) for b in batches]))
    out = two.d_step(*[list(c) for c in cols], apply=False, recon_offsets=offs)
    for k in ("d_loss", "d_recon", "d_tex_recon"):
        mean = 0.5 * (singles[0][k] + singles[1][k])
        assert abs(out[k].item() - mean) <= 1e-5 * abs(mean), (k, out[k].item(), mean)
    assert singles[0]["d_tex_recon"] != singles[1]["d_tex_recon"]
    assert rel_err(t2n(two.d_arena.grads), grads) < 1e-5


def test_graph_replay_draws_new_offsets():
    """The offsets are drawn and read on the device: replays of the captured D step crop new windows, and each replay
    equals the eager step with the same draws."""
    from biggan_tensorflow_amd import model, scope as S, functional as Fn
    flags = dict(d_reconstruction_halfres="true", d_reconstruction_texture="true", d_recon_ch=16, d_tex_recon_ch=24)
    try:
        gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, n_labels=0, **flags),
                           store=S.VariableStore("cuda", seed=5)).build_model()
        data = [gan.synthetic_batch(4) for _ in range(4)]
        snap = gan.state_tensors()
        saved = {k: v.detach().clone() for k, v in snap.items()}
        rng = gan.gen.get_state()
        eager = []
        for real in data:
            l = gan.train_step(real)
            eager.append({k: v.item() for k, v in l.items()})
        assert set(eager[0]) == {"d_loss", "g_loss", "d_recon", "d_tex_recon"}
        with torch.no_grad():
            for k, v in snap.items():
                v.copy_(saved[k])
        gan.counter, gan.d_arena.step, gan.g_arena.step = 0, 0, 0
        gan.capture_graphs()
        assert gan._graphs_ready
        gan.gen.set_state(rng)
        seen = []
        for real, e in zip(data, eager):
            l = gan.train_step(real)
            seen.append((int(gan._g_out_d["rnd_offset_x"][0].item()), int(gan._g_out_d["rnd_offset_y"][0].item())))
            for k, v in e.items():
                assert abs(l[k].item() - v) <= 1e-5 * abs(v), (k, l[k].item(), v)
        print("offsets of the replays:", seen)
        assert all(0 <= a <= 12 and 0 <= b <= 12 for a, b in seen)
        assert len(set(seen)) > 1                                   # fresh draws, not the captured ones
    finally:
        Fn.set_precision("fp32")


def test_bf16_d_step_config3_topology():
    """BASELINE config 3's topology (128^2, ch 96, bf16-resident) at batch 4 with both heads: the bf16 D step against the
    same model in fp32 within the bf16 gate of tests/test_gpu_bf16.py (losses 2e-2 relative; gradients 4e-1 relative L2)."""
    from biggan_tensorflow_amd import model, scope as S, functional as Fn
    kw = dict(img_size=128, ch=96, batch_size=4, d_reconstruction_halfres="true", d_reconstruction_texture="true")
    try:
        g32 = model.BigGAN(make_args(**kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16 = model.BigGAN(make_args(precision="bf16", **kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16.store.load_arrays(g32.store.export_arrays())
        torch.manual_seed(0)
        z = torch.randn(4, 1, 1, g32.z_dim, device="cuda").clamp_(-2, 2)
        real = torch.rand(4, 128, 128, 3, device="cuda") * 2.0 - 1.0
        off = _offsets((12, 5), 4)
        names = ["discriminator/upscaler/upscale0/conv_0/kernel", "discriminator/upscaler/upscale2/conv_0/kernel",
                 "discriminator/upscaler/conv_0/kernel", "discriminator/tex_upscaler/upscale0/conv_0/kernel",
                 "discriminator/tex_upscaler/upscale2/batch_norm/gamma", "discriminator/tex_upscaler/conv_0/kernel",
                 "discriminator/resblock_down_1/res1/conv_0/kernel"]
        outs = []
        for g in (g32, g16):
            o = g.d_step(real, z, None, None, apply=False, recon_offsets=off)
            outs.append(({k: o[k].item() for k in ("d_loss", "d_recon", "d_tex_recon")},
                         {k: t2n(g.store.vars[k].bg_grad).copy() for k in names}, o["coarse_upscaled"].dtype))
            torch.cuda.synchronize()
        (l32, gr32, _), (l16, gr16, imgdt) = outs
        assert imgdt == torch.float32                                # the image conv hands fp32 to the loss
        for k in l32:
            print("%s fp32 %.6f bf16 %.6f" % (k, l32[k], l16[k]))
            assert abs(l16[k] - l32[k]) <= 2e-2 * max(abs(l32[k]), 1e-6), (k, l16[k], l32[k])
        for k in names:
            print(k, rel_err(gr16[k], gr32[k]))
            assert np.isfinite(gr16[k]).all() and rel_err(gr16[k], gr32[k]) < 4e-1, (k, rel_err(gr16[k], gr32[k]))
    finally:
        Fn.set_precision("fp32")


def test_train_loop_prints_the_losses_and_writes_the_four_grids(tmp_path, capsys):
    from biggan_tensorflow_amd import model, scope as S
    args = make_args(img_size=64, ch=8, batch_size=4, z_dim=64, d_reconstruction_halfres="true",
                     d_reconstruction_texture="true", d_save_recon_samples="true", d_recon_ch=16, d_tex_recon_ch=24,
                     print_freq=2, sample_dir=str(tmp_path / "samples"), checkpoint_dir=str(tmp_path / "ckpt"))
    gan = model.BigGAN(args, store=S.VariableStore("cuda", seed=2)).build_model()
    gan.train(iterations=2, resume=False)
    out = capsys.readouterr().out
    assert "d_recon:" in out and "d_tex_recon:" in out
    names = sorted(os.listdir(str(tmp_path / "samples")))
    assert [n.split("_00_")[0] for n in names] == ["BigGAN_recon_fake", "BigGAN_recon_real", "BigGAN_txrecon_fake",
                                                   "BigGAN_txrecon_real"], names
    # checkpoints carry the new variables under their TF names
    path = gan.save(str(tmp_path / "ckpt"), gan.counter)
    from safetensors.torch import load_file
    t = load_file(path)
    assert "discriminator/upscaler/upscale0/conv_0/kernel" in t and "discriminator/tex_upscaler/conv_0/bias/Adam_1" in t


# ---------------------------------------------------------------- data parallel
IMG, CH, ZD, B = 64, 8, 64, 4
DP_FLAGS = dict(d_reconstruction_halfres=True, d_reconstruction_texture=True, d_recon_ch=16, d_tex_recon_ch=24)
DP_OFF = (7, 12)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_d_step(lo, hi):
    """The D step on samples [lo, hi) of the global batch -> losses and the flat gradient arena."""
    tr = RR.trainer(img_size=IMG, ch=CH, z_dim=ZD, batch_size=B, **DP_FLAGS)
    gan = hip_model_like(tr, **DP_FLAGS)
    batch = RM.synthetic_batch(tr.cfg, 5, B)

    def sl(d):
        return {k: v[lo:hi] for k, v in d.items()}
    o = gan.d_step(cu(batch["real"][lo:hi]), cu(batch["z_d"][lo:hi]), dev_draws(sl(batch["aug_real"])),
                   dev_draws(sl(batch["aug_fake_d"])), apply=False, recon_offsets=_offsets(DP_OFF, hi - lo))
    out = {k: o[k].item() for k in ("d_loss", "d_recon", "d_tex_recon")}
    out["d_grads"] = t2n(gan.d_arena.grads).copy()
    return gan, out


def _dp_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch.distributed as dist
    from biggan_tensorflow_amd import parallel
    torch.cuda.set_device(0)
    parallel.init_from_env(backend="gloo")
    mpatch = pytest.MonkeyPatch()
    try:
        RR.install(mpatch)
        lo, hi = parallel.shard_batch(B, rank, world)
        gan, out = _dp_d_step(lo, hi)
        assert gan.world == world and gan.rank == rank
        # drawn offsets: every rank crops rank 0's window
        ro = gan.random_crop_offsets((hi - lo, 16, 16), 4)
        out["drawn"] = (int(ro[0][0].item()), int(ro[1][0].item()))
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    finally:
        mpatch.undo()


def test_two_rank_d_step_matches_the_global_batch(monkeypatch):
    """Cross-replica statistics in the upscalers' batch norms, ONE all-reduced sum of squares under the square root and the
    global element count: two ranks on half the batch each reproduce the single-process step at the global batch."""
    RR.install(monkeypatch)
    _, ref = _dp_d_step(0, B)
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        o = res[r]
        for k in ("d_loss", "d_recon", "d_tex_recon"):
            assert abs(o[k] - ref[k]) <= 1e-5 * abs(ref[k]), (r, k, o[k], ref[k])
        e = rel_err(o["d_grads"], ref["d_grads"])
        assert e < 1e-4, (r, e)
    assert np.array_equal(res[0]["d_grads"], res[1]["d_grads"])
    assert res[0]["drawn"] == res[1]["drawn"]
