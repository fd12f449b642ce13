"""Sub-pixel up-sampling on the GPU (--upsampling_method subpixel2 / subpixel3, ops.py:23-27) and the mixed 3x3 / 5x5
down-sampling conv (--downsampling_method resize_conv35, ops.py:281-285): the shuffle kernels bit-exact against the torch
permutation, functional.SubpixelConvFn against float64, the fused depth-to-space store of the bf16-resident convolution
bit-identical to conv + bg_depth_to_space, whole-step parity against the float64 restatement (tests/subpixel_ref.py
installed over the oracle), EMA sampling, graph replay and a bf16 step at BASELINE config 3's topology."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model as RM
from tests import subpixel_ref as SR
from tests.common import hip_model_like, dev_draws, rel_err, t2n, make_args
from tests.test_gpu_step import _run_parity, cu

pytestmark = pytest.mark.gpu

REFLECT, ZERO = 0, 1


def _hip():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip
    return Fn, hip


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- shuffle kernels
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("C", [8, 24, 96])
@pytest.mark.parametrize("N,H,W", [(3, 5, 7), (2, 33, 17), (1, 1, 1)])
def test_shuffle_kernels_are_the_permutation(dtype, C, N, H, W):
    Fn, _ = _hip()
    g = torch.Generator(device="cpu").manual_seed(C + H)
    x = torch.randn(N, H, W, 4 * C, generator=g).to(dtype).cuda()
    y = Fn.depth_to_space(x, 2)
    assert y.dtype == dtype and tuple(y.shape) == (N, 2 * H, 2 * W, C)
    assert torch.equal(y, SR.depth_to_space(x, 2))
    # the formula itself at a few points: out[n, h*r+i, w*r+j, c] = in[n, h, w, (i*r+j)*C + c]
    for (n, h, w, i, j, c) in [(0, 0, 0, 0, 0, 0), (N - 1, H - 1, W - 1, 1, 1, C - 1), (N - 1, H // 2, W - 1, 1, 0, 3)]:
        assert y[n, 2 * h + i, 2 * w + j, c] == x[n, h, w, (2 * i + j) * C + c]
    back = Fn.space_to_depth(y, 2)
    assert torch.equal(back, x)
    yy = torch.randn(N, 2 * H, 2 * W, C, generator=g).to(dtype).cuda()
    assert torch.equal(Fn.space_to_depth(yy, 2), SR.space_to_depth(yy, 2))


def test_shuffle_kernels_other_block_sizes_and_a_large_tensor():
    Fn, _ = _hip()
    x = torch.randn(2, 3, 5, 9 * 8, device="cuda").to(torch.bfloat16)
    assert torch.equal(Fn.depth_to_space(x, 3), SR.depth_to_space(x, 3))
    assert torch.equal(Fn.space_to_depth(Fn.depth_to_space(x, 3), 3), x)
    big = torch.randn(64, 64, 64, 4 * 96, device="cuda").to(torch.bfloat16)       # more pieces than one grid sweep
    assert torch.equal(Fn.depth_to_space(big, 2), SR.depth_to_space(big, 2))
    assert torch.equal(Fn.space_to_depth(Fn.depth_to_space(big, 2), 2), big)


def test_shuffle_abi_rejects_bad_arguments():
    _, hip = _hip()
    L = hip.lib()
    x = torch.zeros(2, 4, 4, 32, device="cuda", dtype=torch.bfloat16)
    y = torch.zeros(2, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    s = hip.stream()
    assert L.bg_depth_to_space(x.data_ptr(), y.data_ptr(), hip.BF16, 2, 4, 4, 8, 2, s) == 0
    assert L.bg_depth_to_space(None, y.data_ptr(), hip.BF16, 2, 4, 4, 8, 2, s) == 1
    assert L.bg_depth_to_space(x.data_ptr(), y.data_ptr(), hip.BF16, 2, 4, 4, 4, 2, s) == 1      # bf16: C % 8
    assert L.bg_depth_to_space(x.data_ptr(), y.data_ptr(), 7, 2, 4, 4, 8, 2, s) == 1
    assert L.bg_space_to_depth(y.data_ptr(), x.data_ptr(), hip.BF16, 2, 4, 4, 8, 0, s) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- SubpixelConvFn against float64
def _pad_lo(k):
    return SR.subpixel_pad(k)[0]


def _run_fn(x, w, b, k, pad_mode, dtype=torch.float32, compute=None):
    """forward + backward through functional.SubpixelConvFn for dy = g; numpy y, dx, dw, db, g."""
    Fn, hip = _hip()
    prev = Fn.Precision.compute
    if compute is not None:
        Fn.Precision.compute = compute
    try:
        xt = torch.tensor(x, dtype=dtype, device="cuda", requires_grad=True)
        wt = torch.tensor(w, dtype=torch.float32, device="cuda", requires_grad=True)
        bt = torch.tensor(b, dtype=torch.float32, device="cuda", requires_grad=True)
        y = Fn.SubpixelConvFn.apply(xt, wt, bt, _pad_lo(k), pad_mode, 2)
        g = torch.tensor(np.random.default_rng(7).standard_normal(tuple(y.shape)), dtype=y.dtype, device="cuda")
        dx, dw, db = torch.autograd.grad(y, [xt, wt, bt], g)
        torch.cuda.synchronize()
        return t2n(y.float()), t2n(dx.float()), t2n(dw), t2n(db), t2n(g.float())
    finally:
        Fn.Precision.compute = prev


def _ref_fn(x, w, b, k, pad_mode, g, round_bf16=False):
    def r(a):
        t = torch.tensor(a, dtype=torch.float64)
        return t.to(torch.bfloat16).to(torch.float64) if round_bf16 else t
    xt, wt = r(x).requires_grad_(True), r(w).requires_grad_(True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    lo, hi = SR.subpixel_pad(k)
    xin = F.pad(xt.permute(0, 3, 1, 2), (lo, hi, lo, hi), mode="reflect" if pad_mode == REFLECT else "constant")
    y4 = F.conv2d(xin, wt.permute(3, 2, 0, 1)).permute(0, 2, 3, 1) + bt
    y = SR.depth_to_space(y4, 2)
    dx, dw = torch.autograd.grad(y, [xt, wt], r(g))                  # (the gradient is a rounded operand too)
    # (the bias gradient is a plain sum of the unrounded dy, in the conv's channel order)
    db = SR.space_to_depth(torch.tensor(g, dtype=torch.float64), 2).sum(dim=(0, 1, 2))
    return y.detach().numpy(), dx.numpy(), dw.numpy(), db.numpy()


def _case(rng, N, H, W, cin, C, k):
    x = rng.standard_normal((N, H, W, cin))
    w = rng.standard_normal((k, k, cin, 4 * C)) / np.sqrt(k * k * cin)
    b = rng.standard_normal(4 * C)
    return x, w, b


def _check(got, ref, tol):
    for name, a, r_ in zip(("y", "dx", "dw", "db"), got[:4], ref):
        e = rel_err(a, r_)
        print("%s rel err %.3e (tol %.0e)" % (name, e, tol))
        assert e < tol, (name, e)


MAPS = [(4, 4), (5, 7), (32, 32)]


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("pad_mode", [REFLECT, ZERO])
@pytest.mark.parametrize("k", [2, 3])
def test_subpixel_conv_fp32_against_float64(k, pad_mode, H, W):
    rng = np.random.default_rng(100 * k + 10 * pad_mode + H)
    x, w, b = _case(rng, 2, H, W, 16, 8, k)
    got = _run_fn(x, w, b, k, pad_mode)
    assert got[0].shape == (2, 2 * H, 2 * W, 8)
    _check(got, _ref_fn(x, w, b, k, pad_mode, got[4]), 1e-5)


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("pad_mode", [REFLECT, ZERO])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("dtype,compute", [(torch.bfloat16, None), (torch.float32, 1)])
def test_subpixel_conv_bf16_against_float64(dtype, compute, k, pad_mode, H, W):
    """bf16 MFMA with the operands rounded in the reference: bf16-resident tensors (the fused store where the launch has
    it, conv + shuffle elsewhere) and the bf16-staged arithmetic on fp32 tensors."""
    rng = np.random.default_rng(200 * k + 10 * pad_mode + H)
    x, w, b = _case(rng, 4, H, W, 64, 16, k)
    got = _run_fn(x, w, b, k, pad_mode, dtype, compute)
    _check(got, _ref_fn(x, w, b, k, pad_mode, got[4], round_bf16=True), 1e-2)


# ---------------------------------------------------------------- fused store
def _desc(hip, N, H, cin, C, k, pad_mode):
    return hip.conv_desc(N, H, H, cin, H, H, 4 * C, k, 1, _pad_lo(k), pad_mode, hip.COMPUTE_BF16, hip.BF16, hip.BF16, 1)


@pytest.mark.parametrize("k", [2, 3])
def test_fused_store_is_supported_for_config3_shapes(k):
    """BASELINE config 3 (128^2, ch 96, batch 256): the up-sampling convs on the 32 x 32 (384 -> 4 x 192) and 64 x 64
    (192 -> 4 x 96) maps must take the fused store - it cannot silently go unused."""
    _, hip = _hip()
    L = hip.lib()
    for H, cin, C in ((32, 384, 192), (64, 192, 96)):
        for pad_mode in (REFLECT, ZERO):
            assert L.bg_conv2d_fwd_d2s_supported(_desc(hip, 256, H, cin, C, k, pad_mode), 2) == 1, (H, cin, C, pad_mode)


FUSED_SHAPES = [(8, 32, 384, 192), (4, 64, 192, 96), (16, 16, 64, 32), (32, 8, 64, 16), (32, 4, 64, 8), (2, 48, 32, 24),
                (256, 32, 384, 192)]


@pytest.mark.parametrize("N,H,cin,C", FUSED_SHAPES)
@pytest.mark.parametrize("pad_mode", [REFLECT, ZERO])
@pytest.mark.parametrize("k", [2, 3])
def test_fused_store_is_bit_identical_to_conv_plus_shuffle(k, pad_mode, N, H, cin, C):
    Fn, hip = _hip()
    L = hip.lib()
    d = _desc(hip, N, H, cin, C, k, pad_mode)
    supported = L.bg_conv2d_fwd_d2s_supported(d, 2)
    print("N%d H%d Cin%d C%d k%d pad_mode %d: supported %d" % (N, H, cin, C, k, pad_mode, supported))
    g = torch.Generator(device="cpu").manual_seed(N + H + k)
    x = torch.randn(N, H, H, cin, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(k, k, cin, 4 * C, generator=g) / np.sqrt(k * k * cin)).cuda()
    b = torch.randn(4 * C, generator=g).cuda()
    with torch.no_grad():
        with _env(BG_FUSE_D2S="0"):
            ref = Fn.SubpixelConvFn.apply(x, w, b, _pad_lo(k), pad_mode, 2)
        with _env(BG_FUSE_D2S="1"):
            got = Fn.SubpixelConvFn.apply(x, w, b, _pad_lo(k), pad_mode, 2)
            again = Fn.SubpixelConvFn.apply(x, w, b, _pad_lo(k), pad_mode, 2)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (N, 2 * H, 2 * H, C)
    assert torch.equal(got, ref)
    assert torch.equal(got, again)
    if supported:
        # the raw entry point, against the raw pair of the same launch
        pt = Fn.weight_packs(w)[1]
        y4 = torch.empty(N, H, H, 4 * C, dtype=torch.bfloat16, device="cuda")
        ws, nb = hip.scratch(L.bg_conv2d_fwd_workspace_bytes, d, x.device)
        hip.check(L.bg_conv2d_fwd(d, hip.act(x), hip.act(pt), hip.f32(b), None, hip.act(y4), 0, hip.f32(ws), nb,
                                  hip.stream()))
        y = torch.full((N, 2 * H, 2 * H, C), float("nan"), dtype=torch.bfloat16, device="cuda")
        hip.check(L.bg_conv2d_fwd_d2s(d, hip.act(x), hip.act(pt), hip.f32(b), None, hip.act(y), 2, None, 0, hip.stream()))
        assert torch.equal(y, Fn.depth_to_space(y4, 2))
        assert torch.equal(y, got)
    else:
        y = torch.zeros(N, 2 * H, 2 * H, C, dtype=torch.bfloat16, device="cuda")
        pt = Fn.weight_packs(w)[1]
        assert L.bg_conv2d_fwd_d2s(d, hip.act(x), hip.act(pt), hip.f32(b), None, hip.act(y), 2, None, 0,
                                   hip.stream()) == 1                      # refused before any launch
    torch.cuda.synchronize()


def test_backward_is_the_same_with_and_without_the_fused_store():
    Fn, hip = _hip()
    g = torch.Generator(device="cpu").manual_seed(3)
    x0 = torch.randn(8, 32, 32, 64, generator=g).to(torch.bfloat16).cuda()
    w0 = (torch.randn(3, 3, 64, 128, generator=g) / 24.0).cuda()
    dy = torch.randn(8, 64, 64, 32, generator=g).to(torch.bfloat16).cuda()
    outs = []
    for flag in ("0", "1"):
        with _env(BG_FUSE_D2S=flag):
            x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
            y = Fn.SubpixelConvFn.apply(x, w, None, 1, REFLECT, 2)
            outs.append((y.detach(),) + torch.autograd.grad(y, [x, w], dy))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- whole step
STEP_CASES = [
    (64, dict(upsampling_method="subpixel3")),
    (64, dict(upsampling_method="subpixel2")),
    (64, dict(upsampling_method="subpixel3", deep=True)),
    (64, dict(upsampling_method="subpixel3", conv_padding="zero")),
    (64, dict(downsampling_method="resize_conv35")),
    (64, dict(upsampling_method="subpixel2", downsampling_method="resize_conv35")),
]


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_step_parity(monkeypatch, case):
    size, flags = STEP_CASES[case]
    SR.install(monkeypatch)
    tr = SR.trainer(img_size=size, ch=8, z_dim=64, batch_size=4, **flags)
    gan = hip_model_like(tr, **flags)
    assert set(gan.store.vars) == set(tr.vs.vars)
    batch = RM.synthetic_batch(tr.cfg, 61 + case, 4)
    _run_parity(tr, gan, batch)


def test_sample_with_ema_weights(monkeypatch):
    SR.install(monkeypatch)
    flags = dict(upsampling_method="subpixel3")
    tr = SR.trainer(img_size=64, ch=8, z_dim=64, batch_size=2, **flags)
    gan = hip_model_like(tr, **flags)
    batch = RM.synthetic_batch(tr.cfg, 41, 2)
    tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"])
    tr.g_step(batch["z_g"], batch["aug_fake_g"])
    gan.d_step(cu(batch["real"]), cu(batch["z_d"]), dev_draws(batch["aug_real"]), dev_draws(batch["aug_fake_d"]))
    gan.g_step(2, cu(batch["z_g"]), dev_draws(batch["aug_fake_g"]))
    k = "generator/resblock_up_2/skip/subpixel_conv_0/kernel"
    assert not np.array_equal(t2n(gan.g_arena.view(gan.g_arena.ema, k)), t2n(gan.store.vars[k]))
    z = RM.truncated_normal(np.random.default_rng(5), (2, 1, 1, tr.cfg.z_dim))
    ref = tr.sample(z)
    img = gan.sample(cu(z))
    assert rel_err(t2n(img), ref.numpy()) < 1e-4


@pytest.mark.parametrize("flags", [dict(upsampling_method="subpixel3", downsampling_method="resize_conv35"),
                                   dict(upsampling_method="subpixel2")])
def test_hip_graph_replay_matches_eager(flags):
    from biggan_tensorflow_amd import model, scope as S, functional as Fn
    try:
        gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, n_labels=0, **flags),
                           store=S.VariableStore("cuda", seed=5)).build_model()
        data = [gan.synthetic_batch(4) for _ in range(2)]
        snap = gan.state_tensors()
        saved = {k: v.detach().clone() for k, v in snap.items()}
        rng = gan.gen.get_state()
        eager = []
        for real in data:
            l = gan.train_step(real)
            eager.append((l["d_loss"].item(), l["g_loss"].item()))
        with torch.no_grad():
            for k, v in snap.items():
                v.copy_(saved[k])
        gan.counter, gan.d_arena.step, gan.g_arena.step = 0, 0, 0
        gan.capture_graphs()
        assert gan._graphs_ready
        gan.gen.set_state(rng)
        for real, (de, ge) in zip(data, eager):
            l = gan.train_step(real)
            assert abs(l["d_loss"].item() - de) <= 1e-5 * abs(de) and abs(l["g_loss"].item() - ge) <= 1e-5 * abs(ge)
    finally:
        Fn.set_precision("fp32")


@pytest.mark.parametrize("flags", [dict(upsampling_method="subpixel2"),
                                   dict(upsampling_method="subpixel3", downsampling_method="resize_conv35")])
def test_bf16_step_config3_topology(flags):
    """BASELINE config 3's topology (128^2, ch 96, bf16-resident) at batch 4: the bf16 step against the same model in fp32
    within the bf16 gate of tests/test_gpu_bf16.py (losses and images 2e-2 relative; gradients 4e-1 relative L2)."""
    from biggan_tensorflow_amd import model, scope as S, functional as Fn
    kw = dict(img_size=128, ch=96, batch_size=4, **flags)
    try:
        g32 = model.BigGAN(make_args(**kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16 = model.BigGAN(make_args(precision="bf16", **kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16.store.load_arrays(g32.store.export_arrays())
        torch.manual_seed(0)
        z = torch.randn(4, 1, 1, g32.z_dim, device="cuda").clamp_(-2, 2)
        names = ["generator/resblock_up_16/res1/subpixel_conv_0/kernel", "generator/resblock_up_1/skip/subpixel_conv_0/kernel",
                 "generator/resblock_up_2/res1/subpixel_conv_0/kernel", "generator/resblock_up_4/res2/deconv_0/kernel"]
        outs = []
        for g in (g32, g16):
            o = g.g_step(4, z, None, apply=False)
            grads = {k: t2n(g.store.vars[k].bg_grad).copy() for k in names}
            outs.append((o["g_loss"].item(), t2n(o["fake"]) if "fake" in o else None, grads))
            torch.cuda.synchronize()
        (l32, f32_, g32s), (l16, f16_, g16s) = outs
        print("g_loss fp32 %.6f bf16 %.6f" % (l32, l16))
        assert abs(l16 - l32) <= 2e-2 * max(abs(l32), 1e-6), (l16, l32)
        if f32_ is not None:
            assert rel_err(f16_, f32_) < 2e-2
        for k in g32s:
            print(k, rel_err(g16s[k], g32s[k]))
            assert np.isfinite(g16s[k]).all() and rel_err(g16s[k], g32s[k]) < 4e-1, (k, rel_err(g16s[k], g32s[k]))
        if "downsampling_method" in flags:                 # the discriminator's mixed 3x3 / 5x5 skip convs in both modes
            real = torch.rand(4, 128, 128, 3, device="cuda") * 2.0 - 1.0      # (not from a model's own generator)
            dnames = ["discriminator/resblock_down_1/skip/conv_0/conv5_slice/kernel",
                      "discriminator/resblock_down_4/skip/conv_0/conv3_slice/kernel"]
            douts = []
            for g in (g32, g16):
                o = g.d_step(real, z, None, None, apply=False)
                douts.append((o["d_loss"].item(), {k: t2n(g.store.vars[k].bg_grad).copy() for k in dnames}))
                torch.cuda.synchronize()
            (d32, dg32), (d16, dg16) = douts
            print("d_loss fp32 %.6f bf16 %.6f" % (d32, d16))
            assert abs(d16 - d32) <= 2e-2 * max(abs(d32), 1e-6), (d16, d32)
            for k in dnames:
                print(k, rel_err(dg16[k], dg32[k]))
                assert np.isfinite(dg16[k]).all() and rel_err(dg16[k], dg32[k]) < 4e-1, (k, rel_err(dg16[k], dg32[k]))
    finally:
        Fn.set_precision("fp32")


def test_resize_conv35_has_no_gradient_penalty_pass():
    """The multi-branch convolution has no tangent pass: under the gradient-penalty gan_types resize_conv35 keeps raising."""
    from biggan_tensorflow_amd import main as M, model, scope as S
    args = M.parse_args(["--gan_type", "wgan-gp", "--img_size", "64", "--ch", "8", "--batch_size", "2", "--z_dim", "64",
                         "--downsampling_method", "resize_conv35"], make_dirs=False)
    gan = model.BigGAN(args, store=S.VariableStore("cuda", seed=1)).build_model()
    real = gan.synthetic_batch(2)
    with pytest.raises(NotImplementedError):
        gan.train_step(real)
