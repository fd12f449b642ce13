"""Sub-pixel up-sampling (--upsampling_method subpixel2 / subpixel3, ops.py:23-27, 207-210) and the mixed 3x3 / 5x5
down-sampling conv (--downsampling_method resize_conv35, ops.py:281-285): the float64 restatement in
tests/subpixel_ref.py against the formulas, the ops boundary and the variable manifest.  No GPU."""
import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, model, ops, scope as S
from oracle import kat
from oracle import ref_model as RM
from oracle import ref_ops as R
from tests import subpixel_ref as SR


def _argv(size, *extra):
    return M.parse_args(["--gan_type", "hinge", "--img_size", str(size), "--ch", "8"] + list(extra), make_dirs=False)


def _build(size, *extra):
    ops.begin_run()                     # (forget the regularisers earlier tests' shape passes registered)
    store = S.VariableStore("cpu")
    gan = model.BigGAN(_argv(size, *extra), device="cpu", store=store).build_model()
    return gan, {k: tuple(v.shape) for k, v in store.vars.items()}


def test_depth_to_space_is_the_formula():
    """out[n, h*r+i, w*r+j, c] = in[n, h, w, (i*r+j)*C + c], evaluated by four loops."""
    N, H, W, C, r = 2, 3, 5, 4, 2
    x = np.random.default_rng(0).standard_normal((N, H, W, r * r * C))
    want = np.zeros((N, H * r, W * r, C))
    for h in range(H):
        for w in range(W):
            for i in range(r):
                for j in range(r):
                    want[:, h * r + i, w * r + j, :] = x[:, h, w, (i * r + j) * C:(i * r + j + 1) * C]
    xt = torch.tensor(x)
    got = SR.depth_to_space(xt, r)
    assert np.array_equal(got.numpy(), want)
    # not torch's pixel_shuffle channel order (c * r^2 + i * r + j)
    ps = torch.nn.functional.pixel_shuffle(xt.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1)
    assert not np.array_equal(ps.numpy(), want)


def test_space_to_depth_is_the_inverse_and_the_adjoint():
    rng = np.random.default_rng(1)
    x = torch.tensor(rng.standard_normal((2, 3, 5, 16)), requires_grad=True)
    y = SR.depth_to_space(x, 2)
    assert torch.equal(SR.space_to_depth(y, 2), x)
    g = torch.tensor(rng.standard_normal(tuple(y.shape)))
    (dx,) = torch.autograd.grad(y, x, g)
    assert torch.equal(dx, SR.space_to_depth(g, 2))
    yy = torch.tensor(rng.standard_normal((2, 6, 10, 4)))
    assert torch.equal(SR.depth_to_space(SR.space_to_depth(yy, 2), 2), yy)


@pytest.mark.parametrize("padding", ["reflect", "zero"])
@pytest.mark.parametrize("kernel", [2, 3])
def test_restatement_padding_against_explicit_pad_and_valid_conv(padding, kernel):
    """pad = (k-1)/2.0 through ops.py:68-76: k = 2 pads 0 low and 1 high (reflect and TF 'SAME' alike), k = 3 pads 1 / 1;
    the map size is kept."""
    assert SR.subpixel_pad(2) == (0, 1) and SR.subpixel_pad(3) == (1, 1)
    assert kat.same_padding(6, 2, 1) == (6, 0, 1) and kat.same_padding(6, 3, 1) == (6, 1, 1)
    rng = np.random.default_rng(2 + kernel)
    x = rng.standard_normal((2, 5, 5, 3))
    vs = R.VarStore(torch.float64, 0)
    opt = {"sn": False, "padding_type": padding}
    y = SR.subpixel_conv(vs, "generator/t", torch.tensor(x), 2, opt, kernel=kernel, scale=2, use_bias=False)
    assert tuple(y.shape) == (2, 10, 10, 2)
    w = vs.vars["generator/t/subpixel_conv_0/kernel"].detach().numpy()
    assert w.shape == (kernel, kernel, 3, 8)
    lo, hi = SR.subpixel_pad(kernel)
    if padding == "reflect":
        xp = kat.reflect_pad(x, lo, hi)
    else:
        xp = np.pad(x, ((0, 0), (lo, hi), (lo, hi), (0, 0)))
    want = SR.depth_to_space(torch.tensor(kat.conv2d_valid(xp, w, 1)), 2).numpy()
    assert np.abs(y.detach().numpy() - want).max() < 1e-12


@pytest.mark.parametrize("method,k", [("subpixel3", 3), ("subpixel2", 2)])
def test_model_builds_with_subpixel_upsampling(method, k):
    gan, m = _build(64, "--upsampling_method", method)
    # --img_size 64 --ch 8: resblock_up_8 maps 64 -> 64 channels
    p = "generator/resblock_up_8/"
    for br in ("res1", "skip"):
        assert m[p + br + "/subpixel_conv_0/kernel"] == (k, k, 64, 4 * 64)
        assert m[p + br + "/subpixel_conv_0/u"] == (1, 4 * 64)
        assert p + br + "/subpixel_conv_0/bias" not in m          # (the non-deep blocks pass use_bias=False)
        assert not any(n.startswith(p + br + "/deconv_0") for n in m)
    assert m["generator/resblock_up_1/res1/subpixel_conv_0/kernel"] == (k, k, 16, 4 * 8)
    assert p + "res1/subpixel_conv_0/kernel" in gan.store.reg_shapes
    assert gan.store.reg_shapes[p + "skip/subpixel_conv_0/kernel"] == (k, k, 64, 4 * 64)
    img = gan.generator(torch.empty(2, 1, 1, gan.z_dim, device="meta"))
    assert tuple(img.shape) == (2, 64, 64, 3)


@pytest.mark.parametrize("flags", [dict(upsampling_method="subpixel3"), dict(upsampling_method="subpixel2", deep=True),
                                   dict(downsampling_method="resize_conv35"),
                                   dict(upsampling_method="subpixel2", downsampling_method="resize_conv35")])
def test_manifest_matches_restatement(monkeypatch, flags):
    SR.install(monkeypatch)
    extra = []
    for k_, v in flags.items():
        extra += ["--" + k_, str(v)]
    _, mine = _build(64, "--z_dim", "128", *extra)
    tr = SR.trainer(img_size=64, ch=8, z_dim=128, batch_size=2, perturb=False, **flags)
    ref = {k_: tuple(v.shape) for k_, v in tr.vs.vars.items()}
    assert mine == ref


def test_resize_conv35_slices():
    """The two slices and their widths.  They live under the block's ``skip`` scope: resblock_down (ops.py:299-302) runs
    its residual path, ``res1``, with resize_conv3 whenever the method is not strided_conv3, and only the skip path with
    the method itself - so ``res1/conv_0`` keeps one plain 3x3 kernel and has no slices."""
    _, m = _build(64, "--downsampling_method", "resize_conv35")
    p = "discriminator/resblock_down_1/"
    channels = 8                                                  # --ch 8: the first block maps 3 -> 8
    c5 = int(channels * 0.333333333334)
    c3 = channels - c5
    assert (c3, c5) == SR.conv35_widths(channels) == (6, 2)
    assert m[p + "skip/conv_0/conv3_slice/kernel"] == (3, 3, 3, c3)
    assert m[p + "skip/conv_0/conv5_slice/kernel"] == (5, 5, 3, c5)
    assert m[p + "skip/conv_0/conv5_slice/u"] == (1, c5)
    # the residual path of a block uses resize_conv3 whenever the method is not strided_conv3 (ops.py:299-302)
    assert m[p + "res1/conv_0/kernel"] == (3, 3, 3, channels)
    assert not any(n.startswith(p + "res1/conv_0/conv") for n in m)
    assert m["discriminator/resblock_down_2/skip/conv_0/conv3_slice/kernel"] == (3, 3, 8, 16 - int(16 * 0.333333333334))


def test_subpixel_conv_on_a_meta_tensor():
    S.set_default_store(S.VariableStore("cpu"))
    opt = {"conv": {"sn": True, "padding_type": "reflect"}}
    x = torch.empty(3, 4, 6, 16, device="meta")
    with S.variable_scope("generator"):
        y = ops.subpixel_conv(x, 24, opt, kernel=3, scale=2, use_bias=True)
        y2 = ops.subpixel_conv(x, 8, opt, kernel=2, scale=2, use_bias=False, scope="k2")
    assert tuple(y.shape) == (3, 8, 12, 24) and tuple(y2.shape) == (3, 8, 12, 8)
    v = S.default_store().vars
    assert tuple(v["generator/subpixel_conv_0/kernel"].shape) == (3, 3, 16, 96)
    assert tuple(v["generator/subpixel_conv_0/u"].shape) == (1, 96)
    assert tuple(v["generator/subpixel_conv_0/bias"].shape) == (96,)
    assert tuple(v["generator/k2/kernel"].shape) == (2, 2, 16, 32) and "generator/k2/bias" not in v


def test_upconv_dispatch_and_cpu_tensors_still_raise():
    S.set_default_store(S.VariableStore("cpu"))
    opt = {"conv": {"sn": True}, "upsampling_method": "subpixel2"}
    with S.variable_scope("generator"):
        y = ops.upconv(torch.empty(2, 4, 4, 8, device="meta"), 8, opt, use_bias=False)
    assert tuple(y.shape) == (2, 8, 8, 8)
    assert tuple(S.default_store().vars["generator/subpixel_conv_0/kernel"].shape) == (2, 2, 8, 32)


def test_binding_lists_the_new_entry_points():
    for name in ("bg_depth_to_space", "bg_space_to_depth", "bg_conv2d_fwd_d2s", "bg_conv2d_fwd_d2s_supported"):
        assert name in hip.SIGNATURES
    L = hip.lib()
    assert L.bg_abi_version() == hip.ABI_VERSION >= 7
    # argument validation happens before any launch: NULL tensors and bad geometry are BG_ERR_ARG (1)
    assert L.bg_depth_to_space(None, None, hip.BF16, 2, 4, 4, 8, 2, None) == 1
    assert L.bg_space_to_depth(None, None, hip.F32, 2, 4, 4, 8, 2, None) == 1
    d = hip.conv_desc(256, 32, 32, 384, 32, 32, 768, 3, 1, 1, 0, hip.COMPUTE_BF16, hip.BF16, hip.BF16, 1)
    assert L.bg_conv2d_fwd_d2s(d, None, None, None, None, None, 2, None, 0, None) == 1
    # the query is host arithmetic: BASELINE config 3's 32 x 32 and 64 x 64 up-sampling inputs take the fused store
    for (h, cin, c), k, lo in [((32, 384, 192), 3, 1), ((64, 192, 96), 3, 1), ((32, 384, 192), 2, 0), ((64, 192, 96), 2, 0)]:
        d = hip.conv_desc(256, h, h, cin, h, h, 4 * c, k, 1, lo, 0, hip.COMPUTE_BF16, hip.BF16, hip.BF16, 1)
        assert L.bg_conv2d_fwd_d2s_supported(d, 2) == 1, (h, cin, c, k)
    f32 = hip.conv_desc(256, 32, 32, 384, 32, 32, 768, 3, 1, 1, 0)
    assert L.bg_conv2d_fwd_d2s_supported(f32, 2) == 0 and L.bg_conv2d_fwd_d2s_supported(d, 3) == 0
