"""The discriminator's reconstruction heads (--d_reconstruction, --d_reconstruction_halfres, --d_reconstruction_texture:
BigGAN.py:639-661, 744-762, 810-836): flags, attach rule, variable manifest, arenas, the float64 restatement in
tests/recon_ref.py against autograd and finite differences, its identity with the oracle when the flags are off, the new
C entry points, and a mutation check of the parity gate.  No GPU."""
import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, model, ops, scope as S
from oracle import ref_model as RM
from oracle import ref_ops as R
from tests import recon_ref as RR
from tests.test_gpu_step import _grad_err, _scale_ref

LOSS_TOL, GRAD_TOL = 1e-4, 1e-3          # the project's fp32 gates (tests/test_gpu_step.py)


def _argv(size, *extra):
    return M.parse_args(["--gan_type", "hinge", "--img_size", str(size), "--ch", "8"] + list(extra), make_dirs=False)


def _model(size, *extra):
    return model.BigGAN(_argv(size, *extra), device="cpu", store=S.VariableStore("cpu"))


def _build(size, *extra):
    ops.begin_run()
    gan = _model(size, *extra).build_model()
    return gan, {k: tuple(v.shape) for k, v in gan.store.vars.items()}


# ---------------------------------------------------------------- flags and the attach rule
@pytest.mark.parametrize("flag", ["d_reconstruction", "d_reconstruction_halfres", "d_reconstruction_texture"])
def test_model_constructs_with_each_flag(flag):
    gan = _model(64, "--" + flag, "true")
    assert gan.d_reconstruction == (flag != "d_reconstruction_texture")        # halfres implies the coarse head
    assert gan.d_reconstruction_halfres == (flag == "d_reconstruction_halfres")
    assert gan.d_reconstruction_texture == (flag == "d_reconstruction_texture")
    assert (gan.d_recon_ch, gan.d_recon_ld, gan.d_tex_recon_ch, gan.d_tex_recon_ld) == (64, 1.0, 96, 0.5)
    assert (gan.d_tex_recon_feat_size, gan.d_tex_recon_patch_div) == (16, 4)
    assert not gan.d_recon_bn_after_act and not gan.d_save_recon_samples


def test_d_final_conv_is_still_rejected():
    with pytest.raises(NotImplementedError):
        _model(64, "--d_final_conv", "true")


def test_missing_attach_size_is_a_value_error_naming_the_sizes():
    with pytest.raises(ValueError, match="256, 64, 32, 16, 4"):
        _model(512, "--d_reconstruction", "true")                  # no block group ends at 8 x 8
    with pytest.raises(ValueError, match="128, 64, 32, 8, 4"):
        _model(256, "--d_reconstruction_texture", "true")          # none ends at 16 x 16
    _model(256, "--d_reconstruction", "true")
    _model(512, "--d_reconstruction_texture", "true")
    with pytest.raises(ValueError):
        RR.plan(RR.config(img_size=512, ch=8, d_reconstruction=True))
    with pytest.raises(ValueError):
        RR.plan(RR.config(img_size=256, ch=8, d_reconstruction_texture=True))


@pytest.mark.parametrize("size", [64, 128, 256])
@pytest.mark.parametrize("halfres", [False, True])
def test_layer_counts_reach_the_target(size, halfres):
    """layers = log2(target / 8): the reference's depth - 3 (depth - 4) is one short unless --g_final_layer bumped depth."""
    gan = _model(size, "--d_reconstruction_halfres" if halfres else "--d_reconstruction", "true")
    plan = gan.recon_plan["coarse"]
    target = size // 2 if halfres else size
    assert plan["target"] == target and 8 * 2 ** plan["layers"] == target
    depth_bumped = gan.depth + 1                                   # BigGAN.py:30-31 with --g_final_layer
    assert plan["layers"] == depth_bumped - (4 if halfres else 3)
    ref = RR.plan(RR.config(img_size=size, ch=8, d_reconstruction=True, d_reconstruction_halfres=halfres))["coarse"]
    assert ref["layers"] == plan["layers"] and ref["target"] == target


def test_texture_geometry():
    gan = _model(128, "--d_reconstruction_texture", "true")
    assert gan.recon_plan["texture"] == {"size": 16, "patch": 32, "feat_patch": 4, "f": 8, "layers": 3}
    assert RR.plan(RR.config(img_size=128, ch=8, d_reconstruction_texture=True))["texture"] == gan.recon_plan["texture"]


# ---------------------------------------------------------------- variables
def _upscaler_manifest(prefix, cin, base, layers, c_dim):
    want = {}
    for li in range(layers):
        ch = base * 2 ** (layers - li - 1)
        p = "%s/upscale%d/" % (prefix, li)
        want[p + "conv_0/kernel"] = (3, 3, cin, 2 * ch)
        want[p + "conv_0/u"] = (1, 2 * ch)
        want[p + "conv_0/bias"] = (2 * ch,)
        for leaf in ("gamma", "beta", "moving_mean", "moving_variance"):
            want[p + "batch_norm/" + leaf] = (2 * ch,)
        cin = ch
    want[prefix + "/conv_0/kernel"] = (3, 3, cin, c_dim)
    want[prefix + "/conv_0/u"] = (1, c_dim)
    want[prefix + "/conv_0/bias"] = (c_dim,)
    return want


def test_manifest_lists_exactly_the_head_variables(monkeypatch):
    RR.install(monkeypatch)
    _, base = _build(64)
    gan, m = _build(64, "--d_reconstruction", "true", "--d_reconstruction_texture", "true")
    new = {k: v for k, v in m.items() if k not in base}
    assert {k: m[k] for k in base} == base                         # nothing else moved
    # 64 / ch 8: the 8 x 8 map has 8 * 2**2 channels, the 16 x 16 map 8 * 2**1
    want = _upscaler_manifest("discriminator/upscaler", 8 * 2 ** 2, 64, 3, 3)
    want.update(_upscaler_manifest("discriminator/tex_upscaler", 8 * 2 ** 1, 96, 2, 3))
    assert new == want
    assert m["discriminator/upscaler/upscale0/conv_0/kernel"] == (3, 3, 8 * 2 ** 2, 2 * 64 * 2 ** (3 - 1))
    # the restatement creates the same variables
    tr = RR.trainer(img_size=64, ch=8, z_dim=256, batch_size=2, d_reconstruction=True, d_reconstruction_texture=True)
    assert {k: tuple(v.shape) for k, v in tr.vs.vars.items()} == m
    # D variables, no regulariser (the scope has no 'generator' in it), D arena only
    assert all(k in gan.d_arena.offsets for k in want if not k.endswith(("/u", "moving_mean", "moving_variance")))
    assert not any("upscaler" in k for k in gan.g_arena.offsets)
    assert not any("upscaler" in k for k in gan.store.reg_shapes)
    assert all(k in gan.d_vars for k in want if k.endswith(("kernel", "bias", "gamma", "beta")))


def test_halfres_and_c_dim_change_the_shapes():
    _, m = _build(64, "--d_reconstruction_halfres", "true", "--c_dim", "4", "--d_recon_ch", "16")
    assert m["discriminator/upscaler/upscale0/conv_0/kernel"] == (3, 3, 32, 2 * 16 * 2)
    assert m["discriminator/upscaler/upscale1/conv_0/kernel"] == (3, 3, 32, 2 * 16)
    assert "discriminator/upscaler/upscale2/conv_0/kernel" not in m
    assert m["discriminator/upscaler/conv_0/kernel"] == (3, 3, 16, 4)


def test_batch_renorm_type_names_the_upscaler_statistics():
    _, m = _build(64, "--d_reconstruction_halfres", "true", "--bn_type", "batch_renorm")
    assert m["discriminator/upscaler/upscale0/batch_renorm/renorm_stddev"] == (256,)


def test_models_without_the_flags_are_unchanged():
    gan, m = _build(64)
    assert not gan.recon_plan and not any("upscaler" in k for k in m)


def test_glu_on_a_meta_tensor_and_odd_channels():
    assert tuple(ops.glu(torch.empty(2, 4, 4, 16, device="meta")).shape) == (2, 4, 4, 8)
    with pytest.raises(ValueError):
        ops.glu(torch.empty(2, 4, 4, 7, device="meta"))


# ---------------------------------------------------------------- the restatement's arithmetic
def test_glu_matches_the_formula_autograd_and_finite_differences():
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.standard_normal((2, 3, 3, 10)), requires_grad=True)
    y = RR.glu(x)
    want = x.detach().numpy()[..., :5] / (1.0 + np.exp(-x.detach().numpy()[..., 5:]))
    assert np.allclose(y.detach().numpy(), want, rtol=1e-14, atol=0)
    assert torch.autograd.gradcheck(RR.glu, (x,))
    # closed-form gradient: d main = dy s, d gate = dy main s (1 - s)
    g = torch.tensor(rng.standard_normal(tuple(y.shape)))
    (dx,) = torch.autograd.grad(y, x, g)
    s = torch.sigmoid(x.detach()[..., 5:])
    assert torch.allclose(dx[..., :5], g * s, rtol=1e-13, atol=0)
    assert torch.allclose(dx[..., 5:], g * x.detach()[..., :5] * s * (1 - s), rtol=1e-13, atol=1e-300)
    # central finite difference along a random direction
    d = torch.tensor(rng.standard_normal(tuple(x.shape)))
    h = 1e-6
    fd = ((RR.glu(x.detach() + h * d) - RR.glu(x.detach() - h * d)) * g).sum() / (2 * h)
    assert abs(fd.item() - (dx * d).sum().item()) <= 1e-7 * abs(fd.item())


@pytest.mark.parametrize("mode", ["identity", "halfres", "texture"])
def test_loss_gradient_matches_the_closed_form_and_finite_differences(mode):
    """d loss / d y = scale (tanh y - t) / ||tanh y - t|| (1 - tanh^2 y), the formula of the backward kernel."""
    rng = np.random.default_rng(3)
    cfg = RR.config(img_size=64, ch=8, d_reconstruction=True, d_reconstruction_halfres=mode == "halfres",
                    d_reconstruction_texture=mode == "texture")
    real = torch.tensor(rng.uniform(-1, 1, (2, 64, 64, 3)))
    if mode == "texture":
        target, ld = RR.texture_target(cfg, real, 12, 5), cfg.d_tex_recon_ld
        assert torch.equal(target, real[:, 48:64, 20:36, :])
    else:
        target, ld = RR.coarse_target(cfg, real), cfg.d_recon_ld
    if mode == "halfres":
        assert torch.allclose(target[1, 3, 5], real[1, 6:8, 10:12].mean(dim=(0, 1)), rtol=1e-15)
    y = torch.tensor(rng.standard_normal(tuple(target.shape)) * 0.5, requires_grad=True)

    def f(v):
        return RR.recon_loss(torch.tanh(v), target, ld)
    loss = f(y)
    t = torch.tanh(y.detach())
    norm = torch.sqrt(((t - target) ** 2).sum())
    assert abs(loss.item() - norm.item() / y.numel() * 1000.0 * ld) <= 1e-14 * loss.item()
    (dy,) = torch.autograd.grad(loss, y)
    want = (1000.0 * ld / y.numel()) * (t - target) / norm * (1 - t * t)
    assert torch.allclose(dy, want, rtol=1e-12, atol=1e-300)
    d = torch.tensor(rng.standard_normal(tuple(y.shape)))
    h = 1e-6
    fd = (f(y.detach() + h * d) - f(y.detach() - h * d)) / (2 * h)
    assert abs(fd.item() - (dy * d).sum().item()) <= 1e-6 * abs(fd.item())


def _d_step(tr, seed, offsets=None, B=None, **kw):
    batch = RM.synthetic_batch(tr.cfg, seed, B or tr.cfg.batch_size)
    if "gp" in batch:
        kw["gp"] = batch["gp"]
    if offsets is not None:
        kw["recon_offsets"] = offsets
    return tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"], apply=False, **kw), batch


def test_restatement_is_the_oracle_when_the_flags_are_off(monkeypatch):
    plain = RM.Trainer(RM.Config(img_size=64, ch=8, z_dim=64, batch_size=2), torch.float64, 42).build()
    RM.perturb_for_parity(plain.vs)
    batch = RM.synthetic_batch(plain.cfg, 11, 2)
    ref = plain.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"], apply=False)
    ref_g = plain.g_step(batch["z_g"], batch["aug_fake_g"], apply=False)
    RR.install(monkeypatch)
    tr = RR.trainer(img_size=64, ch=8, z_dim=64, batch_size=2)
    assert list(tr.vs.vars) == list(plain.vs.vars)
    got = tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"], apply=False)
    got_g = tr.g_step(batch["z_g"], batch["aug_fake_g"], apply=False)
    assert torch.equal(got["d_loss"], ref["d_loss"]) and torch.equal(got_g["g_loss"], ref_g["g_loss"])
    assert "d_recon" not in got and "d_tex_recon" not in got
    for k, g in ref["grads"].items():
        assert torch.equal(got["grads"][k], g), k
    for k, g in ref_g["grads"].items():
        assert torch.equal(got_g["grads"][k], g), k


@pytest.mark.parametrize("case", range(len(RR.PARITY_CASES)))
def test_parity_configurations_are_far_from_the_singular_point(monkeypatch, case):
    """At initialisation tanh(y) is near 0 and the targets are U(-1, 1): the norm the loss divides by is far above 1 for
    every whole-step parity configuration of tests/test_gpu_recon.py; every head variable gets a gradient; the G step does
    not see the heads."""
    name, flags, offsets = RR.PARITY_CASES[case]
    RR.install(monkeypatch)
    tr = RR.trainer(**dict(RR.PARITY_SHAPE, **flags))
    out, batch = _d_step(tr, 70 + case, offsets)
    real_aug = R.diffaugment(tr._t(batch["real"]), batch["aug_real"], tr.cfg.da_policy)
    total = out["d_loss"] - R.discriminator_loss(tr.cfg.gan_type, out["real_logits"], out["fake_logits"], tr.cfg.d_flood)
    if out.get("gp") is not None:
        total = total - out["gp"]
    want = 0.0
    if "coarse_upscaled" in out:
        norm = torch.sqrt(((out["coarse_upscaled"] - RR.coarse_target(tr.cfg, real_aug)) ** 2).sum()).item()
        print("%s: coarse norm %.3f, d_recon %.6f" % (name, norm, out["d_recon"].item()))
        assert norm > 1.0
        want = want + out["d_recon"]
    if "texture_upscaled" in out:
        norm = torch.sqrt(((out["texture_upscaled"] - RR.texture_target(tr.cfg, real_aug, *offsets)) ** 2).sum()).item()
        print("%s: texture norm %.3f, d_tex_recon %.6f" % (name, norm, out["d_tex_recon"].item()))
        assert norm > 1.0
        want = want + out["d_tex_recon"]
    assert abs(total.item() - want.item()) <= 1e-12 * abs(out["d_loss"].item())     # added after the flood
    for k, g in out["grads"].items():
        if "upscaler" in k:
            assert float(g.abs().max()) > 0, k
    g_out = tr.g_step(batch["z_g"], batch["aug_fake_g"], apply=False)
    assert not any("upscaler" in k for k in g_out["grads"])


# ---------------------------------------------------------------- C ABI
NEW_SYMBOLS = ("bg_bn_glu_fwd", "bg_bn_glu_bwd_reduce", "bg_bn_glu_bwd_dx", "bg_glu_fwd", "bg_glu_bwd", "bg_upsample2_fwd_t", "bg_upsample2_bwd_t", "bg_crop_at_fwd", "bg_crop_at_bwd",
               "bg_recon_loss_sums", "bg_recon_loss_finalize", "bg_recon_loss_bwd")


def test_library_exports_the_new_entry_points():
    for name in NEW_SYMBOLS:
        assert name in hip.SIGNATURES
    L = hip.lib()
    assert L.bg_abi_version() == hip.ABI_VERSION >= 8
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    # argument validation happens before any launch: NULL tensors are BG_ERR_ARG (1)
    assert L.bg_glu_fwd(None, None, hip.BF16, 16, 8, None) == 1
    assert L.bg_bn_glu_fwd(None, None, None, None, None, None, hip.F32, 16, 8, None) == 1
    assert L.bg_upsample2_fwd_t(None, None, hip.F32, 2, 4, 4, 8, None) == 1
    assert L.bg_crop_at_fwd(None, None, hip.BF16, None, None, 2, 16, 16, 4, 8, None) == 1
    assert L.bg_recon_loss_sums(None, None, None, None, None, 0, 1, None, 2, 8, 8, 8, 3, None) == 1
    assert L.bg_recon_loss_finalize(None, 1.0, None, None) == 1
    assert b"NULL" in L.bg_last_error()


# ---------------------------------------------------------------- the gate catches what it must
def _gate(ref, got):
    """The whole-D-step comparison of tests/test_gpu_recon.py: losses 1e-4 relative, every D gradient 1e-3 relative L2
    with the error measure of tests/test_gpu_step.py (a bias in front of a batch norm has an exactly vanishing gradient and
    is measured against its kernel's).  -> list of what is outside."""
    bad = []
    for key in ("d_loss", "d_recon", "d_tex_recon"):
        if key in ref:
            a, b = float(got[key].detach()), float(ref[key].detach())
            if abs(a - b) > LOSS_TOL * max(abs(b), 1e-6):
                bad.append(key)
    for k, g in ref["grads"].items():
        tol = 5e-2 if k.endswith("self_attention/gamma") else GRAD_TOL
        if _grad_err(got["grads"][k].double().numpy(), g.numpy(), _scale_ref(k, ref["grads"])) > tol:
            bad.append(k)
    return bad


def _swapped_glu(x):
    c = x.shape[-1] // 2
    return x[..., c:] * torch.sigmoid(x[..., :c])


def _crop_off_by_one(x, oy, ox, p):
    return x[:, oy:oy + p, max(ox - 1, 0):max(ox - 1, 0) + p, :] if ox > 0 else x[:, oy:oy + p, 1:1 + p, :]


def _per_sample_norm(img, target, ld):
    n = img.shape[0]
    per = torch.sqrt(((img - target) ** 2).reshape(n, -1).sum(dim=1))
    return per.mean() * (1.0 / (img.numel() // n)) * 1000.0 * ld


MUTATIONS = {"swapped gate half": ("glu", _swapped_glu), "crop off by one": ("crop", _crop_off_by_one),
             "per-sample norm": ("recon_loss", _per_sample_norm)}


def _both_heads(dtype=torch.float64):
    _, flags, offsets = RR.PARITY_CASES[3]
    return RR.trainer(dtype=dtype, **dict(RR.PARITY_SHAPE, **flags)), offsets


def test_gate_accepts_a_single_precision_run(monkeypatch):
    """The same restatement evaluated in float32 - the arithmetic precision of the product - is inside the gate."""
    RR.install(monkeypatch)
    tr, offsets = _both_heads()
    ref, _ = _d_step(tr, 73, offsets)
    tr32, _ = _both_heads(torch.float32)
    got, _ = _d_step(tr32, 73, offsets)
    bad = _gate(ref, got)
    assert not bad, bad


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_gate_rejects(monkeypatch, mut):
    RR.install(monkeypatch)
    tr, offsets = _both_heads()
    ref, _ = _d_step(tr, 73, offsets)
    attr, fn = MUTATIONS[mut]
    monkeypatch.setattr(RR, attr, fn)
    got, _ = _d_step(tr, 73, offsets)
    bad = _gate(ref, got)
    print("mutation %-20s rejected: %d quantities outside the gate, e.g. %s" % (mut, len(bad), bad[:3]))
    assert bad
    if mut == "per-sample norm":
        assert "d_recon" in bad and "d_tex_recon" in bad
    if mut == "crop off by one":
        assert "d_tex_recon" in bad and "d_recon" not in bad
