"""Float64 torch-CPU restatement of the discriminator's reconstruction heads (--d_reconstruction,
--d_reconstruction_halfres, --d_reconstruction_texture: BigGAN.py:639-661, 744-762, 810-836, 885-889), built from
``oracle.ref_ops`` primitives: ``glu`` (ops.py:842-845), ``simple_upscale`` / ``simple_upscaler``, the two L2-norm
losses, the attach rule and the layer counts.

``install(monkeypatch)`` puts a reconstruction-aware ``discriminator`` over ``RM.discriminator`` and reconstruction-aware
``d_forward`` / ``d_step`` over the ``Trainer``'s, on top of ``tests/rgba_ref.py`` and ``tests/subpixel_ref.py`` (and
through them the mixed-block and latent-stage restatements).  Configurations without the flags are handed on to what was
installed before, unchanged.  The new attributes are set on the ``Config`` after construction (``config()``).

Stated deviations from the reference (reconstruction heads): the layer count is log2(target / 8) (the
reference's ``depth - 3`` only reaches the target after --g_final_layer has bumped ``depth``); each head works alone; a
missing attach size is a ValueError; the heads run in the real call of the D step only.
"""
import math

import torch

from oracle import ref_model as RM
from oracle import ref_ops as R
from tests import mixed_ref as MR
from tests import rgba_ref as AR
from tests import subpixel_ref as SR

RECON_FLAGS = dict(d_reconstruction=False, d_reconstruction_halfres=False, d_reconstruction_texture=False,
                   d_recon_ch=64, d_recon_ld=1.0, d_tex_recon_ld=0.5, d_tex_recon_ch=96, d_tex_recon_feat_size=16,
                   d_tex_recon_patch_div=4, d_recon_bn_after_act=False)


# the whole-D-step parity configurations (tests/test_gpu_recon.py; tests/test_recon.py checks on the CPU that each one
# is far from the norm's singular point): (flags of both sides, (ro_x[0], ro_y[0]) = (height, width) feature offsets).
# 64 x 64, ch 8: the coarse head sits on the 8 x 8 map (3 layers to 64, 2 to 32), the texture head on the 16 x 16 map
# (4 x 4 feature crop -> 16 x 16 patch, offsets 0 ... 12: both extremes occur).
_SMALL = dict(d_recon_ch=16, d_tex_recon_ch=24)
PARITY_CASES = [
    ("coarse", dict(d_reconstruction=True, **_SMALL), (0, 0)),
    ("halfres", dict(d_reconstruction_halfres=True, **_SMALL), (0, 0)),
    ("texture", dict(d_reconstruction_texture=True, **_SMALL), (12, 0)),
    ("both", dict(d_reconstruction_halfres=True, d_reconstruction_texture=True, **_SMALL), (5, 9)),
    ("bn_after_act", dict(d_reconstruction_halfres=True, d_reconstruction_texture=True, d_recon_bn_after_act=True,
                          **_SMALL), (0, 12)),
    ("c_dim4", dict(d_reconstruction_halfres=True, d_reconstruction_texture=True, c_dim=4, **_SMALL), (3, 12)),
    ("wgan-gp", dict(d_reconstruction_halfres=True, d_reconstruction_texture=True, gan_type="wgan-gp", **_SMALL), (12, 12)),
    ("bn_in_d", dict(d_reconstruction_halfres=True, d_reconstruction_texture=True, bn_in_d=True, **_SMALL), (7, 2)),
    ("c_dim1", dict(d_reconstruction_halfres=True, d_reconstruction_texture=True, c_dim=1, **_SMALL), (1, 11)),
]
PARITY_SHAPE = dict(img_size=64, ch=8, z_dim=64, batch_size=4)


def config(**kw):
    new = {k: kw.pop(k) for k in list(kw) if k in RECON_FLAGS}
    rgba = {k: kw.pop(k) for k in list(kw) if k in AR.RGBA_FLAGS}
    cfg = SR.config(**kw)
    for k, v in AR.RGBA_FLAGS.items():
        setattr(cfg, k, rgba.get(k, v))
    for k, v in RECON_FLAGS.items():
        setattr(cfg, k, new.get(k, v))
    if cfg.d_reconstruction_halfres:
        cfg.d_reconstruction = True
    return cfg


def trainer(dtype=torch.float64, seed=42, perturb=True, **kw):
    tr = RM.Trainer(config(**kw), dtype, seed).build()
    if perturb:
        RM.perturb_for_parity(tr.vs)
        for k, p in tr.g_params().items():
            tr.ema[k] = p.detach().clone()
    return tr


def heads_on(cfg):
    return bool(getattr(cfg, "d_reconstruction", False) or getattr(cfg, "d_reconstruction_halfres", False)
                or getattr(cfg, "d_reconstruction_texture", False))


# ---------------------------------------------------------------- attach rule and layer counts
def group_sizes(cfg):
    """Side of the feature map after each block group of the discriminator (BigGAN.py:607-611, 624-664)."""
    sizes, s = [], cfg.img_size
    for count in cfg.d_block_info()["counts"]:
        s //= 2 ** count
        sizes.append(s)
    return sizes


def plan(cfg):
    """{"coarse": {size, target, layers}, "texture": {size, patch, feat_patch, f, layers}} for the heads that are on."""
    out = {}
    if not heads_on(cfg):
        return out
    sizes = group_sizes(cfg)
    if cfg.d_reconstruction or cfg.d_reconstruction_halfres:
        if 8 not in sizes:
            raise ValueError("no block group ends at 8x8: " + str(sizes))
        target = cfg.img_size // 2 if cfg.d_reconstruction_halfres else cfg.img_size
        out["coarse"] = dict(size=8, target=target, layers=int(math.log2(target // 8)))
    if cfg.d_reconstruction_texture:
        fs, div = cfg.d_tex_recon_feat_size, cfg.d_tex_recon_patch_div
        if fs not in sizes:
            raise ValueError("no block group ends at %dx%d: %s" % (fs, fs, sizes))
        patch, feat_patch = cfg.img_size // div, fs // div
        out["texture"] = dict(size=fs, patch=patch, feat_patch=feat_patch, f=cfg.img_size // fs,
                              layers=int(math.log2(patch // feat_patch)))
    return out


# ---------------------------------------------------------------- the arithmetic
def glu(x):
    """ops.py:842-845: the first half of the channels gated by the sigmoid of the second."""
    c = x.shape[-1] // 2
    return x[..., :c] * torch.sigmoid(x[..., c:])


def crop(x, oy, ox, p):
    """tf.image.crop_to_bounding_box(x, offset_height, offset_width, p, p)."""
    return x[:, oy:oy + p, ox:ox + p, :]


def simple_upscale(vs, scope, x, ch, opt, cfg):
    """BigGAN.py:744-753.  With bf16 rounding on, every tensor the product stores is rounded where it stores it: the
    conv output and the glu output (up_sample is an exact copy; in the default order batch norm and glu are one kernel,
    so nothing is stored between them), with --d_recon_bn_after_act the batch-norm output."""
    x = R.up_sample(x)
    x = R.conv(vs, scope + "/conv_0", x, ch * 2, opt, kernel=3, stride=1, pad=1, use_bias=True)
    if not cfg.d_recon_bn_after_act:
        x = R.batch_norm(vs, scope + "/batch_norm", x, opt, True)
    x = R.r_act(glu(x))
    if cfg.d_recon_bn_after_act:
        x = R.r_act(R.batch_norm(vs, scope + "/batch_norm", x, opt, True))
    return x


def simple_upscaler(vs, scope, x, layers, base_width, opt, cfg):
    """BigGAN.py:755-762 -> the image after tanh."""
    for li in range(layers):
        x = simple_upscale(vs, scope + "/upscale" + str(li), x, base_width * 2 ** (layers - li - 1), opt, cfg)
    if cfg.c_dim == 1 and not R.ROUND.on:
        # (torch's CPU conv2d backward wants a contiguous weight for one output channel: tests/rgba_ref.py)
        y = MR.conv_dilated(vs, scope + "/conv_0", x, cfg.c_dim, opt, 3, 1, 1, True)
    else:
        y = R.conv(vs, scope + "/conv_0", x, cfg.c_dim, opt, kernel=3, stride=1, pad=1, use_bias=True)
    return torch.tanh(y)


def recon_loss(img, target, ld):
    """BigGAN.py:815-817: the Frobenius norm over the WHOLE batch tensor / numel * 1000 * ld."""
    return torch.sqrt(((img - target) ** 2).sum()) * (1.0 / img.numel()) * 1000.0 * ld


def coarse_target(cfg, real_aug):
    return R.avg_pooling(real_aug) if cfg.d_reconstruction_halfres else real_aug


def texture_target(cfg, real_aug, oy, ox):
    p = plan(cfg)["texture"]
    return crop(real_aug, oy * p["f"], ox * p["f"], p["patch"])


# ---------------------------------------------------------------- discriminator with the heads
def _discriminator_with_heads(vs, cfg, x, offsets):
    """RM.discriminator (BigGAN.py:591-715, default branches) with the heads after the block groups (639-661)."""
    opt = RM._conv_opt(cfg, True, False)
    D = "discriminator"
    pl = plan(cfg)
    out = {}
    if AR._mask_on(cfg):
        x = AR.alpha_mask(x)
    info = cfg.d_block_info()
    ch = cfg.scale_channels(cfg.d_ch, cfg.d_grow_factor ** 0)
    b_i, ch_mul = 0, 1
    for block_count in info["counts"]:
        scope = "resblock_down_" + str(ch_mul)
        for sb_i in range(block_count):
            if block_count > 1:
                scope = scope + "_" + str(sb_i)
            if cfg.deep:
                x = R.resblock_down_deep(vs, D + "/" + scope, x, ch, opt, True, cfg.bias_in_d)
                x = R.resblock_down_deep(vs, D + "/" + scope + "_2", x, ch, opt, False, cfg.bias_in_d)
            else:
                x = R.resblock_down(vs, D + "/" + scope, x, ch, opt, use_bias=cfg.bias_in_d)
        b_i += 1
        if b_i == info["sa_index"]:
            x = R.self_attention_2(vs, D + "/self_attention", x, ch, opt)
        if "coarse" in pl and x.shape[1] == pl["coarse"]["size"]:
            out["coarse_upscaled"] = simple_upscaler(vs, D + "/upscaler", x, pl["coarse"]["layers"], cfg.d_recon_ch, opt,
                                                     cfg)
        if "texture" in pl and x.shape[1] == pl["texture"]["size"]:
            oy, ox = offsets
            feat = crop(x, oy, ox, pl["texture"]["feat_patch"])
            out["texture_upscaled"] = simple_upscaler(vs, D + "/tex_upscaler", feat, pl["texture"]["layers"],
                                                      cfg.d_tex_recon_ch, opt, cfg)
        ch = cfg.scale_channels(cfg.d_ch, cfg.d_grow_factor ** b_i)
        ch_mul *= 2
    ch = cfg.scale_channels(cfg.d_ch, cfg.d_grow_factor ** (b_i - 1))
    x = R.resblock(vs, D + "/resblock", x, ch, opt, use_bias=cfg.bias_in_d)
    x = R.activation(vs, D + "/prelu", x, opt)
    feat = R.global_sum_pooling(x)
    out["real"] = R.fully_connected(vs, D + "/D_logit", feat, 1, opt, sn=cfg.d_compat_use_sn_in_critic_output)
    if cfg.n_labels > 0:
        csn = cfg.d_compat_use_sn_in_classification
        if cfg.d_cls_dense_layers:
            C = D + "/classification"
            u1 = R.round_up(ch / 16.0 + cfg.n_labels * 1.25, 8)
            y = R.activation(vs, C + "/prelu", R.fully_connected(vs, C + "/dense1", feat, u1, opt, sn=csn), opt)
            u2 = R.round_up(u1 / 4.0 + cfg.n_labels * 1.1, 4)
            y = R.activation(vs, C + "/prelu_1", R.fully_connected(vs, C + "/dense2", y, u2, opt, sn=csn), opt)
            out["cls"] = R.fully_connected(vs, C + "/DC_logit", y, cfg.n_labels, opt, sn=csn)
        else:
            out["cls"] = R.fully_connected(vs, D + "/DC_logit", feat, cfg.n_labels, opt, sn=csn)
    return out


def _offsets_scalar(offsets):
    """(ro_x[0], ro_y[0]): only element [0] is used, for the whole batch (BigGAN.py:656-657); the first is the height."""
    def first(v):
        return int(v.reshape(-1)[0]) if hasattr(v, "reshape") else int(v[0] if isinstance(v, (list, tuple)) else v)
    return first(offsets[0]), first(offsets[1])


def install(monkeypatch):
    SR.install(monkeypatch)
    AR.install(monkeypatch)                     # (last: its generator wrapper must stay on top of mixed_ref's)
    disc0 = RM.discriminator                    # (the alpha mask of tests/rgba_ref.py over the oracle's)
    d_forward0 = RM.Trainer.d_forward
    d_step0 = RM.Trainer.d_step

    def discriminator(vs, cfg, x, recon=None):
        """``recon``: {"offsets": (oy, ox)} in the real call of the D step.  While the variables are being created
        (Trainer.build) the heads are instantiated as well."""
        if heads_on(cfg) and (recon is not None or not vs.frozen):
            return _discriminator_with_heads(vs, cfg, x, (recon or {}).get("offsets") or (0, 0))
        return disc0(vs, cfg, x)

    def d_forward(self, real, z, aug_real, aug_fake, labels=None, cls_z=None, gp=None, recon_offsets=None):
        cfg, vs = self.cfg, self.vs
        if not heads_on(cfg):
            return d_forward0(self, real, z, aug_real, aug_fake, labels, cls_z, gp)
        if recon_offsets is None:
            recon_offsets = getattr(self, "recon_offsets", None) or (0, 0)
        oy, ox = _offsets_scalar(recon_offsets)
        vs.reg_losses = []
        vs.state_updates.clear()
        real_aug = R.diffaugment(self._t(real), aug_real, cfg.da_policy)
        d_real = RM.discriminator(vs, cfg, real_aug, recon={"offsets": (oy, ox)})
        cz = self._t(cls_z) if cfg.n_labels else None
        fake = RM.generator(vs, cfg, self._t(z), cz, True)
        d_fake = RM.discriminator(vs, cfg, R.diffaugment(fake, aug_fake, cfg.da_policy))
        d_loss = R.discriminator_loss(cfg.gan_type, d_real["real"], d_fake["real"], cfg.d_flood)
        gp_val = None
        if self.gradient_penalty_type():
            gp_val = self.gradient_penalty(self._t(real), fake.detach(), gp)
            d_loss = d_loss + gp_val
        d_cls = None
        if cfg.n_labels:
            w = torch.ones(cfg.n_labels, dtype=self.dtype)
            d_cls = cfg.d_cls_loss_weight * R.cls_loss_logistic(self._t(labels), d_real["cls"], w)
            d_loss = d_loss + d_cls
        out = {"real_logits": d_real["real"], "fake_logits": d_fake["real"], "fake": fake, "d_cls_loss": d_cls,
               "gp": gp_val}
        if "coarse_upscaled" in d_real:                                             # BigGAN.py:810-819, 885-886
            out["coarse_upscaled"] = d_real["coarse_upscaled"]
            out["d_recon"] = recon_loss(d_real["coarse_upscaled"], coarse_target(cfg, real_aug), cfg.d_recon_ld)
            d_loss = d_loss + out["d_recon"]
        if "texture_upscaled" in d_real:                                            # BigGAN.py:823-836, 888-889
            out["texture_upscaled"] = d_real["texture_upscaled"]
            out["d_tex_recon"] = recon_loss(d_real["texture_upscaled"], texture_target(cfg, real_aug, oy, ox),
                                            cfg.d_tex_recon_ld)
            d_loss = d_loss + out["d_tex_recon"]
        out["d_loss"] = d_loss
        return out

    def d_step(self, real, z, aug_real, aug_fake, labels=None, cls_z=None, apply=True, gp=None, recon_offsets=None):
        if not heads_on(self.cfg):
            return d_step0(self, real, z, aug_real, aug_fake, labels, cls_z, apply, gp)
        prev = getattr(self, "recon_offsets", None)
        if recon_offsets is not None:
            self.recon_offsets = recon_offsets
        try:
            return d_step0(self, real, z, aug_real, aug_fake, labels, cls_z, apply, gp)
        finally:
            self.recon_offsets = prev

    monkeypatch.setattr(RM, "discriminator", discriminator)
    monkeypatch.setattr(RM.Trainer, "d_forward", d_forward)
    monkeypatch.setattr(RM.Trainer, "d_step", d_step)
