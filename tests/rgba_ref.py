"""Float64 torch-CPU restatement of the RGBA image ops (--c_dim 4): the generator's alpha helper between G_logit and
tanh (BigGAN.py:572-580) and the discriminator's alpha mask at its input (BigGAN.py:616-619), built on the oracle.

``install(monkeypatch)`` wraps ``oracle.ref_ops.conv`` so that the ``generator/G_logit`` output gets the helper (the
generator's ``torch.tanh`` follows it) and ``RM.discriminator`` so that the mask runs first.  It installs
``tests/mixed_ref.py`` (which hands everything else to ``tests/latent_ref.py`` and the oracle) underneath, so one call
covers the latent stage, the mixed blocks and the alpha ops together.  The new attributes are set on the ``Config``
after construction (``config()``), after the ones of ``mixed_ref.config``.
"""
import torch

from oracle import ref_model as RM
from oracle import ref_ops as R
from tests import mixed_ref as MR

RGBA_FLAGS = dict(alpha_mask=True, g_alpha_helper=True)


def config(**kw):
    new = {k: kw.pop(k) for k in list(kw) if k in RGBA_FLAGS}
    cfg = MR.config(**kw)
    for k, v in RGBA_FLAGS.items():
        setattr(cfg, k, new.get(k, v))
    return cfg


def trainer(dtype=torch.float64, seed=42, perturb=True, **kw):
    tr = RM.Trainer(config(**kw), dtype, seed).build()
    if perturb:
        RM.perturb_for_parity(tr.vs)
        for k, p in tr.g_params().items():
            tr.ema[k] = p.detach().clone()
    return tr


def alpha_helper(x, w):
    """a' = a + w * reduce_sum(x, -1): the sum runs over all four channels, the alpha logit included."""
    rgb, a = x[..., :3], x[..., 3:]
    return torch.cat([rgb, a + x.sum(dim=-1, keepdim=True) * w], dim=-1)


def alpha_mask(x):
    """rgb' = (rgb + 1)(a + 1)/2 - 1, alpha unchanged."""
    rgb, a = x[..., :3], x[..., 3:]
    return torch.cat([(rgb + 1.0) * (a + 1.0) * 0.5 - 1.0, a], dim=-1)


def _helper_on(cfg):
    return cfg.c_dim == 4 and getattr(cfg, "g_alpha_helper", True)


def _mask_on(cfg):
    return cfg.c_dim == 4 and getattr(cfg, "alpha_mask", True)


def install(monkeypatch):
    MR.install(monkeypatch)
    conv0 = R.conv
    disc0 = RM.discriminator
    # the Config of the model being run: the G_logit conv carries only its channel count, the flags live on the cfg
    current = {}

    def conv(vs, scope, x, channels, opt, *a, **kw):
        if scope == "generator/G_logit" and channels == 1 and not a and kw.get("stride") == 1 and not R.ROUND.on:
            # (--c_dim 1: torch's CPU conv2d backward wants a contiguous weight for one output channel, and R.conv hands
            #  it a permuted view; the same stride-1 conv with a contiguous weight)
            y = MR.conv_dilated(vs, scope, x, channels, opt, kw["kernel"], kw["pad"], 1, kw.get("use_bias", True))
        else:
            y = conv0(vs, scope, x, channels, opt, *a, **kw)
        cfg = current.get("cfg")
        if scope == "generator/G_logit" and cfg is not None and _helper_on(cfg):
            w = vs.get("generator/alphahelper_w", (), 5.0)           # created under generator, after G_logit
            y = alpha_helper(y, w)
        return y

    def discriminator(vs, cfg, x):
        if _mask_on(cfg):
            x = alpha_mask(x)
        return disc0(vs, cfg, x)

    gen0 = RM.generator

    def generator(vs, cfg, *a, **kw):
        prev = current.get("cfg")
        current["cfg"] = cfg
        try:
            return gen0(vs, cfg, *a, **kw)
        finally:
            current["cfg"] = prev

    monkeypatch.setattr(R, "conv", conv)
    monkeypatch.setattr(RM, "discriminator", discriminator)
    monkeypatch.setattr(RM, "generator", generator)
