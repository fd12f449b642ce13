"""Float64 torch-CPU restatement of the mixed-kernel generator blocks (--g_mixed_resblocks): clown_conv
(ops.py:403-436), mixed_resblock (ops.py:438-442), the dilated conv (ops.py:95 with tf.pad REFLECT, ops.py:82) and the
generator with one mixed block after every level (BigGAN.py:485-489), for both z paths, built from ``oracle.ref_ops``
primitives.

``install(monkeypatch)`` puts ``generator`` below over ``RM.generator`` the way ``tests/latent_ref.py`` does;
configurations without --g_mixed_resblocks go to the latent-stage restatement (which hands default configurations on
to the oracle).  The new attributes are set on the ``Config`` after construction (``config()``).
"""
import torch
import torch.nn.functional as F

from oracle import ref_model as RM
from oracle import ref_ops as R
from tests import latent_ref as LR

MIXED_FLAGS = dict(g_mixed_resblocks=False, g_mixed_resblock_ch_div=2.0)


def config(**kw):
    new = {k: kw.pop(k) for k in list(kw) if k in MIXED_FLAGS}
    cfg = LR.config(**kw)
    for k, v in MIXED_FLAGS.items():
        setattr(cfg, k, new.get(k, v))
    return cfg


def trainer(dtype=torch.float64, seed=42, perturb=True, **kw):
    tr = RM.Trainer(config(**kw), dtype, seed).build()
    if perturb:
        RM.perturb_for_parity(tr.vs)
        for k, p in tr.g_params().items():
            tr.ema[k] = p.detach().clone()
    return tr


def clown_split(channels, no_deconv2=False):
    """ops.py:405-417: widths of deconv4, deconv3, deconv2, conv3, conv5, dilconv5 (deconv2 = 0 with no_deconv2)."""
    split = channels // 8
    d4, c5 = split + channels - 7 * split, split
    d2 = split
    if no_deconv2:
        d4 += split // 2
        c5 += split - split // 2
        d2 = 0
    return [d4, 2 * split, d2, split, c5, split]


def _round_w(wn, x):
    # the bf16-resident product multiplies bf16 operands: a branch kernel is rounded whenever its input is bf16
    return R._RoundFwd.apply(wn) if R._resident(x) else wn


def conv_dilated(vs, scope, x, channels, opt, kernel, pad, dilation, use_bias=True):
    """ops.py:61-98 with dilation d, stride 1: reflect = tf.pad(pad, pad) + VALID conv2d(dilations=d); zero = TF 'SAME'
    with the effective kernel (k - 1) d + 1."""
    cin = x.shape[-1]
    xin = R._nchw(x)
    keff = (kernel - 1) * dilation + 1
    if opt.get("padding_type", "reflect") == "reflect":
        xin = F.pad(xin, (pad, pad, pad, pad), mode="reflect")
    else:
        lo = (keff - 1) // 2
        xin = F.pad(xin, (lo, keff - 1 - lo, lo, keff - 1 - lo))
    w = vs.get(scope + "/kernel", (kernel, kernel, cin, channels), "trunc_normal")
    R._maybe_regularize(vs, opt, scope, w, "conv")
    wn = R.spectral_norm(vs, scope, w) if opt.get("sn", True) else w
    y = R._nhwc(F.conv2d(xin, _round_w(wn, x).permute(3, 2, 0, 1).contiguous(), dilation=dilation))
    if use_bias:
        y = y + vs.get(scope + "/bias", (channels,), 0.0)
    return y


def _deconv(vs, scope, x, channels, opt, kernel, use_bias):
    """R.deconv (stride 1, TF 'SAME'), with the branch kernel rounded as the multi-branch launch rounds it."""
    cin, h = x.shape[-1], x.shape[1]
    lo = (kernel - 1) // 2
    hi = kernel - 1 - lo
    w = vs.get(scope + "/kernel", (kernel, kernel, channels, cin), "trunc_normal")
    R._maybe_regularize(vs, opt, scope, w, "deconv")
    wn = R.spectral_norm(vs, scope, w) if opt.get("sn", True) else w
    y = F.conv_transpose2d(R._nchw(x), _round_w(wn, x).permute(3, 2, 0, 1).contiguous(), stride=1)
    full = y.shape[-1]
    y = R._nhwc(y[:, :, lo:full - hi, lo:full - hi])
    assert y.shape[1] == h
    if use_bias:
        y = y + vs.get(scope + "/bias", (channels,), 0.0)
    return y


def _conv(vs, scope, x, channels, opt, kernel, pad, use_bias):
    return conv_dilated(vs, scope, x, channels, opt, kernel, pad, 1, use_bias)


def clown_conv(vs, scope, x, channels, opt, is_training=True, z=None, use_bias=True, no_deconv2=False):
    """ops.py:403-436: six branches concatenated, bn (cond_bn with z), then PReLU whatever opt['act'] says."""
    d4, d3, d2, c3, c5, dl = clown_split(channels, no_deconv2)
    parts = [_deconv(vs, scope + "/deconv4", x, d4, opt, 4, use_bias),
             _deconv(vs, scope + "/deconv3", x, d3, opt, 3, use_bias)]
    if not no_deconv2:
        parts.append(_deconv(vs, scope + "/deconv2", x, d2, opt, 2, use_bias))
    parts += [_conv(vs, scope + "/conv3", x, c3, opt, 3, 1, use_bias),
              _conv(vs, scope + "/conv5", x, c5, opt, 5, 2, use_bias),
              conv_dilated(vs, scope + "/dilconv5", x, dl, opt, 5, 4, 2, use_bias)]
    y = R.r_act(torch.cat(parts, dim=-1))
    if z is None:
        y = R.batch_norm(vs, scope + "/batch_norm", y, opt, is_training)
    else:
        y = R.condition_batch_norm(vs, scope + "/batch_norm", y, z, opt, is_training)
    return R.activation(vs, scope + "/prelu", y, dict(opt, act="prelu"))


def mixed_resblock(vs, scope, x, inner_channels, out_channels, opt, is_training=True, z=None):
    """ops.py:438-442: x + conv1x1(clown(x)), no bias on the projection."""
    res = clown_conv(vs, scope + "/clown", x, inner_channels, opt, is_training, z)
    res = R.conv(vs, scope + "/proj", res, out_channels, opt, kernel=1, stride=1, pad=0, use_bias=False)
    return R.r_act(x + res)


def _latent_default(vs, cfg, z, cls_z, opt, ch):
    """RM.generator's z split and first dense layer -> (x [B,4,4,ch], per-block latents)."""
    G = "generator"
    sizes = cfg.z_split_sizes()
    z = z.reshape(z.shape[0], 1, 1, -1)
    z_split = list(torch.split(z, sizes, dim=-1))
    if cfg.n_labels > 0:
        cz = cls_z.reshape(-1, 1, 1, cfg.n_labels)
        z_split = [torch.cat([zz, cz], dim=-1) for zz in z_split]
    f_width = R.round_up((sizes[0] + cfg.n_labels) * 1.85, 8)
    first = G if cfg.activation == "relu" else G + "/first"
    if not cfg.g_first_level_dense_layer:
        x = R.fully_connected(vs, G + "/dense", z_split[0], 4 * 4 * ch, opt)
    else:
        x = R.fully_connected(vs, first + "/dense1", z_split[0], f_width, opt)
        x = R.activation(vs, first + "/prelu", x, opt)
        x = R.fully_connected(vs, first + "/dense2", x, 4 * 4 * ch, opt)
    blocks = []
    ch_mul = 2 ** (len(cfg.g_block_info()["counts"]) - 1)
    zi = 1
    for count in cfg.g_block_info()["counts"]:
        for _ in range(count):
            bz = z_split[zi]
            if cfg.g_other_level_dense_layer:
                zs = G + "/z" + str(ch_mul)
                zw = R.round_up((sizes[zi] + cfg.n_labels) * 1.25, 8)
                bz = R.activation(vs, zs + "/prelu", R.fully_connected(vs, zs + "/dense1", bz, zw, opt), opt)
                bz = bz.reshape(bz.shape[0], 1, 1, -1)
            blocks.append(bz)
            zi += 1
        ch_mul //= 2
    return R.r_act(x.reshape(-1, 4, 4, ch)), blocks


def _latent_new(vs, cfg, z, cls_z, opt, ch):
    """latent_ref.generator's latent stage (BigGAN.py:335-444) -> (x [B,4,4,ch], per-block latents)."""
    G = "generator"
    B = z.shape[0]
    sizes, shared_idx, first_idx, block_idx = LR.split_sizes(cfg)
    z_split = list(torch.split(z.reshape(B, -1), sizes, dim=-1))
    zvec = list(sizes)

    def act(scope, x):
        return R.activation(vs, scope + "/prelu", x, opt)

    cls_vec = None
    if cfg.n_labels > 0:
        cls_vec = cls_z.reshape(B, cfg.n_labels)
        if cfg.cls_embedding:
            e = act(G + "/cls_embed", R.fully_connected(vs, G + "/cls_embed/dense1", cls_vec, LR.embedding_size(cfg),
                                                        opt))
            cls_vec = torch.cat([cls_vec, e], dim=-1) if cfg.cls_embedding_concat else e
        for i in range(len(z_split)):
            if cfg.g_z_dense_concat and i == shared_idx:
                continue
            z_split[i] = torch.cat([z_split[i], cls_vec], dim=-1)
            zvec[i] += cls_vec.shape[-1]
    if shared_idx is not None:
        shared, zd = z_split[shared_idx], sizes[shared_idx]
        sc = G + "/shared_z"
        if cfg.g_z_dense_concat:
            f_width = R.round_up(zd * 0.5, 8)
            f_in = torch.cat([shared, cls_vec], dim=-1) if cls_vec is not None else shared
            d = act(sc, R.fully_connected(vs, sc + "/dense1", f_in, f_width, opt))
            shared = torch.cat([shared, d], dim=-1)
            zvec[shared_idx] += f_width
        else:
            f_width = R.round_up(zd * 1.5, 8)
            shared = act(sc, R.fully_connected(vs, sc + "/dense1", shared, f_width, opt))
            zvec[shared_idx] = f_width
        z_split[shared_idx] = shared
        for i in range(len(z_split)):
            if i != shared_idx:
                z_split[i] = torch.cat([z_split[i], shared], dim=-1)
                zvec[i] += zvec[shared_idx]
    dense_idx = ([first_idx] if cfg.g_first_level_dense_layer else []) + \
                (block_idx if cfg.g_other_level_dense_layer else [])
    for zi in dense_idx:
        sc = G + "/z" + str(zi)
        factor = 1.5 if zi == first_idx else 1.0
        if cfg.g_z_dense_concat:
            factor = (factor - 1.0) * 2.0 + 1.0
            f_width = R.round_up((zvec[zi] * 0.33) * factor, 8)
            layer_z = act(sc, R.fully_connected(vs, sc + "/dense1", z_split[zi], f_width, opt))
            z_split[zi] = torch.cat([z_split[zi], layer_z], dim=-1)
            zvec[zi] += f_width
        else:
            f_width = R.round_up((sizes[zi] * 0.75 + zvec[zi] * 0.5) * factor, 8)
            z_split[zi] = act(sc, R.fully_connected(vs, sc + "/dense1", z_split[zi], f_width, opt))
            zvec[zi] = f_width
    x = R.fully_connected(vs, G + "/first/dense", z_split[first_idx], 4 * 4 * ch, opt)
    return R.r_act(x.reshape(-1, 4, 4, ch)), [z_split[i].reshape(B, 1, 1, -1) for i in block_idx]


def generator(vs, cfg, z, cls_z=None, is_training=True):
    if not getattr(cfg, "g_mixed_resblocks", False):
        return LR.generator(vs, cfg, z, cls_z, is_training)
    opt = RM._conv_opt(cfg, is_training, True)
    G = "generator"
    info = cfg.g_block_info()
    counts = info["counts"]
    n_blocks = len(counts)
    ch_mul = 2 ** (n_blocks - 1)
    ch = cfg.scale_channels(cfg.ch, cfg.g_grow_factor ** (n_blocks - 1))
    latent = _latent_new if LR.new_z_dist(cfg) else _latent_default
    x, block_zs = latent(vs, cfg, z, cls_z, opt, ch)
    levels = iter(block_zs)
    b_i = 0
    for block_count in counts:                                                    # BigGAN.py:449-489
        scope = "resblock_up_" + str(ch_mul)
        for sb_i in range(block_count):
            block_z = next(levels)
            if block_count > 1:
                scope = scope + "_" + str(sb_i)
            is_last = sb_i == block_count - 1 and b_i == len(counts) - 1
            if cfg.g_no_last_resblock and is_last:
                sc = G + "/" + scope
                x = R.upconv(vs, sc, x, ch, opt, use_bias=False)
                x = R.condition_batch_norm(vs, sc + "/batch_norm", x, block_z, opt, is_training)
                x = R.activation(vs, sc + "/prelu", x, opt)
                x = R.g_conv(vs, sc, x, ch, opt, use_bias=False)
            elif cfg.deep:
                x = R.resblock_up_cond_deep(vs, G + "/" + scope, x, block_z, ch, opt, True, True, is_training)
                x = R.resblock_up_cond_deep(vs, G + "/" + scope + "_2", x, block_z, ch, opt, False, True, is_training)
            else:
                x = R.resblock_up_condition(vs, G + "/" + scope, x, block_z, ch, opt, use_bias=False,
                                            is_training=is_training)
        b_i += 1
        if b_i == info["sa_index"]:
            x = R.self_attention_2(vs, G + "/self_attention", x, ch, opt)
        inner = R.round_up(ch / cfg.g_mixed_resblock_ch_div, 8)                   # BigGAN.py:485-486
        x = mixed_resblock(vs, G + "/res_mixed" + str(ch_mul), x, inner, ch, opt, is_training)
        ch = cfg.scale_channels(cfg.ch, cfg.g_grow_factor ** (n_blocks - b_i - 1))
        ch_mul //= 2
    x = R.batch_norm(vs, G + "/batch_norm", x, opt, is_training)
    x = R.activation(vs, G + "/prelu", x, opt)
    x = R.conv(vs, G + "/G_logit", x, cfg.c_dim, opt, kernel=3, stride=1, pad=1, use_bias=False)
    return torch.tanh(x)


def install(monkeypatch):
    monkeypatch.setattr(RM, "generator", generator)
