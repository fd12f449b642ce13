"""Float64 torch-CPU restatement of the generator's latent stage with --cls_embedding / --shared_z / --g_z_dense_concat
(BigGAN.py:278-444, the ``new_z_dist`` branch), built from ``oracle.ref_ops`` primitives.

The oracle's ``ref_model.generator`` covers the default branch only; ``install(monkeypatch)`` puts ``generator`` below in
its place (``Trainer`` looks it up at module level).  Configurations without the new flags are passed to the oracle's
own function unchanged.  The new attributes are read from the ``Config`` with ``getattr`` because its constructor
rejects unknown keys: set them after construction (``config()``).
"""
import math

import torch

from oracle import ref_model as RM
from oracle import ref_ops as R

_oracle_generator = RM.generator

NEW_FLAGS = dict(cls_embedding=False, cls_embedding_size=0, cls_embedding_concat=False, shared_z=0,
                 g_z_dense_concat=False)


def config(**kw):
    """RM.Config with the latent-stage flags set after construction."""
    new = {k: kw.pop(k) for k in list(kw) if k in NEW_FLAGS}
    cfg = RM.Config(**kw)
    for k, v in NEW_FLAGS.items():
        setattr(cfg, k, new.get(k, v))
    return cfg


def trainer(dtype=torch.float64, seed=42, perturb=True, **kw):
    tr = RM.Trainer(config(**kw), dtype, seed).build()
    if perturb:
        RM.perturb_for_parity(tr.vs)
        for k, p in tr.g_params().items():
            tr.ema[k] = p.detach().clone()
    return tr


def new_z_dist(cfg):
    return bool(getattr(cfg, "cls_embedding", False) or getattr(cfg, "shared_z", 0) > 0
                or getattr(cfg, "g_z_dense_concat", False))


def embedding_size(cfg):
    """BigGAN.py:24-28; round_up truncates with int() first (utils.py:335)."""
    if cfg.cls_embedding_size:
        return cfg.cls_embedding_size
    return R.round_up(math.pow(cfg.n_labels, 0.88) + 24, 8)


def split_sizes(cfg):
    """BigGAN.py:314-333 without g_final_layer / mixed kernels: (sizes, shared slot, first slot, block slots)."""
    weights, shared_idx = [], None
    if cfg.shared_z > 0:
        shared_idx = 0
        weights.append(0.0)
    first_idx = len(weights)
    weights.append(cfg.first_split_ratio)
    block_idx = []
    for count in cfg.g_block_info()["counts"]:
        for _ in range(count):
            block_idx.append(len(weights))
            weights.append(1.0)
    total = sum(weights)
    nonshared = cfg.z_dim - cfg.shared_z
    sizes = [0] * len(weights)
    for i, w in reversed(list(enumerate(weights))):
        sizes[i] = int(w / total * nonshared)
    sizes[first_idx] += nonshared - sum(sizes)
    if shared_idx is not None:
        sizes[shared_idx] = cfg.shared_z
    return sizes, shared_idx, first_idx, block_idx


def generator(vs, cfg, z, cls_z=None, is_training=True):
    if not new_z_dist(cfg):
        return _oracle_generator(vs, cfg, z, cls_z, is_training)
    opt = RM._conv_opt(cfg, is_training, True)
    G = "generator"
    info = cfg.g_block_info()
    counts = info["counts"]
    B = z.shape[0]
    sizes, shared_idx, first_idx, block_idx = split_sizes(cfg)
    z_split = list(torch.split(z.reshape(B, -1), sizes, dim=-1))                  # BigGAN.py:335
    zvec = list(sizes)

    def act(scope, x):
        return R.activation(vs, scope + "/prelu", x, opt)

    cls_vec = None
    if cfg.n_labels > 0:                                                          # BigGAN.py:344-365
        cls_vec = cls_z.reshape(B, cfg.n_labels)
        if cfg.cls_embedding:
            e = act(G + "/cls_embed", R.fully_connected(vs, G + "/cls_embed/dense1", cls_vec, embedding_size(cfg), opt))
            cls_vec = torch.cat([cls_vec, e], dim=-1) if cfg.cls_embedding_concat else e
        for i in range(len(z_split)):
            if cfg.g_z_dense_concat and i == shared_idx:
                continue
            z_split[i] = torch.cat([z_split[i], cls_vec], dim=-1)
            zvec[i] += cls_vec.shape[-1]

    if shared_idx is not None:                                                    # BigGAN.py:367-392
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
    for zi in dense_idx:                                                          # BigGAN.py:394-424
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

    n_blocks = len(counts)
    ch_mul = 2 ** (n_blocks - 1)                                                  # BigGAN.py:427
    ch = cfg.scale_channels(cfg.ch, cfg.g_grow_factor ** (n_blocks - 1))
    x = R.fully_connected(vs, G + "/first/dense", z_split[first_idx], 4 * 4 * ch, opt)   # BigGAN.py:444
    x = R.r_act(x.reshape(-1, 4, 4, ch))
    levels = iter(block_idx)
    b_i = 0
    for block_count in counts:                                                    # BigGAN.py:449-489
        scope = "resblock_up_" + str(ch_mul)
        for sb_i in range(block_count):
            block_z = z_split[next(levels)].reshape(B, 1, 1, -1)
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
        ch = cfg.scale_channels(cfg.ch, cfg.g_grow_factor ** (n_blocks - b_i - 1))
        ch_mul //= 2
    x = R.batch_norm(vs, G + "/batch_norm", x, opt, is_training)
    x = R.activation(vs, G + "/prelu", x, opt)
    x = R.conv(vs, G + "/G_logit", x, cfg.c_dim, opt, kernel=3, stride=1, pad=1, use_bias=False)
    return torch.tanh(x)


def install(monkeypatch):
    monkeypatch.setattr(RM, "generator", generator)
