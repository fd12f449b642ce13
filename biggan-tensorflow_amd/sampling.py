"""Host-side planning of the in-training sample grids (BigGAN.py:980-1008, 1125-1230): how many generator batches a grid
takes, the static latent set, the latents of the morph and class grids, file names, the class-vector file.  Pure
functions on numpy / CPU torch: nothing here touches the GPU or the model's random state.

Every host random choice comes from a local ``numpy.random.RandomState`` (``event_rng``), never from numpy's global
generator: the reference seeds the global one for the class grid and leaves the morph picks unseeded; here one
generator seeded from (static_sample_seed, epoch, idx) drives both, so a sampling event is reproducible."""
import math

import numpy as np
import torch

from .utils import round_up


def grid_plan(sample_num, batch_size):
    """(dim, rounded_n, batches): the grid is dim x dim with dim = floor(sqrt(sample_num)) (BigGAN.py:1126-1128), the
    static set holds rounded_n = round_up(sample_num, batch_size) latents (BigGAN.py:981) and a grid takes
    ceil(dim*dim / batch_size) generator batches (BigGAN.py:1130)."""
    sample_num, batch_size = int(sample_num), int(batch_size)
    if sample_num < 1 or batch_size < 1:
        raise ValueError("grid_plan: sample_num=%d batch_size=%d" % (sample_num, batch_size))
    dim = int(math.floor(math.sqrt(sample_num)))
    while dim * dim > sample_num:            # (float sqrt of a huge perfect square minus one)
        dim -= 1
    return dim, round_up(sample_num, batch_size), (dim * dim + batch_size - 1) // batch_size


def draw_z(n, z_dim, generator, trunc):
    """[n,1,1,z_dim] fp32 on the CPU from ``generator``: the +-2 sigma truncated normal of ``BigGAN.sample_z`` when
    ``trunc`` (tf.random.truncated_normal), a plain normal otherwise."""
    z = torch.empty(int(n), 1, 1, int(z_dim), dtype=torch.float32)
    if trunc:
        torch.nn.init.trunc_normal_(z, 0.0, 1.0, -2.0, 2.0, generator=generator)
    else:
        z.normal_(generator=generator)
    return z


def static_z(rounded_n, z_dim, seed, trunc):
    """The static latent set (BigGAN.py:980-985) from a CPU generator seeded with --static_sample_seed: the same values
    on every rank, on every device and after a resume.  (TF's seeded draw itself cannot be reproduced.)"""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed) % (1 << 63))
    return draw_z(rounded_n, z_dim, g, trunc)


def event_rng(static_sample_seed, epoch, iteration, idx):
    """The RandomState of one sampling event: (static_sample_seed + epoch * iteration + idx) mod 2**32 (the reference
    seeds numpy's global generator with epoch * iteration + idx for the class grid, BigGAN.py:1213)."""
    return np.random.RandomState((int(static_sample_seed) + int(epoch) * int(iteration) + int(idx)) % (1 << 32))


def synthetic_label_table(n_labels):
    """The label table of a run without a dataset: one one-hot row per class, so row draws are uniform classes."""
    return np.eye(int(n_labels), dtype=np.float32)


def draw_n_tags(labels, n, rng):
    """BigGAN.py:1447-1452: n rows of the label table, drawn with replacement.  fp32 [n, n_labels]."""
    return np.asarray([labels[rng.randint(len(labels))] for _ in range(int(n))], dtype=np.float32)


def static_cls(labels, rounded_n, seed):
    """The static class vectors (BigGAN.py:992-994), drawn once from RandomState(static_sample_seed)."""
    return draw_n_tags(labels, rounded_n, np.random.RandomState(int(seed) % (1 << 32)))


def morph_corners(sample_num, rng):
    """The four corners of the morph grid: indices into the static set, ``randint(sample_num)`` each (BigGAN.py:1171-1181)."""
    return [int(rng.randint(int(sample_num))) for _ in range(4)]


def morph_latents(z4, cz4, dim, padding=1):
    """BigGAN.py:1183-1193: bilinear blend of four latents (and class vectors) over a (dim + 2*padding)^2 grid, x outer
    and y inner; rx = x / (dim - 1) for x in [-padding, dim + padding), so the border ring extrapolates.  The blend is
    evaluated left to right as a(1-rx)(1-ry) + b rx (1-ry) + c (1-rx) ry + d rx ry on fp32 arrays with Python-float
    weights.  Returns (z rows, class rows or None) as fp32 arrays with (dim + 2*padding)^2 rows."""
    dim = int(dim)
    if dim < 2:
        raise ValueError("morph_latents: the grid needs dim >= 2 (rx = x / (dim - 1)), got %d" % dim)

    def blend(corners, rx, ry):
        a, b, c, d = corners
        return a * (1 - rx) * (1 - ry) + b * rx * (1 - ry) + c * (1 - rx) * ry + d * rx * ry

    zs = [np.asarray(z, dtype=np.float32) for z in z4]
    cs = None if cz4 is None else [np.asarray(c, dtype=np.float32) for c in cz4]
    steps = [v / (dim - 1) for v in range(-padding, dim + padding)]
    z_rows = [blend(zs, rx, ry) for rx in steps for ry in steps]
    cz_rows = None if cs is None else [blend(cs, rx, ry) for rx in steps for ry in steps]
    return (np.stack(z_rows).astype(np.float32),
            None if cz_rows is None else np.stack(cz_rows).astype(np.float32))


def select_by_tag(labels, tag_index, rng):
    """BigGAN.py:1203-1211: a random row of the label table that carries ``tag_index``; after 1000 misses any row."""
    for _ in range(1000):
        row = labels[rng.randint(len(labels))]
        if row[tag_index] > 0:
            return row
    print("Warning: did not find any samples for tag index", tag_index, ", picking at random")
    return labels[rng.randint(len(labels))]


def cls_grid_vectors(labels, n_labels, count, rng):
    """The class grid (BigGAN.py:1213-1223): one tag index ``randint(n_labels)``, then ``count`` rows that carry it.
    Returns (tag index, fp32 [count, n_labels])."""
    rti = int(rng.randint(int(n_labels)))
    rows = [select_by_tag(labels, rti, rng) for _ in range(int(count))]
    return rti, np.asarray(rows, dtype=np.float32)


def sample_names(model_name, epoch, idx, tag=None):
    """File names of one sampling event (BigGAN.py:1155, 1199, 1229); ``cls`` only with a tag index."""
    stem = '_{:02d}_{:05d}'.format(int(epoch), int(idx))
    names = {kind: model_name + '_' + kind + stem + '.png' for kind in ("ema", "noema", "morph")}
    if tag is not None:
        names["cls"] = model_name + '_cls' + stem + '_{:03d}.png'.format(int(tag))
    return names


def write_vectors(path, vectors):
    """--save_cls_samples_to (BigGAN.py:999-1002): one tab-separated row of floats per sample."""
    with open(path, 'w') as f:
        for sample in vectors:
            f.write('\t'.join(map(str, [float(v) for v in sample])) + '\n')
    return path


def read_vectors(path, expect=None):
    """--load_cls_samples_from (utils.py:53-69): (commands, vectors).  A row starting with '!' holds tab-separated
    ``key=value`` commands and is kept out of the vectors.  ``expect``: the number of rows the caller needs (fewer is a
    ValueError)."""
    vectors, cmds = [], {}
    with open(path, 'r') as f:
        for line in f:
            line = line.rstrip('\r\n')
            if not line:
                continue
            fields = line.split('\t')
            if line.startswith('!'):
                fields[0] = fields[0][1:]
                for field in fields:
                    key, _, value = field.partition('=')
                    cmds[key] = value
            else:
                vectors.append([float(v) for v in fields])
    if expect is not None and len(vectors) < expect:
        raise ValueError("%s holds %d class vectors, the static sample set needs %d" % (path, len(vectors), expect))
    return cmds, vectors
