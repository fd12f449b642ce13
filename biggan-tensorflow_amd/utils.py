"""Host-side helpers with the reference's names (``/root/reference/utils.py``) that the hot path
needs: flag parsing helper, channel rounding, directory creation, the generator weight
regularisers and the step-op glue."""
import os

import torch


def check_folder(log_dir):
    """utils.py:164-167."""
    if not os.path.exists(log_dir):
        os.makedirs(log_dir)
    return log_dir


def str2bool(x):
    """utils.py:173-174 - a SUBSTRING test, kept verbatim: '', 't', 'rue' parse as True."""
    return x.lower() in ('true')


def round_up(val, multiple):
    """utils.py:335-336."""
    return (int(val) + multiple - 1) // multiple * multiple


def parse_int_list(str):
    """utils.py:237-239."""
    if str == 'none' or str == '':
        return []
    return [int(x.strip()) for x in str.split(",")]


##################################################################################
# Sample grids (utils.py:133-161)
##################################################################################
def inverse_transform(images):
    """utils.py:160-161: [-1, 1] -> [0, 1]."""
    return (images + 1.) / 2.


def merge(images, size):
    """utils.py:136-154: tile [n, h, w, c] images into a size[0] x size[1] grid (row-major)."""
    import numpy as np
    h, w = images.shape[1], images.shape[2]
    if images.shape[3] in (3, 4):
        c = images.shape[3]
        img = np.zeros((h * size[0], w * size[1], c))
        for idx, image in enumerate(images):
            i = idx % size[1]
            j = idx // size[1]
            img[j * h:j * h + h, i * w:i * w + w, :] = image
        return img
    elif images.shape[3] == 1:
        img = np.zeros((h * size[0], w * size[1]))
        for idx, image in enumerate(images):
            i = idx % size[1]
            j = idx // size[1]
            img[j * h:j * h + h, i * w:i * w + w] = image[:, :, 0]
        return img
    raise ValueError('in merge(images,size) images parameter must have dimensions: HxW or HxWx3 or HxWx4')


def grid_u8(images, size):
    """The 8-bit grid of [n, h, w, c] images in [0, 1]: merge (a float64 grid), x255, round to nearest even, clamp.
    Returns uint8 [h, w, c] (c = 1 for grayscale).  ``functional.image_tiles_u8`` computes the same bytes on the device."""
    import numpy as np
    img = merge(images, size)
    a = np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return a


def write_png(a, path):
    """uint8 [h, w] or [h, w, c] (c = 1, 3 or 4) -> 8-bit PNG written with zlib only (no imaging library here)."""
    import struct
    import zlib
    import numpy as np
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError("write_png: expected uint8, got %s" % a.dtype)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError("write_png: expected [h, w] or [h, w, 1|3|4], got %s" % (a.shape,))
    a = np.ascontiguousarray(a)
    h, w, c = a.shape
    color_type = {1: 0, 3: 2, 4: 6}[c]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * c)], axis=1).tobytes()   # filter type 0 per row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, 0)) +
           chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
    return path


def imsave(images, size, path):
    """utils.py:156-157 (imageio.imwrite)."""
    return write_png(grid_u8(images, size), path)


def save_images(images, size, image_path):
    """utils.py:133-134."""
    return imsave(inverse_transform(images), size, image_path)


##################################################################################
# Vector files of the sampling service (utils.py:53-69, 395-407)
##################################################################################
def read_vectors(path):
    """utils.py:53-69: ``(cmds, vectors)`` of a tab-separated file with ``"`` as the quote character.  A row whose first
    field starts with ``!`` is a command row of ``key[=value]`` fields (a key without a value maps to ''); empty rows are
    skipped; every other row is one vector of floats (ValueError for a field that is no number)."""
    import csv
    vectors, cmds = [], {}
    with open(path, 'r', newline='') as f:
        for row in csv.reader(f, delimiter='\t', quotechar='"'):
            if len(row) == 0:
                continue
            if row[0][:1] == '!':
                row[0] = row[0][1:]
                for cmd in row:
                    p = cmd.split('=', 1)
                    cmds[p[0]] = p[1] if len(p) > 1 else ''
            else:
                vectors.append([float(v) for v in row])
    return cmds, vectors


def write_vectors(path, rows):
    """utils.py:395-407: one line per sample, fields tab-separated, each number as ``str(numpy.float32(v))`` (the
    shortest text that reads back to the same float32).  A sample is a scalar or a sequence of numbers."""
    import numpy as np
    with open(path, 'w') as f:
        for row in rows:
            f.write('\t'.join(str(np.float32(v)) for v in np.asarray(row, dtype=np.float32).reshape(-1)) + '\n')
    return path


##################################################################################
# Regularization (utils.py:180-235)
##################################################################################
def orthogonal_regularizer(scale, type='ortho'):
    """utils.py:185-211.  Returns a callable w[k,k,a,c] -> scalar loss tensor (device)."""
    if type not in ('ortho', 'ortho_cosine'):
        raise ValueError("Unknown regularization method.")

    def ortho_reg(w):
        from . import functional as Fn
        return Fn.OrthoCosineRegFn.apply(w, scale, type)
    return ortho_reg


def l2_regularizer(scale):
    """tf.contrib.layers.l2_regularizer(scale) (BigGAN.py:268-270)."""
    def l2_reg(w):
        from . import functional as Fn
        return Fn.L2RegFn.apply(w, scale)
    return l2_reg


def orthogonal_regularizer_fc(scale, type='ortho'):
    """utils.py:213-235 (same arithmetic on a [Cin, units] kernel)."""
    return orthogonal_regularizer(scale, type)


##################################################################################
# Class-label loss (utils.py:323-377)
##################################################################################
CLS_LOSS_KINDS = {'logistic': 0, 'euclidean': 1}          # the kind codes of include/biggan_hip.h


def parse_cls_loss_type(type, n_labels):
    """The grammar of utils.py:339-375 -> [(kind, size), ...], one entry per column slice, sizes summing to
    ``n_labels``.  'logistic' / 'euclidean' are one slice of every column; a spec containing ',' is a list of
    ``size-type`` parts.  ValueError (naming the spec) for an unknown type - a ``size-type`` spec without a comma, such as
    '10-logistic', is one: it takes the reference's "Invalid label loss type" branch -, for a part that is not
    ``size-type`` with a size >= 1, and for sizes that do not sum to ``n_labels`` (the reference's tf.split fails)."""
    spec = str(type)
    if ',' not in spec:
        if spec not in CLS_LOSS_KINDS:
            raise ValueError("Invalid label loss type: " + spec)
        return [(spec, int(n_labels))]
    out = []
    for part in spec.split(','):
        pieces = part.split('-')
        if len(pieces) != 2 or not pieces[0].strip().isdigit() or int(pieces[0]) < 1:
            raise ValueError("Invalid label loss type: '%s' (part '%s' is not size-type)" % (spec, part))
        if pieces[1] not in CLS_LOSS_KINDS:
            raise ValueError("Invalid label loss type: '%s' (unknown type '%s')" % (spec, pieces[1]))
        out.append((pieces[1], int(pieces[0])))
    if sum(size for _, size in out) != int(n_labels):
        raise ValueError("Invalid label loss type: the slice sizes of '%s' sum to %d, not to n_labels = %d"
                         % (spec, sum(size for _, size in out), int(n_labels)))
    return out


def cls_loss_fn(type, cls_weights):
    """utils.py:339-375.  ``cls_weights`` is a tensor [n_labels]; the returned callable
    ``loss(truth, answer, loss_weight, reduce_fn, world)`` folds ``loss_weight`` into the kernel (BigGAN.py:853,894).
      'logistic'   mean(sigmoid_cross_entropy_with_logits(truth, answer) * w) over [B_global, n_labels] (bg_sigmoid_ce)
      'euclidean'  ||(answer - truth) * w||_2 over the whole block: one norm, not a mean
      'N-type,...' truth / answer / w split column-wise by the sizes; the sum of the slice losses, a logistic slice
                   averaging over its own B_global * size elements
    Everything but plain 'logistic' runs the two launches of csrc/labels.hip (functional.LabelLossFn).  Where a euclidean
    slice's sum of squares is exactly 0 the gradient is 0 (TensorFlow's sqrt gradient gives NaN there)."""
    import torch
    if cls_weights is None and str(type) != 'logistic':
        raise ValueError("cls_loss_type '%s' needs the label weights (their length is n_labels)" % type)
    slices = parse_cls_loss_type(type, 0 if cls_weights is None else cls_weights.shape[0])
    if str(type) == 'logistic':
        def loss(truth, answer, loss_weight=1.0, reduce_fn=None, world=1):
            from . import functional as Fn
            return Fn.SigmoidCeLossFn.apply(truth, answer, cls_weights, loss_weight, reduce_fn, world)
        return loss
    # device-resident slice description, uploaded once: (kind, size) per slice and the slice index of every column
    dev = cls_weights.device
    slice_tab = torch.tensor([[CLS_LOSS_KINDS[k], size] for k, size in slices], dtype=torch.int32).to(dev)
    col_slice = torch.tensor([i for i, (_, size) in enumerate(slices) for _ in range(size)], dtype=torch.int32).to(dev)
    weights = cls_weights.to(torch.float32).contiguous()

    def loss(truth, answer, loss_weight=1.0, reduce_fn=None, world=1):
        from . import functional as Fn
        return Fn.LabelLossFn.apply(truth, answer, weights, slice_tab, col_slice, loss_weight, reduce_fn, world)
    loss.slices = slices
    return loss


def add_n(tensors):
    """tf.add_n over 1-element device tensors (loss bookkeeping, BigGAN.py:898)."""
    out = tensors[0]
    for t in tensors[1:]:
        out = out + t
    return out
