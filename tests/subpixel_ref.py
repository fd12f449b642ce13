"""Float64 torch-CPU restatement of sub-pixel up-sampling (--upsampling_method subpixel2 / subpixel3: ops.py:23-27,
207-210) and of the mixed 3x3 / 5x5 down-sampling conv (--downsampling_method resize_conv35: ops.py:281-285 with the
string kernel of ops.py:52-59), built from ``oracle.ref_ops`` primitives.

``install(monkeypatch)`` puts ``upconv`` / ``downconv`` below over the oracle's (every block of ``oracle.ref_ops`` and
``tests.mixed_ref`` reaches them through the module) and the mixed-block generator over ``RM.generator``, the way
``tests/mixed_ref.py`` and ``tests/latent_ref.py`` install theirs; configurations without the new methods are handed on
to the oracle's own functions.
"""
import torch

from oracle import ref_model as RM
from oracle import ref_ops as R
from tests import mixed_ref as MR

_oracle_upconv = R.upconv
_oracle_downconv = R.downconv

SUBPIXEL_KERNEL = {"subpixel2": 2, "subpixel3": 3}


def depth_to_space(x, r=2):
    """tf.nn.depth_to_space, NHWC: out[n, h*r+i, w*r+j, c] = in[n, h, w, (i*r+j)*C + c].  (torch's pixel_shuffle orders
    the channels c*r*r + i*r + j: a different permutation.)"""
    n, h, w, c4 = x.shape
    c = c4 // (r * r)
    assert c * r * r == c4
    return x.reshape(n, h, w, r, r, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h * r, w * r, c)


def space_to_depth(y, r=2):
    """tf.nn.space_to_depth: the inverse permutation (and therefore the adjoint) of depth_to_space."""
    n, hr, wr, c = y.shape
    h, w = hr // r, wr // r
    assert h * r == hr and w * r == wr
    return y.reshape(n, h, r, w, r, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, r * r * c)


def subpixel_pad(kernel):
    """(low, high) padding of subpixel_conv's conv: pad = (k-1)/2.0 through ops.py:68-76 (pad*2, int(pad//2) low, the
    rest high) - 1/1 for k = 3, 0/1 for k = 2; TF 'SAME' (zero) splits k - 1 the same way."""
    tot = ((kernel - 1) / 2.0) * 2
    lo = int(tot // 2)
    return lo, int(tot - lo)


def subpixel_conv(vs, scope, x, channels, opt, kernel=3, scale=2, use_bias=True):
    """ops.py:23-27: conv to channels * scale^2 under ``scope``/subpixel_conv_0 (one spectral norm over the whole
    kernel, the generator's regulariser on it), then depth_to_space.  R.conv applies the float pad exactly as
    ops.py:68-76 does."""
    y = R.conv(vs, scope + "/subpixel_conv_0", x, channels * scale * scale, opt, kernel=kernel, stride=1,
               pad=(kernel - 1) / 2.0, use_bias=use_bias, _round_out=channels % 8 == 0)
    return depth_to_space(y, scale)


def upconv(vs, scope, x, channels, opt, use_bias=True):
    k = SUBPIXEL_KERNEL.get(opt.get("upsampling_method", "deconv4"))
    if k is None:
        return _oracle_upconv(vs, scope, x, channels, opt, use_bias=use_bias)
    return subpixel_conv(vs, scope, x, channels, opt, kernel=k, scale=2, use_bias=use_bias)


def conv35_widths(channels):
    """ops.py:282-283: (channels3, channels5)."""
    c5 = int(channels * 0.333333333334)
    return channels - c5, c5


def downconv(vs, scope, x, channels, opt, use_bias=True, method=None):
    m = method or opt.get("downsampling_method", "strided_conv3")
    if m != "resize_conv35":
        return _oracle_downconv(vs, scope, x, channels, opt, use_bias=use_bias, method=method)
    c3, c5 = conv35_widths(channels)
    parts = []
    for width, k in ((c3, 3), (c5, 5)):                 # ops.py:52-59: one conv per slice, pad (k-1)//2, own variables
        sc = scope + "/conv_0/conv%d_slice" % k
        if R._resident(x):                              # (bf16 input: the multi-branch launch rounds every branch kernel)
            parts.append(MR.conv_dilated(vs, sc, x, width, opt, k, (k - 1) // 2, 1, use_bias))
        else:
            parts.append(R.conv(vs, sc, x, width, opt, kernel=k, stride=1, pad=(k - 1) // 2, use_bias=use_bias,
                                _round_out=False))
    return R.avg_pooling(R.r_act(torch.cat(parts, dim=-1)))


def config(**kw):
    return MR.config(**kw)


def trainer(dtype=torch.float64, seed=42, perturb=True, **kw):
    return MR.trainer(dtype, seed, perturb, **kw)


def install(monkeypatch):
    MR.install(monkeypatch)
    monkeypatch.setattr(R, "upconv", upconv)
    monkeypatch.setattr(R, "downconv", downconv)
