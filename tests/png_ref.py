"""Host references of the device-side PNG encoder (csrc/png.hip, biggan_tensorflow_amd/png.py).  Test helper, numpy and
zlib only: nothing here touches the GPU or the library.

``filter_rows`` is the filter rule of DESIGN.md "Device-side PNG encoding", the exact gate of bg_png_filter.
``segments_with_zlib`` stands in for bg_deflate_segments: independent byte-aligned segments of the same shape (an empty
stored block behind every segment but the last, BFINAL on the last), made by zlib, so that ``png.assemble`` and
``png.adler32_fold`` can be exercised without a GPU."""
import zlib

import numpy as np


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _shift(row, bpp):
    out = np.zeros_like(row)
    out[bpp:] = row[:row.shape[0] - bpp]
    return out


def filter_rows(a):
    """uint8 [h, w, c] (or [h, w]) -> uint8 [h, 1 + w*c]: per row the filter type, then the filtered bytes.  The type is
    the type 0-4 with the smallest sum of abs((int8)residual), ties to the lowest type; the row above the first row is
    zeros; bpp = c."""
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.dtype == np.uint8 and a.ndim == 3
    h, w, c = a.shape
    rows = a.reshape(h, w * c).astype(np.int32)
    out = np.zeros((h, 1 + w * c), np.uint8)
    up = np.zeros(w * c, np.int32)
    for r in range(h):
        x = rows[r]
        left, ul = _shift(x, c), _shift(up, c)
        residuals = [x, x - left, x - up, x - ((left + up) >> 1), x - _paeth(left, up, ul)]
        coded = [(v & 255).astype(np.uint8) for v in residuals]
        cost = [int(np.abs(v.view(np.int8).astype(np.int32)).sum()) for v in coded]
        t = int(np.argmin(cost))                                   # the first minimum: ties go to the lowest type
        out[r, 0] = t
        out[r, 1:] = coded[t]
        up = x
    return out


def segments_with_zlib(stream, seg_bytes):
    """bytes -> ([segment bytes], [(adler_a, adler_b, len)]): every ``seg_bytes`` piece compressed on its own as raw
    DEFLATE (level 6, Z_RLE: distance-1 matches only), closed with Z_FULL_FLUSH, the last one with Z_FINISH."""
    stream = bytes(stream)
    segs, parts = [], []
    for pos in range(0, len(stream), seg_bytes):
        piece = stream[pos:pos + seg_bytes]
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        last = pos + seg_bytes >= len(stream)
        segs.append(co.compress(piece) + co.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH))
        ad = zlib.adler32(piece)
        parts.append((ad & 0xffff, ad >> 16, len(piece)))
    return segs, parts


def sinusoid_image(h, w, c, sigma, seed):
    """A smooth test image: per channel a sum of six sinusoids with random frequency, direction and phase, scaled to
    [0.05, 0.95], plus Gaussian noise of standard deviation ``sigma``; uint8 [h, w, c]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    img = np.zeros((h, w, c))
    for ch in range(c):
        acc = np.zeros((h, w))
        for _ in range(6):
            fy, fx = rng.uniform(-0.06, 0.06, 2)
            acc += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fy * yy + fx * xx) + rng.uniform(0, 2 * np.pi))
        acc = (acc - acc.min()) / (acc.max() - acc.min())
        img[:, :, ch] = 0.05 + 0.9 * acc
    if sigma:
        img = img + rng.normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)


def five_filter_image(w=48, seed=0):
    """uint8 [8, w, 1] whose rows are built so that each filter type wins at least once: noise, zeros (type 0 by the tie
    rule), a ramp (Sub), a copy of the row above (Up), noise, the rounded-down mean of left and up (Average), noise, the
    Paeth predictor with a step added at every third byte (the steps keep left != upper-left, so that the predictor does
    not collapse to Up)."""
    rng = np.random.RandomState(seed)
    noise = rng.randint(0, 256, w).astype(np.int32)
    ramp = (np.arange(w) * 3 + 7) % 256
    rows = [noise, np.zeros(w, np.int32), ramp, ramp.copy()]
    noise2 = rng.randint(0, 256, w).astype(np.int32)
    rows.append(noise2)
    avg = np.zeros(w, np.int32)
    for i in range(w):
        avg[i] = ((avg[i - 1] if i else 0) + noise2[i]) >> 1
    rows.append(avg)
    noise3 = rng.randint(0, 256, w).astype(np.int32)
    rows.append(noise3)
    pae = np.zeros(w, np.int32)
    for i in range(w):
        a, b, c = (pae[i - 1] if i else 0), noise3[i], (noise3[i - 1] if i else 0)
        pae[i] = (int(_paeth(np.int64(a), np.int64(b), np.int64(c))) + (37 if i % 3 == 0 else 0)) % 256
    rows.append(pae)
    return np.stack(rows).astype(np.uint8)[:, :, None]
