"""Shared by tests/test_input.py and tests/test_gpu_input.py: the case table of the device-side input preprocessing
(bg_image_batch_u8), the host path it has to reproduce bit for bit, a restatement of the kernel's arithmetic in single
fp32 steps, and simulated wrong kernels that the case table has to tell apart from the right one."""
import numpy as np

from biggan_tensorflow_amd import data as D

F = np.float32


class Case:
    def __init__(self, name, shapes, size, channels, flips):
        self.name, self.shapes, self.size, self.channels, self.flips = name, list(shapes), size, channels, list(flips)
        self._images = self._want = None

    def images(self):
        if self._images is None:
            rng = np.random.default_rng(1000 + 31 * self.size + self.channels + sum(h * 7 + w for h, w in self.shapes))
            self._images = [rng.integers(0, 256, (h, w, self.channels), dtype=np.uint8) for h, w in self.shapes]
            for a in self._images:
                a.setflags(write=False)
        return self._images

    def want(self):
        """The host path, computed once: [n, S, S, C] fp32."""
        if self._want is None:
            self._want = host_path(self.images(), self.flips, self.size, self.channels)
            self._want.setflags(write=False)
        return self._want

    def __repr__(self):
        return self.name


def _single(h, w, size, c):
    # the same source once plain and once flipped
    return Case("%dx%d_to_%d_c%d" % (h, w, size, c), [(h, w), (h, w)], size, c, [0, 1])


RAGGED = Case("ragged_to_6_c3", [(11, 7), (3, 11), (6, 6), (1, 1), (17, 5), (12, 13)], 6, 3, [0, 1, 1, 0, 1, 0])
CASES = [_single(3, 11, 6, 4), _single(11, 7, 6, 3), _single(7, 10, 3, 1), _single(13, 9, 12, 3),
         _single(10, 10, 12, 4),                      # upscale: the hi clamp
         _single(5, 6, 7, 3), _single(2, 9, 5, 1), _single(1, 1, 4, 3),
         _single(9, 9, 9, 1), _single(9, 9, 9, 3), _single(9, 9, 9, 4),          # identity
         _single(100, 75, 96, 3), _single(80, 80, 64, 3),
         Case("160x160_to_128_c3_x8", [(160, 160)] * 8, 128, 3, [0, 1, 0, 0, 1, 1, 0, 1]),
         RAGGED]
# more output pixels than one pass of the kernel's capped grid (4096 blocks of 256 threads)
GRID_STRIDE = Case("33x47_to_256_c1_x64", [(33, 47)] * 64, 256, 1, [i % 3 == 0 for i in range(64)])   # four passes


def host_path(images, flips, size, channels):
    """data.py's host path: ImageData.image_processing per image, the flip as the table gives it (the normalisation is
    elementwise, so flipping after it is the same bits as flipping before it)."""
    idata = D.ImageData(size, channels, False, False)
    out = []
    for img, flip in zip(images, flips):
        x = idata.image_processing(img)
        out.append(x[:, ::-1] if flip else x)
    return np.stack(out).astype(np.float32)


# ------------------------------------------------------------------------------------------
# the kernel, restated: every line one fp32 operation on all output pixels of one image
# ------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl32(a * b + c) with one rounding (a * b is exact in float64 for a byte times an fp32)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _axis(n_out, scale, n_in, wrong):
    i = np.arange(n_out, dtype=F)
    if wrong == "half_pixel":
        src = np.maximum((i + F(0.5)) * scale - F(0.5), F(0))
    else:
        src = i * scale
    fl = np.floor(src)
    lo = fl.astype(np.int64)
    hi = lo + 1 if wrong == "hi_unclamped" else np.minimum(lo + 1, n_in - 1)
    f = (src - fl).astype(F)
    return lo, hi, f, (F(1) - f).astype(F)


def kernel_model(raw, table, size, channels, wrong=None):
    """What bg_image_batch_u8 computes from a packed batch (``raw`` uint8, ``table`` of data.TABLE_DTYPE).  ``wrong``
    names one of WRONG_KERNELS."""
    C = channels
    mem = np.concatenate([np.asarray(raw, np.uint8), np.zeros(1 << 16, np.uint8)])      # what lies behind the buffer
    out = np.empty((len(table), size, size, C), F)
    for n, e in enumerate(table):
        h, w, off = int(e["h"]), int(e["w"]), int(e["offset"])
        y0, y1, fy, gy = _axis(size, F(e["scale_y"]), h, wrong)
        x0, x1, fx, gx = _axis(size, F(e["scale_x"]), w, wrong)

        def tap(ys, xs):
            if wrong == "source_flipped" and e["flip"]:
                xs = w - 1 - xs
            idx = off + (ys[:, None, None] * w + xs[None, :, None]) * C + np.arange(C)[None, None, :]
            return mem[idx].astype(F)
        a, b, c, d = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
        fxb, gxb, fyb, gyb = fx[None, :, None], gx[None, :, None], fy[:, None, None], gy[:, None, None]
        if wrong == "fma":
            top = _fma(a, gxb, (b * fxb).astype(F))
            bot = _fma(c, gxb, (d * fxb).astype(F))
            v = _fma(top, gyb, (bot * fyb).astype(F))
        else:
            top = ((a * gxb).astype(F) + (b * fxb).astype(F)).astype(F)
            bot = ((c * gxb).astype(F) + (d * fxb).astype(F)).astype(F)
            v = ((top * gyb).astype(F) + (bot * fyb).astype(F)).astype(F)
        if wrong == "reciprocal":
            o = ((v * (F(1) / F(127.5))).astype(F) - F(1)).astype(F)
        elif wrong == "wide_finish":
            o = (v.astype(np.float64) / 127.5 - 1.0).astype(F)
        else:
            o = ((v / F(127.5)).astype(F) - F(1)).astype(F)
        if e["flip"] and wrong != "source_flipped":
            o = o[::-1] if wrong == "rows_flipped" else o[:, ::-1]
        out[n] = o
    return out


def pixel(img, size, flip, oy, ox, c):
    """One output element in np.float32 scalars, in the kernel's order."""
    h, w = img.shape[:2]
    sy, sx = F(h / float(size)), F(w / float(size))
    j = size - 1 - ox if flip else ox
    src_y, src_x = F(F(oy) * sy), F(F(j) * sx)
    y0, x0 = int(np.floor(src_y)), int(np.floor(src_x))
    y1, x1 = min(y0 + 1, h - 1), min(x0 + 1, w - 1)
    fy, fx = F(src_y - F(y0)), F(src_x - F(x0))
    gy, gx = F(F(1) - fy), F(F(1) - fx)
    a, b, cc, d = F(img[y0, x0, c]), F(img[y0, x1, c]), F(img[y1, x0, c]), F(img[y1, x1, c])
    top = F(F(a * gx) + F(b * fx))
    bot = F(F(cc * gx) + F(d * fx))
    v = F(F(top * gy) + F(bot * fy))
    return F(F(v / F(127.5)) - F(1))


def pack(case, wrong=None):
    """(raw, table) of a case as numpy arrays; ``wrong == "unpadded_offsets"``: a table whose offsets ignore the padding
    to 16 bytes."""
    raw, tab, geom = D.pack_batch(case.images(), case.flips, case.size, case.channels)
    table = tab.numpy().view(D.TABLE_DTYPE).reshape(-1).copy()
    if wrong == "unpadded_offsets":
        sizes = [h * w * case.channels for h, w in case.shapes]
        table["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return raw.numpy(), table


WRONG_KERNELS = ("fma", "reciprocal", "wide_finish", "half_pixel", "hi_unclamped", "source_flipped", "rows_flipped",
                 "unpadded_offsets")


def restated(case, wrong=None):
    raw, table = pack(case, wrong)
    return kernel_model(raw, table, case.size, case.channels, None if wrong == "unpadded_offsets" else wrong)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
