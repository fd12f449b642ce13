"""Writes tests/golden/jpeg_cases.npz: JPEG files encoded by Pillow and Pillow's (libjpeg-turbo's) decoded pixels for
each, the fixtures of tests/test_jpeg.py and tests/test_gpu_jpeg.py.  Needs Pillow; the tests do not.

    python tests/golden/make_jpeg.py

Keys: ``names`` (one string per case), ``jpeg_<name>`` the file's bytes (uint8), ``rgb_<name>`` Pillow's decode at its
default settings ([h, w, 3] for colour files, [h, w] for grey ones), ``y_<name>`` for the colour files the greyscale
output of the decoder (``draft('L')``: the Y plane), ``versions``.  The progressive case stores no pixels."""
import io
import os

import numpy as np
from PIL import Image, features

SIZES = [(1, 1), (8, 8), (16, 16), (29, 37), (33, 18), (50, 41)]                 # (width, height)
MODES = [("444q90", "RGB", 0, 90), ("444q100", "RGB", 0, 100), ("422q75", "RGB", 1, 75), ("420q30", "RGB", 2, 30),
         ("420q75", "RGB", 2, 75), ("420q100", "RGB", 2, 100), ("greyq85", "L", None, 85)]


def pattern(w, h, seed):
    """A smooth pattern plus noise that reaches 0 and 255, so that q100 saturates the clamp."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([127.5 + 127.5 * np.sin(0.21 * x + 0.13 * y + k) * np.cos(0.08 * x - 0.17 * y + 2 * k)
                     for k in range(3)], axis=2)
    noisy = base + rng.normal(0, 40, (h, w, 3))
    noisy[rng.random((h, w)) < 0.1] = 255
    noisy[rng.random((h, w)) < 0.1] = 0
    return np.clip(np.rint(noisy), 0, 255).astype(np.uint8)


def encode(img, mode, **kw):
    im = Image.fromarray(img if mode == "RGB" else img[:, :, 0], mode)
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def decode_y(data):
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert im.mode == "L"
    return np.asarray(im)


def main():
    out, names = {}, []

    def add(name, data, pixels=True, y=False):
        names.append(name)
        out["jpeg_" + name] = np.frombuffer(data, np.uint8)
        if pixels:
            out["rgb_" + name] = decode(data)
        if y:
            out["y_" + name] = decode_y(data)
    seed = 0
    for w, h in SIZES:
        for tag, mode, sub, q in MODES:
            seed += 1
            kw = dict(quality=q) if sub is None else dict(quality=q, subsampling=sub)
            add("%dx%d_%s" % (w, h, tag), encode(pattern(w, h, seed), mode, **kw),
                y=mode == "RGB")
    add("optimize_29x37", encode(pattern(29, 37, 101), "RGB", quality=80, subsampling=2, optimize=True), y=True)
    rb = encode(pattern(50, 41, 102), "RGB", quality=75, subsampling=2, restart_marker_blocks=2)
    rr = encode(pattern(33, 50, 103), "RGB", quality=85, subsampling=1, restart_marker_rows=1)
    assert b"\xff\xdd" in rb and b"\xff\xd0" in rb and b"\xff\xdd" in rr and b"\xff\xd0" in rr
    add("restart_blocks_50x41", rb, y=True)
    add("restart_rows_33x50", rr, y=True)
    add("rows_160x144", encode(pattern(160, 144, 104), "RGB", quality=75, subsampling=2), y=True)
    add("progressive_16x16", encode(pattern(16, 16, 105), "RGB", quality=75, progressive=True), pixels=False)
    out["names"] = np.array(names)
    out["versions"] = np.array(["Pillow " + Image.__version__ if hasattr(Image, "__version__") else "Pillow",
                                "libjpeg-turbo " + str(features.version("libjpeg_turbo") or features.version("jpg"))])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases;", " / ".join(out["versions"]))


if __name__ == "__main__":
    main()
