"""Shared by tests/test_jpeg.py and tests/test_gpu_jpeg.py: the fixtures of tests/golden/jpeg_cases.npz (JPEG files
written by Pillow and libjpeg-turbo's decoded pixels, see tests/golden/make_jpeg.py), loaded once and left unchanged."""
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")
_Z = np.load(_PATH)

NAMES = [str(n) for n in _Z["names"]]
VERSIONS = [str(v) for v in _Z["versions"]]
BYTES = {n: _Z["jpeg_" + n].tobytes() for n in NAMES}
DECODABLE = [n for n in NAMES if "rgb_" + n in _Z.files]
PROGRESSIVE = [n for n in NAMES if n not in DECODABLE]
Y_NAMES = [n for n in NAMES if "y_" + n in _Z.files]
_RGB = {n: _Z["rgb_" + n] for n in DECODABLE}
_Y = {n: _Z["y_" + n] for n in Y_NAMES}
for _a in list(_RGB.values()) + list(_Y.values()):
    _a.setflags(write=False)


def is_grey(name):
    return _RGB[name].ndim == 2


def want(name, channels):
    """Pillow's pixels [h, w, channels]; a colour file at one channel is the decoder's greyscale output, its Y plane."""
    px = _RGB[name]
    if px.ndim == 2:
        return np.repeat(px[:, :, None], channels, axis=2)
    if channels == 3:
        return px
    return _Y[name][:, :, None]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
