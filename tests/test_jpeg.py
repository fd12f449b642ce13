"""JPEG input, the part that needs no GPU: data.decode_jpeg (numpy, the specification) against libjpeg-turbo's pixels for
every fixture of tests/golden/jpeg_cases.npz, the C entropy decoder against the Python one, what is refused and how,
truncated and corrupted files, decode_image's dispatch, pack_batch's tables for a mixed batch, and the C ABI.  All gates
are exact equality: the arithmetic is integer and fully specified."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data as D, functional as Fn, hip, utils
from tests import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "8x8_420q75"                                    # the file that is truncated and corrupted below


def test_the_fixture_grid_is_complete():
    sizes = ["1x1", "8x8", "16x16", "29x37", "33x18", "50x41"]
    modes = ["444q90", "444q100", "422q75", "420q30", "420q75", "420q100", "greyq85"]
    assert [n for n in J.NAMES[:42]] == ["%s_%s" % (s, m) for s in sizes for m in modes]
    assert J.NAMES[42:] == ["optimize_29x37", "restart_blocks_50x41", "restart_rows_33x50", "rows_160x144",
                            "progressive_16x16"]
    assert J.PROGRESSIVE == ["progressive_16x16"] and len(J.Y_NAMES) >= 2
    assert J.VERSIONS[0].startswith("Pillow ") and J.VERSIONS[1].startswith("libjpeg-turbo ")
    for name in ("restart_blocks_50x41", "restart_rows_33x50"):             # DRI and RSTn are in the files
        assert b"\xff\xdd" in J.BYTES[name] and b"\xff\xd0" in J.BYTES[name]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")) < 1 << 20
    assert int(J.want("16x16_420q100", 3).max()) == 255 and int(J.want("16x16_420q100", 3).min()) == 0      # saturating


@pytest.mark.parametrize("use_lib", [True, False], ids=["c-helper", "python"])
@pytest.mark.parametrize("channels", [3, 1])
def test_decode_jpeg_equals_libjpeg_for_every_fixture(channels, use_lib):
    for name in J.DECODABLE:
        got = D.decode_jpeg(J.BYTES[name], channels, use_lib=use_lib)
        want = J.want(name, channels)
        assert got.dtype == np.uint8 and got.shape == want.shape, name
        diff = int((got != want).sum())
        if diff:
            print(name, "channels", channels, "pixels that differ: %d of %d" % (diff, want.size))
        assert diff == 0, name


def test_c_helper_coefficients_equal_the_python_decoder():
    for name in J.DECODABLE:
        info_c, coef_c = D.jpeg_entropy_decode(J.BYTES[name], use_lib=True)
        info_p, coef_p = D.jpeg_entropy_decode(J.BYTES[name], use_lib=False)
        assert coef_c.dtype == np.int16 and coef_c.shape == (info_p["blocks"], 64)
        assert np.array_equal(coef_c, coef_p), name
        for key in ("w", "h", "ncomp", "hs", "vs", "blocks"):
            assert info_c[key] == info_p[key], (name, key)
        assert [tuple(g) for g in info_c["grids"]] == [tuple(g) for g in info_p["grids"]]
        assert all(np.array_equal(a, b) for a, b in zip(info_c["q"], info_p["q"]))
        h, w = J.want(name, 3).shape[:2]
        assert (info_c["w"], info_c["h"]) == (w, h) and info_c["ncomp"] == (1 if J.is_grey(name) else 3)
    assert D.jpeg_entropy_decode(J.BYTES["33x18_422q75"])[0]["grids"] == [(6, 3), (3, 3), (3, 3)]
    assert D.jpeg_entropy_decode(J.BYTES["29x37_420q75"])[0]["grids"] == [(4, 6), (2, 3), (2, 3)]


@pytest.mark.parametrize("use_lib", [True, False], ids=["c-helper", "python"])
def test_what_is_refused(use_lib):
    with pytest.raises(NotImplementedError, match="progressive"):
        D.decode_jpeg(J.BYTES["progressive_16x16"], 3, use_lib=use_lib)
    with pytest.raises(ValueError):
        D.decode_jpeg(J.BYTES[SMALL], 4, use_lib=use_lib)
    with pytest.raises(ValueError):
        D.decode_jpeg(J.BYTES[SMALL], 2, use_lib=use_lib)
    data = bytearray(J.BYTES[SMALL])
    sof = data.index(b"\xff\xc0")
    for at, value, exc in ((4, 12, NotImplementedError),                    # 12-bit samples
                           (9, 4, ValueError),                               # 4 components in a header sized for 3
                           (11, 0x41, NotImplementedError),                  # luma 4x1
                           (14, 0x21, NotImplementedError),                  # chroma 2x1
                           (1, 0xC9, NotImplementedError)):                  # SOF9: arithmetic coding
        bad = bytearray(data)
        bad[sof + at] = value
        with pytest.raises(exc):
            D.decode_jpeg(bytes(bad), 3, use_lib=use_lib)


@pytest.mark.parametrize("use_lib", [True, False], ids=["c-helper", "python"])
def test_every_truncation_and_some_corruptions_raise_cleanly(use_lib):
    data = J.BYTES[SMALL]
    assert len(data) < 1024
    for k in range(len(data)):                          # every prefix, the one without the end-of-image marker included
        with pytest.raises((ValueError, NotImplementedError)):
            D.decode_jpeg(data[:k], 3, use_lib=use_lib)
    sos = data.index(b"\xff\xda")
    rng = np.random.default_rng(11)
    outcomes = set()
    for at in sorted(set(int(i) for i in rng.integers(2, sos + 14, 200))):   # header bytes, each with three new values
        for value in (0x00, 0xFF, data[at] ^ 0x55):
            bad = bytearray(data)
            bad[at] = value
            try:
                px = D.decode_jpeg(bytes(bad), 3, use_lib=use_lib)
                assert px.dtype == np.uint8 and px.ndim == 3
                outcomes.add("decoded")
            except (ValueError, NotImplementedError) as e:
                outcomes.add(type(e).__name__)
    assert {"ValueError", "NotImplementedError"} <= outcomes


def test_both_entropy_decoders_agree_on_corrupted_scans():
    data = J.BYTES["16x16_420q30"]
    sos = data.index(b"\xff\xda") + 14
    rng = np.random.default_rng(12)
    for at in rng.integers(sos, len(data) - 2, 40):
        bad = bytearray(data)
        bad[int(at)] ^= 1 << int(rng.integers(0, 8))
        res = []
        for use_lib in (True, False):
            try:
                res.append(D.jpeg_entropy_decode(bytes(bad), use_lib=use_lib)[1])
            except ValueError:
                res.append(None)
        assert (res[0] is None) == (res[1] is None), int(at)
        assert res[0] is None or np.array_equal(res[0], res[1])


def test_decode_image_dispatches_by_content(tmp_path):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    utils.write_png(img, str(tmp_path / "a.jpg"))       # the name says nothing
    png = open(str(tmp_path / "a.jpg"), "rb").read()
    assert np.array_equal(D.decode_image(png, 3), img)
    assert np.array_equal(D.decode_image(J.BYTES["29x37_422q75"], 3), J.want("29x37_422q75", 3))
    assert np.array_equal(D.decode_image(J.BYTES["29x37_422q75"], 1), J.want("29x37_422q75", 1))
    with pytest.raises(ValueError):
        D.decode_image(b"GIF89a" + bytes(32), 3)
    with pytest.raises(ValueError, match="not a PNG"):
        D.decode_png(b"not a png at all")
    with pytest.raises(ValueError, match="not a PNG"):
        D.decode_png(J.BYTES[SMALL])                    # decode_png still takes PNG only
    (tmp_path / "b.png").write_bytes(J.BYTES["33x18_420q75"])
    idata = D.ImageData(16, 3, True, False)
    assert np.array_equal(D.decode_file(idata, str(tmp_path / "b.png")), J.want("33x18_420q75", 3))
    j = D.decode_file(idata, str(tmp_path / "b.png"), entropy_only=True)
    assert isinstance(j, D.JpegImage) and j.shape == (18, 33, 3) and np.array_equal(j.decode(), J.want("33x18_420q75", 3))
    assert isinstance(D.decode_file(idata, str(tmp_path / "a.jpg"), entropy_only=True), np.ndarray)
    want = D.finish_on_host(J.want("33x18_420q75", 3), 16, False)
    assert np.array_equal(J.bits(idata.image_processing(str(tmp_path / "b.png"))), J.bits(want))


def test_pack_batch_of_a_mixed_batch():
    names = ["29x37_420q75", "1x1_greyq85", "33x18_422q75", "16x16_444q100"]
    rng = np.random.default_rng(5)
    png = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    imgs = [D.JpegImage(*D.jpeg_entropy_decode(J.BYTES[n]), channels=3) for n in names]
    imgs.insert(2, png)
    flips = [0, 1, 0, 1, 1]
    raw, table, geom = D.pack_batch(imgs, flips, 16, 3)
    t = table.numpy().reshape(-1).view(D.TABLE_DTYPE)
    pos = 0
    for i, img in enumerate(imgs):                      # the image table is what it is for decoded arrays
        h, w = img.shape[:2]
        assert (int(t[i]["offset"]), int(t[i]["h"]), int(t[i]["w"]), int(t[i]["flip"])) == (pos, h, w, flips[i])
        assert pos % 16 == 0 and geom["offsets"][i] == pos and geom["shapes"][i] == (h, w)
        assert t[i]["scale_y"] == np.float32(h / 16.0) and t[i]["scale_x"] == np.float32(w / 16.0)
        pos += -(-(h * w * 3) // 16) * 16
    assert raw.numel() == pos == geom["raw_bytes"]
    view = raw.numpy()
    assert np.array_equal(view[geom["offsets"][2]:geom["offsets"][2] + png.size], png.reshape(-1))      # filled
    for i in (0, 1, 3, 4):                              # JPEG slots arrive empty
        assert not view[geom["offsets"][i]:geom["offsets"][i + 1] if i < 4 else raw.numel()].any()
    j = geom["jpeg"]
    assert j["n"] == 4 and j["images"] == [0, 1, 3, 4] and j["max_pixels"] == 29 * 37
    assert j["table"].dtype == torch.int32 and tuple(j["table"].shape) == (4, 120)
    assert j["coef"].dtype == torch.int16 and j["coef"].numel() == 64 * j["blocks"]
    jt = j["table"].numpy().reshape(-1).view(D.JPEG_TABLE_DTYPE)
    block0 = 0
    for e, i in zip(jt, j["images"]):
        info, coef = imgs[i].info, imgs[i].coef
        assert int(e["slot"]) == geom["offsets"][i] and (int(e["w"]), int(e["h"])) == (info["w"], info["h"])
        assert (int(e["channels"]), int(e["ncomp"]), int(e["hs"]), int(e["vs"])) == (3, info["ncomp"], info["hs"], info["vs"])
        assert int(e["block0"]) == block0 and int(e["image"]) == i and not e["reserved"].any()
        c0 = 64 * block0
        for c, (bw, bh) in enumerate(info["grids"]):
            comp = e["comp"][c]
            assert (int(comp["coef"]), int(comp["bw"]), int(comp["bh"])) == (64 * block0, bw, bh)
            assert int(comp["coef"]) % 8 == 0 and int(comp["coef"]) + 64 * bw * bh <= j["coef"].numel()    # in range
            assert np.array_equal(e["q"][c], info["q"][c])
            block0 += bw * bh
        assert np.array_equal(j["coef"].numpy()[c0:64 * block0], coef.reshape(-1))
        assert int(e["slot"]) + info["w"] * info["h"] * 3 <= raw.numel()
    assert block0 == j["blocks"]
    # without a JPEG image nothing is added; a batch of another channel count does not take the image
    assert D.pack_batch([png], [0], 16, 3)[2]["jpeg"] is None
    assert D.packable(imgs[0], 3) and not D.packable(imgs[0], 1) and not D.packable(imgs[0], 4)
    with pytest.raises(ValueError):
        D.pack_batch(imgs, flips, 16, 1)
    with pytest.raises(ValueError):
        D.JpegImage(imgs[0].info, imgs[0].coef, 4)
    broken = D.JpegImage(dict(imgs[0].info, w=64), imgs[0].coef, 3)         # a header that its coefficients do not fit
    with pytest.raises(ValueError, match="do not agree"):
        D.pack_batch([broken], [0], 16, 3)
    # the automatic switch counts what is uploaded: coefficients and entry for a JPEG, the slot otherwise
    assert D.upload_bytes(imgs[0]) == imgs[0].coef.nbytes + 480 and D.upload_bytes(png) == 112
    assert D.switch_bytes([png, png]) == 224 and D.switch_bytes([png, imgs[0]]) == 112 + D.upload_bytes(imgs[0]) / 40.0
    # 29x37 4:2:0 -> 36 blocks: 5088 bytes; a decoded image of as many bytes would stop paying at 1272 fp32 bytes
    assert D.device_path_pays(D.switch_bytes([imgs[0]]), 1, 4, 3) and not D.device_path_pays(D.upload_bytes(imgs[0]), 1, 4, 3)
    assert not D.device_path_pays(D.switch_bytes([imgs[0]]), 1, 1, 3)


def test_new_symbols_and_the_abi_version():
    L = hip.lib()
    assert hip.ABI_VERSION == 10 and L.bg_abi_version() == 10
    header = open(os.path.join(ROOT, "include", "biggan_hip.h")).read()
    assert re.search(r"#define BG_ABI_VERSION 10\b", header)
    _P, c_int, c_int64, c_size_t, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_char_p
    declared = {
        "bg_jpeg_info": (c_int, [c_char_p, c_size_t, _P]),
        "bg_jpeg_coefficients": (c_int, [c_char_p, c_size_t, _P, c_size_t]),
        "bg_jpeg_batch_workspace_bytes": (c_size_t, [c_int, c_int64]),
        "bg_jpeg_batch_u8": (c_int, [_P, c_int64, _P, c_int, c_int64, c_int, _P, c_int64, _P, c_int, _P, c_size_t, _P]),
    }
    for name, sig in declared.items():
        assert hip.SIGNATURES[name] == sig, name
        assert re.search(r"\b%s\(" % name, header) and getattr(L, name) is not None
    assert "typedef struct BgJpegEntry" in header and "typedef struct BgJpegInfo" in header
    assert ctypes.sizeof(hip.BgJpegInfo) == 440 and D.JPEG_TABLE_DTYPE.itemsize == 480
    assert D.JPEG_TABLE_DTYPE.fields["q"][1] == 96 and D.JPEG_TABLE_DTYPE.fields["comp"][1] == 48
    # the host calls report through the return code and bg_last_error
    info = hip.BgJpegInfo()
    data = J.BYTES[SMALL]
    assert L.bg_jpeg_info(None, 10, ctypes.byref(info)) == 1 and L.bg_jpeg_info(data, len(data), None) == 1
    assert L.bg_jpeg_info(data, len(data), ctypes.byref(info)) == 0
    assert (info.width, info.height, info.ncomp, info.hs, info.vs, info.blocks) == (8, 8, 3, 2, 2, 6)
    coef = np.full(64 * 6 + 64, 77, np.int16)
    ptr = coef.ctypes.data_as(_P)
    assert L.bg_jpeg_coefficients(data, len(data), ptr, 64 * 6 - 1) == 1 and b"coef_count" in L.bg_last_error()
    assert L.bg_jpeg_coefficients(data, len(data), ptr, 64 * 6 + 1) == 1
    assert (coef == 77).all()                           # nothing was written
    assert L.bg_jpeg_coefficients(data, len(data), ptr, 64 * 6) == 0 and (coef[64 * 6:] == 77).all()
    assert L.bg_jpeg_info(J.BYTES["progressive_16x16"], len(J.BYTES["progressive_16x16"]), ctypes.byref(info)) == 3
    assert b"progressive" in L.bg_last_error()
    # the device entry point refuses its arguments before it would launch (no GPU here)
    assert L.bg_jpeg_batch_workspace_bytes(3, 10) == 32 + 640 and L.bg_jpeg_batch_workspace_bytes(0, 10) == 0
    assert L.bg_jpeg_batch_u8(None, 64, None, 1, 1, 1, None, 16, None, 1, None, 1 << 20, None) == 1
    assert b"bg_jpeg_batch_u8" in L.bg_last_error()
    with pytest.raises(RuntimeError):
        Fn.jpeg_batch_u8(torch.zeros(64, dtype=torch.int32), torch.zeros((1, 120), dtype=torch.int32), 1, 1, 1,
                         torch.zeros(16, dtype=torch.uint8), torch.zeros((1, 8), dtype=torch.int32), 1)
