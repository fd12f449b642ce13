"""JPEG input on the GPU: bg_jpeg_batch_u8 (dequantisation, inverse DCT, upsampling, colour) on every fixture of
tests/golden/jpeg_cases.npz as ONE batch of mixed sizes and samplings, byte for byte against libjpeg-turbo's pixels; the
resize after it against the host path bit for bit; a slot filled from a PNG stays as it is; argument errors; the per-entry
guard; then BatchLoader's device path against its host path on a JPEG folder and a mixed one, two ranks, and training
from a JPEG folder.  All gates are exact equality."""
import math
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data as D, functional as Fn, hip, model, scope as S, utils
from tests import jpeg_ref as J
from tests.common import make_args

pytestmark = pytest.mark.gpu

BAND = 4096                                             # guard bytes on either side of raw and of the workspace


def _images(names, channels):
    return [D.JpegImage(*D.jpeg_entropy_decode(J.BYTES[n]), channels=channels) for n in names]


def _banded(t, fill):
    """A device copy of the 1-D tensor t between two guard bands (BAND is a multiple of 16: alignment is kept)."""
    buf = torch.full((BAND + t.numel() + BAND,), fill, dtype=t.dtype, device="cuda")
    buf[BAND:BAND + t.numel()] = t.cuda()
    return buf, buf[BAND:BAND + t.numel()]


def _bands_intact(buf, numel, fill):
    return bool((buf[:BAND] == fill).all()) and bool((buf[BAND + numel:] == fill).all())


def _run(raw, table, geom, jtable=None):
    """bg_jpeg_batch_u8 on a packed batch; raw and the workspace sit between guard bands.  Returns the filled raw (numpy),
    the device tensors and the image table after the call."""
    j = geom["jpeg"]
    jt = (j["table"] if jtable is None else jtable).cuda()
    coef_d, table_d = j["coef"].cuda(), table.cuda()
    raw_buf, raw_d = _banded(raw, 0xA5)
    need = Fn.jpeg_batch_workspace_bytes(j["n"], j["blocks"])
    ws_buf, ws = _banded(torch.zeros(need, dtype=torch.uint8), 0x5A)
    out = Fn.jpeg_batch_u8(coef_d, jt, j["n"], j["blocks"], j["max_pixels"], raw_d, table_d, geom["n"], ws=ws)
    assert out.data_ptr() == raw_d.data_ptr()
    torch.cuda.synchronize()
    assert _bands_intact(raw_buf, raw.numel(), 0xA5) and _bands_intact(ws_buf, need, 0x5A)
    assert torch.equal(coef_d.cpu(), j["coef"]) and torch.equal(jt.cpu(), j["table"] if jtable is None else jtable)
    return raw_d.cpu().numpy(), raw_d, table_d


def _slot(view, geom, i, channels):
    h, w = geom["shapes"][i]
    off = geom["offsets"][i]
    return view[off:off + h * w * channels].reshape(h, w, channels)


@pytest.mark.parametrize("channels", [3, 1])
def test_all_fixtures_as_one_batch_equal_libjpeg_byte_for_byte(channels):
    """1x1, single MCUs, sizes that are no multiple of 8 or 16, odd chroma widths, restart intervals, saturating blocks, all
    three samplings and grey files in one launch; the 160x144 file alone has 270 blocks, more than eight workgroups."""
    names = J.DECODABLE
    imgs = _images(names, channels)
    raw, table, geom = D.pack_batch(imgs, [False] * len(imgs), 16, channels)
    assert geom["jpeg"]["blocks"] > 32 * 8 and {im.info["hs"] * 10 + im.info["vs"] for im in imgs} == {11, 21, 22}
    view, raw_d, table_d = _run(raw, table, geom)
    assert torch.equal(table_d.cpu(), table)            # every entry was valid: nothing is marked
    wrong = []
    for i, name in enumerate(names):
        want = J.want(name, channels)
        diff = int((_slot(view, geom, i, channels) != want).sum())
        if diff:
            wrong.append((name, diff, want.size))
    print("fixtures with bytes that differ from libjpeg-turbo (name, bytes, of):", wrong)
    assert not wrong
    for i in range(len(names)):                         # the padding between slots stays zero
        end = geom["offsets"][i + 1] if i + 1 < len(names) else raw.numel()
        h, w = geom["shapes"][i]
        assert not view[geom["offsets"][i] + h * w * channels:end].any()


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
def test_the_resize_after_it_equals_the_host_path_bit_for_bit(flip):
    names = ["29x37_420q75", "33x18_422q75", "50x41_444q90", "1x1_420q30", "16x16_greyq85", "restart_rows_33x50"]
    imgs = _images(names, 3)
    flips = [flip] * len(names)
    batch = D.PackedBatch(*D.pack_batch(imgs, flips, 24, 3))
    got = batch.to_device(torch.device("cuda")).cpu().numpy()
    want = np.stack([D.finish_on_host(D.decode_jpeg(J.BYTES[n], 3), 24, flip) for n in names])
    assert got.shape == want.shape == (6, 24, 24, 3)
    assert np.array_equal(J.bits(got), J.bits(want))
    ref = np.stack([D.finish_on_host(J.want(n, 3), 24, flip) for n in names])      # and so libjpeg-turbo's pixels
    assert np.array_equal(J.bits(got), J.bits(ref))


def test_a_slot_filled_from_a_png_is_left_untouched():
    rng = np.random.default_rng(9)
    png = [rng.integers(0, 256, (13, 11, 3), dtype=np.uint8), rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)]
    names = ["29x37_420q100", "8x8_444q100"]
    jp = _images(names, 3)
    imgs = [png[0], jp[0], png[1], jp[1]]
    raw, table, geom = D.pack_batch(imgs, [0, 1, 1, 0], 16, 3)
    assert geom["jpeg"]["images"] == [1, 3]
    view, raw_d, table_d = _run(raw, table, geom)
    assert np.array_equal(_slot(view, geom, 0, 3), png[0]) and np.array_equal(_slot(view, geom, 2, 3), png[1])
    assert np.array_equal(_slot(view, geom, 1, 3), J.want(names[0], 3))
    assert np.array_equal(_slot(view, geom, 3, 3), J.want(names[1], 3))
    got = Fn.image_batch_u8(raw_d.contiguous(), table_d, 4, 16, 3).cpu().numpy()
    want = np.stack([D.finish_on_host(a, 16, f) for a, f in zip([png[0], J.want(names[0], 3), png[1], J.want(names[1], 3)],
                                                                 [0, 1, 1, 0])])
    assert np.array_equal(J.bits(got), J.bits(want))


def test_argument_errors_return_before_any_launch():
    imgs = _images(["16x16_420q75", "8x8_greyq85"], 3)
    raw, table, geom = D.pack_batch(imgs, [0, 0], 16, 3)
    j = geom["jpeg"]
    coef_d, jt, table_d = j["coef"].cuda(), j["table"].cuda(), table.cuda()
    raw_buf, raw_d = _banded(raw, 0xA5)
    raw_d.fill_(0xA5)
    need = Fn.jpeg_batch_workspace_bytes(2, j["blocks"])
    assert need == 16 + 64 * j["blocks"]
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    L = hip.lib()
    ok = dict(coef=hip.ptr(coef_d), coef_count=coef_d.numel(), jpegs=hip.ptr(jt), n_jpeg=2, blocks=j["blocks"],
              max_pixels=j["max_pixels"], raw=hip.ptr(raw_d), raw_bytes=raw.numel(), table=hip.ptr(table_d), n=2,
              ws=hip.ptr(ws), ws_bytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return L.bg_jpeg_batch_u8(a["coef"], a["coef_count"], a["jpegs"], a["n_jpeg"], a["blocks"], a["max_pixels"],
                                  a["raw"], a["raw_bytes"], a["table"], a["n"], a["ws"], a["ws_bytes"], hip.stream())
    odd = hip.c_void_p(coef_d.data_ptr() + 2)
    for bad in (dict(coef=None), dict(jpegs=None), dict(raw=None), dict(table=None), dict(ws=None), dict(n_jpeg=0),
                dict(n_jpeg=-1), dict(n_jpeg=3), dict(n=1), dict(blocks=0), dict(blocks=-5), dict(coef_count=0),
                dict(raw_bytes=0), dict(max_pixels=0), dict(ws_bytes=need - 1), dict(coef=odd)):
        assert call(**bad) == 1, bad                    # BG_ERR_ARG
        assert b"bg_jpeg_batch_u8" in L.bg_last_error()
    torch.cuda.synchronize()
    assert bool((raw_buf == 0xA5).all()) and bool((ws == 0x5A).all()) and torch.equal(table_d.cpu(), table)
    for kw in (dict(coef=coef_d.int()), dict(jt=jt.float()), dict(n=3), dict(ws=ws[:need - 1])):
        with pytest.raises(RuntimeError):
            Fn.jpeg_batch_u8(kw.get("coef", coef_d), kw.get("jt", jt), 2, j["blocks"], j["max_pixels"], raw_d, table_d,
                             kw.get("n", 2), ws=kw.get("ws", ws))
    with pytest.raises(RuntimeError):
        Fn.jpeg_batch_u8(coef_d, jt, 2, j["blocks"], j["max_pixels"], raw_d, table_d, 2, raw_bytes=raw.numel() + 1)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_slot(raw_d.cpu().numpy(), geom, 0, 3), J.want("16x16_420q75", 3))


# word indices of BgJpegEntry as int32 [120] (data.JPEG_TABLE_DTYPE)
W_SLOT, W_W, W_H, W_CHANNELS, W_NCOMP, W_HS, W_VS, W_BLOCK0, W_IMAGE, W_COEF0, W_BW0, W_BH0, W_COEF2 = \
    0, 2, 3, 4, 5, 6, 7, 8, 9, 12, 14, 15, 20


@pytest.mark.parametrize("word,value", [
    (W_SLOT, 8), (W_SLOT, -16), (W_SLOT, 1 << 30),      # misaligned, negative, past raw
    (W_W, 0), (W_W, 64), (W_H, -3), (W_H, 1 << 20),     # sizes that the block grid does not cover, or no size
    (W_CHANNELS, 4), (W_CHANNELS, 0), (W_NCOMP, 2), (W_NCOMP, 4),
    (W_HS, 3), (W_HS, 1), (W_VS, 1), (W_VS, 0),         # samplings that are not supported, or not this grid's
    (W_BLOCK0, -1), (W_BLOCK0, 1 << 30), (W_BLOCK0, 8), # block range outside the batch, or inside its predecessor's
    (W_COEF0, -64), (W_COEF0, 4), (W_COEF0, 1 << 30), (W_COEF2, 1 << 30),      # coefficient extents
    (W_BW0, 1 << 12), (W_BH0, 1 << 12), (W_BW0, 0),     # block grids
], ids=lambda v: str(v))
def test_an_entry_that_leaves_a_buffer_gives_a_nan_image_and_correct_neighbours(word, value):
    """Entry 1 (29x37, 4:2:0) is broken in one word; its slot must stay as it was and its image come out as NaN, while
    the images before and after it are decoded as always.  The guard bands around raw and the workspace stay intact."""
    names = ["33x18_422q75", "29x37_420q75", "16x16_444q90"]
    imgs = _images(names, 3)
    raw, table, geom = D.pack_batch(imgs, [0, 1, 0], 16, 3)
    jtable = geom["jpeg"]["table"].clone()
    jtable[1, word] = value
    if word in (W_SLOT, W_COEF0, W_COEF2) and value < 0:
        jtable[1, word + 1] = -1                        # the high word of the int64
    view, raw_d, table_d = _run(raw, table, geom, jtable)
    assert not _slot(view, geom, 1, 3).any()            # nothing was written for it
    assert np.array_equal(_slot(view, geom, 0, 3), J.want(names[0], 3))
    assert np.array_equal(_slot(view, geom, 2, 3), J.want(names[2], 3))
    got = Fn.image_batch_u8(raw_d.contiguous(), table_d, 3, 16, 3).cpu().numpy()
    want = np.stack([D.finish_on_host(J.want(n, 3), 16, f) for n, f in zip(names, [0, 1, 0])])
    assert np.isnan(got[1]).all()
    assert np.array_equal(J.bits(got[0]), J.bits(want[0])) and np.array_equal(J.bits(got[2]), J.bits(want[2]))


# ---------------------------------------------------------------- the loader
JPEG_FILES = ["29x37_420q75", "33x18_422q75", "50x41_444q90", "16x16_greyq85", "restart_blocks_50x41", "rows_160x144",
              "50x41_420q100", "29x37_444q100", "optimize_29x37", "33x18_420q30", "restart_rows_33x50", "50x41_greyq85"]


def _folder(root, mixed, n=12):
    """n files written from the fixture bytes; ``mixed``: every third one is a PNG instead."""
    folder = os.path.join(str(root), "dataset", "toy")
    os.makedirs(folder)
    rng = np.random.default_rng(3)
    for i in range(n):
        path = os.path.join(folder, "%02d.jpg" % i)
        if mixed and i % 3 == 1:
            utils.write_png(rng.integers(0, 256, (40 + i, 30, 3), dtype=np.uint8), path)
        else:
            with open(path, "wb") as f:
                f.write(J.BYTES[JPEG_FILES[i % len(JPEG_FILES)]])
    with open(os.path.join(str(root), "labels.tsv"), "w") as f:
        for i in range(n):
            f.write("%02d.jpg\t%d\t%d\n" % (i, i, i % 3))
    return os.path.join(str(root), "dataset")


def _batches(files, labels, flip, option, count=3, batch=4, channels=3, **kw):
    ld = D.BatchLoader(files, labels, batch, D.ImageData(32, channels, True, flip, seed=5), "cuda", seed=7, workers=1,
                       device_preprocess=option, **kw)
    assert ld.device_preprocess is bool(option)
    try:
        out = [next(ld) for _ in range(count)]
        torch.cuda.synchronize()
        return [(x.cpu(), l.cpu()) for x, l in out]
    finally:
        ld.close()


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("mixed", [False, True], ids=["jpeg", "mixed"])
def test_loader_device_path_equals_its_host_path(tmp_path, mixed, flip):
    root = _folder(tmp_path, mixed)
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), root=root)
    dev = _batches(files, labels, flip, True)
    host = _batches(files, labels, flip, False)
    for (x, l), (xr, lr) in zip(dev, host):
        assert x.dtype == torch.float32 and tuple(x.shape) == (4, 32, 32, 3) and bool(torch.isfinite(x).all())
        assert np.array_equal(J.bits(x.numpy()), J.bits(xr.numpy())) and torch.equal(l, lr)
    assert not torch.equal(dev[0][0], dev[1][0])
    # the device path did go through the coefficients: the worker packs JpegImage objects
    ld = D.BatchLoader(files, labels, 4, D.ImageData(32, 3, True, False, seed=5), "cuda", seed=7, workers=1,
                       device_preprocess=True)
    try:
        packed = ld._decode_and_pack([0, 1, 2, 3])
        assert isinstance(packed, D.PackedBatch) and packed.geom["jpeg"]["n"] == (3 if mixed else 4)
    finally:
        ld.close()


def test_loader_at_one_channel_and_the_automatic_switch(tmp_path):
    """One output channel takes the Y plane on both paths.  Under the automatic switch a batch whose uploaded bytes
    (coefficients and entries) exceed JPEG_OVER_OUT_MAX times its fp32 bytes is finished on the host, with the same bits."""
    root = _folder(tmp_path, False)
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), root=root)
    dev = _batches(files, labels, True, True, count=2, channels=1)
    host = _batches(files, labels, True, False, count=2, channels=1)
    for (x, _), (xr, _) in zip(dev, host):
        assert tuple(x.shape) == (4, 32, 32, 1) and np.array_equal(J.bits(x.numpy()), J.bits(xr.numpy()))
    big = [files[5]] * 4                                 # 160x144 4:2:0: 270 blocks = 34560 bytes against 8 * 8 * 3 fp32
    assert D.JPEG_OVER_OUT_MAX == 40.0 and 35040 > 40 * 768 and 35040 < 40 * 12288

    def one(option, size):
        ld = D.BatchLoader(big, None, 4, D.ImageData(size, 3, True, False, seed=5), "cuda", seed=7, workers=1,
                           device_preprocess=option)
        try:
            packed = ld.device_preprocess and isinstance(ld._decode_and_pack([0, 1, 2, 3]), D.PackedBatch)
            return packed, next(ld).cpu()
        finally:
            ld.close()
    (pn, xn), (pt, xt), (pf, xf) = one(None, 8), one(True, 8), one(False, 8)
    assert (pn, pt, pf) == (False, True, False)
    assert torch.equal(xt, xf) and torch.equal(xn, xf) and bool(torch.isfinite(xt).all())
    assert one(None, 32)[0] is True                     # 34560 + 480 bytes against 40 * 12288


def test_two_ranks_partition_an_epoch_on_the_device_path(tmp_path):
    root = _folder(tmp_path, True)
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), root=root)
    seen = []
    for rank in range(2):
        for x, l in _batches(files, labels, True, True, count=2, batch=3, rank=rank, world=2):
            assert tuple(x.shape) == (3, 32, 32, 3) and bool(torch.isfinite(x).all())
            seen += [int(v) for v in l[:, 0]]
    assert sorted(seen) == list(range(12))              # 2 ranks x 2 steps x 3 images: one epoch, every file once


# ---------------------------------------------------------------- training
def test_train_from_a_jpeg_folder_on_the_device_path(tmp_path, monkeypatch):
    _folder(tmp_path, False, n=8)
    monkeypatch.chdir(tmp_path)                         # train() opens ./dataset/<name>
    monkeypatch.delenv("BG_DEVICE_INPUT", raising=False)
    gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, iteration=2, epoch=1, dataset="toy",
                                 random_flip="false", checkpoint_dir=str(tmp_path / "ckpt")),
                       store=S.VariableStore("cuda")).build_model()
    dev, host = gan.open_dataset(device_preprocess=None), gan.open_dataset(device_preprocess=False)
    try:
        assert dev.device_preprocess and not host.device_preprocess
        assert isinstance(dev._decode_and_pack([0, 1, 2, 3]), D.PackedBatch)       # the switch keeps the device path
        a, b = next(dev), next(host)
        assert a.is_cuda and tuple(a.shape) == (4, 64, 64, 3)
        assert np.array_equal(J.bits(a.cpu().numpy()), J.bits(b.cpu().numpy()))
    finally:
        dev.close()
        host.close()
    seen, step = [], gan.train_step

    def recording(*args, **kw):
        losses = step(*args, **kw)
        seen.append({k: float(v.item()) for k, v in losses.items()})
        return losses
    monkeypatch.setattr(gan, "train_step", recording)
    gan.train(resume=False)
    assert gan.counter == 2 and len(seen) == 2
    assert all(math.isfinite(v) for d in seen for v in d.values())
