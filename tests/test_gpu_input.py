"""Device-side input preprocessing on the GPU: bg_image_batch_u8 against data.py's host path bit for bit on the case
table of tests/input_ref.py (guard bands, inputs untouched, a second run), the capped grid, the argument checks, the
per-entry bounds guard, then BatchLoader's device path against its host path and training from a PNG folder."""
import math
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data as D, functional as Fn, hip, model, scope as S, utils
from tests import input_ref as R
from tests.common import make_args

pytestmark = pytest.mark.gpu

BAND = 4096                                             # floats on either side of the output (keeps its 16-byte alignment)


def _banded_out(n, size, c, shift=0):
    numel = n * size * size * c
    buf = torch.full((BAND + shift + numel + BAND,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[BAND + shift:BAND + shift + numel].view(n, size, size, c)


def _bands_intact(buf, numel, shift=0):
    return bool(torch.isnan(buf[:BAND + shift]).all()) and bool(torch.isnan(buf[BAND + shift + numel:]).all())


def _check_case(case, shift=0):
    raw, table, geom = D.pack_batch(case.images(), case.flips, case.size, case.channels)
    n, size, c = geom["n"], case.size, case.channels
    raw_d, table_d = raw.cuda(), table.cuda()
    buf, out = _banded_out(n, size, c, shift)
    got = Fn.image_batch_u8(raw_d, table_d, n, size, c, out=out)
    assert got.data_ptr() == out.data_ptr()
    first = out.cpu().numpy()
    want = case.want()
    diff = int((R.bits(first) != R.bits(want)).sum())
    print(case, "elements that differ from the host path: %d of %d" % (diff, want.size))
    assert diff == 0
    assert _bands_intact(buf, out.numel(), shift)
    assert torch.equal(raw_d.cpu(), raw) and torch.equal(table_d.cpu(), table)
    # again, through the C entry point itself: return code 0 and the same bits
    out.fill_(float("nan"))
    rc = hip.lib().bg_image_batch_u8(hip.ptr(raw_d), raw.numel(), hip.ptr(table_d), n, size, c, hip.ptr(out), hip.stream())
    assert rc == 0
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(first))
    assert _bands_intact(buf, out.numel(), shift)


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_kernel_equals_the_host_path_bit_for_bit(case):
    _check_case(case)


@pytest.mark.parametrize("case", [c for c in R.CASES if c.channels == 4], ids=repr)
def test_four_channels_into_an_output_that_is_not_16_byte_aligned(case):
    _check_case(case, shift=1)                          # the scalar-store variant of C = 4


def test_more_pixels_than_one_pass_of_the_grid():
    case = R.GRID_STRIDE
    assert len(case.shapes) * case.size ** 2 > 3 * 4096 * 256      # the third and later strides too
    _check_case(case)


def test_argument_errors_return_before_any_launch():
    case = R.RAGGED
    raw, table, geom = D.pack_batch(case.images(), case.flips, case.size)
    raw_d, table_d = raw.cuda(), table.cuda()
    buf, out = _banded_out(6, 6, 3)
    L = hip.lib()
    ok = dict(raw=hip.ptr(raw_d), raw_bytes=raw.numel(), table=hip.ptr(table_d), n=6, S=6, C=3, out=hip.ptr(out))

    def call(**kw):
        a = dict(ok, **kw)
        return L.bg_image_batch_u8(a["raw"], a["raw_bytes"], a["table"], a["n"], a["S"], a["C"], a["out"], hip.stream())
    for bad in (dict(raw=None), dict(table=None), dict(out=None), dict(C=2), dict(S=0), dict(S=-3), dict(n=0), dict(n=-1),
                dict(raw_bytes=0), dict(raw_bytes=-1)):
        assert call(**bad) == 1, bad                    # BG_ERR_ARG
        assert b"bg_image_batch_u8" in L.bg_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                 # nothing was launched
    with pytest.raises(RuntimeError):
        Fn.image_batch_u8(raw_d, table_d.float(), 6, 6, 3)
    with pytest.raises(RuntimeError):
        Fn.image_batch_u8(raw_d, table_d, 5, 6, 3)
    with pytest.raises(RuntimeError):
        Fn.image_batch_u8(raw_d, table_d, 6, 6, 3, raw_bytes=raw.numel() + 1)
    assert call() == 0


@pytest.mark.parametrize("channels", [3, 4])
def test_an_entry_past_raw_bytes_gives_nan_and_reads_nothing(channels):
    """Image 1's pixels lie last in the buffer and the DECLARED raw_bytes stop short of their end, while the allocation
    holds all of them: even a kernel without the guard reads valid memory here."""
    rng = np.random.default_rng(17)
    imgs = [rng.integers(0, 256, s + (channels,), dtype=np.uint8) for s in ((11, 7), (9, 10), (5, 13))]
    flips = [1, 0, 1]
    raw, table, geom = D.pack_batch([imgs[0], imgs[2], imgs[1]], [flips[0], flips[2], flips[1]], 6, channels)
    table = table[[0, 2, 1]].contiguous()               # entry 1 -> the last image of the buffer
    declared = geom["offsets"][2] + imgs[1].size - 1
    assert geom["offsets"][2] + imgs[1].size <= raw.numel() and declared > geom["offsets"][1] + imgs[2].size
    raw_d, table_d = raw.cuda(), table.cuda()
    buf, out = _banded_out(3, 6, channels)
    Fn.image_batch_u8(raw_d, table_d, 3, 6, channels, raw_bytes=declared, out=out)
    got = out.cpu().numpy()
    want = R.host_path(imgs, flips, 6, channels)
    assert np.isnan(got[1]).all()
    assert np.array_equal(R.bits(got[0]), R.bits(want[0])) and np.array_equal(R.bits(got[2]), R.bits(want[2]))
    assert _bands_intact(buf, out.numel())
    # with all bytes declared the same table is complete
    Fn.image_batch_u8(raw_d, table_d, 3, 6, channels, out=out)
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(want))
    # a bad height, a bad width and a misaligned offset are refused the same way
    for word, value in ((2, 0), (3, -4), (0, 8)):
        t = table.clone()
        t[1, word] = value
        Fn.image_batch_u8(raw_d, t.cuda(), 3, 6, channels, out=out)
        got = out.cpu().numpy()
        assert np.isnan(got[1]).all() and np.array_equal(R.bits(got[0]), R.bits(want[0])), (word, value)


# ---------------------------------------------------------------- the loader
SIZES = [(80, 80), (70, 90), (64, 64)]


def _png_folder(root, n=12, channels=3):
    folder = os.path.join(str(root), "dataset", "toy")
    os.makedirs(folder)
    rng = np.random.default_rng(3)
    for i in range(n):
        h, w = SIZES[i % 3]
        utils.write_png(rng.integers(0, 256, (h, w, channels), dtype=np.uint8), os.path.join(folder, "%02d.png" % i))
    with open(os.path.join(str(root), "labels.tsv"), "w") as f:
        for i in range(n):
            f.write("%02d.png\t%d\t%d\n" % (i, i, i % 3))
    return os.path.join(str(root), "dataset")


def _batches(files, labels, flip, option, count=3, batch=4, **kw):
    ld = D.BatchLoader(files, labels, batch, D.ImageData(64, 3, True, flip, seed=5), "cuda", seed=7, workers=1,
                       device_preprocess=option, **kw)
    assert ld.device_preprocess is bool(option)
    try:
        out = [next(ld) for _ in range(count)]
        torch.cuda.synchronize()
        return [(x.cpu(), l.cpu()) for x, l in out]
    finally:
        ld.close()


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
def test_loader_device_path_equals_its_host_path(tmp_path, flip):
    root = _png_folder(tmp_path)
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), root=root)
    dev = _batches(files, labels, flip, True)
    host = _batches(files, labels, flip, False)
    for (x, l), (xr, lr) in zip(dev, host):
        assert x.dtype == torch.float32 and tuple(x.shape) == (4, 64, 64, 3)
        assert np.array_equal(R.bits(x.numpy()), R.bits(xr.numpy())) and torch.equal(l, lr)
    assert not torch.equal(dev[0][0], dev[1][0])
    if flip:                                            # the draws did flip something
        plain = _batches(files, labels, False, True)
        assert any(not torch.equal(a[0], b[0]) for a, b in zip(dev, plain))


def test_two_ranks_partition_an_epoch_on_the_device_path(tmp_path):
    root = _png_folder(tmp_path)
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), root=root)
    seen = []
    for rank in range(2):
        for x, l in _batches(files, labels, True, True, count=2, batch=3, rank=rank, world=2):
            assert tuple(x.shape) == (3, 64, 64, 3) and bool(torch.isfinite(x).all())
            seen += [int(v) for v in l[:, 0]]
    assert sorted(seen) == list(range(12))              # 2 ranks x 2 steps x 3 images: one epoch, every file once


def test_a_batch_that_cannot_be_packed_takes_the_host_path(tmp_path):
    folder = tmp_path / "dataset" / "odd"
    folder.mkdir(parents=True)
    rng = np.random.default_rng(4)
    for i in range(4):
        a = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
        np.save(str(folder / ("%d.npy" % i)), a.astype(np.float32) if i == 2 else a)
    files, _ = D.load_data("odd", "", root=str(tmp_path / "dataset"))

    def one(option):
        ld = D.BatchLoader(files, None, 4, D.ImageData(16, 3, True, True, seed=5), "cuda", seed=7, workers=1,
                           device_preprocess=option)
        try:
            return next(ld).cpu()
        finally:
            ld.close()
    assert torch.equal(one(True), one(False))


def test_the_automatic_switch_finishes_large_sources_on_the_host(tmp_path):
    """80 x 80 -> 16: the packed bytes are 6.25 x the fp32 batch, so None decodes and finishes on the host (no packed
    batch reaches the queue), True still packs, and all three settings give the same bits."""
    root = _png_folder(tmp_path)
    files, _ = D.load_data("toy", "", root=root)
    files = [f for i, f in enumerate(files) if i % 3 == 0]                # the four 80 x 80 files

    def one(option):
        ld = D.BatchLoader(files, None, 4, D.ImageData(16, 3, True, False, seed=5), "cuda", seed=7, workers=1,
                           device_preprocess=option)                      # no flips: the probe below draws nothing
        try:
            packed = ld.device_preprocess and isinstance(ld._decode_and_pack([0, 1, 2, 3]), D.PackedBatch)
            return packed, next(ld).cpu()
        finally:
            ld.close()
    (pn, xn), (pt, xt), (pf, xf) = one(None), one(True), one(False)
    assert (pn, pt, pf) == (False, True, False)
    assert torch.equal(xt, xf) and torch.equal(xn, xf) and bool(torch.isfinite(xt).all())


# ---------------------------------------------------------------- training
def test_train_from_a_png_folder_on_the_device_path(tmp_path, monkeypatch):
    _png_folder(tmp_path, n=8)
    monkeypatch.chdir(tmp_path)                         # train() opens ./dataset/<name>
    monkeypatch.delenv("BG_DEVICE_INPUT", raising=False)
    gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, iteration=2, epoch=1, dataset="toy",
                                 random_flip="false", checkpoint_dir=str(tmp_path / "ckpt")),
                       store=S.VariableStore("cuda")).build_model()
    dev, host = gan.open_dataset(device_preprocess=None), gan.open_dataset(device_preprocess=False)
    try:
        assert dev.device_preprocess and not host.device_preprocess
        a, b = next(dev), next(host)
        assert a.is_cuda and tuple(a.shape) == (4, 64, 64, 3)
        assert np.array_equal(R.bits(a.cpu().numpy()), R.bits(b.cpu().numpy()))
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
