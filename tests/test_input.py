"""Device-side input preprocessing, the part that needs no GPU: the restatement of bg_image_batch_u8's arithmetic equals
data.py's host path bit for bit on every case and tells every simulated wrong kernel apart; pack_batch's layout and
checks; --weight_file; the ABI; and a CPU loader that the new switch leaves alone."""
import os
import re

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data as D, hip, utils
from tests import input_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the arithmetic contract
@pytest.mark.parametrize("case", R.CASES + [R.GRID_STRIDE], ids=repr)
def test_restatement_equals_the_host_path(case):
    got, want = R.restated(case), case.want()
    assert got.shape == want.shape == (len(case.shapes), case.size, case.size, case.channels)
    assert np.array_equal(R.bits(got), R.bits(want))
    assert -1.0 <= want.min() and want.max() <= 1.0


@pytest.mark.parametrize("case", [c for c in R.CASES if c.size <= 12], ids=repr)
def test_scalar_steps_equal_the_host_path(case):
    want = case.want()
    for n, (img, flip) in enumerate(zip(case.images(), case.flips)):
        for oy in range(case.size):
            for ox in range(case.size):
                for c in range(case.channels):
                    assert R.pixel(img, case.size, flip, oy, ox, c).view(np.uint32) == want[n, oy, ox, c].view(np.uint32)


@pytest.mark.parametrize("wrong", R.WRONG_KERNELS)
def test_every_wrong_kernel_is_told_apart(wrong):
    changed = {}
    for case in R.CASES:
        n = int((R.bits(R.restated(case, wrong)) != R.bits(case.want())).sum())
        if n:
            changed[case.name] = n
    print(wrong, changed)
    assert changed, wrong


def test_fma_needs_the_non_dyadic_cases():
    """80 -> 64 and 160 -> 128 have dyadic weights: every product is exact and a fused lerp changes nothing there."""
    by = {c.name: int((R.bits(R.restated(c, "fma")) != R.bits(c.want())).sum()) for c in R.CASES}
    assert by["80x80_to_64_c3"] == 0 and by["160x160_to_128_c3_x8"] == 0
    assert by["3x11_to_6_c4"] > 0 and by["10x10_to_12_c4"] > 0 and by["100x75_to_96_c3"] > 0


# ---------------------------------------------------------------- pack_batch
def test_pack_batch_layout_of_a_ragged_batch():
    case = R.RAGGED
    raw, table, geom = D.pack_batch(case.images(), case.flips, case.size)
    assert raw.dtype == torch.uint8 and raw.dim() == 1 and not raw.is_pinned()
    assert table.dtype == torch.int32 and tuple(table.shape) == (6, 8)
    assert geom["n"] == 6 and geom["size"] == 6 and geom["channels"] == 3 and geom["raw_bytes"] == raw.numel()
    assert geom["shapes"] == case.shapes
    t = table.numpy().view(D.TABLE_DTYPE).reshape(-1)
    assert D.TABLE_DTYPE.itemsize == 32
    pos = 0
    for i, (img, (h, w)) in enumerate(zip(case.images(), case.shapes)):
        off = int(t["offset"][i])
        assert off == pos == geom["offsets"][i] and off % 16 == 0
        nb = h * w * 3
        assert np.array_equal(raw.numpy()[off:off + nb].reshape(h, w, 3), img)
        pos = off + (nb + 15) // 16 * 16
        assert not raw.numpy()[off + nb:pos].any()                            # the padding is zeroed
        assert (t["h"][i], t["w"][i], t["flip"][i], t["reserved"][i]) == (h, w, case.flips[i], 0)
        assert t["scale_y"][i] == np.float32(h / 6.0) and t["scale_x"][i] == np.float32(w / 6.0)
    assert pos == raw.numel()
    assert [o for o in geom["offsets"]] == [0, 240, 352, 464, 480, 736]
    # little-endian words, as the header documents them
    words = table.numpy()
    assert words[1, 0] == 240 and words[1, 1] == 0 and words[1, 2] == 3 and words[1, 3] == 11 and words[1, 4] == 1
    assert words[1, 5:7].view(np.float32).tolist() == [np.float32(3 / 6.0), np.float32(11 / 6.0)]


def test_pack_batch_rejects_what_the_kernel_cannot_read():
    ok = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError):
        D.pack_batch([], [], 8)
    with pytest.raises(ValueError):
        D.pack_batch([ok, ok.astype(np.float32)], [0, 0], 8)
    with pytest.raises(ValueError):
        D.pack_batch([ok, np.zeros((4, 5, 4), np.uint8)], [0, 0], 8)             # not the batch's channel count
    with pytest.raises(ValueError):
        D.pack_batch([ok], [0], 8, channels=4)
    with pytest.raises(ValueError):
        D.pack_batch([np.zeros((4, 5, 2), np.uint8)], [0], 8)                    # 2 channels
    with pytest.raises(ValueError):
        D.pack_batch([np.zeros((4, 5), np.uint8)], [0], 8, channels=1)           # not [h, w, C]
    with pytest.raises(ValueError):
        D.pack_batch([np.zeros((0, 5, 3), np.uint8)], [0], 8)
    with pytest.raises(ValueError):
        D.pack_batch([ok], [0, 1], 8)
    assert D.pack_batch([ok], [1], 8)[2]["raw_bytes"] == 64


# ---------------------------------------------------------------- --weight_file
def _png_folder(root, name, sizes, channels=3, seed=3):
    folder = os.path.join(str(root), "dataset", name)
    os.makedirs(folder)
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(sizes):
        utils.write_png(rng.integers(0, 256, (h, w, channels), dtype=np.uint8), os.path.join(folder, "%02d.png" % i))
    return os.path.join(str(root), "dataset")


def test_weight_file_repeats_files_as_the_reference_does(tmp_path):
    root = _png_folder(tmp_path, "toy", [(8, 8)] * 4)
    with open(str(tmp_path / "w.tsv"), "w") as f:
        f.write("00.png\t0.5\n02.png\t2.7\n03.png\t3.0\n")                      # 01.png is absent: once
    with open(str(tmp_path / "labels.tsv"), "w") as f:
        for i in range(4):
            f.write("%02d.png\t%d\t%d\n" % (i, i, 10 * i))
    assert D.read_weights(str(tmp_path / "w.tsv")) == {"00.png": 0.5, "02.png": 2.7, "03.png": 3.0}
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), str(tmp_path / "w.tsv"), root=root)
    names = [os.path.basename(p) for p in files]
    assert names == ["01.png"] + ["02.png"] * 2 + ["03.png"] * 3                 # int(w) copies: 0 / 1 / 2 / 3
    assert labels == [[1.0, 10.0]] + [[2.0, 20.0]] * 2 + [[3.0, 30.0]] * 3       # labels follow the repeated list
    plain, _ = D.load_data("toy", "", "", root=root)
    assert len(plain) == 4
    # a dataset that the weights leave smaller than one global batch
    with open(str(tmp_path / "w0.tsv"), "w") as f:
        f.write("00.png\t0\n01.png\t0.9\n02.png\t0\n")
    few, _ = D.load_data("toy", "", str(tmp_path / "w0.tsv"), root=root)
    assert [os.path.basename(p) for p in few] == ["03.png"]
    with pytest.raises(ValueError):
        D.BatchLoader(few, None, 2, D.ImageData(8, 3, True, False), "cpu")


# ---------------------------------------------------------------- ABI
def test_abi_10_declares_and_binds_the_kernel():
    assert hip.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "biggan_hip.h")).read()
    assert re.search(r"#define BG_ABI_VERSION 10\b", header)
    assert re.search(r"\bint bg_image_batch_u8\(", header) and "typedef struct BgImageEntry" in header
    assert "bg_image_batch_u8" in hip.SIGNATURES
    assert "input.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    if os.path.exists(hip.LIB_PATH):
        assert hip.lib().bg_abi_version() == 10


def test_the_entry_point_checks_its_arguments_before_any_launch():
    import ctypes
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                    # never dereferenced: every call below fails validation
    ok = dict(raw=fake, raw_bytes=1024, table=fake, n=2, S=8, C=3, out=fake)

    def call(**kw):
        a = dict(ok, **kw)
        return L.bg_image_batch_u8(a["raw"], a["raw_bytes"], a["table"], a["n"], a["S"], a["C"], a["out"], None)
    for bad in (dict(raw=None), dict(table=None), dict(out=None), dict(C=2), dict(C=5), dict(S=0), dict(S=-1), dict(n=0),
                dict(raw_bytes=0), dict(raw_bytes=-16), dict(table=ctypes.c_void_p(4100)), dict(out=ctypes.c_void_p(4098))):
        assert call(**bad) == 1, bad
        assert b"bg_image_batch_u8" in L.bg_last_error()


def test_the_wrapper_has_no_host_fallback():
    from biggan_tensorflow_amd import functional as Fn
    raw, table, geom = D.pack_batch(R.RAGGED.images(), R.RAGGED.flips, 6)
    with pytest.raises(RuntimeError):
        Fn.image_batch_u8(raw, table, 6, 6, 3)


# ---------------------------------------------------------------- the loader on a CPU device
def test_a_cpu_loader_ignores_the_switch(tmp_path, monkeypatch):
    root = _png_folder(tmp_path, "toy", [(10, 10), (9, 12), (8, 8), (10, 10), (12, 9), (8, 8)])
    files, _ = D.load_data("toy", "", root=root)
    labels = [[float(i)] for i in range(len(files))]
    assert not D.device_input_enabled("cpu", True) and not D.device_input_enabled("cpu", None)
    monkeypatch.setenv("BG_DEVICE_INPUT", "1")

    def batches(option):
        ld = D.BatchLoader(files, labels, 2, D.ImageData(8, 3, True, True, seed=5), "cpu", seed=7, workers=1,
                           device_preprocess=option)
        assert ld.device_preprocess is False
        try:
            return [next(ld) for _ in range(4)]
        finally:
            ld.close()
    ref = batches(False)
    for option in (True, None):
        got = batches(option)
        for (x, l), (xr, lr) in zip(got, ref):
            assert x.dtype == torch.float32 and tuple(x.shape) == (2, 8, 8, 3)
            assert torch.equal(x, xr) and torch.equal(l, lr)


def test_the_switch_resolution(monkeypatch):
    monkeypatch.delenv("BG_DEVICE_INPUT", raising=False)
    assert D.device_input_enabled("cuda", None) and D.device_input_enabled("cuda:1", True)
    assert not D.device_input_enabled("cuda", False)
    monkeypatch.setenv("BG_DEVICE_INPUT", "0")
    assert not D.device_input_enabled("cuda", None)
    assert D.device_input_enabled("cuda", True)             # an explicit option wins over the environment


def test_host_finish_equals_image_processing():
    """The loader's host fallback for a batch that cannot be packed (flip drawn beforehand) is image_processing's own
    arithmetic."""
    case = R.RAGGED
    for img, flip, want in zip(case.images(), case.flips, case.want()):
        assert np.array_equal(R.bits(D.finish_on_host(img, case.size, flip)), R.bits(want))


def test_the_automatic_switch_packs_a_batch_only_while_its_bytes_are_at_most_the_fp32_batch():
    """data.device_path_pays: the two measured datasets fall on either side of the threshold, and the boundary itself
    (raw bytes = fp32 bytes) still packs."""
    assert D.RAW_OVER_OUT_MAX == 1.0
    assert D.device_path_pays(256 * 160 * 160 * 3, 256, 128, 3)              # 0.39: the device path won
    assert not D.device_path_pays(64 * 512 * 512 * 3, 64, 128, 3)            # 4.0: the host path won
    assert D.device_path_pays(4 * 16 * 16 * 3 * 4, 4, 16, 3) and not D.device_path_pays(4 * 16 * 16 * 3 * 4 + 16, 4, 16, 3)
