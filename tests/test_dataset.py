"""The device-resident dataset, the part that needs no GPU: the planner (kinds, offsets, order, deduplication, budget,
fallback), its header reads against full decodes, the numpy model of the two kernels against the host path bit for bit,
simulated wrong kernels, the switch, a loader that the switch leaves alone, and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data as D, hip, utils
from tests import dataset_ref as DR, jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the planner
def test_the_kind_at_the_boundary():
    """h * w == 4 * S * S is still the uint8 source (its bytes equal the finished image's), one pixel more is not."""
    S = 6
    assert D.entry_kind(12, 12, S) == D.KIND_U8 and D.entry_kind(144, 1, S) == D.KIND_U8
    assert D.entry_kind(12, 13, S) == D.KIND_F32 and D.entry_kind(29, 5, S) == D.KIND_F32
    p = D.plan_entries([(12, 12), (12, 13), (1, 145), (1, 144)], S, 3, 1 << 30)
    assert list(p.kinds) == [0, 1, 1, 0]
    assert list(p.nbytes) == [432, 432, 432, 432]      # at the boundary both forms have the same bytes
    # the same comparison as device_path_pays
    for h, w in ((12, 12), (12, 13), (11, 7), (3, 50)):
        assert (D.entry_kind(h, w, S) == D.KIND_U8) == D.device_path_pays(h * w * 3, 1, S, 3)


def test_ragged_is_naturally_mixed():
    p = DR.plan(DR.RAGGED)
    assert list(p.kinds) == [0, 0, 0, 0, 0, 1]          # 12 x 13 > 4 * 36
    c = [c for c in DR.CASES if c.name == "7x10_to_3_c1"][0]
    assert list(DR.plan(c).kinds) == [1, 1]
    assert list(DR.plan(DR.RAGGED, D.KIND_F32).kinds) == [1] * 6 and list(DR.plan(c, D.KIND_U8).kinds) == [0, 0]


def test_offsets_are_16_byte_aligned_and_slots_do_not_overlap():
    for case in DR.CASES:
        for force in DR.FORCES:
            p = DR.plan(case, force)
            assert p.n_cached == p.n and (p.offsets % 16 == 0).all() and p.offsets[0] == 0
            ends = p.offsets + p.nbytes
            assert (ends[:-1] <= p.offsets[1:]).all() and ends[-1] <= p.arena_bytes == p.cached_bytes
            assert p.arena_bytes - ends[-1] < 16 and len(p.table) == p.n        # exactly the planned size, no scratch
            for i, e in enumerate(p.table):
                h, w = case.shapes[i]
                if p.kinds[i] == D.KIND_F32:
                    assert (e["h"], e["w"], e["kind"]) == (case.size, case.size, 1)
                else:
                    assert (e["h"], e["w"], e["kind"]) == (h, w, 0)
                    assert e["scale_y"] == np.float32(h / float(case.size)) and e["scale_x"] == np.float32(w / float(case.size))
                assert e["offset"] == p.offsets[i] and e["reserved"] == 0


def test_the_budget_keeps_a_prefix_and_plans_a_scratch_tail():
    shapes = [(11, 7), (3, 11), (6, 6), (1, 1), (17, 5), (12, 13)]     # aligned slots at C = 3: 240 112 112 16 256 432
    full = D.plan_entries(shapes, 6, 3, 1 << 30, batch_size=3)
    assert full.n_cached == 6 and full.slot_bytes == 0 and full.arena_bytes == 1168
    p = D.plan_entries(shapes, 6, 3, 500, batch_size=3)
    assert p.n_cached == 4 and p.cached_bytes == 480 and list(p.offsets) == [0, 240, 352, 464, -1, -1]
    assert p.slot_bytes == 432 and p.scratch_bytes == 3 * 432 and p.depth == 4
    assert p.arena_bytes == 480 + 4 * 3 * 432 and len(p.table) == 6 + 4 * 3
    assert (p.table["h"][4:] == 0).all()                # rows of uncached images and scratch rows: refused until written
    assert D.plan_entries(shapes, 6, 3, 480, batch_size=3).n_cached == 4        # a slot that ends on the budget fits
    assert D.plan_entries(shapes, 6, 3, 479, batch_size=3).n_cached == 3
    # a file that does not fit ends the prefix even when a later, smaller one would fit
    q = D.plan_entries(shapes, 6, 3, 250, batch_size=2)
    assert q.n_cached == 1 and q.slot_bytes == 432
    none = D.plan_entries(shapes, 6, 3, 1, batch_size=2)
    assert none.n_cached == 0 and none.cached_bytes == 0 and none.arena_bytes == 4 * 2 * 432
    with pytest.raises(ValueError):
        D.plan_entries(shapes, 6, 3, 250)               # a scratch tail needs the batch size
    with pytest.raises(ValueError):
        D.plan_entries([(0, 4)], 6, 3, 250)
    with pytest.raises(ValueError):
        D.plan_entries(shapes, 6, 2, 250)


def _folder(root, name="toy"):
    folder = os.path.join(str(root), "dataset", name)
    os.makedirs(folder)
    return folder


def _mixed_folder(tmp_path, channels=3):
    """PNG (RGB, grey, RGBA, palette), baseline JPEG (colour 4:2:0 and grey) and .npy files; returns the file list."""
    folder = _folder(tmp_path)
    rng = np.random.default_rng(11)
    utils.write_png(rng.integers(0, 256, (9, 14, 3), dtype=np.uint8), os.path.join(folder, "a.png"))
    utils.write_png(rng.integers(0, 256, (5, 3, 1), dtype=np.uint8), os.path.join(folder, "b.png"))
    utils.write_png(rng.integers(0, 256, (7, 7, 4), dtype=np.uint8), os.path.join(folder, "c.png"))
    for k, name in enumerate(J.DECODABLE):
        with open(os.path.join(folder, "d%02d.jpg" % k), "wb") as f:
            f.write(J.BYTES[name])
    np.save(os.path.join(folder, "e.npy"), rng.integers(0, 256, (8, 21, channels), dtype=np.uint8))
    files, _ = D.load_data("toy", "", root=os.path.join(str(tmp_path), "dataset"))
    return files


@pytest.mark.parametrize("channels", [1, 3])
def test_header_reads_take_the_shape_of_a_full_decode(tmp_path, channels):
    files = _mixed_folder(tmp_path, channels)
    assert len(files) == 4 + len(J.DECODABLE) and len(J.DECODABLE) >= 4
    idata = D.ImageData(8, channels, True, False)
    for f in files:
        full = D.finish_decode(D.decode_file(idata, f))
        assert D.image_header(idata, f) == tuple(full.shape), f
        assert D.image_header(idata, f) == tuple(D.decode_file(idata, f, entropy_only=True).shape)


def test_header_reads_of_four_channel_and_refused_files(tmp_path):
    folder = _folder(tmp_path)
    rng = np.random.default_rng(12)
    png, npy, jpg = (os.path.join(folder, n) for n in ("a.png", "b.npy", "c.jpg"))
    utils.write_png(rng.integers(0, 256, (6, 5, 4), dtype=np.uint8), png)
    np.save(npy, rng.integers(0, 256, (4, 9, 4), dtype=np.uint8))
    with open(jpg, "wb") as f:
        f.write(J.BYTES[J.DECODABLE[0]])
    rgba = D.ImageData(8, 4, True, False)
    assert D.image_header(rgba, png) == (6, 5, 4) == D.decode_file(rgba, png).shape
    assert D.image_header(rgba, npy) == (4, 9, 4)
    assert D.image_header(rgba, jpg) is None            # JPEG has no alpha: packable refuses it, and so does decode_jpeg
    rgb = D.ImageData(8, 3, True, False)
    assert D.image_header(rgb, npy) is None             # an array of another channel count
    for k, bad in enumerate((np.zeros((4, 9, 3), np.float32), np.zeros((4, 9), np.uint8), np.zeros((2, 4, 9, 3), np.uint8))):
        path = os.path.join(folder, "bad%d.npy" % k)
        np.save(path, bad)
        assert D.image_header(rgb, path) is None
    for k, name in enumerate(J.PROGRESSIVE):            # refused by the decoder, so not cacheable either
        path = os.path.join(folder, "p%d.jpg" % k)
        with open(path, "wb") as f:
            f.write(J.BYTES[name])
        assert D.image_header(rgb, path) is None
    other = os.path.join(folder, "notes.txt")
    with open(other, "w") as f:
        f.write("neither")
    assert D.image_header(rgb, other) is None
    assert D.image_header(D.ImageData(8, 3, False, False), np.zeros((4, 4, 3), np.uint8)) is None    # in-memory dataset


def test_a_jpeg_header_behind_a_long_segment_is_found(tmp_path):
    """The frame header lies past the first bytes the planner reads: it reads on."""
    data = J.BYTES[J.DECODABLE[0]]
    pad = b"\xff\xfe" + (60000).to_bytes(2, "big") + bytes(59998)           # a COM segment
    path = os.path.join(_folder(tmp_path), "long.jpg")
    with open(path, "wb") as f:
        f.write(data[:2] + pad + data[2:])
    idata = D.ImageData(8, 3, True, False)
    assert len(pad) > D.HEADER_PREFIX and D.image_header(idata, path) == D.decode_file(idata, path).shape


def test_first_occurrence_order_and_deduplication_under_a_weight_file(tmp_path):
    folder = _folder(tmp_path)
    rng = np.random.default_rng(13)
    shapes = [(20, 20), (4, 5), (6, 7), (30, 9)]
    for i, (h, w) in enumerate(shapes):
        utils.write_png(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), os.path.join(folder, "%02d.png" % i))
    with open(str(tmp_path / "w.tsv"), "w") as f:
        f.write("00.png\t2\n01.png\t0\n02.png\t3\n")
    files, _ = D.load_data("toy", "", str(tmp_path / "w.tsv"), root=os.path.join(str(tmp_path), "dataset"))
    assert [os.path.basename(f) for f in files] == ["00.png"] * 2 + ["02.png"] * 3 + ["03.png"]
    idata = D.ImageData(8, 3, True, False)
    p, refused = D.plan_dataset(files, idata, 1 << 30, 2)
    assert refused is None and p.n == 3 and [os.path.basename(f) for f in p.files] == ["00.png", "02.png", "03.png"]
    assert list(p.entry_of) == [0, 0, 1, 1, 1, 2]
    assert p.shapes == [(20, 20), (6, 7), (30, 9)] and list(p.kinds) == [1, 0, 1]
    assert list(p.offsets) == [0, 768, 768 + 128] and p.arena_bytes == 768 + 128 + 768
    # a shuffled list: entries are numbered by first occurrence
    order = [files[5], files[2], files[0], files[3], files[1]]
    q, _ = D.plan_dataset(order, idata, 1 << 30, 2)
    assert [os.path.basename(f) for f in q.files] == ["03.png", "02.png", "00.png"] and list(q.entry_of) == [0, 1, 2, 1, 2]
    forced, _ = D.plan_dataset(files, idata, 1 << 30, 2, force_kind=D.KIND_U8)
    assert list(forced.kinds) == [0, 0, 0] and list(forced.nbytes) == [1200, 126, 810]


def test_a_float_npy_turns_the_cache_off_for_the_whole_dataset(tmp_path):
    folder = _folder(tmp_path, "odd")
    rng = np.random.default_rng(4)
    for i in range(4):
        a = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
        np.save(os.path.join(folder, "%d.npy" % i), a.astype(np.float32) if i == 2 else a)
    files, _ = D.load_data("odd", "", root=os.path.join(str(tmp_path), "dataset"))
    p, refused = D.plan_dataset(files, D.ImageData(16, 3, True, False), 1 << 30, 2)
    assert p is None and refused.endswith("2.npy")


# ---------------------------------------------------------------- the numpy model of the kernels
@pytest.mark.parametrize("force", DR.FORCES, ids=DR.force_id)
@pytest.mark.parametrize("case", DR.CASES, ids=repr)
def test_model_equals_the_host_path(case, force):
    got, want = DR.modelled(case, force), case.want()
    assert got.shape == want.shape
    assert np.array_equal(DR.bits(got), DR.bits(want))


def test_model_store_refuses_a_segment_whole():
    src = np.arange(64, dtype=np.uint8)
    arena = np.full(64, DR.FILL, np.uint8)
    ok = DR.model_store(src, [(4, 16, 12, 0)], arena)
    assert (ok[16:28] == src[4:16]).all() and (ok[:16] == DR.FILL).all() and (ok[28:] == DR.FILL).all()
    for seg in ((-4, 16, 12, 0), (4, -16, 12, 0), (4, 16, -4, 0), (2, 16, 12, 0), (4, 18, 12, 0), (4, 16, 10, 0),
                (56, 16, 12, 0), (4, 56, 12, 0)):
        assert (DR.model_store(src, [seg], arena) == DR.FILL).all(), seg
    assert (DR.model_store(src, [(4, 16, 12, 0)], arena, src_bytes=12) == DR.FILL).all()
    assert (DR.model_store(src, [(4, 16, 12, 0)], arena, arena_bytes=24) == DR.FILL).all()


@pytest.mark.parametrize("wrong", DR.WRONG_KERNELS)
def test_every_wrong_kernel_is_told_apart(wrong):
    changed = {}
    for case in DR.CASES:
        for force in DR.FORCES:
            n = int((DR.bits(DR.modelled(case, force, wrong)) != DR.bits(case.want())).sum())
            if n:
                changed[case.name + "/" + DR.force_id(force)] = n
    print(wrong, changed)
    assert changed, wrong
    if wrong == "kind1_row_reversed":                   # only where a pixel has more than one channel
        assert any("_c3" in k for k in changed) and any("_c4" in k for k in changed)
        assert not any("_c1" in k for k in changed)
    if wrong.startswith("kind1"):
        assert not any(k.endswith("all_u8") for k in changed)
    if wrong.startswith("kind0"):
        assert not any(k.endswith("all_f32") for k in changed)


# ---------------------------------------------------------------- the switch
def test_the_switch_resolution(monkeypatch):
    monkeypatch.delenv("BG_DEVICE_DATASET_GB", raising=False)
    assert D.dataset_cache_bytes("cuda", None) == 0
    for off in ("", "0", "0.0", " "):
        monkeypatch.setenv("BG_DEVICE_DATASET_GB", off)
        assert D.dataset_cache_bytes("cuda", None) == 0
    monkeypatch.setenv("BG_DEVICE_DATASET_GB", "1.5")
    assert D.dataset_cache_bytes("cuda", None) == 3 << 29 and D.dataset_cache_bytes("cuda:1", None) == 3 << 29
    assert D.dataset_cache_bytes("cpu", None) == 0 and D.dataset_cache_bytes("cpu", 1 << 20) == 0
    assert D.dataset_cache_bytes("cuda", 0) == 0 and D.dataset_cache_bytes("cuda", 4096) == 4096    # an option wins
    monkeypatch.setenv("BG_DEVICE_DATASET_GB", "lots")
    with pytest.raises(ValueError):
        D.dataset_cache_bytes("cuda", None)
    monkeypatch.setenv("BG_DEVICE_DATASET_GB", "-1")
    with pytest.raises(ValueError):
        D.dataset_cache_bytes("cuda", None)


def test_with_the_switch_off_the_loader_is_todays(tmp_path, monkeypatch):
    folder = _folder(tmp_path)
    rng = np.random.default_rng(3)
    for i, (h, w) in enumerate([(10, 10), (9, 12), (8, 8), (10, 10), (12, 9), (8, 8)]):
        utils.write_png(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), os.path.join(folder, "%02d.png" % i))
    files, _ = D.load_data("toy", "", root=os.path.join(str(tmp_path), "dataset"))
    labels = [[float(i)] for i in range(len(files))]

    def batches(**kw):
        ld = D.BatchLoader(files, labels, 2, D.ImageData(8, 3, True, True, seed=5), "cpu", seed=7, workers=1, **kw)
        assert ld.cache is None
        try:
            return [next(ld) for _ in range(6)]
        finally:
            ld.close()
    monkeypatch.delenv("BG_DEVICE_DATASET_GB", raising=False)
    ref = batches()
    # today's arithmetic, restated: the permutation of the loader's rng, image_processing with the flips of ImageData's
    idata, order = D.ImageData(8, 3, True, True, seed=5), np.random.default_rng(7)
    want = []
    for _ in range(2):
        perm = order.permutation(len(files))
        want += [(np.stack([idata.image_processing(files[i]) for i in perm[s:s + 2]]), perm[s:s + 2]) for s in range(0, 6, 2)]
    for (x, l), (xw, iw) in zip(ref, want):
        assert np.array_equal(DR.bits(x.numpy()), DR.bits(xw)) and l[:, 0].tolist() == [float(i) for i in iw]
    monkeypatch.setenv("BG_DEVICE_DATASET_GB", "1")     # a CPU device ignores the switch, and so does an explicit 0
    for kw in (dict(), dict(cache_bytes=0), dict(cache_bytes=1 << 20)):
        for (x, l), (xr, lr) in zip(batches(**kw), ref):
            assert torch.equal(x, xr) and torch.equal(l, lr)


# ---------------------------------------------------------------- ABI
def test_abi_10_declares_and_binds_both_entry_points():
    assert hip.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "biggan_hip.h")).read()
    assert re.search(r"#define BG_ABI_VERSION 10\b", header)
    assert re.search(r"\bint bg_dataset_store\(", header) and re.search(r"\bint bg_dataset_batch\(", header)
    assert "typedef struct BgDatasetEntry" in header and "typedef struct BgCopySeg" in header
    assert "bg_dataset_store" in hip.SIGNATURES and "bg_dataset_batch" in hip.SIGNATURES
    assert "dataset.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    L = hip.lib()
    assert L.bg_abi_version() == 10 and L.bg_dataset_store and L.bg_dataset_batch
    assert D.ENTRY_DTYPE.itemsize == 32 and np.dtype("<i8").itemsize * 4 == 32      # BgDatasetEntry, BgCopySeg
    assert [D.ENTRY_DTYPE.fields[n][1] for n in ("offset", "h", "w", "kind", "scale_y", "scale_x", "reserved")] == \
        [0, 8, 12, 16, 20, 24, 28]


def test_the_entry_points_check_their_arguments_before_any_launch():
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails validation
    ok = dict(arena=fake, arena_bytes=1024, entries=fake, n_entries=2, sel=fake, n=2, S=8, C=3, out=fake)

    def batch(**kw):
        a = dict(ok, **kw)
        return L.bg_dataset_batch(a["arena"], a["arena_bytes"], a["entries"], a["n_entries"], a["sel"], a["n"], a["S"], a["C"],
                                  a["out"], None)
    for bad in (dict(arena=None), dict(entries=None), dict(sel=None), dict(out=None), dict(C=2), dict(C=5), dict(S=0),
                dict(S=-1), dict(n=0), dict(n_entries=0), dict(arena_bytes=0), dict(arena_bytes=-16),
                dict(arena=ctypes.c_void_p(4100)), dict(entries=ctypes.c_void_p(4100)), dict(sel=ctypes.c_void_p(4098)),
                dict(out=ctypes.c_void_p(4098))):
        assert batch(**bad) == 1, bad
        assert b"bg_dataset_batch" in L.bg_last_error()
    ok = dict(src=fake, src_bytes=64, segs=fake, n_segs=1, arena=fake, arena_bytes=1024)

    def store(**kw):
        a = dict(ok, **kw)
        return L.bg_dataset_store(a["src"], a["src_bytes"], a["segs"], a["n_segs"], a["arena"], a["arena_bytes"], None)
    for bad in (dict(src=None), dict(segs=None), dict(arena=None), dict(n_segs=0), dict(n_segs=-2), dict(src_bytes=0),
                dict(arena_bytes=0), dict(arena_bytes=-4), dict(src=ctypes.c_void_p(4098)), dict(arena=ctypes.c_void_p(4097)),
                dict(segs=ctypes.c_void_p(4100))):
        assert store(**bad) == 1, bad
        assert b"bg_dataset_store" in L.bg_last_error()


def test_the_wrappers_have_no_host_fallback():
    from biggan_tensorflow_amd import functional as Fn
    p = DR.plan(DR.RAGGED)
    arena = torch.from_numpy(DR.model_arena(DR.RAGGED, p))
    table = torch.from_numpy(p.table.view("<i4").reshape(-1, 8))
    with pytest.raises(RuntimeError):
        Fn.dataset_batch(arena, table, torch.from_numpy(DR.sel_of(DR.RAGGED)), 6, 6, 3)
    src, segs = DR.stages(DR.RAGGED, p)[0]
    with pytest.raises(RuntimeError):
        Fn.dataset_store(torch.from_numpy(src), torch.from_numpy(segs), arena)
