"""The device-resident dataset on the GPU: bg_dataset_store then bg_dataset_batch against data.py's host path bit for
bit on the case table of tests/input_ref.py (under the kind rule and with either kind forced, guard bands, inputs
untouched, the C entry points), repeated entries, the capped grid, the guards of both kernels, the argument checks, then
BatchLoader with the cache against the streaming loader (epochs, ranks, a weight file, a budget) and training."""
import os
import threading

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data as D, functional as Fn, hip, model, scope as S, utils
from tests import dataset_ref as DR, input_ref as R, jpeg_ref as J
from tests.common import make_args

pytestmark = pytest.mark.gpu

BAND = 4096                     # floats on either side of the output, bytes on either side of the arena (keeps 16 bytes)
NAN = float("nan")


def _banded_out(n, size, c, shift=0):
    numel = n * size * size * c
    buf = torch.full((BAND + shift + numel + BAND,), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[BAND + shift:BAND + shift + numel].view(n, size, size, c)


def _out_bands_intact(buf, numel, shift=0):
    return bool(torch.isnan(buf[:BAND + shift]).all()) and bool(torch.isnan(buf[BAND + shift + numel:]).all())


def _banded_arena(nbytes):
    buf = torch.full((BAND + nbytes + BAND,), DR.FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[BAND:BAND + nbytes]


def _arena_bytes_are(buf, model):
    """The whole allocation: both bands still filled, the arena between them equal to the model's."""
    host = buf.cpu().numpy()
    return bool((host[:BAND] == DR.FILL).all()) and bool((host[-BAND:] == DR.FILL).all()) and \
        np.array_equal(host[BAND:-BAND], model)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(p):
    return _dev(p.table.view("<i4").reshape(-1, 8))


def _store(staged, arena, through_c):
    for src, segs in staged:
        src_d, segs_d = _dev(src), _dev(segs)
        if through_c:
            rc = hip.lib().bg_dataset_store(hip.ptr(src_d), src_d.numel(), hip.ptr(segs_d), segs_d.shape[0], hip.ptr(arena),
                                            arena.numel(), hip.stream())
            assert rc == 0
        else:
            assert Fn.dataset_store(src_d, segs_d, arena).data_ptr() == arena.data_ptr()
        assert np.array_equal(src_d.cpu().numpy(), src) and np.array_equal(segs_d.cpu().numpy(), segs)


def _check_case(case, force, shift=0):
    p = DR.plan(case, force)
    n, size, c = len(case.shapes), case.size, case.channels
    want, model = case.want(), DR.model_arena(case, p)
    staged, table, sel = DR.stages(case, p), p.table.view("<i4").reshape(-1, 8), DR.sel_of(case)
    first = None
    for through_c in (False, True):                     # the functional wrappers, then the C entry points themselves
        abuf, arena = _banded_arena(p.arena_bytes)
        _store(staged, arena, through_c)
        torch.cuda.synchronize()
        assert _arena_bytes_are(abuf, model)            # slots filled, every byte outside them as it was
        table_d, sel_d = _dev(table), _dev(sel)
        obuf, out = _banded_out(n, size, c, shift)
        if through_c:
            rc = hip.lib().bg_dataset_batch(hip.ptr(arena), arena.numel(), hip.ptr(table_d), table_d.shape[0], hip.ptr(sel_d),
                                            n, size, c, hip.ptr(out), hip.stream())
            assert rc == 0
        else:
            assert Fn.dataset_batch(arena, table_d, sel_d, n, size, c, out=out).data_ptr() == out.data_ptr()
        got = out.cpu().numpy()
        diff = int((R.bits(got) != R.bits(want)).sum())
        print(case, DR.force_id(force), "C entry" if through_c else "wrapper",
              "elements that differ from the host path: %d of %d" % (diff, want.size))
        assert diff == 0
        assert _out_bands_intact(obuf, out.numel(), shift)
        assert _arena_bytes_are(abuf, model)            # the gather changed no byte of the arena
        assert np.array_equal(table_d.cpu().numpy(), table) and np.array_equal(sel_d.cpu().numpy(), sel)
        if first is None:
            first = got
        assert np.array_equal(R.bits(got), R.bits(first))


@pytest.mark.parametrize("force", DR.FORCES, ids=DR.force_id)
@pytest.mark.parametrize("case", DR.CASES, ids=repr)
def test_store_then_gather_equals_the_host_path_bit_for_bit(case, force):
    _check_case(case, force)


@pytest.mark.parametrize("force", DR.FORCES, ids=DR.force_id)
@pytest.mark.parametrize("case", [c for c in DR.CASES if c.channels == 4], ids=repr)
def test_four_channels_into_an_output_that_is_not_16_byte_aligned(case, force):
    _check_case(case, force, shift=1)                   # the scalar variant of C = 4


@pytest.mark.parametrize("force", [D.KIND_F32, D.KIND_U8], ids=DR.force_id)
def test_more_pixels_than_one_pass_of_the_grid(force):
    case = DR.GRID_STRIDE
    assert len(case.shapes) * case.size ** 2 > 3 * 4096 * 256      # the third and later strides too
    _check_case(case, force)


def test_a_source_that_is_only_4_byte_aligned_is_copied_in_words():
    """The same segments from a source buffer 4 bytes off a 16-byte boundary: the word variant of the store."""
    case = DR.RAGGED
    p = DR.plan(case)
    abuf, arena = _banded_arena(p.arena_bytes)
    for src, segs in DR.stages(case, p):
        holder = torch.zeros(src.size + 16, dtype=torch.uint8, device="cuda")
        holder[4:4 + src.size] = _dev(src)
        assert holder[4:].data_ptr() % 16 == 4
        Fn.dataset_store(holder[4:4 + src.size], _dev(segs), arena)
    torch.cuda.synchronize()
    assert _arena_bytes_are(abuf, DR.model_arena(case, p))


@pytest.mark.parametrize("force", DR.FORCES, ids=DR.force_id)
@pytest.mark.parametrize("name", ["7x10_to_3_c1", "11x7_to_6_c3", "3x11_to_6_c4"])
def test_one_entry_three_times_in_descending_order(name, force):
    case = [c for c in DR.CASES if c.name == name][0]
    p = DR.plan(case, force)
    size, c = case.size, case.channels
    abuf, arena = _banded_arena(p.arena_bytes)
    _store(DR.stages(case, p), arena, False)
    sel = np.array([(1, 0), (1, 1), (1, 0), (0, 1), (0, 0)], np.int32)
    imgs = case.images()
    want = R.host_path([imgs[i] for i, _ in sel], [f for _, f in sel], size, c)
    for shift in ((0, 1) if c == 4 else (0,)):          # C = 4: also the scalar-store variant
        obuf, out = _banded_out(5, size, c, shift)
        Fn.dataset_batch(arena, _table(p), _dev(sel), 5, size, c, out=out)
        got = out.cpu().numpy()
        assert np.array_equal(R.bits(got), R.bits(want)), shift
        assert np.array_equal(R.bits(got[0]), R.bits(got[2])) and not np.array_equal(R.bits(got[0]), R.bits(got[1]))
        assert _out_bands_intact(obuf, out.numel(), shift)


# ---------------------------------------------------------------- guards
@pytest.mark.parametrize("force", [None, D.KIND_U8], ids=DR.force_id)
def test_a_refused_entry_gives_nan_for_that_image_only(force):
    """Entry 5 (12 x 13: kind 1 under the rule) lies last in the arena.  For the extent guard the DECLARED arena_bytes
    stop one byte short of its end while the allocation holds all of it: even a kernel without the guard reads valid
    memory here."""
    case = DR.RAGGED
    p = DR.plan(case, force)
    S, C, n = case.size, case.channels, len(case.shapes)
    want = case.want()
    abuf, arena = _banded_arena(p.arena_bytes)
    _store(DR.stages(case, p), arena, False)
    table, sel = p.table.copy(), DR.sel_of(case)
    obuf, out = _banded_out(n, S, C)

    def run(table=table, sel=sel, bad=None, **kw):
        out.fill_(NAN)
        Fn.dataset_batch(arena, _dev(table.view("<i4").reshape(-1, 8)), _dev(sel), n, S, C, out=out, **kw)
        got = out.cpu().numpy()
        for i in range(n):
            if i == bad:
                assert np.isnan(got[i]).all(), (bad, kw)
            else:
                assert np.array_equal(R.bits(got[i]), R.bits(want[i])), (i, bad, kw)
        assert _out_bands_intact(obuf, out.numel())
    run()
    assert int(p.offsets[5]) + int(p.nbytes[5]) > int(p.offsets[4]) + int(p.nbytes[4])        # entry 5 is the last one
    run(arena_bytes=int(p.offsets[5]) + int(p.nbytes[5]) - 1, bad=5)
    run(arena_bytes=int(p.offsets[5]) + int(p.nbytes[5]))                                     # all of it declared: complete
    for row, index in ((1, -1), (1, n), (4, 1 << 30), (5, -(1 << 31))):                       # sel outside [0, n_entries)
        s = sel.copy()
        s[row, 0] = index
        run(sel=s, bad=row)
    edits = [(1, "kind", 2), (1, "kind", -1), (1, "h", 0), (1, "w", -4), (1, "offset", -16), (1, "offset", int(p.offsets[1]) + 8),
             (5, "offset", int(p.offsets[5]) + 4), (5, "h", 0)]
    if p.kinds[5] == D.KIND_F32:                        # kind 1 whose h or w is not S
        edits += [(5, "h", S + 1), (5, "w", S - 1), (5, "h", S - 1)]
    for row, field, value in edits:
        t = table.copy()
        t[field][row] = value
        run(table=t, bad=row)
    assert _arena_bytes_are(abuf, DR.model_arena(case, p))


def test_a_refused_segment_leaves_its_destination_as_it_was():
    rng = np.random.default_rng(23)
    src = rng.integers(0, 256, 4096, dtype=np.uint8)
    good = [(0, 64, 160, 0), (1024, 2048, 52, 0)]       # one that moves in 16-byte words, one in 4-byte words
    src_d = _dev(src)
    for bad, kw in (((-16, 512, 32, 0), {}), ((256, -16, 32, 0), {}), ((256, 512, -32, 0), {}), ((258, 512, 32, 0), {}),
                    ((256, 514, 32, 0), {}), ((256, 512, 30, 0), {}),
                    ((3968, 512, 128, 0), dict(src_bytes=4095)),           # the source extent ends past src_bytes
                    ((256, 2944, 128, 0), dict(arena_bytes=3071)),         # the destination extent ends past arena_bytes
                    ((256, 1 << 40, 32, 0), {}), ((1 << 40, 512, 32, 0), {}), ((256, 512, 1 << 40, 0), {})):
        segs = np.array([good[0], bad, good[1]], np.int64)
        abuf, arena = _banded_arena(3072)
        Fn.dataset_store(src_d, _dev(segs), arena, **kw)
        torch.cuda.synchronize()
        model = DR.model_store(src, segs, np.full(3072, DR.FILL, np.uint8), **kw)
        assert (model[64:224] == src[:160]).all() and (model[2048:2100] == src[1024:1076]).all()
        assert int((model != DR.FILL).sum()) <= 160 + 52                    # the model copied nothing of the bad segment
        assert _arena_bytes_are(abuf, model), bad


def test_argument_errors_return_before_any_launch():
    case = DR.RAGGED
    p = DR.plan(case)
    abuf, arena = _banded_arena(p.arena_bytes)
    (src, segs), _ = DR.stages(case, p)
    src_d, segs_d, table_d, sel_d = _dev(src), _dev(segs), _table(p), _dev(DR.sel_of(case))
    obuf, out = _banded_out(6, 6, 3)
    L = hip.lib()
    ok = dict(arena=hip.ptr(arena), arena_bytes=arena.numel(), entries=hip.ptr(table_d), n_entries=6, sel=hip.ptr(sel_d),
              n=6, S=6, C=3, out=hip.ptr(out))

    def batch(**kw):
        a = dict(ok, **kw)
        return L.bg_dataset_batch(a["arena"], a["arena_bytes"], a["entries"], a["n_entries"], a["sel"], a["n"], a["S"], a["C"],
                                  a["out"], hip.stream())
    for bad in (dict(arena=None), dict(entries=None), dict(sel=None), dict(out=None), dict(C=2), dict(S=0), dict(S=-3),
                dict(n=0), dict(n=-1), dict(n_entries=0), dict(arena_bytes=0), dict(arena_bytes=-1)):
        assert batch(**bad) == 1, bad                   # BG_ERR_ARG
        assert b"bg_dataset_batch" in L.bg_last_error()
    sk = dict(src=hip.ptr(src_d), src_bytes=src_d.numel(), segs=hip.ptr(segs_d), n_segs=segs_d.shape[0], arena=hip.ptr(arena),
              arena_bytes=arena.numel())

    def store(**kw):
        a = dict(sk, **kw)
        return L.bg_dataset_store(a["src"], a["src_bytes"], a["segs"], a["n_segs"], a["arena"], a["arena_bytes"], hip.stream())
    for bad in (dict(src=None), dict(segs=None), dict(arena=None), dict(n_segs=0), dict(n_segs=-1), dict(src_bytes=0),
                dict(src_bytes=-4), dict(arena_bytes=0), dict(arena_bytes=-16)):
        assert store(**bad) == 1, bad
        assert b"bg_dataset_store" in L.bg_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(obuf).all()) and bool((abuf == DR.FILL).all())         # nothing was launched
    with pytest.raises(RuntimeError):
        Fn.dataset_batch(arena, table_d.float(), sel_d, 6, 6, 3)
    with pytest.raises(RuntimeError):
        Fn.dataset_batch(arena, table_d, sel_d, 5, 6, 3)
    with pytest.raises(RuntimeError):
        Fn.dataset_batch(arena, table_d, sel_d, 6, 6, 3, arena_bytes=arena.numel() + 1)
    with pytest.raises(RuntimeError):
        Fn.dataset_store(src_d, segs_d.int(), arena)
    with pytest.raises(RuntimeError):
        Fn.dataset_store(src_d, segs_d, arena, src_bytes=src_d.numel() + 1)
    assert store() == 0 and batch() == 0


# ---------------------------------------------------------------- the loader
S_LOAD = 16                                             # 4 * S * S = 1024 source pixels: 40 x 40 is kind 1, the others kind 0
SIZES = [(40, 40), (20, 24), (16, 16)]
JPEGS = {4: "33x18_420q75", 9: "29x37_444q90"}          # 18 x 33 (kind 0) and 37 x 29 (kind 1, 1073 pixels)


def _folder(root, n=12):
    folder = os.path.join(str(root), "dataset", "toy")
    os.makedirs(folder)
    rng = np.random.default_rng(3)
    with open(os.path.join(str(root), "labels.tsv"), "w") as lab:
        for i in range(n):
            name = "%02d.%s" % (i, "jpg" if i in JPEGS else "png")
            if i in JPEGS:
                with open(os.path.join(folder, name), "wb") as f:
                    f.write(J.BYTES[JPEGS[i]])
            else:
                h, w = SIZES[i % 3]
                utils.write_png(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), os.path.join(folder, name))
            lab.write("%s\t%d\t%d\n" % (name, i, i % 3))
    return os.path.join(str(root), "dataset")


def _batches(files, labels, count, cache_bytes, batch=5, workers=1, counts=None, monkeypatch=None, **kw):
    """``count`` batches of a loader as CPU tensors, and the loader (closed).  ``counts``: a dict that receives the
    number of data.decode_file calls per path while this loader lives."""
    if counts is not None:
        real, lock = D.decode_file, threading.Lock()

        def counting(image_data, filename, entropy_only=False):
            with lock:
                counts[filename] = counts.get(filename, 0) + 1
            return real(image_data, filename, entropy_only)
        monkeypatch.setattr(D, "decode_file", counting)
    ld = D.BatchLoader(files, labels, batch, D.ImageData(S_LOAD, 3, True, True, seed=5), "cuda", seed=7, workers=workers,
                       cache_bytes=cache_bytes, **kw)
    try:
        assert (ld.cache is not None) == (cache_bytes > 0)
        out = [next(ld) for _ in range(count)]
        torch.cuda.synchronize()
        return [(x.cpu(), l.cpu()) for x, l in out], ld
    finally:
        ld.close()
        if counts is not None:
            monkeypatch.setattr(D, "decode_file", real)


def _same(got, ref):
    assert len(got) == len(ref)
    for k, ((x, l), (xr, lr)) in enumerate(zip(got, ref)):
        assert x.dtype == torch.float32 and tuple(x.shape) == tuple(xr.shape) and bool(torch.isfinite(x).all())
        assert np.array_equal(R.bits(x.numpy()), R.bits(xr.numpy())), "batch %d" % k
        assert torch.equal(l, lr), "labels of batch %d" % k


@pytest.mark.parametrize("world", [1, 2])
def test_cached_loader_equals_the_streaming_loader(tmp_path, monkeypatch, world):
    """12 files, batch 5: two files drop out of every epoch and are cached when a later epoch names them.  Four epochs;
    with world = 2 the ranks are two loaders in one process, each with its own cache."""
    root = _folder(tmp_path)
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), root=root)
    epochs = 4
    count = epochs * (12 // (5 * world))
    for rank in range(world):
        counts = {}
        ref, _ = _batches(files, labels, count, 0, rank=rank, world=world)
        got, ld = _batches(files, labels, count, 1 << 30, workers=4, counts=counts, monkeypatch=monkeypatch, rank=rank,
                           world=world)
        _same(got, ref)
        p = ld.cache.plan
        assert p.n == p.n_cached == 12 and set(p.kinds.tolist()) == {0, 1} and ld.cache.arena.numel() == p.arena_bytes
        assert [int(k) for k in p.kinds] == [1 if (i == 9 or (i not in JPEGS and i % 3 == 0)) else 0 for i in range(12)]
        seen = {files[int(v)] for x, l in got for v in l[:, 0]}
        assert len(seen) >= 7 and all(counts[f] == 1 for f in seen)       # decoded on the first visit ...
        assert all(v == 1 for v in counts.values()), counts               # ... and never again, prefetched batches included
        assert not torch.equal(got[0][0], got[1][0])
    # the flips did flip something: the same run without them differs
    plain = D.BatchLoader(files, labels, 5, D.ImageData(S_LOAD, 3, True, False, seed=5), "cuda", seed=7, workers=1,
                          cache_bytes=1 << 30, rank=world - 1, world=world)
    try:
        x, _ = next(plain)
        assert not torch.equal(x.cpu(), got[0][0])
    finally:
        plain.close()


def test_cached_loader_with_a_weight_file_that_repeats_files(tmp_path, monkeypatch):
    root = _folder(tmp_path)
    with open(str(tmp_path / "w.tsv"), "w") as f:
        f.write("00.png\t3\n01.png\t0\n04.jpg\t2\n09.jpg\t2.5\n")
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), str(tmp_path / "w.tsv"), root=root)
    assert len(files) == 15 and len(set(files)) == 11
    counts = {}
    ref, _ = _batches(files, labels, 12, 0)
    got, ld = _batches(files, labels, 12, 1 << 30, workers=3, counts=counts, monkeypatch=monkeypatch)
    _same(got, ref)
    p = ld.cache.plan
    assert p.n == 11 and len(p.entry_of) == 15 and [int(e) for e in p.entry_of[:4]] == [0, 0, 0, 1]
    assert set(counts) == set(files) and all(v == 1 for v in counts.values()), counts      # four epochs name every file


def test_a_budget_that_holds_seven_of_the_twelve_entries(tmp_path, monkeypatch):
    root = _folder(tmp_path)
    files, labels = D.load_data("toy", str(tmp_path / "labels.tsv"), root=root)
    full, _ = D.plan_dataset(files, D.ImageData(S_LOAD, 3, True, True), 1 << 30, 5)
    budget = int(full.offsets[7]) + 8                   # the first seven slots and not the eighth
    counts = {}
    ref, _ = _batches(files, labels, 6, 0)              # three epochs
    got, ld = _batches(files, labels, 6, budget, workers=4, counts=counts, monkeypatch=monkeypatch)
    _same(got, ref)
    p = ld.cache.plan
    assert p.n_cached == 7 and p.cached_bytes == int(full.offsets[7]) and p.slot_bytes == 4 * S_LOAD * S_LOAD * 3
    assert ld.cache.arena.numel() == p.arena_bytes == p.cached_bytes + p.depth * 5 * p.slot_bytes
    assert ld.cache.arena.numel() <= budget + p.depth * 5 * p.slot_bytes
    assert all(counts.get(f, 0) <= 1 for f in files[:7])                  # cached files: once
    assert any(counts.get(f, 0) > 1 for f in files[7:])                   # files past the budget are streamed every time
    # nothing fits: every image goes through the scratch tail, and the batches are still the same
    got, ld = _batches(files, labels, 6, 16)
    _same(got, ref)
    assert ld.cache.plan.n_cached == 0


def test_a_dataset_with_a_float_array_runs_without_the_cache(tmp_path, capsys):
    folder = tmp_path / "dataset" / "odd"
    folder.mkdir(parents=True)
    rng = np.random.default_rng(4)
    for i in range(4):
        a = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
        np.save(str(folder / ("%d.npy" % i)), a.astype(np.float32) if i == 2 else a)
    files, _ = D.load_data("odd", "", root=str(tmp_path / "dataset"))

    def one(cache_bytes):
        ld = D.BatchLoader(files, None, 4, D.ImageData(16, 3, True, True, seed=5), "cuda", seed=7, workers=1,
                           cache_bytes=cache_bytes)
        try:
            assert ld.cache is None
            return next(ld).cpu()
        finally:
            ld.close()
    assert torch.equal(one(1 << 30), one(0))
    assert "dataset cache: off" in capsys.readouterr().out


def test_a_file_whose_pixels_contradict_its_header_raises(tmp_path, monkeypatch):
    root = _folder(tmp_path)
    files, _ = D.load_data("toy", "", root=root)
    real = D.decode_file

    def short(idata, f, entropy_only=False):            # every PNG comes back one row short of its header
        a = real(idata, f, entropy_only)
        return a[:-1] if isinstance(a, np.ndarray) else a
    monkeypatch.setattr(D, "decode_file", short)
    ld = D.BatchLoader(files, None, 5, D.ImageData(S_LOAD, 3, True, True, seed=5), "cuda", seed=7, workers=1,
                       cache_bytes=1 << 30)
    try:
        with pytest.raises(ValueError, match="its header said"):
            next(ld)
    finally:
        ld.close()


# ---------------------------------------------------------------- training
def _train(tmp_path, tag):
    gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, epoch=1, dataset="toy", random_flip="true",
                                 checkpoint_dir=str(tmp_path / tag / "ckpt"), sample_dir=str(tmp_path / tag / "samples")),
                       store=S.VariableStore("cuda", seed=5)).build_model()
    seen, step = [], gan.train_step

    def recording(*a, **k):
        out = step(*a, **k)
        seen.append({name: np.float32(v.item()).view(np.uint32) for name, v in out.items()})
        return out
    gan.train_step = recording
    gan.train(iterations=3, resume=False)
    return seen


def test_training_with_the_cache_gives_the_same_losses_bit_for_bit(tmp_path, monkeypatch, capsys):
    folder = tmp_path / "dataset" / "toy"
    folder.mkdir(parents=True)
    rng = np.random.default_rng(3)
    for i in range(8):
        h, w = [(80, 80), (70, 90), (64, 64), (160, 150)][i % 4]           # 160 x 150 > 4 * 64 * 64: kind 1
        utils.write_png(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), str(folder / ("%02d.png" % i)))
    monkeypatch.chdir(tmp_path)                         # train() opens ./dataset/<name>
    monkeypatch.delenv("BG_DEVICE_INPUT", raising=False)
    monkeypatch.setenv("BG_DEVICE_DATASET_GB", "0.25")
    on = _train(tmp_path, "on")
    assert "# dataset cache: 8 of 8 files cached" in capsys.readouterr().out
    monkeypatch.setenv("BG_DEVICE_DATASET_GB", "0")
    off = _train(tmp_path, "off")
    assert "dataset cache" not in capsys.readouterr().out
    assert len(on) == len(off) == 3 and "d_loss" in on[0] and "g_loss" in on[0]
    assert on == off
