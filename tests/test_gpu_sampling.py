"""In-training sample grids on the device: bg_image_tiles_u8 against the host path (utils.inverse_transform, merge, the
8-bit conversion of utils.grid_u8) byte for byte - tile placement, both element types, every bf16 bit pattern, the fp32
rounding ties - then BigGAN.save_samples (files, sizes, state preservation, determinism, agreement with sample()) and
the training loop's hook."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import functional as Fn, model, sampling as Sp, scope as S, utils
from tests.common import make_args

pytestmark = pytest.mark.gpu


def _host_grid(x, gh, gw, tile0=0):
    """utils.grid_u8 on the same values: ``tile0`` images of -1.0 (byte 0) in front, surplus images dropped."""
    a = x.detach().float().cpu().numpy()                     # (bf16 -> fp32 is exact)
    if tile0:
        a = np.concatenate([np.full((tile0,) + a.shape[1:], -1.0, np.float32), a])
    with np.errstate(invalid="ignore"):
        return torch.from_numpy(utils.grid_u8(utils.inverse_transform(a[:gh * gw]), [gh, gw]))


def _images(n, H, W, C, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(n, H, W, C, device="cuda", generator=g) * 2.5) - 1.25).to(dtype)


def _dev_grid(x, gh, gw, tile0=0):
    n, H, W, C = x.shape
    grid = torch.zeros(gh * H, gw * W, C, dtype=torch.uint8, device="cuda")
    Fn.image_tiles_u8(x, grid, gh, gw, tile0)
    return grid.cpu()


CASES = [(8, 8, 3, 2, 3, 5, 0),          # one empty tile stays 0
         (8, 8, 4, 2, 2, 4, 0),
         (8, 8, 1, 3, 1, 3, 0),
         (6, 10, 3, 2, 2, 3, 1),         # H != W, W*C = 30: one element per thread; offset start
         (4, 4, 3, 1, 2, 5, 0)]          # surplus images are skipped


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_equals_the_host_path(case, dtype):
    H, W, C, gh, gw, n, tile0 = case
    x = _images(n, H, W, C, dtype, seed=sum(case))
    want = _host_grid(x, gh, gw, tile0)
    got = _dev_grid(x, gh, gw, tile0)
    assert got.shape == want.shape == (gh * H, gw * W, C)
    assert torch.equal(got, want)
    assert int(want.max()) == 255 and int((want == 0).sum()) > 0          # the clamp is exercised both ways


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [CASES[4], CASES[3]], ids=["wide", "scalar"])
def test_nothing_is_written_outside_the_grid(case, dtype):
    H, W, C, gh, gw, n, tile0 = case
    x = _images(n, H, W, C, dtype, seed=3)
    numel, band = gh * H * gw * W * C, 4096
    buf = torch.full((band + numel + band,), 0xAB, dtype=torch.uint8, device="cuda")
    grid = buf[band:band + numel].view(gh * H, gw * W, C)
    grid.zero_()
    Fn.image_tiles_u8(x, grid, gh, gw, tile0)
    assert torch.equal(grid.cpu(), _host_grid(x, gh, gw, tile0))
    assert bool((buf[:band] == 0xAB).all()) and bool((buf[band + numel:] == 0xAB).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_grid_filled_by_two_calls(dtype):
    x = _images(6, 8, 8, 3, dtype, seed=5)
    grid = torch.zeros(16, 24, 3, dtype=torch.uint8, device="cuda")
    Fn.image_tiles_u8(x[0:3], grid, 2, 3, 0)
    Fn.image_tiles_u8(x[3:6], grid, 2, 3, 3)
    one = _dev_grid(x, 2, 3)
    assert torch.equal(grid.cpu(), one) and torch.equal(one, _host_grid(x, 2, 3))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_non_contiguous_view(dtype):
    base = _images(4, 8, 8, 4, dtype, seed=6)
    view = base[..., :3]
    assert not view.is_contiguous()
    assert torch.equal(_dev_grid(view, 2, 2), _host_grid(view.contiguous(), 2, 2))


def test_wrapper_rejects_what_it_cannot_run():
    x = _images(2, 4, 4, 3, torch.float32)
    grid = torch.zeros(4, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        Fn.image_tiles_u8(x.half(), grid, 1, 2)
    with pytest.raises(RuntimeError):
        Fn.image_tiles_u8(x, grid.float(), 1, 2)
    with pytest.raises(RuntimeError):
        Fn.image_tiles_u8(x, grid, 2, 2)                   # grid shape does not match gh x gw tiles
    with pytest.raises(RuntimeError):
        Fn.image_tiles_u8(x, grid, 1, 2, tile0=-1)
    assert not grid.any()


def test_every_bf16_bit_pattern():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16).reshape(1, 128, 128, 4).cuda()
    got = _dev_grid(x, 1, 1).reshape(-1)
    nan = torch.isnan(x.float().cpu()).reshape(-1)
    want = _host_grid(x, 1, 1).reshape(-1)
    assert int(nan.sum()) == 2 * 127                        # exponent all ones, mantissa non-zero, both signs
    assert torch.equal(got[~nan], want[~nan])
    assert not got[nan].any()                               # NaN writes 0 (the host cast of NaN is undefined)


def test_fp32_rounding_ties():
    """x_k = fp32((2k+1)/255 - 1) maps next to the tie k + 0.5: an fp32 product t * 255 rounds some of these and of their
    neighbours to the other byte than numpy's float64 grid does."""
    vals = []
    for k in range(255):
        x = np.float32((2 * k + 1) / 255.0 - 1.0)
        lo1 = np.nextafter(x, np.float32(-np.inf))
        hi1 = np.nextafter(x, np.float32(np.inf))
        vals += [np.nextafter(lo1, np.float32(-np.inf)), lo1, x, hi1, np.nextafter(hi1, np.float32(np.inf))]
    one = np.float32(1.0)
    for s in (one, -one):
        vals += [s, np.nextafter(s, np.float32(np.inf)), np.nextafter(s, np.float32(-np.inf)), np.float32(2.0) * s,
                 np.float32(np.inf) * s]
    vals.append(np.float32(-0.0))
    a = np.zeros(1600, np.float32)
    a[:len(vals)] = np.asarray(vals, np.float32)
    assert len(vals) == 255 * 5 + 11 <= 1600
    x = torch.from_numpy(a.reshape(1, 40, 40, 1)).cuda()
    want = _host_grid(x, 1, 1)
    assert torch.equal(_dev_grid(x, 1, 1), want)
    # the case is live: an fp32 product disagrees with the float64 grid somewhere in this set
    t = (a + np.float32(1.0)) * np.float32(0.5)
    f32 = np.clip(np.rint(t * np.float32(255.0)), 0, 255).astype(np.uint8)
    assert (f32 != want.numpy().reshape(-1)).any()


# ---------------------------------------------------------------- model level
def _read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, depth, ctype = struct.unpack(">IIBB", data[16:26])
    c = {0: 1, 2: 3, 6: 4}[ctype]
    n = struct.unpack(">I", data[33:37])[0]
    assert depth == 8 and data[37:41] == b"IDAT"
    raw = np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(h, 1 + w * c)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, c)


def _sampling_model(tmp_path, **kw):
    flags = dict(img_size=64, ch=8, z_dim=64, batch_size=4, sample_num=10, n_labels=3, sample_ema="both",
                 save_morphs="true", save_cls_samples="true", sample_dir=str(tmp_path / "samples"),
                 checkpoint_dir=str(tmp_path / "ckpt"))
    flags.update(kw)
    gan = model.BigGAN(make_args(**flags), store=S.VariableStore("cuda", seed=2)).build_model()
    gan.train_step(gan.synthetic_batch())                  # the moving averages now differ from the live weights
    return gan


def _snapshot(gan):
    gan.sync_sharded_state()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in gan.state_tensors().items()}, gan.gen.get_state().clone(), gan.counter,
            (gan.d_arena.step, gan.g_arena.step))


def _assert_untouched(gan, snap):
    tensors, rng, counter, steps = snap
    now = gan.state_tensors()
    assert set(now) == set(tensors)
    changed = [k for k, v in now.items() if not torch.equal(v, tensors[k])]
    assert not changed, changed[:5]
    assert any(k.endswith("/u") for k in tensors if k.startswith("generator/"))
    assert torch.equal(gan.gen.get_state(), rng)
    assert gan.counter == counter and (gan.d_arena.step, gan.g_arena.step) == steps


def _kinds(paths):
    return sorted(os.path.basename(p) for p in paths)


def test_save_samples_writes_the_grids_and_leaves_the_run_alone(tmp_path):
    gan = _sampling_model(tmp_path)
    snap = _snapshot(gan)
    np_state = np.random.get_state()[1].copy()
    paths = gan.save_samples(0, 1)
    _assert_untouched(gan, snap)
    assert np.array_equal(np.random.get_state()[1], np_state)
    names = _kinds(paths)
    assert names == sorted(os.listdir(str(tmp_path / "samples")))
    assert len(names) == 4 and names[1:] == ["BigGAN_ema_00_00001.png", "BigGAN_morph_00_00001.png",
                                              "BigGAN_noema_00_00001.png"]
    tag = Sp.event_rng(gan.static_sample_seed, 0, gan.iterations_per_epoch, 1)
    Sp.morph_corners(10, tag)
    assert names[0] == "BigGAN_cls_00_00001_%03d.png" % tag.randint(3)
    by = {n.split("_")[1]: _read_png(os.path.join(str(tmp_path / "samples"), n)) for n in names}
    assert by["ema"].shape == by["noema"].shape == by["cls"].shape == (192, 192, 3)
    assert by["morph"].shape == (320, 320, 3)
    assert not np.array_equal(by["ema"], by["noema"])
    assert by["ema"].std() > 0 and by["morph"].std() > 0
    # the same event again: the same bytes
    first = {n: open(os.path.join(str(tmp_path / "samples"), n), "rb").read() for n in names}
    assert _kinds(gan.save_samples(0, 1)) == names
    for n in names:
        assert open(os.path.join(str(tmp_path / "samples"), n), "rb").read() == first[n], n
    _assert_untouched(gan, snap)
    # every tile is a function of its latent only: tiles 0-3 (two generator batches' worth of rows) are what sample()
    # gives for the first four static latents from the same preserved state
    zs, cs = gan.static_sample_set()
    img = gan.sample(torch.from_numpy(zs[0:4]).cuda(), torch.from_numpy(cs[0:4]).cuda(), use_ema=True)
    want = utils.grid_u8(utils.inverse_transform(img.float().cpu().numpy()), [1, 4])
    for t in range(4):
        r, c = divmod(t, 3)
        assert np.array_equal(by["ema"][r * 64:(r + 1) * 64, c * 64:(c + 1) * 64], want[:, t * 64:(t + 1) * 64]), t
    # generate() without a grid returns the same images, trimmed to the list
    out = gan.generate(zs[0:3], cs[0:3])
    assert out.shape == (3, 64, 64, 3)


def test_save_samples_bf16(tmp_path):
    gan = _sampling_model(tmp_path, precision="bf16")
    snap = _snapshot(gan)
    paths = gan.save_samples(2, 7)
    _assert_untouched(gan, snap)
    names = _kinds(paths)
    assert [n.rsplit("_02_00007", 1)[0] for n in names] == ["BigGAN_cls", "BigGAN_ema", "BigGAN_morph", "BigGAN_noema"]
    for n in names:
        side = 320 if "morph" in n else 192
        assert _read_png(os.path.join(str(tmp_path / "samples"), n)).shape == (side, side, 3), n


def test_fresh_latents_leave_the_training_generator_alone(tmp_path):
    gan = _sampling_model(tmp_path, static_sample_z="false", sample_ema="ema", save_morphs="false",
                          save_cls_samples="false")
    snap = _snapshot(gan)
    a = open(gan.save_samples(0, 1)[0], "rb").read()
    b = open(gan.save_samples(0, 2)[0], "rb").read()
    _assert_untouched(gan, snap)
    assert a != b                                           # fresh draws, from the sampling generator


def test_train_loop_writes_the_ema_grid_every_print_freq(tmp_path):
    args = make_args(img_size=64, ch=8, batch_size=4, z_dim=64, print_freq=2, sample_num=4,
                     sample_dir=str(tmp_path / "samples"), checkpoint_dir=str(tmp_path / "ckpt"))
    gan = model.BigGAN(args, store=S.VariableStore("cuda", seed=2)).build_model()
    gan.train(iterations=2, resume=False, samples=True)
    assert os.listdir(str(tmp_path / "samples")) == ["BigGAN_ema_00_00002.png"]
    assert _read_png(str(tmp_path / "samples" / "BigGAN_ema_00_00002.png")).shape == (128, 128, 3)


def test_sampling_between_graph_replays_leaves_the_graphs_state_alone(tmp_path):
    """With captured graphs sampling runs eagerly on the tensors the graphs read and write: it must leave them as they
    were, and the next replay must run."""
    args = make_args(img_size=64, ch=8, batch_size=4, z_dim=64, sample_num=4, sample_dir=str(tmp_path / "samples"))
    gan = model.BigGAN(args, store=S.VariableStore("cuda", seed=2)).build_model()
    gan.capture_graphs()
    for _ in range(2):
        gan.train_step(gan.synthetic_batch())
    snap = _snapshot(gan)
    paths = gan.save_samples(0, 2)
    _assert_untouched(gan, snap)
    assert _kinds(paths) == ["BigGAN_ema_00_00002.png"] and _read_png(paths[0]).shape == (128, 128, 3)
    losses = gan.train_step(gan.synthetic_batch())
    assert all(bool(torch.isfinite(v.detach()).all()) for v in losses.values())


# ---------------------------------------------------------------- weight-sharded power iteration
def test_a_sharded_spectral_norm_batch_can_iterate_locally():
    """Under data parallelism the power iteration is sharded by weight and ends in an all-gather; only rank 0 runs the
    generator for the sample grids, so ``generate`` switches the generator's batches to ``local_only``: every weight is
    iterated on this rank by the entry point an unsharded batch uses.  Same kernel, same sizes, same inputs: the result
    must be bit-identical to the unsharded batch's, and agree with the sharded phases (power, gather, normalise) within
    the 1e-6 of the spectral-norm tests."""
    from tests.common import rel_err, t2n
    g = torch.Generator(device="cuda").manual_seed(11)
    ws = [torch.randn(3, 3, 8, 16, device="cuda", generator=g) * 0.05, torch.randn(1, 1, 16, 6, device="cuda", generator=g),
          torch.randn(20, 24, device="cuda", generator=g) * 0.1]
    us = [torch.randn(1, w.shape[-1], device="cuda", generator=g) for w in ws]

    def batch(shard, local):
        sb = Fn.SnBatch([(w.clone(), u.clone()) for w, u in zip(ws, us)], None, shard)
        sb.local_only = local
        wn = [t.clone() for t in sb.forward()]
        return wn, [u.clone() for u in sb.u]
    plain = batch(None, False)
    local = batch((0, 1, None), True)
    phases = batch((0, 1, None), False)
    for i in range(len(ws)):
        for a, b, c in zip((plain[0][i], plain[1][i]), (local[0][i], local[1][i]), (phases[0][i], phases[1][i])):
            assert torch.equal(a, b), i
            assert rel_err(t2n(c), t2n(b)) < 1e-6, i
        assert not torch.equal(local[1][i], us[i])                  # the iteration did advance u
