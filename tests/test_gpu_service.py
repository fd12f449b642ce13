"""--phase service on the device: bg_image_place_u8 against utils.grid_u8 per image, byte for byte, inside guard bands;
BigGAN.generate(with_discriminator=True) against the generator followed by the discriminator called directly; the
service itself, in-process on a temporary request folder: strips and .out files against generate() of each file's own
latents, shared generator batches, slot independence, ema, load_checkpoint, bf16."""
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data, functional as Fn, hip, model, ops, scope as S, service as Sv, utils
from tests.common import make_args, rel_err, t2n

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3            # the fp32 gate of tests/test_gpu_step.py for logits and images: relative L2 per tensor
BAND, FILL = 4096, 0xAB


# ---------------------------------------------------------------- kernel against numpy
def _images(n, H, W, C, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(n, H, W, C, device="cuda", generator=g) * 2.5) - 1.25).to(dtype)


def _host_bytes(x):
    """utils.grid_u8 per image: uint8 [n, H, W*C]."""
    a = x.detach().float().cpu().numpy()                     # (bf16 -> fp32 is exact)
    with np.errstate(invalid="ignore"):
        return np.stack([utils.grid_u8(utils.inverse_transform(a[i:i + 1]), [1, 1]).reshape(a.shape[1], -1)
                         for i in range(a.shape[0])])


def _valid(e, H, tw, nbytes):
    off, pitch, skip = e
    return not skip and off >= 0 and pitch >= tw and off + (H - 1) * pitch + tw <= nbytes


def _expect(x, entries, nbytes):
    n, H, W, C = x.shape
    want = np.full(nbytes, FILL, np.uint8)
    img = _host_bytes(x)
    for i, e in enumerate(entries):
        if _valid(e, H, W * C, nbytes):
            for r in range(H):
                lo = e[0] + r * e[1]
                want[lo:lo + W * C] = img[i, r]
    return want


def _run(x, entries, nbytes, band=BAND):
    buf = torch.full((band + nbytes + BAND,), FILL, dtype=torch.uint8, device="cuda")
    arena = buf[band:band + nbytes]
    table = torch.from_numpy(Sv.place_table(entries)).cuda()
    Fn.image_place_u8(x, table, arena)
    got = buf.cpu().numpy()
    assert (got[:band] == FILL).all() and (got[band + nbytes:] == FILL).all()      # the guard bytes stay
    return got[band:band + nbytes]


def _layout(kind, n, H, tw):
    """(entries, arena bytes).  tight: the images side by side in one strip; slack: a pitch wider than the strip;
    offgrid: offsets and pitch off the 4-byte grid; skip: image 1 is a padding slot; rows: every image a strip of its
    own, 16-byte aligned (what the planner makes for one-latent files)."""
    if kind == "tight":
        return [(i * tw, n * tw, 0) for i in range(n)], H * n * tw
    if kind == "slack":
        pitch = n * tw + 8
        return [(4 + i * tw, pitch, 0) for i in range(n)], 4 + H * pitch
    if kind == "offgrid":
        pitch = n * tw + 5
        return [(3 + i * tw, pitch, 0) for i in range(n)], 3 + H * pitch + 2
    if kind == "skip":
        return [(i * tw, n * tw, 1 if i == 1 else 0) for i in range(n)], H * n * tw
    if kind == "rows":
        step = (H * tw + 15) // 16 * 16
        return [(i * step, tw, 0) for i in range(n)], n * step
    raise ValueError(kind)


SHAPES = [(5, 4, 6), (3, 5, 7), (5, 4, 8)]      # W*C % 4 == 0 at (6, C=4) and (8, any C): the 4-wide path; else scalar


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["tight", "slack", "offgrid", "skip", "rows"])
def test_kernel_equals_grid_u8_per_image(kind, shape, C, dtype):
    n, H, W = shape
    x = _images(n, H, W, C, dtype, seed=n + H + W + C)
    entries, nbytes = _layout(kind, n, H, W * C)
    want = _expect(x, entries, nbytes)
    assert np.array_equal(_run(x, entries, nbytes), want)
    assert int((want != FILL).sum()) > 0 and int(want.max()) == 255 and int((want == 0).sum()) > 0
    if kind == "skip":                                         # the padding slot wrote nothing
        assert (want.reshape(H, n, W * C)[:, 1] == FILL).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,C", [((1, 4, 8), 3), ((1, 5, 7), 3), ((1, 4, 6), 4), ((1, 3, 5), 1)])
def test_kernel_one_image(shape, C, dtype):
    n, H, W = shape
    x = _images(n, H, W, C, dtype, seed=9)
    entries, nbytes = _layout("slack", n, H, W * C)
    assert np.array_equal(_run(x, entries, nbytes), _expect(x, entries, nbytes))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_kernel_arena_off_the_word_grid(dtype):
    """An arena whose first byte is not 4-byte aligned takes the one-element path whatever the table says."""
    x = _images(5, 4, 8, 4, dtype, seed=4)
    entries, nbytes = _layout("tight", 5, 4, 32)
    assert np.array_equal(_run(x, entries, nbytes, band=BAND + 1), _expect(x, entries, nbytes))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,C", [((4, 4, 8), 3), ((4, 5, 7), 3)], ids=["wide", "scalar"])
def test_entries_that_do_not_fit_write_nothing(shape, C, dtype):
    """One good entry and three that each break one condition: offset < 0, pitch < W*C, and an extent one step past the
    arena.  The three images stay unwritten whole (not clipped)."""
    n, H, W = shape
    tw = W * C
    x = _images(n, H, W, C, dtype, seed=12)
    step = 4 if tw % 4 == 0 else 1
    nbytes = 4 * H * tw
    entries = [(0, tw, 0),
               (-step, tw, 0),                                     # offset < 0
               (H * tw, tw - step, 0),                             # pitch < W*C (its rows would still lie inside)
               (nbytes - H * tw + step, tw, 0)]                    # offset + (H-1)*pitch + W*C = arena_bytes + step
    assert [_valid(e, H, tw, nbytes) for e in entries] == [True, False, False, False]
    want = _expect(x, entries, nbytes)
    assert (want[H * tw:] == FILL).all() and (want[:H * tw] != FILL).any()
    assert np.array_equal(_run(x, entries, nbytes), want)
    # the last one fits once it ends exactly at the arena's end
    entries[3] = (nbytes - H * tw, tw, 0)
    want = _expect(x, entries, nbytes)
    assert (want[nbytes - H * tw:] != FILL).any()
    assert np.array_equal(_run(x, entries, nbytes), want)


def test_a_far_offset_is_checked_without_overflow():
    x = _images(2, 4, 8, 3, torch.float32, seed=1)
    big = (1 << 63) - 1
    entries = [(big, 24, 0), (big - 100, (1 << 31) - 1, 0)]
    assert (_run(x, entries, 4 * 24 * 2) == FILL).all()


def test_argument_errors_carry_a_message():
    x = _images(2, 4, 4, 3, torch.float32)
    arena = torch.zeros(2 * 48, dtype=torch.uint8, device="cuda")
    table = torch.from_numpy(Sv.place_table([(0, 12, 0), (48, 12, 0)])).cuda()
    with pytest.raises(RuntimeError):
        Fn.image_place_u8(x.half(), table, arena)
    with pytest.raises(RuntimeError):
        Fn.image_place_u8(x, table.long(), arena)
    with pytest.raises(RuntimeError):
        Fn.image_place_u8(x, table[:1], arena)                     # one entry per image
    with pytest.raises(RuntimeError):
        Fn.image_place_u8(x, table, arena.float())
    with pytest.raises(RuntimeError, match="bg_image_place_u8: C=2"):
        Fn.image_place_u8(x[..., :2], table, arena)
    flat = torch.zeros(9, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="bg_image_place_u8: table"):
        Fn.image_place_u8(x, flat[1:].view(2, 4), arena)           # 4-byte aligned only
    L = hip.lib()
    rc = L.bg_image_place_u8(hip.ptr(x), hip.F32, 2, 4, 4, 3, hip.ptr(table), hip.ptr(arena), 0, None)
    assert rc != 0 and b"arena_bytes" in L.bg_last_error()
    torch.cuda.synchronize()
    assert not arena.any()


# ---------------------------------------------------------------- model level
def _model(tmp_path, **kw):
    flags = dict(img_size=64, ch=8, z_dim=64, batch_size=4, request_dir=str(tmp_path / "request"),
                 checkpoint_dir=str(tmp_path / "ckpt"))
    flags.update(kw)
    seed = flags.pop("seed", 2)
    gan = model.BigGAN(make_args(**flags), store=S.VariableStore("cuda", seed=seed)).build_model()
    gan.train_step(gan.synthetic_batch())                  # the moving averages now differ from the live weights
    os.makedirs(flags["request_dir"], exist_ok=True)
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
    assert any(k.endswith("/u") for k in tensors if k.startswith("discriminator/"))
    assert torch.equal(gan.gen.get_state(), rng)
    assert gan.counter == counter and (gan.d_arena.step, gan.g_arena.step) == steps


def _latents(gan, n, seed):
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, gan.z_dim)).astype(np.float32)
    cls = (rng.rand(n, gan.n_labels) < 0.5).astype(np.float32) if gan.acgan else None
    return z, cls


def _direct(gan, z, cls, ema=True):
    """The generator followed by the discriminator (is_training=False), called directly, batch_size rows at a time, the
    list padded with entry 0; every ``u`` put back afterwards."""
    B, n = gan.batch_size, z.shape[0]
    pad = -n % B
    zt = torch.from_numpy(np.concatenate([z, np.repeat(z[:1], pad, 0)])).cuda()
    ct = None if cls is None else torch.from_numpy(np.concatenate([cls, np.repeat(cls[:1], pad, 0)])).cuda()
    us = [gan.store.vars[u] for u in gan.store.sn_pairs.values()]
    saved = [u.clone() for u in us]
    imgs, outs = [], {}
    for b in range(0, n + pad, B):
        with torch.no_grad():
            torch._foreach_copy_(us, saved)
        img = gan.sample(zt[b:b + B].reshape(B, 1, 1, -1), None if ct is None else ct[b:b + B], use_ema=ema)
        S.set_default_store(gan.store)
        ops.begin_run(None, 1)
        with torch.no_grad():
            d = gan.discriminator(img, is_training=False, reuse=True)
        imgs.append(img.float())
        for k, v in d.items():
            outs.setdefault(k, []).append(v.float())
    with torch.no_grad():
        torch._foreach_copy_(us, saved)
    return torch.cat(imgs)[:n], {k: torch.cat(v)[:n] for k, v in outs.items()}


@pytest.mark.parametrize("n_labels", [0, 3])
def test_with_discriminator_equals_the_direct_calls_and_leaves_the_model_alone(tmp_path, n_labels):
    gan = _model(tmp_path, n_labels=n_labels)
    z, cls = _latents(gan, 5, 7)
    want_img, want = _direct(gan, z, cls)
    snap = _snapshot(gan)
    img, outs = gan.generate(z, cls, with_discriminator=True)
    _assert_untouched(gan, snap)
    assert sorted(outs) == (["cls", "real"] if n_labels else ["real"])
    assert img.shape == (5, 64, 64, 3) and outs["real"].shape == (5, 1) and outs["real"].dtype == torch.float32
    assert rel_err(t2n(img.float()), t2n(want_img)) < GRAD_TOL
    assert rel_err(t2n(outs["real"]), t2n(want["real"])) < GRAD_TOL
    if n_labels:
        assert outs["cls"].shape == (5, 3)
        assert rel_err(t2n(outs["cls"]), t2n(want["cls"])) < GRAD_TOL
    assert float(outs["real"].std()) > 0
    # without the flag nothing changes: the images alone, the same bits
    assert torch.equal(gan.generate(z, cls), img)
    # and with a grid the bytes of the grid path
    grid = torch.zeros(128, 192, 3, dtype=torch.uint8, device="cuda")
    g2, o2 = gan.generate(z, cls, grid=grid, gh=2, gw=3, with_discriminator=True)
    assert g2 is grid and all(torch.equal(o2[k], outs[k]) for k in outs)
    _assert_untouched(gan, snap)


def _write_request(gan, name, z, cls, cmd=None):
    rows = z if cls is None else np.concatenate([z, cls], axis=1)
    path = os.path.join(gan.args.request_dir, name + ".txt")
    utils.write_vectors(path + ".part", rows)
    body = open(path + ".part").read()
    os.remove(path + ".part")
    with open(path + ".part", "w") as f:
        f.write(("!" + "\t".join(cmd) + "\n" if cmd else "") + body)
    os.rename(path + ".part", path)
    return path


def _quit(gan, name="zzz_quit"):
    with open(os.path.join(gan.args.request_dir, name + ".txt"), "w") as f:
        f.write("!quit\n")


def _strip(img):
    a = img.float().cpu().numpy()
    return utils.grid_u8(utils.inverse_transform(a), [1, a.shape[0]])


def _png(gan, name):
    return data.decode_png(open(os.path.join(gan.args.request_dir, name + ".png"), "rb").read())


def _out(gan, name, key):
    return np.asarray(utils.read_vectors(os.path.join(gan.args.request_dir, "%s_%s.out" % (name, key)))[1], np.float32)


def _count_generator(gan, monkeypatch):
    calls = []
    real = gan.generator

    def counted(*a, **kw):
        calls.append(a[0].shape[0])
        return real(*a, **kw)
    monkeypatch.setattr(gan, "generator", counted)
    return calls


def _end_to_end(gan, monkeypatch):
    lat = {"a": _latents(gan, 1, 1), "b": _latents(gan, 5, 2), "c": _latents(gan, 2, 3)}
    want = {k: gan.generate(z, cls, with_discriminator=True) for k, (z, cls) in lat.items()}
    gan.save(gan.checkpoint_dir, gan.counter)              # service() starts from the latest checkpoint: this state
    snap = _snapshot(gan)
    cmds = {"a": ["use_discriminator=1"], "b": ["use_discriminator=1", "discriminator_outputs=real"],
            "c": ["ema=1", "use_discriminator=1", "discriminator_outputs=cls,real"]}
    paths = [_write_request(gan, k, z, cls, cmds[k]) for k, (z, cls) in lat.items()]
    _quit(gan)
    calls = _count_generator(gan, monkeypatch)
    assert gan.service() == 3
    assert calls == [4, 4]                                 # 8 latents share two batches: not 3 (per file) or 8
    monkeypatch.undo()
    _assert_untouched(gan, snap)
    keys = sorted(want["a"][1])
    expect = ["a.png", "b.png", "b_real.out", "c.png", "c_real.out"] + ["a_%s.out" % k for k in keys]
    if "cls" in keys:
        expect.append("c_cls.out")
    assert sorted(os.listdir(gan.args.request_dir)) == sorted(expect)      # the requests and the quit file are gone
    assert not any(os.path.exists(p) for p in paths)
    for k, (z, cls) in lat.items():
        img, outs = want[k]
        got = _png(gan, k)
        assert got.shape == (64, 64 * z.shape[0], 3)
        assert np.array_equal(got, _strip(img)), k
        for key in keys:
            if os.path.exists(os.path.join(gan.args.request_dir, "%s_%s.out" % (k, key))):
                assert np.array_equal(_out(gan, k, key), t2n(outs[key]).reshape(z.shape[0], -1)), (k, key)
    assert _png(gan, "b").std() > 0


def test_end_to_end(tmp_path, monkeypatch):
    _end_to_end(_model(tmp_path, n_labels=3), monkeypatch)


def test_end_to_end_bf16(tmp_path, monkeypatch):
    """--precision bf16 at the smallest topology at which tests/test_gpu_bf16.py runs a whole step (64^2, ch 16, B 4)."""
    _end_to_end(_model(tmp_path, ch=16, precision="bf16"), monkeypatch)


def test_the_slot_does_not_matter_and_ema_does(tmp_path, monkeypatch):
    gan = _model(tmp_path)
    z, _ = _latents(gan, 1, 5)
    w, _ = _latents(gan, 2, 6)
    # one group: z in slot 0 (a), w in slots 1-2 (b), z again in slot 3 (c)
    _write_request(gan, "a", z, None)
    _write_request(gan, "b", w, None)
    _write_request(gan, "c", z, None)
    # ema=0 opens a second group: z from the live weights, in slot 0 (d) and in slot 3 (f)
    _write_request(gan, "d", z, None, ["ema=0"])
    _write_request(gan, "e", w, None, ["ema=0"])
    _write_request(gan, "f", z, None, ["ema=0"])
    _quit(gan)
    calls = _count_generator(gan, monkeypatch)
    snap = _snapshot(gan)
    assert gan.service() == 6 and calls == [4, 4]
    monkeypatch.undo()
    _assert_untouched(gan, snap)
    a, c, d, f = (_png(gan, k) for k in "acdf")
    assert np.array_equal(a, c) and np.array_equal(d, f)           # the same latent from slot 0 and from slot 3
    assert not np.array_equal(a, d)                                # the averages differ from the live weights
    assert np.array_equal(a, _strip(gan.generate(z, None, ema=True)))
    assert np.array_equal(d, _strip(gan.generate(z, None, ema=False)))


def test_load_checkpoint_between_two_identical_requests(tmp_path):
    gan = _model(tmp_path)
    z, _ = _latents(gan, 3, 8)
    first = gan.save(gan.checkpoint_dir, 1)
    want_first = _strip(gan.generate(z, None))
    gan.train_step(gan.synthetic_batch())
    gan.save(gan.checkpoint_dir, 2)                        # the latest: what the service starts from
    want_second = _strip(gan.generate(z, None))
    assert not np.array_equal(want_first, want_second)
    _write_request(gan, "a", z, None)
    _write_request(gan, "b", z, None, ["load_checkpoint=" + first])
    _write_request(gan, "c", z, None)
    _quit(gan)
    assert gan.service() == 3
    assert np.array_equal(_png(gan, "a"), want_second)
    assert np.array_equal(_png(gan, "b"), want_first) and np.array_equal(_png(gan, "c"), want_first)
    assert gan.counter == 1
