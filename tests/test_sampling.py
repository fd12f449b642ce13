"""In-training sample grids (BigGAN.py:980-1008, 1125-1230), the host side: --sample_ema validation, the grid plan, the
static latent set, the morph latents against a literal restatement of the reference's double loop, file names, the
class-vector file, utils.grid_u8 / write_png, the C entry point's argument checks and the command line's opt-in.
No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, model, sampling as Sp, scope as S, utils


def _model(*extra, seed=42):
    args = M.parse_args(["--gan_type", "hinge", "--img_size", "64", "--ch", "8"] + list(extra), make_dirs=False)
    return model.BigGAN(args, device="cpu", store=S.VariableStore("cpu", seed))


# ---------------------------------------------------------------- --sample_ema
def test_sample_ema_bogus_is_a_value_error():
    with pytest.raises(ValueError):
        _model("--sample_ema", "bogus")


@pytest.mark.parametrize("mode,ema,noema", [("ema", True, False), ("noema", False, True), ("both", True, True)])
def test_sample_ema_sets_the_two_flags(mode, ema, noema):
    gan = _model("--sample_ema", mode)
    assert (gan.generate_ema_samples, gan.generate_noema_samples) == (ema, noema)


def test_save_morphs_needs_a_grid_side_of_two():
    with pytest.raises(ValueError):
        _model("--save_morphs", "true", "--sample_num", "3")
    _model("--save_morphs", "true", "--sample_num", "4")


# ---------------------------------------------------------------- grid_plan
def test_grid_plan():
    assert Sp.grid_plan(64, 16) == (8, 64, 4)
    assert Sp.grid_plan(10, 4) == (3, 12, 3)
    assert Sp.grid_plan(1, 16) == (1, 16, 1)


# ---------------------------------------------------------------- static_z
def test_static_z_is_a_function_of_its_seed():
    a = Sp.static_z(12, 64, 123456789, True)
    assert a.shape == (12, 1, 1, 64) and a.dtype == torch.float32 and a.device.type == "cpu"
    assert torch.equal(a, Sp.static_z(12, 64, 123456789, True))
    assert not torch.equal(a, Sp.static_z(12, 64, 123456790, True))


def test_static_z_truncation():
    assert float(Sp.static_z(64, 64, 7, True).abs().max()) <= 2.0
    assert float(Sp.static_z(64, 64, 7, False).abs().max()) > 2.0          # 4096 plain-normal draws: P(none) ~ 1e-83


def test_static_set_is_independent_of_the_store_seed_and_of_global_generators():
    a = _model(seed=1).static_sample_set()[0]
    torch.manual_seed(99)
    np.random.seed(99)
    b = _model(seed=2).static_sample_set()[0]
    assert a.shape == (64, 1, 1, 256) and a.dtype == np.float32
    assert np.array_equal(a, b)
    assert np.array_equal(a, Sp.static_z(64, 256, 123456789, True).numpy())


def test_static_class_vectors():
    gan = _model("--n_labels", "5", "--sample_num", "10", "--batch_size", "4")
    state = np.random.get_state()[1].copy()
    z, cls = gan.static_sample_set()
    assert np.array_equal(np.random.get_state()[1], state)                  # the global generator is not used
    assert z.shape == (12, 1, 1, 256) and cls.shape == (12, 5) and cls.dtype == np.float32
    assert np.array_equal(cls.sum(1), np.ones(12)) and set(np.unique(cls)) == {0.0, 1.0}      # synthetic: one-hots
    assert np.array_equal(cls, Sp.static_cls(np.eye(5, dtype=np.float32), 12, 123456789))
    # rows of a label table when there is one
    table = [[1.0, 0.0, 1.0], [0.0, 0.5, 0.0]]
    rows = Sp.static_cls(table, 9, 3)
    assert rows.shape == (9, 3) and all(r.tolist() in table for r in rows)


# ---------------------------------------------------------------- morph latents
def _morph_literal(z_a, z_b, z_c, z_d, cz, manifold):
    """BigGAN.py:1183-1193 restated: x outer, y inner, the border ring extrapolates."""
    morph_padding = 1
    zs, czs = [], ([] if cz is not None else None)
    for x in range(-morph_padding, manifold + morph_padding):
        rx = x / (manifold - 1)
        for y in range(-morph_padding, manifold + morph_padding):
            ry = y / (manifold - 1)
            zs.append(z_a * (1 - rx) * (1 - ry) + z_b * (rx) * (1 - ry) + z_c * (1 - rx) * (ry) + z_d * (rx) * (ry))
            if cz is not None:
                czs.append(cz[0] * (1 - rx) * (1 - ry) + cz[1] * (rx) * (1 - ry) + cz[2] * (1 - rx) * (ry) + cz[3] * (rx) * (ry))
    return zs, czs


@pytest.mark.parametrize("dim", [3, 8])
@pytest.mark.parametrize("with_cls", [False, True])
def test_morph_latents_are_the_reference_double_loop(dim, with_cls):
    rs = np.random.RandomState(dim)
    z4 = [rs.randn(1, 1, 24).astype(np.float32) for _ in range(4)]
    cz4 = [rs.rand(5).astype(np.float32) for _ in range(4)] if with_cls else None
    z, cz = Sp.morph_latents(z4, cz4, dim)
    want_z, want_cz = _morph_literal(z4[0], z4[1], z4[2], z4[3], cz4, dim)
    assert z.shape == ((dim + 2) ** 2, 1, 1, 24) and z.dtype == np.float32
    assert np.array_equal(z, np.stack(want_z))
    if with_cls:
        assert cz.shape == ((dim + 2) ** 2, 5) and cz.dtype == np.float32
        assert np.array_equal(cz, np.stack(want_cz))
    else:
        assert cz is None
    # the inner dim x dim corners are the four latents themselves
    side = dim + 2
    assert np.array_equal(z[1 * side + 1], z4[0]) and np.array_equal(z[dim * side + 1], z4[1])
    assert np.array_equal(z[1 * side + dim], z4[2]) and np.array_equal(z[dim * side + dim], z4[3])


def test_morph_latents_reject_a_one_tile_grid():
    z4 = [np.zeros((1, 1, 8), np.float32)] * 4
    with pytest.raises(ValueError):
        Sp.morph_latents(z4, None, 1)


# ---------------------------------------------------------------- host random choices
def test_event_choices_come_from_a_local_generator():
    state = np.random.get_state()[1].copy()
    rng = Sp.event_rng(123456789, 3, 10000, 250)
    corners = Sp.morph_corners(10, rng)
    table = np.eye(4, dtype=np.float32)
    tag, rows = Sp.cls_grid_vectors(table, 4, 9, rng)
    assert np.array_equal(np.random.get_state()[1], state)
    assert len(corners) == 4 and all(0 <= c < 10 for c in corners)
    assert 0 <= tag < 4 and rows.shape == (9, 4) and np.all(rows[:, tag] > 0)
    # the same event gives the same choices, another iteration does not share its generator's seed
    rng2 = Sp.event_rng(123456789, 3, 10000, 250)
    assert Sp.morph_corners(10, rng2) == corners and Sp.cls_grid_vectors(table, 4, 9, rng2)[0] == tag
    want = np.random.RandomState((123456789 + 3 * 10000 + 250) % 2 ** 32)
    assert corners == [int(want.randint(10)) for _ in range(4)]
    assert Sp.event_rng(2 ** 32 - 1, 1, 1, 5).randint(100) == np.random.RandomState(5).randint(100)      # mod 2**32


def test_select_by_tag_falls_back_after_1000_misses(capsys):
    table = np.asarray([[1.0, 0.0], [1.0, 0.0]], np.float32)
    row = Sp.select_by_tag(table, 1, np.random.RandomState(0))
    assert row.tolist() == [1.0, 0.0] and "did not find" in capsys.readouterr().out


# ---------------------------------------------------------------- file names
def test_sample_file_names():
    names = Sp.sample_names("BigGAN", 3, 250, tag=7)
    assert names == {"ema": "BigGAN_ema_03_00250.png", "noema": "BigGAN_noema_03_00250.png",
                     "morph": "BigGAN_morph_03_00250.png", "cls": "BigGAN_cls_03_00250_007.png"}
    assert "cls" not in Sp.sample_names("BigGAN", 3, 250)


# ---------------------------------------------------------------- class-vector file
def test_vector_file_round_trip(tmp_path):
    rows = np.asarray([[0.0, 1.0, 0.25], [1.0, 0.0, 1e-3], [0.5, 0.5, 0.5]], np.float32)
    path = Sp.write_vectors(str(tmp_path / "cls.tsv"), rows)
    text = open(path).read()
    assert text.splitlines()[0] == "\t".join(map(str, [0.0, 1.0, 0.25]))
    cmds, back = Sp.read_vectors(path, expect=3)
    assert cmds == {} and np.array_equal(np.asarray(back, np.float32), rows)
    with open(path, "w") as f:
        f.write("!cmd=1\tflag\n" + text)
    cmds, back = Sp.read_vectors(path, expect=3)
    assert cmds == {"cmd": "1", "flag": ""} and np.array_equal(np.asarray(back, np.float32), rows)
    with pytest.raises(ValueError) as e:
        Sp.read_vectors(path, expect=4)
    assert "3" in str(e.value) and "4" in str(e.value)


def test_static_class_vectors_from_and_to_files(tmp_path):
    src, dst = str(tmp_path / "in.tsv"), str(tmp_path / "out.tsv")
    rows = np.random.RandomState(0).rand(12, 3).astype(np.float32)
    Sp.write_vectors(src, rows)
    gan = _model("--n_labels", "3", "--sample_num", "10", "--batch_size", "4", "--load_cls_samples_from", src,
                 "--save_cls_samples_to", dst)
    assert np.array_equal(gan.static_sample_set()[1], rows)
    assert np.array_equal(np.asarray(Sp.read_vectors(dst)[1], np.float32), rows)
    Sp.write_vectors(src, rows[:11])
    gan = _model("--n_labels", "3", "--sample_num", "10", "--batch_size", "4", "--load_cls_samples_from", src)
    with pytest.raises(ValueError) as e:
        gan.static_sample_set()
    assert "11" in str(e.value) and "12" in str(e.value)


# ---------------------------------------------------------------- grid_u8 / write_png
@pytest.mark.parametrize("c", [1, 3, 4])
def test_grid_u8_and_write_png_are_imsave(tmp_path, c):
    x = (np.random.RandomState(c).rand(5, 6, 10, c).astype(np.float32) * 2.5 - 1.25)
    size = [2, 3]
    g = utils.grid_u8(utils.inverse_transform(x), size)
    want = np.clip(np.rint(utils.merge(utils.inverse_transform(x), size) * 255.0), 0, 255).astype(np.uint8)
    assert g.dtype == np.uint8 and g.shape == (12, 30, c)
    assert np.array_equal(g.reshape(want.shape), want)
    assert g.min() == 0 and g.max() == 255 and not g[6:, 20:].any()          # clamped both ways; the empty tile is 0
    a = utils.write_png(g, str(tmp_path / "a.png"))
    b = utils.imsave(utils.inverse_transform(x), size, str(tmp_path / "b.png"))
    d = utils.save_images(x, size, str(tmp_path / "d.png"))
    assert open(a, "rb").read() == open(b, "rb").read() == open(d, "rb").read()
    if c == 1:
        e = utils.write_png(g[:, :, 0], str(tmp_path / "e.png"))              # [h, w] is grayscale
        assert open(e, "rb").read() == open(a, "rb").read()


def test_write_png_rejects_floats(tmp_path):
    with pytest.raises(ValueError):
        utils.write_png(np.zeros((4, 4, 3), np.float32), str(tmp_path / "x.png"))


# ---------------------------------------------------------------- C entry point
def test_image_tiles_u8_is_bound_and_checks_its_arguments():
    L = hip.lib()
    assert L.bg_abi_version() == hip.ABI_VERSION >= 9
    assert "bg_image_tiles_u8" in hip.SIGNATURES
    fake = ctypes.c_void_p(4096)                    # never dereferenced: every call below fails validation
    ok = dict(x=fake, dt=hip.F32, n=2, H=8, W=8, C=3, grid=fake, gh=1, gw=2, tile0=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.bg_image_tiles_u8(a["x"], a["dt"], a["n"], a["H"], a["W"], a["C"], a["grid"], a["gh"], a["gw"], a["tile0"],
                                   None)
    for bad in (dict(x=None), dict(grid=None), dict(dt=2), dict(C=2), dict(C=5), dict(n=0), dict(H=0), dict(W=-1),
                dict(gh=0), dict(gw=0), dict(tile0=-1)):
        assert call(**bad) == 1, bad
        assert b"bg_image_tiles_u8" in L.bg_last_error()
    assert call(tile0=2) == 0                      # every image falls past the grid: nothing to launch


def test_image_tiles_u8_has_no_host_fallback():
    from biggan_tensorflow_amd import functional as Fn
    with pytest.raises(RuntimeError):
        Fn.image_tiles_u8(torch.zeros(1, 4, 4, 3), torch.zeros(4, 4, 3, dtype=torch.uint8), 1, 1)


# ---------------------------------------------------------------- command line
def test_the_command_line_trains_with_samples(monkeypatch):
    calls = []

    class Stub:
        def __init__(self, args):
            calls.append(("init", args.sample_ema))

        def build_model(self):
            calls.append(("build",))

        def train(self, *a, **kw):
            calls.append(("train", a, kw))

    monkeypatch.setattr(model, "BigGAN", Stub)
    monkeypatch.setattr(M, "check_folder", lambda d: d)
    M.main(["--phase", "train"])
    assert calls == [("init", "ema"), ("build",), ("train", (), {"samples": True})]


def test_train_does_not_sample_unless_asked():
    import inspect
    sig = inspect.signature(model.BigGAN.train)
    assert list(sig.parameters)[1:] == ["data_fn", "iterations", "resume", "samples"]
    assert sig.parameters["samples"].default is False
