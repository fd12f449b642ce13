"""Generator latent stage with --cls_embedding / --shared_z / --g_z_dense_concat (BigGAN.py:278-444): variable manifest
against the float64 restatement in tests/latent_ref.py, checkpoints and the flag gate.  No GPU needed."""
import os

import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import main as M, model, scope as S
from oracle import ref_ops as R
from tests import latent_ref as LR

CASES = [
    (128, dict(n_labels=10, cls_embedding=True)),
    (128, dict(shared_z=32)),
    (64, dict(n_labels=10, cls_embedding=True, cls_embedding_concat=True, shared_z=16)),
    (256, dict(n_labels=5, shared_z=24, g_z_dense_concat=True)),
    (512, dict(g_z_dense_concat=True, g_other_level_dense_layer=True)),
    (128, dict(n_labels=20, cls_embedding=True, cls_embedding_size=16, g_other_level_dense_layer=True, deep=True)),
    (256, dict(shared_z=32, g_first_level_dense_layer=False)),
    (512, dict(n_labels=12, cls_embedding=True, cls_embedding_concat=True, shared_z=20, g_z_dense_concat=True,
               g_other_level_dense_layer=True)),
    (64, dict(n_labels=7, shared_z=16, g_other_level_dense_layer=True, deep=True)),
]


def _argv(size, kw):
    argv = ["--gan_type", "hinge", "--img_size", str(size), "--ch", "8"]
    for k, v in kw.items():
        argv += ["--" + k, str(v)]
    return M.parse_args(argv, make_dirs=False)


def _hip_generator_manifest(size, kw):
    store = S.VariableStore("cpu")
    gan = model.BigGAN(_argv(size, kw), device="cpu", store=store)
    img = gan.generator(torch.empty(2, 1, 1, gan.z_dim, device="meta"))
    assert tuple(img.shape) == (2, size, size, 3)
    return [(k, tuple(v.shape)) for k, v in store.vars.items()], store


def _ref_generator_manifest(size, kw):
    cfg = LR.config(img_size=size, ch=8, batch_size=2, **kw)
    vs = R.VarStore(torch.float64, 0)
    z = torch.zeros(2, 1, 1, cfg.z_dim, dtype=torch.float64)
    cz = torch.zeros(2, cfg.n_labels, dtype=torch.float64) if cfg.n_labels else None
    with torch.no_grad():
        img = LR.generator(vs, cfg, z, cz, True)
    assert tuple(img.shape) == (2, size, size, 3)
    return [(k, tuple(v.shape)) for k, v in vs.vars.items()], vs


def _latent_names(manifest):
    top = ("cls_embed/", "shared_z/", "first/")
    return [k for k, _ in manifest if k.endswith("/kernel") and
            (k.split("/", 1)[1].startswith(top) or k.split("/")[1][1:].isdigit())]


@pytest.mark.parametrize("size,kw", CASES)
def test_manifest_matches_restatement(size, kw):
    mine, store = _hip_generator_manifest(size, kw)
    ref, vs = _ref_generator_manifest(size, kw)
    assert dict(mine) == dict(ref)
    assert {k for k, _ in mine if store.trainable[k]} == {k for k, _ in ref if vs.trainable[k]}
    # the latent stage's variables are created in the reference's order: embedding, shared z, per-level layers, first
    assert _latent_names(mine) == _latent_names(ref)
    assert not any(k.startswith("generator/dense") or k.startswith("generator/first/dense1") for k, _ in mine)


def test_worked_examples_of_the_split():
    """z_dim 256, --img_size 128 --ch 8: the two hand-worked rows (embedding 32 = round_up(int(10**0.88 + 24), 8))."""
    m = dict(_hip_generator_manifest(128, dict(n_labels=10, cls_embedding=True))[0])
    assert m["generator/cls_embed/dense1/kernel"] == (10, 32)
    assert m["generator/z0/dense1/kernel"] == (128, 208)
    assert m["generator/first/dense/kernel"] == (208, 2048)
    assert m["generator/resblock_up_8/res2/batch_norm/gamma/kernel"][0] == 64
    m = dict(_hip_generator_manifest(128, dict(shared_z=32))[0])
    assert m["generator/shared_z/dense1/kernel"] == (32, 48)
    assert m["generator/z1/dense1/kernel"] == (132, 200)
    assert m["generator/first/dense/kernel"] == (200, 2048)
    assert m["generator/resblock_up_1/res1/batch_norm/beta/kernel"][0] == 76
    gan = model.BigGAN(_argv(128, dict(shared_z=32)), device="cpu", store=S.VariableStore("cpu"))
    assert gan.new_z_split_sizes(gan.g_block_info())[0] == [32, 84, 28, 28, 28, 28, 28]
    assert LR.split_sizes(LR.config(img_size=128, shared_z=32))[0] == [32, 84, 28, 28, 28, 28, 28]


def test_defaults_build_unchanged():
    """Without the three flags the generator keeps its old variables (first/dense1, dense2; no latent scopes)."""
    mine, _ = _hip_generator_manifest(128, dict(n_labels=10))
    names = dict(mine)
    assert names["generator/first/dense1/kernel"] == (106, 200)
    assert not any("cls_embed" in k or "shared_z" in k or "/z0/" in k for k in names)


def test_checkpoint_roundtrip_with_latent_variables(tmp_path):
    def make():
        g = model.BigGAN(_argv(64, dict(n_labels=10, cls_embedding=True, shared_z=16, g_z_dense_concat=True,
                                        g_other_level_dense_layer=True)),
                         device="cpu", store=S.VariableStore("cpu", seed=3))
        return g.build_model()
    a = make()
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for arena in a.store.arenas.values():
            for buf in (arena.params, arena.m, arena.v) + ((arena.ema,) if arena.ema is not None else ()):
                buf.copy_(torch.randn(buf.shape, generator=gen))
    a.counter, a.d_arena.step, a.g_arena.step = 5, 5, 4
    path = a.save(str(tmp_path), 5)
    from safetensors import safe_open
    with safe_open(path, "pt") as f:
        keys = set(f.keys())
    for k in ("generator/cls_embed/dense1/kernel", "generator/shared_z/dense1/kernel", "generator/z2/dense1/kernel",
              "generator/first/dense/kernel"):
        assert {k, k + "/Adam", k + "/Adam_1", k + "/ExponentialMovingAverage"} <= keys, k
    assert "generator/cls_embed/dense1/u" in keys and "generator/cls_embed/prelu/alpha" in keys
    b = make()
    ok, counter = b.load(str(tmp_path))
    assert ok and counter == 5
    sa, sb = a.state_tensors(), b.state_tensors()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_gate_still_rejects_the_other_generator_heads():
    for extra in (["--g_final_layer", "true"], ["--g_final_layer", "true", "--shared_z", "16"],
                  ["--cls_embedding", "true"]):                 # (no labels: no embedding to learn)
        argv = ["--gan_type", "hinge", "--img_size", "64"] + extra
        with pytest.raises(NotImplementedError):
            model.BigGAN(M.parse_args(argv, make_dirs=False), device="cpu", store=S.VariableStore("cpu"))
    for extra in (["--shared_z", "16"], ["--g_z_dense_concat", "true"], ["--n_labels", "4", "--cls_embedding", "true"]):
        argv = ["--gan_type", "hinge", "--img_size", "64"] + extra
        model.BigGAN(M.parse_args(argv, make_dirs=False), device="cpu", store=S.VariableStore("cpu"))


def test_restatement_follows_the_oracle_without_the_flags(monkeypatch):
    """The restatement hands default configurations to the oracle's own generator, and is what Trainer then calls."""
    from oracle import ref_model as RM
    LR.install(monkeypatch)
    assert RM.generator is LR.generator
    tr = LR.trainer(img_size=64, ch=8, z_dim=64, batch_size=2, n_labels=4, cls_embedding=True)
    assert "generator/cls_embed/dense1/kernel" in tr.vs.vars
    assert os.path.basename(LR.__file__) == "latent_ref.py"
