"""Mixed-kernel generator blocks (--g_mixed_resblocks, ops.py:29-59 / 403-442, BigGAN.py:485-489): the ops boundary,
the variable manifest against the float64 restatement in tests/mixed_ref.py, checkpoints and the flag gate.  No GPU."""
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import main as M, model, ops, scope as S
from oracle import ref_ops as R
from tests import mixed_ref as MR

CASES = [
    (64, dict()),
    (128, dict(g_mixed_resblock_ch_div=1.0)),
    (128, dict(bn_type="batch_renorm", conv_padding="zero")),
    (256, dict(deep=True, n_labels=4)),
    (512, dict(shared_z=32)),
    (64, dict(n_labels=6, cls_embedding=True, g_no_last_resblock=True, g_conv="conv3", activation="relu")),
    (128, dict(g_other_level_dense_layer=True, n_labels=3)),
]


def _argv(size, kw):
    argv = ["--gan_type", "hinge", "--img_size", str(size), "--ch", "8", "--g_mixed_resblocks", "true"]
    for k, v in kw.items():
        argv += ["--" + k, str(v)]
    return M.parse_args(argv, make_dirs=False)


def _hip_manifest(size, kw):
    store = S.VariableStore("cpu")
    gan = model.BigGAN(_argv(size, kw), device="cpu", store=store)
    img = gan.generator(torch.empty(2, 1, 1, gan.z_dim, device="meta"))
    assert tuple(img.shape) == (2, size, size, 3)
    return [(k, tuple(v.shape)) for k, v in store.vars.items()], store


def _ref_manifest(size, kw):
    cfg = MR.config(img_size=size, ch=8, batch_size=2, g_mixed_resblocks=True, **kw)
    vs = R.VarStore(torch.float64, 0)
    z = torch.zeros(2, 1, 1, cfg.z_dim, dtype=torch.float64)
    cz = torch.zeros(2, cfg.n_labels, dtype=torch.float64) if cfg.n_labels else None
    with torch.no_grad():
        img = MR.generator(vs, cfg, z, cz, True)
    assert tuple(img.shape) == (2, size, size, 3)
    return [(k, tuple(v.shape)) for k, v in vs.vars.items()], vs


def _mixed(manifest):
    return [(k, s) for k, s in manifest if "/res_mixed" in k]


@pytest.mark.parametrize("size", [64, 128, 256, 512])
def test_flag_builds_one_block_per_level(size):
    mine, _ = _hip_manifest(size, {})
    levels = {k.split("/")[1] for k, _ in _mixed(mine)}
    n = len(model.BigGAN(_argv(size, {}), device="cpu", store=S.VariableStore("cpu")).g_block_info()["counts"])
    assert levels == {"res_mixed%d" % (2 ** i) for i in range(n)}


@pytest.mark.parametrize("size,kw", CASES)
def test_manifest_matches_restatement(size, kw):
    mine, store = _hip_manifest(size, kw)
    ref, vs = _ref_manifest(size, kw)
    assert dict(mine) == dict(ref)
    assert {k for k, _ in mine if store.trainable[k]} == {k for k, _ in ref if vs.trainable[k]}
    # creation order of the new variables: deconv4, deconv3, deconv2, conv3, conv5, dilconv5, the norm, prelu, proj
    assert _mixed(mine) == _mixed(ref)


def test_worked_example_of_one_block():
    """--img_size 64 --ch 8: the 4 levels have ch 64, 32, 16, 8 (inner = round_up(ch / 2, 8))."""
    m = dict(_hip_manifest(64, {})[0])
    p = "generator/res_mixed8/clown/"
    assert m[p + "deconv4/kernel"] == (4, 4, 8, 64)            # inner 32: split 4, rest 4
    assert m[p + "deconv3/kernel"] == (3, 3, 8, 64)
    assert m[p + "deconv2/kernel"] == (2, 2, 4, 64)
    assert m[p + "conv3/kernel"] == (3, 3, 64, 4)
    assert m[p + "conv5/kernel"] == (5, 5, 64, 4)
    assert m[p + "dilconv5/kernel"] == (5, 5, 64, 4)
    assert m[p + "batch_norm/gamma"] == (32,) and m[p + "prelu/alpha"] == (32,)
    assert m["generator/res_mixed8/proj/kernel"] == (1, 1, 32, 64)
    assert "generator/res_mixed8/proj/bias" not in m
    assert m["generator/res_mixed1/clown/deconv4/kernel"] == (4, 4, 2, 8)   # ch 8: inner 8, split 1, rest 1 -> 2


@pytest.mark.parametrize("channels", [8, 48, 768, 61])
@pytest.mark.parametrize("no_deconv2", [False, True])
def test_clown_channel_split(channels, no_deconv2):
    S.set_default_store(S.VariableStore("cpu"))
    opt = {"conv": {"sn": True}, "bn": {"type": "bn"}, "is_training": True, "act": ops.relu,
           "mixed_conv_no_deconv2": no_deconv2}
    with S.variable_scope("generator"):
        y = ops.clown_conv(torch.empty(2, 8, 8, 16, device="meta"), channels, opt)
    assert tuple(y.shape) == (2, 8, 8, channels)
    v = S.default_store().vars
    names = ["deconv4", "deconv3"] + ([] if no_deconv2 else ["deconv2"]) + ["conv3", "conv5", "dilconv5"]
    widths = [v["generator/clown/%s/kernel" % n].shape[2 if n.startswith("deconv") else 3] for n in names]
    want = MR.clown_split(channels, no_deconv2)
    if no_deconv2:
        want = want[:2] + want[3:]
    assert widths == want and sum(widths) == channels
    split = channels // 8
    assert widths[0] == split + channels - 7 * split + (split // 2 if no_deconv2 else 0)
    # the variables follow the reference's creation order; the clown's activation is PReLU although opt['act'] is relu
    kernels = [k for k in v if k.endswith("/kernel")]
    assert kernels == ["generator/clown/%s/kernel" % n for n in names]
    assert list(v)[-1] == "generator/clown/prelu/alpha"


def test_kernel_size_strings_round_trip():
    s = "32x3,32x5,16x7"
    d = ops.decode_kernel_sizes(s)
    assert d == {"slices": [{"size": 32, "kernel": 3}, {"size": 32, "kernel": 5}, {"size": 16, "kernel": 7}],
                 "total_channels": 80}
    assert ops.encode_kernel_sizes(d["slices"]) == s
    assert ops.encode_kernel_sizes(d["slices"], 0.5) == "16x3,16x5,8x7"
    # int(float(size) * ch_mul + 1e-8): 3 * (1/3) is 0.999... in floating point, still 1
    assert ops.encode_kernel_sizes([{"size": 3, "kernel": 3}], 1.0 / 3.0) == "1x3"
    assert ops.encode_kernel_sizes([{"size": 10, "kernel": 1}], 0.25) == "2x1"


def test_string_kernels_and_dilation_shapes_and_variables():
    S.set_default_store(S.VariableStore("cpu"))
    opt = {"conv": {"sn": True, "padding_type": "reflect"}}
    x = torch.empty(2, 16, 16, 24, device="meta")
    with S.variable_scope("discriminator"):
        y = ops.conv(x, 0, opt, kernel="8x3,16x5", stride=1, scope="mix")
        z = ops.conv(x, 12, opt, kernel=5, stride=1, pad=4, dilation=2, scope="dil")
    assert tuple(y.shape) == (2, 16, 16, 24) and tuple(z.shape) == (2, 16, 16, 12)
    v = S.default_store().vars
    assert tuple(v["discriminator/mix/conv3_slice/kernel"].shape) == (3, 3, 24, 8)
    assert tuple(v["discriminator/mix/conv5_slice/kernel"].shape) == (5, 5, 24, 16)
    assert "discriminator/mix/conv5_slice/u" in v and "discriminator/mix/conv5_slice/bias" in v
    assert tuple(v["discriminator/dil/kernel"].shape) == (5, 5, 24, 12)
    with S.variable_scope("discriminator"):
        with pytest.raises(ValueError):              # TF: dilation together with stride > 1
            ops.conv(x, 12, opt, kernel=3, stride=2, pad=1, dilation=2, scope="bad")
        with pytest.raises(ValueError):              # reflect padding 4 on a 4x4 map (TF: must be < 4)
            ops.conv(torch.empty(2, 4, 4, 24, device="meta"), 12, opt, kernel=5, stride=1, pad=4, dilation=2,
                     scope="bad2")
        zero = {"conv": {"sn": True, "padding_type": "zero"}}
        y = ops.conv(torch.empty(2, 4, 4, 24, device="meta"), 12, zero, kernel=5, stride=1, pad=4, dilation=2,
                     scope="ok")
        assert tuple(y.shape) == (2, 4, 4, 12)


def test_checkpoint_roundtrip_with_mixed_blocks(tmp_path):
    def make():
        g = model.BigGAN(_argv(64, dict(n_labels=4)), device="cpu", store=S.VariableStore("cpu", seed=3))
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
    for k in ("generator/res_mixed4/clown/deconv2/kernel", "generator/res_mixed1/clown/dilconv5/kernel",
              "generator/res_mixed2/proj/kernel", "generator/res_mixed8/clown/conv3/bias"):
        assert {k, k + "/Adam", k + "/Adam_1", k + "/ExponentialMovingAverage"} <= keys, k
    for k in ("generator/res_mixed4/clown/batch_norm/moving_mean", "generator/res_mixed4/clown/deconv4/u",
              "generator/res_mixed4/clown/prelu/alpha"):
        assert k in keys, k
    b = make()
    ok, counter = b.load(str(tmp_path))
    assert ok and counter == 5
    sa, sb = a.state_tensors(), b.state_tensors()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_regulariser_covers_the_new_kernels():
    """The deconv branch kernels are regularised whatever their scope (ops.py:127); conv kernels under 'generator'."""
    ops.begin_run()                     # (forget the regularisers earlier tests' shape passes registered)
    gan = model.BigGAN(_argv(64, {}), device="cpu", store=S.VariableStore("cpu")).build_model()
    regs = set(gan.store.reg_shapes)
    for n in ("deconv4", "deconv3", "deconv2", "conv3", "conv5", "dilconv5"):
        assert "generator/res_mixed2/clown/%s/kernel" % n in regs, n
    assert "generator/res_mixed2/proj/kernel" in regs


def test_gate_still_rejects_the_final_layer():
    for extra in (["--g_final_layer", "true"], ["--g_final_layer", "true", "--g_mixed_resblocks", "true"],
                  ["--g_final_layer", "true", "--g_final_mixed_conv", "true"], ["--multi_head", "true"]):
        argv = ["--gan_type", "hinge", "--img_size", "64"] + extra
        with pytest.raises(NotImplementedError):
            model.BigGAN(M.parse_args(argv, make_dirs=False), device="cpu", store=S.VariableStore("cpu"))


def test_restatement_is_what_the_trainer_calls(monkeypatch):
    from oracle import ref_model as RM
    MR.install(monkeypatch)
    assert RM.generator is MR.generator
    tr = MR.trainer(img_size=64, ch=8, z_dim=64, batch_size=2, g_mixed_resblocks=True)
    assert "generator/res_mixed1/clown/dilconv5/kernel" in tr.vs.vars
