"""Generator latent stage on the GPU (--cls_embedding / --shared_z / --g_z_dense_concat, BigGAN.py:278-444): the grouped
projections' input gradient and the latent fan-out / fan-in kernels against float64, whole-step parity against the
float64 restatement (tests/latent_ref.py installed over the oracle's generator), EMA sampling, graph replay and bf16."""
import numpy as np
import pytest
import torch

from oracle import ref_model as RM
from tests import latent_ref as LR
from tests.common import hip_model_like, dev_draws, rel_err, t2n
from tests.test_gpu_step import _run_parity, cu

pytestmark = pytest.mark.gpu


def _hip():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip
    return Fn, hip


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,K,Ns,acc", [(13, 37, (96, 96, 200, 1), False), (8, 76, (256, 256), True),
                                        (3, 1, (1,), False), (130, 65, (300, 17, 64), True)])
def test_dense_group_input_gradient(B, K, Ns, acc):
    """dx (+)= sum_i dy_i w_i^T: ragged K and N, N = 1, batches that are not a multiple of the 8-row strip; bit-identical
    when repeated."""
    Fn, hip = _hip()
    rng = np.random.default_rng(B * 7 + K)
    ws = [rng.standard_normal((K, n)) for n in Ns]
    dys = [rng.standard_normal((B, n)) for n in Ns]
    base = rng.standard_normal((B, K + 5))                      # output rows K + 5 apart (a column view)
    ref = sum(dy @ w.T for dy, w in zip(dys, ws)) + (base[:, :K] if acc else 0.0)
    wt = [torch.tensor(w, dtype=torch.float32, device="cuda") for w in ws]
    gt = [torch.tensor(g, dtype=torch.float32, device="cuda") for g in dys]
    outs = []
    for _ in range(2):
        buf = torch.tensor(base, dtype=torch.float32, device="cuda")
        items = (hip.BgDenseItem * len(Ns))()
        for it, w, g in zip(items, wt, gt):
            it.w, it.y, it.K, it.N = w.data_ptr(), g.data_ptr(), K, w.shape[1]
        hip.check(hip.lib().bg_dense_group_dgrad(items, len(Ns), B, buf.data_ptr(), K + 5, int(acc), hip.stream()))
        torch.cuda.synchronize()
        outs.append(t2n(buf))
        assert np.array_equal(outs[-1][:, K:], base[:, K:].astype(np.float32))     # columns past K untouched
    assert np.array_equal(outs[0], outs[1])
    assert rel_err(outs[0][:, :K], ref) < 1e-5


def test_latent_fanout_and_fanin():
    """Fan-out writes [z_i | e | s] rows into one packed buffer; fan-in sums each source's gradient over every level that
    reads it (accumulate and overwrite targets), in float64 agreement and bit-identical when repeated."""
    Fn, hip = _hip()
    rng = np.random.default_rng(3)
    B = 13
    z = torch.tensor(rng.standard_normal((B, 40)), dtype=torch.float32, device="cuda")
    e = torch.tensor(rng.standard_normal((B, 9)), dtype=torch.float32, device="cuda", requires_grad=True)
    s = torch.tensor(rng.standard_normal((B, 1)), dtype=torch.float32, device="cuda", requires_grad=True)
    widths = [10 + 9 + 1, 30 + 9 + 1, 9]
    segs = [(0, 0, 0, 0, 10), (1, 0, 0, 10, 9), (2, 0, 0, 19, 1),
            (0, 10, 1, 0, 30), (1, 0, 1, 30, 9), (2, 0, 1, 39, 1),
            (1, 0, 2, 0, 9)]
    outs = Fn.LatentFanoutFn.apply(widths, segs, z, e, s)
    zn, en, sn = t2n(z), t2n(e), t2n(s)
    assert np.array_equal(t2n(outs[0]), np.concatenate([zn[:, :10], en, sn], 1))
    assert np.array_equal(t2n(outs[1]), np.concatenate([zn[:, 10:40], en, sn], 1))
    assert np.array_equal(t2n(outs[2]), en)
    assert outs[0].stride(0) == sum(widths)                     # column views of one packed buffer
    gs = [torch.tensor(rng.standard_normal((B, w)), dtype=torch.float32, device="cuda") for w in widths]
    got = []
    for _ in range(2):
        e.grad = s.grad = None
        outs = Fn.LatentFanoutFn.apply(widths, segs, z, e, s)
        torch.autograd.backward(outs, gs)
        got.append((t2n(e.grad), t2n(s.grad)))
    g = [t2n(t).astype(np.float64) for t in gs]
    assert rel_err(got[0][0], g[0][:, 10:19] + g[1][:, 30:39] + g[2]) < 1e-6
    assert rel_err(got[0][1], g[0][:, 19:20] + g[1][:, 39:40]) < 1e-6
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    # raw fan-in with an accumulating target and a column that no segment covers
    base = rng.standard_normal((B, 12)).astype(np.float32)
    acc = torch.tensor(base, device="cuda")
    over = torch.full((B, 4), 7.0, device="cuda")
    tg = (hip.BgLatentTarget * 2)()
    tg[0].dst, tg[0].ldd, tg[0].width, tg[0].accumulate = acc.data_ptr(), 12, 12, 1
    tg[1].dst, tg[1].ldd, tg[1].width, tg[1].accumulate = over.data_ptr(), 4, 3, 0
    sg = (hip.BgLatentSeg * 3)()
    for d, (src, sc, dc, w, t) in zip(sg, [(gs[1], 0, 0, 12, 0), (gs[0], 5, 2, 3, 0), (gs[2], 0, 0, 2, 1)]):
        d.src, d.lds, d.src_col, d.dst_col, d.width, d.target = src.data_ptr(), src.shape[1], sc, dc, w, t
    hip.check(hip.lib().bg_latent_fanin(tg, 2, sg, 3, B, hip.stream()))
    want = base.astype(np.float64) + g[1][:, :12]
    want[:, 2:5] += g[0][:, 5:8]
    assert rel_err(t2n(acc), want) < 1e-6
    o = t2n(over)
    assert rel_err(o[:, :2], g[2][:, :2]) < 1e-6 and np.all(o[:, 2] == 0) and np.all(o[:, 3] == 7)
    # fan-out refuses a gap or an overlap
    tg[0].accumulate = 0
    sg2 = (hip.BgLatentSeg * 1)()
    sg2[0].src, sg2[0].lds, sg2[0].width = z.data_ptr(), 40, 11
    assert hip.lib().bg_latent_fanout(tg, 1, sg2, 1, B, hip.stream()) == 1


# ---------------------------------------------------------------- whole step
def _multi_hot(batch, rng):
    for k in ("labels", "cls_z_d", "cls_z_g"):
        m = (rng.random(batch[k].shape) < 0.3).astype(np.float32)
        m[np.arange(m.shape[0]), rng.integers(0, m.shape[1], m.shape[0])] = 1
        batch[k] = m


STEP_CASES = [
    dict(n_labels=10, cls_embedding=True),
    dict(n_labels=10, cls_embedding=True, cls_embedding_concat=True, shared_z=16),
    dict(n_labels=6, shared_z=16, g_z_dense_concat=True),
    dict(g_z_dense_concat=True, g_other_level_dense_layer=True),
]


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_step_parity_latent_stage(monkeypatch, case):
    flags = STEP_CASES[case]
    LR.install(monkeypatch)
    tr = LR.trainer(img_size=64, ch=8, z_dim=64, batch_size=4, **flags)
    gan = hip_model_like(tr, **flags)
    assert set(gan.store.vars) == set(tr.vs.vars)
    batch = RM.synthetic_batch(tr.cfg, 11 + case, 4)
    if case == 2:
        _multi_hot(batch, np.random.default_rng(5))
    _run_parity(tr, gan, batch)


def test_sample_with_ema_weights_and_embedding(monkeypatch):
    """sample(): generator(test_z, zero_cls_z) on the EMA shadows - the zero labels still give act(bias) as embedding."""
    flags = dict(n_labels=10, cls_embedding=True, shared_z=16)
    LR.install(monkeypatch)
    tr = LR.trainer(img_size=64, ch=8, z_dim=64, batch_size=2, **flags)
    gan = hip_model_like(tr, **flags)
    batch = RM.synthetic_batch(tr.cfg, 41, 2)
    tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"], labels=batch["labels"],
              cls_z=batch["cls_z_d"])
    tr.g_step(batch["z_g"], batch["aug_fake_g"], cls_z=batch["cls_z_g"])
    gan.d_step(cu(batch["real"]), cu(batch["z_d"]), dev_draws(batch["aug_real"]), dev_draws(batch["aug_fake_d"]),
               labels=cu(batch["labels"]), cls_z=cu(batch["cls_z_d"]))
    gan.g_step(2, cu(batch["z_g"]), dev_draws(batch["aug_fake_g"]), cls_z=cu(batch["cls_z_g"]))
    k = "generator/cls_embed/dense1/bias"
    assert not np.array_equal(t2n(gan.g_arena.view(gan.g_arena.ema, k)), t2n(gan.store.vars[k]))
    z = RM.truncated_normal(np.random.default_rng(5), (2, 1, 1, tr.cfg.z_dim))
    ref = tr.sample(z)
    img = gan.sample(cu(z))
    assert rel_err(t2n(img), ref.numpy()) < 1e-4


def test_hip_graph_replay_matches_eager_with_shared_z():
    """capture_graphs() with --shared_z --g_z_dense_concat --g_other_level_dense_layer (fan-out, fan-in and the grouped
    input gradient inside the captured G op): replayed iterations follow the eager ones."""
    from tests.common import make_args
    from biggan_tensorflow_amd import model, scope as S
    gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, shared_z=16, g_z_dense_concat=True,
                                 g_other_level_dense_layer=True), store=S.VariableStore("cuda", seed=5)).build_model()
    data = [gan.synthetic_batch(4) for _ in range(2)]
    snap = gan.state_tensors()
    saved = {k: v.detach().clone() for k, v in snap.items()}
    rng = gan.gen.get_state()
    eager = []
    for real in data:
        l = gan.train_step(real)
        eager.append((l["d_loss"].item(), l["g_loss"].item()))
    with torch.no_grad():
        for k, v in snap.items():
            v.copy_(saved[k])
    gan.counter, gan.d_arena.step, gan.g_arena.step = 0, 0, 0
    gan.capture_graphs()
    assert gan._graphs_ready
    gan.gen.set_state(rng)
    for real, (de, ge) in zip(data, eager):
        l = gan.train_step(real)
        assert abs(l["d_loss"].item() - de) <= 1e-5 * abs(de) and abs(l["g_loss"].item() - ge) <= 1e-5 * abs(ge)


def test_bf16_step_config3_topology_with_embedding():
    """BASELINE config 3's generator topology (128^2, ch 96, bf16-resident) at batch 4 with --n_labels 1000
    --cls_embedding: the bf16 step against the same model in fp32 within the bf16 gate of tests/test_gpu_bf16.py (losses
    and images 2e-2 relative; latent-stage gradients 4e-1 relative L2)."""
    from tests.common import make_args
    from biggan_tensorflow_amd import model, scope as S, functional as Fn
    kw = dict(img_size=128, ch=96, batch_size=4, n_labels=1000, cls_embedding=True)
    try:
        g32 = model.BigGAN(make_args(**kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16 = model.BigGAN(make_args(precision="bf16", **kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16.store.load_arrays(g32.store.export_arrays())
        torch.manual_seed(0)
        z = torch.randn(4, 1, 1, g32.z_dim, device="cuda").clamp_(-2, 2)
        lab = torch.nn.functional.one_hot(torch.tensor([3, 999, 0, 512], device="cuda"), 1000).float()
        outs = []
        for g in (g32, g16):
            o = g.g_step(4, z, None, apply=False, cls_z=lab)
            grads = {k: t2n(g.store.vars[k].bg_grad).copy() for k in ("generator/cls_embed/dense1/kernel",
                                                                      "generator/z0/dense1/kernel",
                                                                      "generator/first/dense/kernel")}
            outs.append((o["g_loss"].item(), t2n(o["fake"]) if "fake" in o else None, grads))
            torch.cuda.synchronize()
        (l32, f32_, g32s), (l16, f16_, g16s) = outs
        assert abs(l16 - l32) <= 2e-2 * max(abs(l32), 1e-6), (l16, l32)
        if f32_ is not None:
            assert rel_err(f16_, f32_) < 2e-2
        for k in g32s:
            assert np.isfinite(g16s[k]).all() and rel_err(g16s[k], g32s[k]) < 4e-1, (k, rel_err(g16s[k], g32s[k]))
    finally:
        Fn.set_precision("fp32")
