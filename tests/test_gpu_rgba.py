"""RGBA and grayscale training on the GPU (--c_dim 4 / 1, BigGAN.py:572-580 and 616-619): the alpha kernels
(bg_alpha_*) against float64, whole-step parity against the float64 restatement (tests/rgba_ref.py installed over the
oracle), EMA sampling, graph replay, bf16 and data parallelism."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_model as RM
from tests import rgba_ref as AR
from tests.common import hip_model_like, dev_draws, rel_err, t2n
from tests.test_gpu_step import _run_parity, cu

pytestmark = pytest.mark.gpu

HELPER = "generator/alphahelper_w"


def _hip():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip
    return Fn, hip


def _rgba(rng, rows, scale=1.0):
    return rng.standard_normal((rows, 4)) * scale


# ---------------------------------------------------------------- kernels
ROWS = [1, 1000, 600_001]           # not multiples of the 256-thread block; the last one spans the grid-stride loop


def _head_ref(x, w):
    return torch.tanh(AR.alpha_helper(x, w))


@pytest.mark.parametrize("rows", ROWS)
def test_alpha_head_against_float64(rows):
    Fn, hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(rows)
    x = _rgba(rng, rows, 0.3)
    dy = _rgba(rng, rows)
    w = 1.7
    xd, dyd = cu(x), cu(dy)
    wd = torch.tensor(w, dtype=torch.float32, device="cuda")
    y = torch.empty_like(xd)
    assert L.bg_alpha_head_fwd(hip.f32(xd), hip.f32(wd), hip.f32(y), rows, hip.stream()) == 0
    dx = torch.empty_like(xd)
    dw = torch.full((), 0.25, dtype=torch.float32, device="cuda")
    assert L.bg_alpha_head_bwd(hip.f32(xd), hip.f32(wd), hip.f32(dyd), hip.f32(dx), hip.f32(dw), rows, hip.stream()) == 0
    torch.cuda.synchronize()
    x64 = torch.tensor(xd.cpu().numpy(), dtype=torch.float64).requires_grad_(True)
    w64 = torch.tensor(float(wd.cpu()), dtype=torch.float64, requires_grad=True)
    y64 = _head_ref(x64, w64)
    gx, gw = torch.autograd.grad(y64, (x64, w64), torch.tensor(dyd.cpu().numpy(), dtype=torch.float64))
    assert np.abs(t2n(y) - y64.detach().numpy()).max() < 2e-6
    assert np.abs(t2n(dx) - gx.numpy()).max() < 1e-5 * (1 + w)
    assert abs(float(dw.cpu()) - (0.25 + float(gw))) <= 1e-5 * (1.0 + abs(float(gw)))
    # reruns are bit-identical (the dw sum: per-block fp64 partials, added in a fixed order)
    y2, dx2 = torch.empty_like(xd), torch.empty_like(xd)
    dw2 = torch.full((), 0.25, dtype=torch.float32, device="cuda")
    assert L.bg_alpha_head_fwd(hip.f32(xd), hip.f32(wd), hip.f32(y2), rows, hip.stream()) == 0
    assert L.bg_alpha_head_bwd(hip.f32(xd), hip.f32(wd), hip.f32(dyd), hip.f32(dx2), hip.f32(dw2), rows,
                               hip.stream()) == 0
    dx3 = torch.empty_like(xd)
    assert L.bg_alpha_head_bwd(hip.f32(xd), hip.f32(wd), hip.f32(dyd), hip.f32(dx3), None, rows, hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(dx, dx3)


@pytest.mark.parametrize("rows", ROWS)
def test_alpha_mask_and_tangent_against_float64(rows):
    Fn, hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(100 + rows)
    x = np.clip(_rgba(rng, rows, 0.6), -1, 1)
    dy, xdot = _rgba(rng, rows), _rgba(rng, rows)
    xd, dyd, td = cu(x), cu(dy), cu(xdot)
    outs = []
    for _ in range(2):
        y, dx, yt = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
        assert L.bg_alpha_mask_fwd(hip.f32(xd), hip.f32(y), rows, hip.stream()) == 0
        assert L.bg_alpha_mask_bwd(hip.f32(xd), hip.f32(dyd), hip.f32(dx), rows, hip.stream()) == 0
        assert L.bg_alpha_mask_tangent(hip.f32(xd), hip.f32(td), hip.f32(yt), rows, hip.stream()) == 0
        outs.append((y, dx, yt))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    y, dx, yt = outs[0]
    x64 = torch.tensor(xd.cpu().numpy(), dtype=torch.float64).requires_grad_(True)
    y64 = AR.alpha_mask(x64)
    g64, = torch.autograd.grad(y64, x64, torch.tensor(dyd.cpu().numpy(), dtype=torch.float64))
    t64 = torch.autograd.functional.jvp(AR.alpha_mask, x64.detach(),
                                        torch.tensor(td.cpu().numpy(), dtype=torch.float64))[1]
    assert np.abs(t2n(y) - y64.detach().numpy()).max() < 1e-6
    assert np.abs(t2n(dx) - g64.numpy()).max() < 1e-5
    assert np.abs(t2n(yt) - t64.numpy()).max() < 1e-5


def test_alpha_abi_rejects_bad_arguments():
    Fn, hip = _hip()
    L = hip.lib()
    x = torch.zeros(9, 4, device="cuda")
    y = torch.zeros(9, 4, device="cuda")
    w = torch.zeros((), device="cuda")
    s = hip.stream()
    p = hip.f32
    off = hip.c_void_p(x.data_ptr() + 4)              # not 16-byte aligned
    assert L.bg_alpha_head_fwd(p(x), p(w), p(y), 0, s) == 1
    assert L.bg_alpha_head_fwd(p(x), None, p(y), 8, s) == 1
    assert L.bg_alpha_head_fwd(off, p(w), p(y), 8, s) == 1
    assert L.bg_alpha_head_bwd(p(x), p(w), p(x), None, p(w), 8, s) == 1
    assert L.bg_alpha_head_bwd(p(x), p(w), off, p(y), p(w), 8, s) == 1
    assert L.bg_alpha_mask_fwd(p(x), p(y), -1, s) == 1
    assert L.bg_alpha_mask_bwd(p(x), off, p(y), 8, s) == 1
    assert L.bg_alpha_mask_tangent(p(x), p(x), off, 8, s) == 1
    assert L.bg_alpha_mask_fwd(p(x), p(y), 9, s) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- whole step
STEP_CASES = [
    (4, dict()),
    (4, dict(gan_type="ra-dragan")),
    (4, dict(alpha_mask=False)),
    (4, dict(g_alpha_helper=False)),
    (1, dict()),
    (4, dict(n_labels=4)),
]


def _hip_flags(c_dim, flags):
    out = dict(c_dim=c_dim)
    for k, v in flags.items():
        out[k] = ("true" if v else "false") if isinstance(v, bool) else v
    return out


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_step_parity_rgba(monkeypatch, case):
    c_dim, flags = STEP_CASES[case]
    AR.install(monkeypatch)
    tr = AR.trainer(img_size=64, ch=8, z_dim=64, batch_size=4, c_dim=c_dim, **flags)
    gan = hip_model_like(tr, **_hip_flags(c_dim, flags))
    assert set(gan.store.vars) == set(tr.vs.vars)
    assert (HELPER in gan.store.vars) == (c_dim == 4 and flags.get("g_alpha_helper", True))
    batch = RM.synthetic_batch(tr.cfg, 31 + case, 4)
    assert batch["real"].shape[-1] == c_dim
    _run_parity(tr, gan, batch)


def test_sample_with_ema_helper(monkeypatch):
    """sample() reads the EMA shadow of generator/alphahelper_w like every other generator variable."""
    AR.install(monkeypatch)
    tr = AR.trainer(img_size=64, ch=8, z_dim=64, batch_size=2, c_dim=4)
    gan = hip_model_like(tr, c_dim=4)
    batch = RM.synthetic_batch(tr.cfg, 43, 2)
    tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"])
    tr.g_step(batch["z_g"], batch["aug_fake_g"])
    gan.d_step(cu(batch["real"]), cu(batch["z_d"]), dev_draws(batch["aug_real"]), dev_draws(batch["aug_fake_d"]))
    gan.g_step(2, cu(batch["z_g"]), dev_draws(batch["aug_fake_g"]))
    live = float(gan.store.vars[HELPER].detach().cpu())
    ema = float(gan.g_arena.view(gan.g_arena.ema, HELPER).cpu())
    assert live != ema
    assert abs(ema - float(tr.ema[HELPER])) <= 1e-6 * abs(ema)
    z = RM.truncated_normal(np.random.default_rng(6), (2, 1, 1, tr.cfg.z_dim))
    ref = tr.sample(z)
    img = gan.sample(cu(z))
    assert img.shape[-1] == 4
    assert rel_err(t2n(img), ref.numpy()) < 1e-4
    # the live weight is back after sampling
    assert float(gan.store.vars[HELPER].detach().cpu()) == live


def test_hip_graph_replay_matches_eager():
    from tests.common import make_args
    from biggan_tensorflow_amd import model, scope as S
    gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, c_dim=4),
                       store=S.VariableStore("cuda", seed=5)).build_model()
    data = [gan.synthetic_batch(4) for _ in range(2)]
    snap = gan.state_tensors()
    saved = {k: v.detach().clone() for k, v in snap.items()}
    rng = gan.gen.get_state()
    eager = []
    for real in data:
        l = gan.train_step(real)
        eager.append((l["d_loss"].item(), l["g_loss"].item(), float(gan.store.vars[HELPER].detach().cpu())))
    with torch.no_grad():
        for k, v in snap.items():
            v.copy_(saved[k])
    gan.counter, gan.d_arena.step, gan.g_arena.step = 0, 0, 0
    gan.capture_graphs()
    assert gan._graphs_ready
    gan.gen.set_state(rng)
    for real, (de, ge, we) in zip(data, eager):
        l = gan.train_step(real)
        assert abs(l["d_loss"].item() - de) <= 1e-5 * abs(de) and abs(l["g_loss"].item() - ge) <= 1e-5 * abs(ge)
        assert abs(float(gan.store.vars[HELPER].detach().cpu()) - we) <= 1e-6 * abs(we)
    assert float(gan.store.vars[HELPER].detach().cpu()) != 5.0


def test_bf16_step_config3_topology():
    """BASELINE config 3's topology (128^2, ch 96, bf16-resident) at batch 4 with --c_dim 4: the bf16 G+D step against
    the same model in fp32 within the bf16 gate of tests/test_gpu_bf16.py (losses and images 2e-2 relative; gradients
    4e-1 relative L2)."""
    from tests.common import make_args
    from biggan_tensorflow_amd import model, scope as S, functional as Fn
    kw = dict(img_size=128, ch=96, batch_size=4, c_dim=4)
    try:
        g32 = model.BigGAN(make_args(**kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16 = model.BigGAN(make_args(precision="bf16", **kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16.store.load_arrays(g32.store.export_arrays())
        torch.manual_seed(0)
        z = torch.randn(4, 1, 1, g32.z_dim, device="cuda").clamp_(-2, 2)
        real = (torch.rand(4, 128, 128, 4, device="cuda") * 2 - 1)
        d_names = ("discriminator/resblock_down_1/res1/conv_0/kernel", "discriminator/resblock_down_1/res1/prelu/alpha")
        g_names = (HELPER, "generator/G_logit/kernel", "generator/prelu/alpha")
        outs = []
        for g in (g32, g16):
            torch.manual_seed(1)
            od = g.d_step(real, z, None, None, apply=False)
            dg = {k: t2n(g.store.vars[k].bg_grad).copy() for k in d_names}
            dl = od["d_loss"].item()
            torch.manual_seed(2)
            o = g.g_step(4, z, None, apply=False)
            gg = {k: t2n(g.store.vars[k].bg_grad).copy() for k in g_names}
            outs.append((dl, o["g_loss"].item(), t2n(o["fake"]) if "fake" in o else None, dict(dg, **gg)))
            torch.cuda.synchronize()
        (d32, l32, f32_, g32s), (d16, l16, f16_, g16s) = outs
        assert abs(d16 - d32) <= 2e-2 * max(abs(d32), 1e-6), (d16, d32)
        assert abs(l16 - l32) <= 2e-2 * max(abs(l32), 1e-6), (l16, l32)
        if f32_ is not None:
            assert f32_.shape[-1] == 4 and rel_err(f16_, f32_) < 2e-2
        for k in g32s:
            assert np.isfinite(g16s[k]).all() and rel_err(g16s[k], g32s[k]) < 4e-1, (k, rel_err(g16s[k], g32s[k]))
    finally:
        Fn.set_precision("fp32")


# ---------------------------------------------------------------- data parallel
IMG, CH, ZD, B = 64, 8, 64, 4


def _dp_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch.distributed as dist
    from _pytest.monkeypatch import MonkeyPatch
    from biggan_tensorflow_amd import parallel
    from tests import rgba_ref as AR_
    from tests.test_gpu_mixed import _steps as steps
    torch.cuda.set_device(0)
    parallel.init_from_env(backend="gloo")
    mp_ = MonkeyPatch()
    AR_.install(mp_)
    tr = AR_.trainer(img_size=IMG, ch=CH, z_dim=ZD, batch_size=B, c_dim=4)
    gan = hip_model_like(tr, c_dim=4)
    assert gan.world == world and gan.rank == rank
    batch = RM.synthetic_batch(tr.cfg, 5, B)
    lo, hi = parallel.shard_batch(B, rank, world)
    out = steps(gan, batch, lo, hi)
    out["helper_grad"] = float(gan.store.vars[HELPER].bg_grad.cpu())
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()
    mp_.undo()


def test_two_rank_data_parallel_matches_single_process(monkeypatch):
    """Two ranks (gloo, both on one card) with half the batch each reproduce the single process: the helper's
    gradient is summed over the batch, so it meets the other rank's half in the SUM all-reduce."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dp import _free_port, _rel
    from tests.test_gpu_mixed import _steps
    AR.install(monkeypatch)
    tr = AR.trainer(img_size=IMG, ch=CH, z_dim=ZD, batch_size=B, c_dim=4)
    gan = hip_model_like(tr, c_dim=4)
    ref = _steps(gan, RM.synthetic_batch(tr.cfg, 5, B), 0, B)
    ref_w = float(gan.store.vars[HELPER].bg_grad.cpu())
    assert ref_w != 0.0
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        o = res[r]
        assert abs(o["d_loss"] - ref["d_loss"]) <= 1e-5 * abs(ref["d_loss"]), (r, o["d_loss"], ref["d_loss"])
        assert abs(o["g_adv"] - ref["g_adv"]) <= 1e-5 * abs(ref["g_adv"]), (r, o["g_adv"], ref["g_adv"])
        assert _rel(o["d_grads"], ref["d_grads"]) < 1e-4, (r, _rel(o["d_grads"], ref["d_grads"]))
        assert _rel(o["g_grads"], ref["g_grads"]) < 1e-4, (r, _rel(o["g_grads"], ref["g_grads"]))
        assert abs(o["helper_grad"] - ref_w) <= 1e-4 * abs(ref_w), (r, o["helper_grad"], ref_w)
    assert np.array_equal(res[0]["g_grads"], res[1]["g_grads"])
