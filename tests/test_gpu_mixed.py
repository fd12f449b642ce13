"""Mixed-kernel generator blocks on the GPU (--g_mixed_resblocks, ops.py:403-442, BigGAN.py:485-489): the multi-branch
convolution kernels (bg_mixconv_*) against float64, whole-step parity against the float64 restatement
(tests/mixed_ref.py installed over the oracle's generator), EMA sampling, graph replay, bf16 and data parallelism."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model as RM
from tests import mixed_ref as MR
from tests.common import hip_model_like, dev_draws, rel_err, t2n
from tests.test_gpu_step import _run_parity, cu

pytestmark = pytest.mark.gpu

REFLECT, ZERO = 0, 1


def _hip():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip
    return Fn, hip


def _branch(kind, cb, k, dil=1, pad_mode=REFLECT):
    """(cb, k, dil, lo, pad_mode, transposed) of a clown-style branch."""
    if kind == "deconv":
        return (cb, k, 1, k - 1 - (k - 1) // 2, ZERO, 1)
    keff = (k - 1) * dil + 1
    return (cb, k, dil, (keff - 1) // 2, pad_mode, 0)


def _clown_table(inner, pad_mode=REFLECT):
    d4, d3, d2, c3, c5, dl = MR.clown_split(inner)
    return [_branch("deconv", d4, 4), _branch("deconv", d3, 3), _branch("deconv", d2, 2),
            _branch("conv", c3, 3, 1, pad_mode), _branch("conv", c5, 5, 1, pad_mode), _branch("conv", dl, 5, 2, pad_mode)]


def _ref_branch(x, w, br):
    """float64 restatement of one branch: explicit padding + torch conv2d (dilation=), transposed branches as the
    correlation with the flipped kernel."""
    cb, k, dil, lo, mode, tr = br
    hi = (k - 1) * dil - lo
    xin = x.permute(0, 3, 1, 2)
    xin = F.pad(xin, (lo, hi, lo, hi), mode="reflect" if mode == REFLECT else "constant")
    wt = (w.permute(2, 3, 0, 1).flip(2, 3) if tr else w.permute(3, 2, 0, 1)).contiguous()
    return F.conv2d(xin, wt, dilation=dil).permute(0, 2, 3, 1)


def _weights(rng, table, cin):
    ws = []
    for cb, k, dil, lo, mode, tr in table:
        shape = (k, k, cb, cin) if tr else (k, k, cin, cb)
        ws.append(rng.standard_normal(shape) / np.sqrt(k * k * cin))
    return ws


def _spec(table):
    spec, off = [], 0
    for cb, k, dil, lo, mode, tr in table:
        spec.append((off, cb, k, dil, lo, mode, tr))
        off += cb
    return tuple(spec)


def _run_fn(x, ws, bs, table, dtype=torch.float32, compute=None):
    """forward + backward through functional.MixConvFn; returns y, dx, dws, dbs (numpy) for dy = g."""
    Fn, hip = _hip()
    prev = Fn.Precision.compute
    if compute is not None:
        Fn.Precision.compute = compute
    try:
        xt = torch.tensor(x, dtype=dtype, device="cuda", requires_grad=True)
        wt = [torch.tensor(w, dtype=torch.float32, device="cuda", requires_grad=True) for w in ws]
        bt = [torch.tensor(b, dtype=torch.float32, device="cuda", requires_grad=True) for b in bs]
        params = []
        for w, b in zip(wt, bt):
            params += [w, b]
        y = Fn.MixConvFn.apply(xt, _spec(table), *params)
        g = torch.tensor(np.random.default_rng(7).standard_normal(tuple(y.shape)), dtype=y.dtype, device="cuda")
        dx, *grads = torch.autograd.grad(y, [xt] + params, g)
        torch.cuda.synchronize()
        return (t2n(y.float()), t2n(dx.float()), [t2n(t) for t in grads[0::2]], [t2n(t) for t in grads[1::2]],
                t2n(g.float()))
    finally:
        Fn.Precision.compute = prev


def _ref_all(x, ws, bs, table, g, round_bf16=False):
    def r(a):
        t = torch.tensor(a, dtype=torch.float64)
        return t.to(torch.bfloat16).to(torch.float64) if round_bf16 else t
    xt = r(x).requires_grad_(True)
    wt = [r(w).requires_grad_(True) for w in ws]
    bt = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in bs]
    y = torch.cat([_ref_branch(xt, w, br) + b for w, b, br in zip(wt, bt, table)], dim=-1)
    grads = torch.autograd.grad(y, [xt] + wt + bt, r(g))              # (the gradient is a rounded operand too)
    n = len(table)
    # (bias gradients are plain sums of the unrounded dy)
    db = torch.tensor(g, dtype=torch.float64).sum(dim=(0, 1, 2))
    offs = np.cumsum([0] + [br[0] for br in table])
    return (y.detach().numpy(), grads[0].numpy(), [t.numpy() for t in grads[1:1 + n]],
            [db[offs[i]:offs[i + 1]].numpy() for i in range(n)])


def _check(got, ref, tol):
    y, dx, dws, dbs, _ = got
    ry, rdx, rdws, rdbs = ref
    assert rel_err(y, ry) < tol, rel_err(y, ry)
    assert rel_err(dx, rdx) < tol, rel_err(dx, rdx)
    for i, (a, b) in enumerate(zip(dws, rdws)):
        assert rel_err(a, b) < tol, (i, rel_err(a, b))
    for i, (a, b) in enumerate(zip(dbs, rdbs)):
        assert rel_err(a, b) < tol, (i, rel_err(a, b))


# ---------------------------------------------------------------- kernels
KINDS = [("deconv", 4), ("deconv", 3), ("deconv", 2), ("conv", 3), ("conv", 5), ("dil", 5), ("conv", 1)]


@pytest.mark.parametrize("kind,k", KINDS)
@pytest.mark.parametrize("pad_mode", [REFLECT, ZERO])
def test_single_branch_against_float64(kind, k, pad_mode):
    """Each branch kind alone (6 channels: not a multiple of 8), fp32 exact, reflect and zero padding; forward, input
    gradient (with the reflect adjoint at the border), weight and bias gradients."""
    rng = np.random.default_rng(k * 3 + pad_mode)
    br = _branch("deconv", 6, k) if kind == "deconv" else _branch("conv", 6, k, 2 if kind == "dil" else 1, pad_mode)
    table = [br]
    x = rng.standard_normal((2, 9, 7, 5))
    ws, bs = _weights(rng, table, 5), [rng.standard_normal(6)]
    got = _run_fn(x, ws, bs, table)
    _check(got, _ref_all(x, ws, bs, table, got[4]), 1e-5)


@pytest.mark.parametrize("inner,cin,hw", [(8, 16, 16), (48, 96, 8), (768, 1536, 8)])
@pytest.mark.parametrize("pad_mode", [REFLECT, ZERO])
def test_full_clown_table_against_float64(inner, cin, hw, pad_mode):
    rng = np.random.default_rng(inner + pad_mode)
    table = _clown_table(inner, pad_mode)
    x = rng.standard_normal((2, hw, hw, cin))
    ws = _weights(rng, table, cin)
    bs = [rng.standard_normal(br[0]) for br in table]
    got = _run_fn(x, ws, bs, table)
    assert got[0].shape == (2, hw, hw, inner)
    _check(got, _ref_all(x, ws, bs, table, got[4]), 1e-5)


@pytest.mark.parametrize("dtype,compute", [(torch.bfloat16, None), (torch.float32, 1)])
def test_bf16_operands(dtype, compute):
    """bf16 tensors (bf16-resident) and fp32 tensors with BG_COMPUTE_BF16: the products see bf16 operands, the sums
    are fp32 - against float64 on the rounded operands."""
    rng = np.random.default_rng(11)
    table = _clown_table(48)
    x = rng.standard_normal((2, 8, 8, 64))
    ws = _weights(rng, table, 64)
    bs = [rng.standard_normal(br[0]) for br in table]
    got = _run_fn(x, ws, bs, table, dtype=dtype, compute=compute)
    ref = _ref_all(x, ws, bs, table, got[4], round_bf16=True)
    # (bf16 outputs / input gradients are stored rounded: 2^-9 relative)
    tol = 1e-2 if dtype == torch.bfloat16 else 1e-4
    _check(got, ref, tol)


@pytest.mark.parametrize("inner,cin,hw,pad_mode", [(768, 1536, 8, REFLECT), (192, 384, 16, ZERO),
                                                   (48, 96, 32, REFLECT), (8, 32, 9, REFLECT)])
def test_bf16_mfma_path_against_float64(inner, cin, hw, pad_mode):
    """The bf16-resident calls (bf16 x and dy, Cin % 32 == 0) run on the MFMA kernels: the full clown table at the
    generator's level shapes (and a 9x9 map whose pixel count is not a multiple of the 64-row tile), forward, input and
    weight gradients against float64 on the rounded operands, and bit-identical when repeated."""
    rng = np.random.default_rng(inner + cin)
    table = _clown_table(inner, pad_mode)
    x = rng.standard_normal((2, hw, hw, cin))
    ws = _weights(rng, table, cin)
    bs = [rng.standard_normal(br[0]) for br in table]
    got = _run_fn(x, ws, bs, table, dtype=torch.bfloat16)
    _check(got, _ref_all(x, ws, bs, table, got[4], round_bf16=True), 1e-2)
    again = _run_fn(x, ws, bs, table, dtype=torch.bfloat16)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    assert all(np.array_equal(u, v) for u, v in zip(got[2], again[2]))


def test_weight_gradient_only_where_needed():
    """A branch whose kernel needs no gradient gets none computed (its dw is NULL in the table)."""
    rng = np.random.default_rng(12)
    table = _clown_table(16)
    x = rng.standard_normal((2, 8, 8, 32))
    Fn, hip = _hip()
    xt = torch.tensor(x, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    ws = [torch.tensor(w, dtype=torch.float32, device="cuda", requires_grad=(i % 2 == 0))
          for i, w in enumerate(_weights(rng, table, 32))]
    params = []
    for w in ws:
        params += [w, None]
    y = Fn.MixConvFn.apply(xt, _spec(table), *params)
    y.float().sum().backward()
    torch.cuda.synchronize()
    assert all((w.grad is not None) == (i % 2 == 0) for i, w in enumerate(ws))
    wa = [w.detach().clone().requires_grad_(True) for w in ws]
    params = []
    for w in wa:
        params += [w, None]
    Fn.MixConvFn.apply(xt, _spec(table), *params).float().sum().backward()
    torch.cuda.synchronize()
    for i in range(0, len(ws), 2):               # the same gradients as when every branch computes one
        assert torch.equal(ws[i].grad, wa[i].grad), i


def _raw(table, x, cin, ldy, c_base, y_init, compute=0):
    Fn, hip = _hip()
    N, H, W, _ = x.shape
    ws = [torch.tensor(w, dtype=torch.float32, device="cuda") for w in _weights(np.random.default_rng(2), table, cin)]
    t = (hip.BgMixBranch * len(table))()
    off = c_base
    for e, w, (cb, k, dil, lo, mode, tr) in zip(t, ws, table):
        e.c_off, e.cb, e.k, e.dil, e.lo, e.pad_mode, e.transposed, e.w = off, cb, k, dil, lo, mode, tr, w.data_ptr()
        off += cb
    d = hip.conv_desc(N, H, W, cin, H, W, ldy, 1, 1, 0, 0, compute)
    xt = torch.tensor(x, dtype=torch.float32, device="cuda")
    y = torch.tensor(y_init, dtype=torch.float32, device="cuda")
    hip.check(hip.lib().bg_mixconv_fwd(d, ctypes.cast(t, ctypes.c_void_p), len(table), xt.data_ptr(), y.data_ptr(), ldy,
                                       hip.stream()))
    torch.cuda.synchronize()
    return t2n(y), [t2n(w).astype(np.float64) for w in ws]


def test_output_at_a_channel_offset_leaves_other_channels():
    """String-kernel form: the branches write channels [5, 5 + 18) of a 29-channel tensor; the rest keeps its values."""
    rng = np.random.default_rng(4)
    table = [_branch("conv", 8, 3), _branch("conv", 4, 5), _branch("conv", 6, 5, 2)]
    x = rng.standard_normal((2, 10, 10, 12))
    y0 = rng.standard_normal((2, 10, 10, 29)).astype(np.float32)
    y, ws = _raw(table, x, 12, 29, 5, y0)
    assert np.array_equal(y[..., :5], y0[..., :5]) and np.array_equal(y[..., 23:], y0[..., 23:])
    ref = torch.cat([_ref_branch(torch.tensor(x), torch.tensor(w), br) for w, br in zip(ws, table)], -1).numpy()
    assert rel_err(y[..., 5:23], ref) < 1e-5


def test_adjoint_identity_with_reflect_padding():
    """<conv(x), dy> = <x, dgrad(dy)> for the whole table with reflect padding (dilated taps reflect up to 4 rows)."""
    Fn, hip = _hip()
    rng = np.random.default_rng(8)
    table = _clown_table(16)
    x = rng.standard_normal((3, 8, 8, 24))
    ws = _weights(rng, table, 24)
    got = _run_fn(x, ws, [np.zeros(br[0]) for br in table], table)
    y, dx, _, _, g = got
    lhs = float(np.sum(y.astype(np.float64) * g))
    rhs = float(np.sum(x * dx.astype(np.float64)))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0), (lhs, rhs)


def test_repeated_runs_are_bit_identical():
    rng = np.random.default_rng(9)
    table = _clown_table(48)
    x = rng.standard_normal((4, 16, 16, 96))
    ws = _weights(rng, table, 96)
    bs = [rng.standard_normal(br[0]) for br in table]
    a = _run_fn(x, ws, bs, table)
    b = _run_fn(x, ws, bs, table)
    for u, v in zip(a[:2], b[:2]):
        assert np.array_equal(u, v)
    for us, vs in zip(a[2:4], b[2:4]):
        for u, v in zip(us, vs):
            assert np.array_equal(u, v)


def test_abi_rejects_bad_tables():
    Fn, hip = _hip()
    L = hip.lib()
    d = hip.conv_desc(2, 4, 4, 8, 4, 4, 8, 1, 1, 0, 0)
    x = torch.zeros(2, 4, 4, 8, device="cuda")
    y = torch.zeros(2, 4, 4, 8, device="cuda")
    w = torch.zeros(5, 5, 8, 8, device="cuda")
    t = (hip.BgMixBranch * 1)()
    t[0].cb, t[0].k, t[0].dil, t[0].lo, t[0].pad_mode, t[0].w = 8, 5, 2, 4, REFLECT, w.data_ptr()
    tp = ctypes.cast(t, ctypes.c_void_p)
    assert L.bg_mixconv_fwd(d, tp, 1, x.data_ptr(), y.data_ptr(), 8, hip.stream()) == 1      # reflect 4 on a 4x4 map
    t[0].pad_mode = ZERO
    assert L.bg_mixconv_fwd(d, tp, 1, x.data_ptr(), y.data_ptr(), 8, hip.stream()) == 0
    assert L.bg_mixconv_fwd(d, tp, 1, x.data_ptr(), y.data_ptr(), 7, hip.stream()) == 1      # slice past the row
    assert L.bg_mixconv_fwd(d, None, 1, x.data_ptr(), y.data_ptr(), 8, hip.stream()) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- whole step
STEP_CASES = [
    (64, dict()),
    (128, dict(conv_padding="zero")),
    (64, dict(n_labels=4)),
    (64, dict(bn_type="batch_renorm")),
    (64, dict(deep=True)),
    (64, dict(shared_z=16, n_labels=4, cls_embedding=True)),
]


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_step_parity_mixed_blocks(monkeypatch, case):
    size, flags = STEP_CASES[case]
    MR.install(monkeypatch)
    tr = MR.trainer(img_size=size, ch=8, z_dim=64, batch_size=4, g_mixed_resblocks=True, **flags)
    gan = hip_model_like(tr, g_mixed_resblocks=True, **flags)
    assert set(gan.store.vars) == set(tr.vs.vars)
    batch = RM.synthetic_batch(tr.cfg, 21 + case, 4)
    _run_parity(tr, gan, batch)


def test_sample_with_ema_weights(monkeypatch):
    """sample(): the mixed blocks' batch norms on their moving statistics, EMA shadows of the new weights."""
    MR.install(monkeypatch)
    tr = MR.trainer(img_size=64, ch=8, z_dim=64, batch_size=2, g_mixed_resblocks=True)
    gan = hip_model_like(tr, g_mixed_resblocks=True)
    batch = RM.synthetic_batch(tr.cfg, 41, 2)
    tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"])
    tr.g_step(batch["z_g"], batch["aug_fake_g"])
    gan.d_step(cu(batch["real"]), cu(batch["z_d"]), dev_draws(batch["aug_real"]), dev_draws(batch["aug_fake_d"]))
    gan.g_step(2, cu(batch["z_g"]), dev_draws(batch["aug_fake_g"]))
    k = "generator/res_mixed2/clown/conv5/kernel"
    assert not np.array_equal(t2n(gan.g_arena.view(gan.g_arena.ema, k)), t2n(gan.store.vars[k]))
    z = RM.truncated_normal(np.random.default_rng(5), (2, 1, 1, tr.cfg.z_dim))
    ref = tr.sample(z)
    img = gan.sample(cu(z))
    assert rel_err(t2n(img), ref.numpy()) < 1e-4


def test_hip_graph_replay_matches_eager():
    from tests.common import make_args
    from biggan_tensorflow_amd import model, scope as S
    gan = model.BigGAN(make_args(img_size=64, ch=8, batch_size=4, z_dim=64, g_mixed_resblocks=True, n_labels=0),
                       store=S.VariableStore("cuda", seed=5)).build_model()
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


def test_bf16_step_config3_topology():
    """BASELINE config 3's generator topology (128^2, ch 96, bf16-resident) at batch 4 with --g_mixed_resblocks: the bf16
    step against the same model in fp32 within the bf16 gate of tests/test_gpu_bf16.py (losses and images 2e-2
    relative; gradients 4e-1 relative L2)."""
    from tests.common import make_args
    from biggan_tensorflow_amd import model, scope as S, functional as Fn
    kw = dict(img_size=128, ch=96, batch_size=4, g_mixed_resblocks=True)
    try:
        g32 = model.BigGAN(make_args(**kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16 = model.BigGAN(make_args(precision="bf16", **kw), store=S.VariableStore("cuda", seed=3)).build_model()
        g16.store.load_arrays(g32.store.export_arrays())
        torch.manual_seed(0)
        z = torch.randn(4, 1, 1, g32.z_dim, device="cuda").clamp_(-2, 2)
        names = ("generator/res_mixed16/clown/deconv4/kernel", "generator/res_mixed1/clown/dilconv5/kernel",
                 "generator/res_mixed4/proj/kernel", "generator/res_mixed2/clown/prelu/alpha")
        outs = []
        for g in (g32, g16):
            o = g.g_step(4, z, None, apply=False)
            grads = {k: t2n(g.store.vars[k].bg_grad).copy() for k in names}
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


# ---------------------------------------------------------------- data parallel
IMG, CH, ZD, B = 64, 8, 64, 4


def _steps(gan, batch, lo, hi):
    out = {}
    d = gan.d_step(cu(batch["real"][lo:hi]), cu(batch["z_d"][lo:hi]), dev_draws(_slice(batch["aug_real"], lo, hi)),
                   dev_draws(_slice(batch["aug_fake_d"], lo, hi)), apply=False)
    out["d_loss"] = d["d_loss"].item()
    out["d_grads"] = t2n(gan.d_arena.grads).copy()
    g = gan.g_step(hi - lo, cu(batch["z_g"][lo:hi]), dev_draws(_slice(batch["aug_fake_g"], lo, hi)), apply=False)
    out["g_adv"] = g["g_adv"].item()
    out["g_grads"] = t2n(gan.g_arena.grads).copy()
    return out


def _slice(d, lo, hi):
    from tests.test_gpu_dp import _slice_draws
    return _slice_draws(d, lo, hi)


def _dp_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch.distributed as dist
    from biggan_tensorflow_amd import parallel
    from tests import mixed_ref as MR_
    from tests.test_gpu_mixed import _steps as steps
    torch.cuda.set_device(0)
    parallel.init_from_env(backend="gloo")
    RM.generator = MR_.generator
    tr = MR_.trainer(img_size=IMG, ch=CH, z_dim=ZD, batch_size=B, g_mixed_resblocks=True)
    gan = hip_model_like(tr, g_mixed_resblocks=True)
    assert gan.world == world and gan.rank == rank
    batch = RM.synthetic_batch(tr.cfg, 5, B)
    lo, hi = parallel.shard_batch(B, rank, world)
    q.put((rank, steps(gan, batch, lo, hi)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_data_parallel_matches_single_process(monkeypatch):
    """Two ranks (gloo, both on one card) with half the batch each reproduce the single process: the mixed blocks'
    batch norms take cross-replica statistics, their weight gradients meet in the SUM all-reduce."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dp import _free_port, _rel
    MR.install(monkeypatch)
    tr = MR.trainer(img_size=IMG, ch=CH, z_dim=ZD, batch_size=B, g_mixed_resblocks=True)
    gan = hip_model_like(tr, g_mixed_resblocks=True)
    ref = _steps(gan, RM.synthetic_batch(tr.cfg, 5, B), 0, B)
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
    assert np.array_equal(res[0]["g_grads"], res[1]["g_grads"])
