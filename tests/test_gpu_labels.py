"""Labelled datasets on the GPU: the two label-loss launches of csrc/labels.hip against the float64 restatement of
tests/label_ref.py (every dlogits element and the loss inside bounds counted from the formulas), the bit-exact row gather,
the generator's label draws from the label table (eager, per step, and under HIP-graph replay), whole-step parity with the
oracle following the configured loss, --virtual_batches, and two data-parallel ranks."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import ref_model as RM
from tests import label_ref as LR
from tests import launch_replay as R
from tests.common import oracle_trainer, hip_model_like, dev_draws, make_args, t2n
from tests.test_gpu_step import (_run_parity, _loss_close, _vanishing, _exemption_report, cu,  # noqa: F401
                                 MAX_VANISHING, LOSS_TOL)

pytestmark = pytest.mark.gpu

SIXTEEN = ",".join("%d-%s" % (1 + i % 2, "euclidean" if i % 3 == 0 else "logistic") for i in range(16))   # n = 24
EDGES = "1-euclidean,997-logistic,2-euclidean"          # slice edges off every vector boundary
LOSS_CASES = [(B, n, "euclidean") for B, n in ((1, 1), (3, 5), (4, 10), (32, 1000), (256, 1000))] + [
    (3, 5, "2-logistic,3-euclidean"), (4, 10, "6-logistic,4-euclidean"), (32, 1000, EDGES), (256, 1000, EDGES),
    (3, 24, SIXTEEN), (32, 24, SIXTEEN)]
TABLE = [[1, 0, 0, 1, 0, 0], [0, 1, 1, 0, 0, 1], [1, 1, 0, 0, 1, 0], [0, 0, 1, 1, 1, 1], [1, 0, 1, 0, 1, 0]]


def _lib():
    from biggan_tensorflow_amd import hip
    return hip, hip.lib()


def _launch(t, x, w, spec, lw, rows_global=None, sums=None, finish=True):
    """The two launches on device tensors -> (loss [1], dlogits Buf, sums); NaN-prefilled outputs behind guard bands."""
    hip, L = _lib()
    B, n = x.shape
    slices, cols = (a.cuda() for a in LR.table(spec, n))
    S = slices.shape[0]
    P = hip.ptr
    if sums is None:
        sums = torch.zeros(S, dtype=torch.float64, device="cuda")
    hip.check(L.bg_label_loss_sums(P(x), P(t), P(w), P(slices), P(cols), P(sums), B, n, S, hip.stream()))
    if not finish:
        return None, None, sums
    loss = R.Buf(1, torch.float32, "cuda")
    dl = R.Buf(B * n, torch.float32, "cuda", shape=(B, n))
    loss.prefill()
    dl.prefill()
    hip.check(L.bg_label_loss_finish(P(x), P(t), P(w), P(slices), P(cols), P(sums), float(rows_global or B), float(lw),
                                     loss.ptr(), dl.ptr(), B, n, S, hip.stream()))
    torch.cuda.synchronize()
    assert loss.guards_ok() and dl.guards_ok()
    return loss.view, dl, sums


def _check(tag, t, x, w, spec, lw, loss, dx):
    """Print each figure, then gate: every dlogits element and the loss."""
    ref, E = LR.grad_bound(t, x, w, spec, lw)
    ok, ratio, _, _, nbad = R.gate(dx.cpu(), ref, E)
    lref, lE = LR.loss_bound(t, x, w, spec, lw)
    lok, lratio, _, _, _ = R.gate(loss.cpu().reshape(1), lref.reshape(1), lE.reshape(1))
    print("[label gate] %s: dlogits err/bound %.4f (%d outside), loss %.9g ref %.9g err/bound %.4f"
          % (tag, ratio, nbad, float(loss), float(lref), lratio))
    assert not bool(torch.isnan(dx).any()), tag
    assert ok, (tag, "dlogits", ratio, nbad)
    assert lok, (tag, "loss", float(loss), float(lref), float(lE))


# ---------------------------------------------------------------- 1. the loss kernels against float64
@pytest.mark.parametrize("weights", ["ones", "random", "zero-slice"])
@pytest.mark.parametrize("B,n,spec", LOSS_CASES)
def test_label_loss_kernels_against_float64(B, n, spec, weights):
    t, x, w = LR.inputs(B, n, 100 + B + n, weights, spec)
    loss, dl, _ = _launch(t.cuda(), x.cuda(), w.cuda(), spec, 5.0)
    _check("%dx%d %s %s" % (B, n, spec[:24], weights), t, x, w, spec, 5.0, loss, dl.view)
    if weights == "zero-slice":          # the stated deviation: a zero norm gives gradient 0, not NaN
        a, b = [(a, b) for kind, _, a, b in LR._columns(spec, n) if kind == "euclidean"][-1]
        assert float(dl.view[:, a:b].abs().max()) == 0.0


def test_label_loss_of_two_half_batches_is_the_whole_batch():
    """What two ranks do: both halves add into one sums buffer (the all-reduce), each finishes its own rows with
    rows_global = the whole batch.  The square root is taken of the global sum of squares."""
    spec, lw = "6-logistic,4-euclidean", 5.0
    t, x, w = LR.inputs(4, 10, 9, "random", spec)
    tc, xc, wc = t.cuda(), x.cuda(), w.cuda()
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    _launch(tc[:2].contiguous(), xc[:2].contiguous(), wc, spec, lw, sums=sums, finish=False)
    loss1, dl1, _ = _launch(tc[2:].contiguous(), xc[2:].contiguous(), wc, spec, lw, rows_global=4, sums=sums)
    ref, E = LR.grad_bound(t, x, w, spec, lw)
    assert R.gate(dl1.view.cpu(), ref[2:], E[2:])[0]
    lref, lE = LR.loss_bound(t, x, w, spec, lw)
    assert R.gate(loss1.cpu().reshape(1), lref.reshape(1), lE.reshape(1))[0]


def test_cls_loss_fn_runs_the_kernels_through_autograd():
    """utils.cls_loss_fn -> functional.LabelLossFn: forward value, and backward = upstream gradient x stored dlogits."""
    from biggan_tensorflow_amd import utils
    spec, lw = "6-logistic,4-euclidean", 5.0
    t, x, w = LR.inputs(4, 10, 21, "random", spec)
    fn = utils.cls_loss_fn(spec, w.cuda())
    xg = x.cuda().requires_grad_(True)
    loss = fn(t.cuda(), xg, lw, None, 1)
    loss.backward(torch.full((1,), 2.0, device="cuda"))
    ref, E = LR.grad_bound(t, x, w, spec, 2.0 * lw)
    assert R.gate(xg.grad.cpu(), ref, E + R.U32 * ref.abs())[0]          # (one more rounding: the scale by 2 is exact)
    lref, lE = LR.loss_bound(t, x, w, spec, lw)
    assert R.gate(loss.detach().cpu().reshape(1), lref.reshape(1), lE.reshape(1))[0]
    # plain 'logistic' keeps its one-launch kernel
    from biggan_tensorflow_amd import functional as Fn
    xl = x.cuda().requires_grad_(True)
    l1 = utils.cls_loss_fn("logistic", w.cuda())(t.cuda(), xl, lw, None, 1)
    assert type(l1.grad_fn).__name__.startswith("SigmoidCeLossFn") and Fn.LabelLossFn is not Fn.SigmoidCeLossFn
    lref = lw * LR.label_loss(t, x.double(), w, "logistic")
    assert abs(l1.item() - float(lref)) <= 1e-5 * abs(float(lref))


# ---------------------------------------------------------------- 2. the row gather
@pytest.mark.parametrize("rows,n,B", [(1, 1, 4), (5, 7, 3), (1000, 1000, 32)])
def test_gather_rows_is_bit_exact(rows, n, B):
    hip, L = _lib()
    g = torch.Generator().manual_seed(rows + n)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, n), generator=g, dtype=torch.int64).to(torch.int32)
    table = bits.view(torch.float32).cuda()                 # every bit pattern, NaNs included
    idx = torch.randint(0, rows, (B,), generator=g)
    idx[0], idx[-1] = 0, rows - 1
    if B > 2:
        idx[1] = idx[-1]                                     # a repeated index
    out = R.Buf(B * n, torch.float32, "cuda", shape=(B, n))
    out.prefill()
    hip.check(L.bg_gather_rows(hip.ptr(table), hip.ptr(idx.cuda()), out.ptr(), rows, n, B, hip.stream()))
    torch.cuda.synchronize()
    assert out.guards_ok()
    assert torch.equal(out.view.view(torch.int32).cpu(), bits[idx])
    from biggan_tensorflow_amd import functional as Fn
    assert torch.equal(Fn.gather_rows(table, idx.cuda()).view(torch.int32).cpu(), bits[idx])


# ---------------------------------------------------------------- 3. the draws
def _gan(**flags):
    from biggan_tensorflow_amd import model, scope as S
    kw = dict(img_size=64, ch=8, batch_size=4, z_dim=64, n_labels=6)
    kw.update(flags)
    return model.BigGAN(make_args(**kw), store=S.VariableStore("cuda", seed=5)).build_model()


def _labelled_gan(tmp_path, **flags):
    """A model whose label table comes from a label file next to a PNG folder, through open_dataset."""
    from biggan_tensorflow_amd import utils
    folder = tmp_path / "dataset" / "toy"
    folder.mkdir(parents=True)
    lines = []
    for i, row in enumerate(TABLE):
        utils.save_images(np.zeros((1, 8, 8, 3), np.float32), [1, 1], str(folder / ("%d.png" % i)))
        lines.append("\t".join(["%d.png" % i] + [str(v) for v in row]))
    (tmp_path / "labels.tsv").write_text("\n".join(lines) + "\n")
    gan = _gan(dataset="toy", label_file=str(tmp_path / "labels.tsv"), **flags)
    gan.open_dataset(root=str(tmp_path / "dataset")).close()
    assert gan.label_table.is_cuda and gan.label_table.tolist() == [list(map(float, r)) for r in TABLE]
    return gan


def _next_indices(gan, B, rows):
    """The indices draw_labels will draw next, from a clone of the generator's state."""
    g2 = torch.Generator(device="cuda")
    g2.set_state(gan.gen.get_state())
    return torch.randint(0, rows, (B,), device="cuda", generator=g2).cpu().tolist()


def test_steps_draw_their_labels_from_the_table(tmp_path):
    gan = _labelled_gan(tmp_path)
    gan.gen.manual_seed(1234)
    table = torch.tensor(TABLE, dtype=torch.float32)
    real, labels = gan.synthetic_batch(4), gan.label_table[:4].clone()
    z = [gan.sample_z(4) for _ in range(3)]
    drawn = []
    for k in range(3):                                   # D, G, D: with z given, the labels are a step's first draw
        # the device generator's randint cannot be computed on the host, so the expected indices come from a clone of
        # its state, read back and checked on the host BEFORE the step runs: seed 1234 gives three different draws
        want = _next_indices(gan, 4, 5)
        assert len(set(want)) > 1 and want not in drawn, (k, want, drawn)
        if k == 1:
            out = gan.g_step(4, z[k], apply=False)
        else:
            out = gan.d_step(real, z[k], labels=labels, apply=False)
        got = out["cls_z"].cpu()
        assert torch.equal(got.view(torch.int32), table[want].view(torch.int32)), (k, want)
        drawn.append(want)
    assert len({tuple(d) for d in drawn}) == 3
    # an explicit cls_z still wins
    given = gan.label_table[[4, 4, 0, 1]].clone()
    assert gan.d_step(real, z[0], labels=labels, cls_z=given, apply=False)["cls_z"] is given


def test_identity_table_draws_what_synthetic_labels_draws():
    gan = _gan()
    state = gan.gen.get_state()
    want = gan.synthetic_labels(4)
    after = gan.gen.get_state()
    gan.gen.set_state(state)
    gan.label_table = torch.eye(6, device="cuda")
    got = gan.draw_labels(4)
    assert torch.equal(got, want) and torch.equal(gan.gen.get_state(), after)


def test_without_a_table_nothing_changes():
    gan = _gan()
    assert gan.label_table is None
    real, labels = gan.synthetic_batch(4), gan.synthetic_labels(4)
    state = gan.gen.get_state()
    want = gan.synthetic_labels(4)
    gan.gen.set_state(state)
    assert torch.equal(gan.draw_labels(4), want)
    snap = {k: v.detach().clone() for k, v in gan.state_tensors().items()}
    runs = []
    for draw in (gan.draw_labels, gan.synthetic_labels):          # this commit's call, the parent's call
        with torch.no_grad():
            for k, v in gan.state_tensors().items():
                v.copy_(snap[k])
        gan.gen.set_state(state)
        gan.draw_labels = draw
        out = gan.d_step(real, labels=labels, apply=False)
        runs.append((out["d_loss"].item(), out["cls_z"].clone(), gan.gen.get_state().clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


# ---------------------------------------------------------------- 4. whole-step parity
@pytest.mark.parametrize("spec", ["6-logistic,4-euclidean", "euclidean"])
def test_step_parity_with_the_configured_label_loss(spec, tmp_path, monkeypatch):
    weights = np.linspace(0.5, 1.5, 10)
    wfile = tmp_path / "weights.txt"
    wfile.write_text(" ".join("%r" % float(v) for v in weights))
    LR.install(monkeypatch, spec, weights)
    tr = oracle_trainer(64, 8, 64, 4, n_labels=10)
    batch = RM.synthetic_batch(tr.cfg, 11, 4)
    # the oracle alone, on the CPU: finite losses, no zero norm in play, vanishing-gradient tensors inside the cap
    ro = tr.d_step(batch["real"], batch["z_d"], batch["aug_real"], batch["aug_fake_d"], labels=batch["labels"],
                   cls_z=batch["cls_z_d"], apply=False)
    tr.vs.state_updates.clear()
    assert np.isfinite(ro["d_loss"].item()) and ro["d_cls_loss"].item() > 0
    assert sum(_vanishing(k, ro["grads"]) for k in ro["grads"]) <= MAX_VANISHING
    assert float(np.linalg.norm(ro["grads"]["discriminator/DC_logit/kernel"].numpy())) > 0
    gan = hip_model_like(tr, n_labels=10, cls_loss_type=spec, cls_loss_weights=str(wfile))
    _run_parity(tr, gan, batch)


# ---------------------------------------------------------------- 5. --virtual_batches
def test_virtual_batches_average_the_euclidean_norms(monkeypatch):
    """--virtual_batches 2 with 'euclidean': the reported d_cls_loss is the mean of the two passes' norms, not the norm
    over both passes."""
    LR.install(monkeypatch, "euclidean", np.ones(10))
    tr = oracle_trainer(64, 8, 64, 2, n_labels=10)
    gan = hip_model_like(tr, virtual_batches=2, n_labels=10, cls_loss_type="euclidean")
    b0, b1 = RM.synthetic_batch(tr.cfg, 31, 2), RM.synthetic_batch(tr.cfg, 32, 2)
    cz = b0["cls_z_d"]
    r0 = tr.d_step(b0["real"], b0["z_d"], b0["aug_real"], b0["aug_fake_d"], labels=b0["labels"], cls_z=cz, apply=False)
    tr.vs.commit()
    r1 = tr.d_step(b1["real"], b1["z_d"], b1["aug_real"], b1["aug_fake_d"], labels=b1["labels"], cls_z=cz, apply=False)
    ho = gan.d_step([cu(b0["real"]), cu(b1["real"])], [cu(b0["z_d"]), cu(b1["z_d"])],
                    [dev_draws(b0["aug_real"]), dev_draws(b1["aug_real"])],
                    [dev_draws(b0["aug_fake_d"]), dev_draws(b1["aug_fake_d"])], apply=False,
                    labels=[cu(b0["labels"]), cu(b1["labels"])], cls_z=cu(cz))
    n0, n1 = r0["d_cls_loss"].item(), r1["d_cls_loss"].item()
    mean, joint = 0.5 * (n0 + n1), float(np.hypot(n0, n1))
    assert abs(joint - mean) > 100 * LOSS_TOL * mean                 # the two readings are far apart
    assert _loss_close(ho["d_cls_loss"].item(), mean), (ho["d_cls_loss"].item(), mean, joint)
    assert _loss_close(ho["d_loss"].item(), 0.5 * (r0["d_loss"].item() + r1["d_loss"].item()))


# ---------------------------------------------------------------- 6. graph replay
def test_graph_replay_draws_fresh_table_rows(tmp_path):
    """Three eager iterations from a saved state, then capture, rewind and replay (once; three replays): every replayed
    d_loss / g_loss within 1e-5 relative of the eager one, fresh rows of the label table in every replay.  1e-5 is the
    bound of test_hip_graph_replay_matches_eager_iterations, for its reason: replay and eager run the same kernels on the
    same draws, and what may differ is the order of a few atomically accumulated sums."""
    gan = _labelled_gan(tmp_path, cls_loss_type="4-logistic,2-euclidean")
    table = gan.label_table.clone()
    reals = [gan.synthetic_batch(4) for _ in range(3)]
    labels = [table[[i, i + 1, i + 2, 0]].clone() for i in range(3)]
    snap = gan.state_tensors()
    saved = {k: v.detach().clone() for k, v in snap.items()}
    rng = gan.gen.get_state()

    def rewind():
        with torch.no_grad():
            for k, v in snap.items():
                v.copy_(saved[k])
        gan.counter, gan.d_arena.step, gan.g_arena.step = 0, 0, 0
        gan.gen.set_state(rng)
    eager = []
    for real, lab in zip(reals, labels):
        l = gan.train_step(real, lab)
        eager.append((l["d_loss"].item(), l["g_loss"].item()))
    rewind()
    gan.capture_graphs()
    assert gan._graphs_ready and gan.counter == 0
    gan.gen.set_state(rng)
    drawn = []
    for real, lab, (de, ge) in zip(reals, labels, eager):
        l = gan.train_step(real, lab)
        print("[label graph] replay d_loss %.9g g_loss %.9g, eager %.9g %.9g" % (l["d_loss"].item(), l["g_loss"].item(),
                                                                               de, ge))
        assert abs(l["d_loss"].item() - de) <= 1e-5 * abs(de), (l["d_loss"].item(), de)
        assert abs(l["g_loss"].item() - ge) <= 1e-5 * abs(ge), (l["g_loss"].item(), ge)
        drawn.append((gan._g_out_d["cls_z"].clone(), gan._g_out_g["cls_z"].clone()))
    for d, g in drawn:
        for buf in (d, g):
            assert all(any(torch.equal(row, trow) for trow in table) for row in buf)
    for which in (0, 1):                                 # the D op's buffer, the G op's buffer: all three replays differ
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert not torch.equal(drawn[a][which], drawn[b][which]), (which, a, b)


# ---------------------------------------------------------------- 7. two ranks
DP_B = 4


def _dp_run(rank, world):
    """A D step and a G step (no update) with 'euclidean' on this rank's rows of the 4-image batch."""
    from biggan_tensorflow_amd import parallel
    tr = oracle_trainer(64, 8, 64, DP_B, n_labels=10)          # same seed everywhere: identical replicas
    gan = hip_model_like(tr, n_labels=10, cls_loss_type="euclidean")
    batch = RM.synthetic_batch(tr.cfg, 5, DP_B)
    lo, hi = parallel.shard_batch(DP_B, rank, world)

    def sl(d):
        return dev_draws({k: v[lo:hi] for k, v in d.items()})
    d = gan.d_step(cu(batch["real"][lo:hi]), cu(batch["z_d"][lo:hi]), sl(batch["aug_real"]), sl(batch["aug_fake_d"]),
                   apply=False, labels=cu(batch["labels"][lo:hi]), cls_z=cu(batch["cls_z_d"][lo:hi]))
    out = {"d_cls_loss": d["d_cls_loss"].item(),
           "dc_kernel": t2n(gan.store.vars["discriminator/DC_logit/kernel"].bg_grad).copy(),
           "dc_bias": t2n(gan.store.vars["discriminator/DC_logit/bias"].bg_grad).copy()}
    gan.store.load_arrays({k: v.astype(np.float32) for k, v in tr.vs.export().items()}, reset_ema=False)
    g = gan.g_step(hi - lo, cu(batch["z_g"][lo:hi]), sl(batch["aug_fake_g"]), apply=False,
                   cls_z=cu(batch["cls_z_g"][lo:hi]))
    out["g_cls_loss"] = g["g_cls_loss"].item()
    out["g_grads"] = t2n(gan.g_arena.grads).copy()
    return out


def _dp_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch.distributed as dist
    from biggan_tensorflow_amd import parallel
    torch.cuda.set_device(0)
    parallel.init_from_env(backend="gloo")
    out = _dp_run(rank, world)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reduce_the_sum_of_squares_before_the_root():
    from tests.test_gpu_dp import _free_port, _rel
    ref = _dp_run(0, 1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(2):
        o = res[r]
        for key in ("d_cls_loss", "g_cls_loss"):
            assert abs(o[key] - ref[key]) <= 1e-5 * abs(ref[key]), (r, key, o[key], ref[key])
        for key in ("dc_kernel", "dc_bias", "g_grads"):
            assert _rel(o[key], ref[key]) < 1e-4, (r, key, _rel(o[key], ref[key]))
