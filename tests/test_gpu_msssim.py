"""The MS-SSIM kernels (csrc/msssim.hip) and the diversity score on the device against the float64 restatement of
tests/msssim_ref.py.  Every output sits between guard bands that must stay untouched; every launch is repeated once and
must be bit-identical.  Gates: msssim_ref.py measures them on the CPU (4 x the distance of an fp32 emulation from
float64 over these very inputs) and derives the pooling bound from the fp32 unit round-off; nothing is fitted to the
device."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import functional as Fn, metrics, model, scope as S
from tests import msssim_ref as R, trainlog_ref as TR
from tests.common import make_args

pytestmark = pytest.mark.gpu

BAND, FILL = 4096, 12345.0


def _guarded(shape, dtype=torch.float32):
    """(buffer, view): the view sits between two bands of FILL."""
    n = int(np.prod(shape))
    buf = torch.full((BAND + n + BAND,), FILL, dtype=dtype, device="cuda")
    return buf, buf[BAND:BAND + n].view(*shape)


def _bands_untouched(buf):
    return bool((buf[:BAND] == FILL).all()) and bool((buf[-BAND:] == FILL).all())


def _n64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _device_inputs(k, dtype, layout):
    """The case's pairs on the device as (a, b): two buffers [P,...], or one interleaved buffer [2P,...] and None."""
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    a, b = torch.from_numpy(k["a"]).cuda().to(td), torch.from_numpy(k["b"]).cuda().to(td)
    assert np.array_equal(_n64(a), k["a"].astype(np.float64))            # (the bf16 case holds bf16-exact values)
    if layout == "two-buffer":
        return a, b
    return torch.stack([a, b], dim=1).reshape((-1,) + tuple(a.shape[1:])).contiguous(), None


def _run_levels(a, b, S_, C, P):
    """Every level of the pyramid, each launched twice: (ws, [pooled outputs per level], scores [P])."""
    L = len(R.sides(S_))
    wbuf, ws = _guarded((Fn.msssim_workspace(P, S_, C, "cuda").numel(),), torch.float64)
    ws.zero_()
    pools, bufs = [], [wbuf]
    for i in range(L):
        h = S_ >> i
        pool = None
        if i + 1 < L:
            pbuf, pool = _guarded((2, P, h // 2, h // 2, C))
            bufs.append(pbuf)
        Fn.msssim_level(a, b, S_, i, ws, pool)
        first = (Fn.msssim_level_sums(ws, P, S_, C, i).clone(), None if pool is None else pool.clone())
        Fn.msssim_level(a, b, S_, i, ws, pool)
        assert torch.equal(first[0], Fn.msssim_level_sums(ws, P, S_, C, i))
        if pool is not None:
            assert torch.equal(first[1], pool)
            assert not bool((pool == FILL).any())
            pools.append((a, b, pool))
            a, b = pool[0], pool[1]
    sbuf, scores = _guarded((P + 2,), torch.float64)
    scores.fill_(-7.0)
    Fn.msssim_finish(ws, P, S_, C, scores, 1)                              # at a row offset
    first = scores.clone()
    Fn.msssim_finish(ws, P, S_, C, scores, 1)
    assert torch.equal(first, scores) and scores[0] == -7.0 and scores[-1] == -7.0
    assert all(_bands_untouched(x) for x in bufs + [sbuf])
    return ws, pools, scores[1:1 + P].cpu().numpy()


# ---------------------------------------------------------------- level launches, pooled outputs, scores
@pytest.mark.parametrize("S_,C,P", R.LEVEL_CASES, ids=["%dpx-C%d-P%d" % c for c in R.LEVEL_CASES])
def test_levels_against_the_reference(S_, C, P):
    """16 px: one tile of 6 x 6 positions, the last level, no pooled output; 64 px: 54 positions, so edge tiles of 6; the
    pair counts are odd; level 0 reads fp32 or bf16, as two buffers or as rows (2p, 2p + 1) of one."""
    sides = R.sides(S_)
    results = {}
    for dtype in ("fp32", "bf16"):
        k = R.case(S_, C, P, dtype)
        ref = k["ref"]
        for layout in ("two-buffer", "interleaved"):
            a, b = _device_inputs(k, dtype, layout)
            ws, pools, scores = _run_levels(a, b, S_, C, P)
            results[(dtype, layout)] = (ws.clone(), scores)
            worst_mean = 0.0
            for i, h in enumerate(sides):
                sums = Fn.msssim_level_sums(ws, P, S_, C, i).cpu().numpy()
                assert sums.shape == (P, (h // 16) ** 2, C, 2)
                means = sums.sum(axis=1) / float((h - 10) ** 2)
                for j, name in enumerate(("cs", "ssim")):
                    gap = np.abs(means[..., j] - ref[name][i]).max()
                    worst_mean = max(worst_mean, gap)
                    print("%s %s level %d %s: worst gap %.3g (gate %.3g)" % (dtype, layout, h, name, gap, R.MEAN_GATE))
                    assert gap <= R.MEAN_GATE, (dtype, layout, h, name)
            gap = np.abs(scores - ref["scores"]).max()
            print("%s %s scores: worst gap %.3g (gate %.3g), scores %s" % (dtype, layout, gap, R.SCORE_GATE, scores))
            assert gap <= R.SCORE_GATE
            for p, kind in enumerate(k["kinds"]):
                if kind == "negated":
                    assert ref["scores"][p] == 0.0 and scores[p] == 0.0           # the clamp: exactly zero
            # pooled outputs: level 0 against float64 of the inputs, the levels below against float64 of what they read
            for i, (src_a, src_b, pool) in enumerate(pools):
                for s in range(2):
                    x = _n64(src_a)[s::2] if src_b is None else _n64((src_a, src_b)[s])   # (interleaved at level 0)
                    err, bound = np.abs(_n64(pool[s]) - R.pool(x)), R.pool_bound(x)
                    assert (err <= bound).all(), (dtype, layout, i, s, (err / np.maximum(bound, 1e-300)).max())
    # the two layouts run the same arithmetic
    for dtype in ("fp32", "bf16"):
        assert torch.equal(results[(dtype, "two-buffer")][0], results[(dtype, "interleaved")][0])
        assert np.array_equal(results[(dtype, "two-buffer")][1], results[(dtype, "interleaved")][1])


def test_wrappers_reject_what_they_cannot_run():
    x = torch.zeros(4, 32, 32, 3, device="cuda")
    ws = Fn.msssim_workspace(2, 32, 3, "cuda")
    pool = torch.empty(2, 2, 16, 16, 3, device="cuda")
    with pytest.raises(RuntimeError):
        Fn.msssim_level(x.half(), None, 32, 0, ws, pool)
    with pytest.raises(RuntimeError):
        Fn.msssim_level(x[:3], None, 32, 0, ws, pool)                  # three images are not pairs
    with pytest.raises(RuntimeError):
        Fn.msssim_level(x, None, 32, 0, ws, None)                      # level 0 of 2 needs the pooled output
    with pytest.raises(RuntimeError):
        Fn.msssim_level(x, None, 32, 0, ws[:8], pool)                  # workspace too small
    with pytest.raises(RuntimeError):
        Fn.msssim_level(x[:2], x[2:].bfloat16(), 32, 0, ws, pool)
    with pytest.raises(RuntimeError):
        Fn.msssim_level(x.cpu(), None, 32, 0, ws, pool)                # no CPU fallback
    with pytest.raises(RuntimeError):
        Fn.msssim_workspace(2, 48, 3, "cuda")
    with pytest.raises(RuntimeError):
        Fn.msssim_finish(ws, 2, 32, 3, torch.zeros(1, dtype=torch.float64, device="cuda"))


# ---------------------------------------------------------------- metrics.Msssim end to end
def test_msssim_in_batches_of_three_and_of_four():
    S_, C, P = R.E2E_CASE
    k = R.case(S_, C, P)
    stream = torch.stack([torch.from_numpy(k["a"]), torch.from_numpy(k["b"])], dim=1).reshape(2 * P, S_, S_, C).cuda()
    plan = metrics.MsssimPlan(S_, C, 4, P, 1)
    m = metrics.Msssim(plan, "cuda")
    runs = []
    for size in (3, 4, 12):
        m.begin()
        for lo in range(0, 2 * P, size):
            m.add(stream[lo:lo + size])
        m.add(stream[:2])                                              # padding past 2 P is dropped
        runs.append((m.finish(), m.per_pair.copy()))
    for mean, per_pair in runs[1:]:
        assert mean == runs[0][0] and per_pair.tobytes() == runs[0][1].tobytes()
    gap = np.abs(runs[0][1] - k["ref"]["scores"]).max()
    print("per-pair scores %s, worst gap %.3g (gate %.3g)" % (runs[0][1], gap, R.SCORE_GATE))
    assert gap <= R.SCORE_GATE
    assert abs(runs[0][0] - k["ref"]["scores"].mean()) <= R.SCORE_GATE
    assert runs[0][1][1] > 1.0 - R.SCORE_GATE and runs[0][1][2] == 0.0           # the identical and the negated pair


# ---------------------------------------------------------------- model level
def _model(tmp_path, tag, **kw):
    d = tmp_path / tag
    flags = dict(img_size=64, ch=8, batch_size=4, msssim_pairs=5, log_dir=str(d / "logs"), checkpoint_dir=str(d / "ckpt"),
                 sample_dir=str(d / "samples"), result_dir=str(d / "results"))
    flags.update(kw)
    return model.BigGAN(make_args(**flags), store=S.VariableStore("cuda", seed=5)).build_model()


def _snapshot(gan):
    gan.sync_sharded_state()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in gan.state_tensors().items()}, gan.gen.get_state().clone(), gan.counter)


def _same_state(gan, snap):
    now = gan.state_tensors()
    assert set(now) == set(snap[0])
    changed = [k for k, v in now.items() if not torch.equal(v, snap[0][k])]
    assert not changed, changed[:5]
    assert torch.equal(gan.gen.get_state(), snap[1]) and gan.counter == snap[2]


def _reference_with_its_own_gate(images):
    """Pairs as consecutive rows [2P,...] (fp32 values) -> (float64 mean score, 4 x the emulation's distance from it on
    these very images: the rule of msssim_ref.py applied to inputs that are not among its cases)."""
    a, b = images[0::2], images[1::2]
    ref = R.pair_scores(a, b)
    _, score_gap = R.gaps(a, b, ref)
    return float(ref["scores"].mean()), 4 * max(score_gap, R.U32)


def test_model_scores_agree_with_the_reference_and_leave_the_run_alone(tmp_path):
    gan = _model(tmp_path, "msssim")
    gan.train_step(gan.synthetic_batch())                  # the moving averages now differ from the live weights
    snap = _snapshot(gan)
    np_state = np.random.get_state()[1].copy()
    first = gan.msssim()
    second = gan.msssim()
    _same_state(gan, snap)
    assert np.array_equal(np.random.get_state()[1], np_state)
    assert list(first) == ["msssim", "msssim_real"] and list(second) == ["msssim"]       # the baseline: the first call only
    assert second["msssim"] == first["msssim"] and all(0.0 <= v <= 1.0 + 1e-6 for v in first.values())
    # the same images through the float64 restatement: 5 pairs = 10 images in batches of 4, so a pair is carried
    plan = gan.monitor_plan("msssim")
    assert plan.n_pairs == 5 and not plan.from_files and plan.n_real_pairs == 5
    z, cls_z = gan.monitor_fake_inputs(plan)
    assert z.shape[0] == 10 and cls_z is None
    fake = gan.generate(z, cls_z, ema=True).float().cpu().numpy()
    want, gate = _reference_with_its_own_gate(fake)
    print("msssim: device %.9g reference %.9g gate %.3g" % (first["msssim"], want, gate))
    assert abs(first["msssim"] - want) <= gate
    real = torch.cat(list(gan.monitor_real_batches(plan))).cpu().numpy()
    want, gate = _reference_with_its_own_gate(real)
    print("msssim_real: device %.9g reference %.9g gate %.3g" % (first["msssim_real"], want, gate))
    assert abs(first["msssim_real"] - want) <= gate
    _same_state(gan, snap)
    # --sample_ema both: the live weights under their own tag
    gan.generate_noema_samples = True
    both = gan.msssim()
    assert list(both) == ["msssim", "msssim_noema"] and both["msssim"] == first["msssim"]
    live = gan.generate(z, cls_z, ema=False).float().cpu().numpy()
    want, gate = _reference_with_its_own_gate(live)
    assert abs(both["msssim_noema"] - want) <= gate
    _same_state(gan, snap)


def test_pairs_share_a_class_vector_with_labels(tmp_path):
    gan = _model(tmp_path, "labels", n_labels=4)
    plan = gan.monitor_plan("msssim")
    z, cls_z = gan.monitor_fake_inputs(plan)
    assert cls_z.shape == (10, 4) and np.array_equal(cls_z[0::2], cls_z[1::2])
    scores = gan.msssim()
    fake = gan.generate(z, cls_z, ema=True).float().cpu().numpy()
    want, gate = _reference_with_its_own_gate(fake)
    assert abs(scores["msssim"] - want) <= gate and "msssim_real" in scores


def test_the_real_baseline_pairs_the_first_files_without_flips(tmp_path):
    from biggan_tensorflow_amd import data as D, utils
    root = tmp_path / "dataset"
    (root / "toy").mkdir(parents=True)
    rng = np.random.RandomState(9)
    for i in range(7):
        utils.write_png(rng.randint(0, 256, size=(70, 80, 3)).astype(np.uint8), str(root / "toy" / ("%02d.png" % i)))
    gan = _model(tmp_path, "files", dataset="toy")
    plan = gan.monitor_plan("msssim", str(root))
    assert plan.from_files and plan.n_real_pairs == 3                   # min(5 asked, 7 // 2 files)
    files = gan._dataset_files(str(root))
    order = plan.draw_real_pairs().reshape(-1)
    assert sorted(order) == list(range(6))
    real = torch.cat(list(gan.monitor_real_batches(plan, str(root))))
    want = np.stack([D.ImageData(64, 3, True, False).image_processing(files[i]) for i in order])
    assert np.array_equal(real.cpu().numpy(), want)
    scores = gan.msssim(str(root))
    ref, gate = _reference_with_its_own_gate(want)
    assert abs(scores["msssim_real"] - ref) <= gate
    assert list(gan.msssim(str(root))) == ["msssim"]


def _train(tmp_path, tag, msssim_freq, **kw):
    gan = _model(tmp_path, tag, msssim_freq=msssim_freq, **kw)
    seen = []
    step = gan.train_step

    def recording_step(*a, **k):
        out = step(*a, **k)
        seen.append({name: np.float32(v.item()) for name, v in out.items()})
        return out

    gan.train_step = recording_step
    gan.log_events = True
    gan.train(iterations=3, resume=False)
    return gan, seen


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def run_pair(request, tmp_path_factory):
    """Three training steps with --msssim_freq 1 and with --msssim_freq 0 from the same seed, run once per precision."""
    tmp_path = tmp_path_factory.mktemp("pair_" + request.param)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        scored, seen = _train(tmp_path, "scored", 1, precision=request.param)
    lines = [l for l in out.getvalue().splitlines() if l.startswith("MS-SSIM: ")]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        plain, seen2 = _train(tmp_path, "plain", 0, precision=request.param)
    assert "MS-SSIM: " not in out.getvalue()
    return dict(scored=scored, plain=plain, seen=seen, seen2=seen2, lines=lines, tmp_path=tmp_path)


def test_training_state_and_losses_with_the_score_are_bit_identical(run_pair):
    scored, plain = run_pair["scored"], run_pair["plain"]
    a, b = scored.state_tensors(), plain.state_tensors()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(k.endswith("/u") for k in a) and any(k.endswith("/Adam_1") for k in a)
    assert torch.equal(scored.gen.get_state(), plain.gen.get_state()) and scored.counter == plain.counter == 3
    assert plain._monitors.get("msssim") is None and scored._monitors.get("msssim") is not None
    assert len(run_pair["seen"]) == 3 and run_pair["seen"] == run_pair["seen2"]


def test_training_logs_the_scores(run_pair):
    scored, lines = run_pair["scored"], run_pair["lines"]
    d = os.path.join(str(run_pair["tmp_path"] / "scored" / "logs"), scored.model_dir)
    ev = TR.read_events(os.path.join(d, os.listdir(d)[0]))
    events = [e for e in ev[1:] if e["values"][0][0].startswith("msssim")]
    assert [e["step"] for e in events] == [e["step"] for e in ev[1:] if "d_loss" in [t for t, _, _ in e["values"]]]
    assert len(events) == 3 == len(lines)
    assert [[t for t, _, _ in e["values"]] for e in events] == [["msssim", "msssim_real"], ["msssim"], ["msssim"]]
    for e, line in zip(events, lines):
        assert all(kind == "scalar" and 0.0 <= v <= 1.0 + 1e-6 for _, kind, v in e["values"])
        assert [f.split(": ")[0] for f in line[len("MS-SSIM: "):].split(", ")] == [t for t, _, _ in e["values"]]
        assert abs(float(line.split("msssim: ")[1].split(",")[0]) - float(e["values"][0][2])) <= 1e-4
    assert events[0]["values"][0] != events[2]["values"][0]           # the weights moved between the events


def test_phase_test_writes_the_scores(tmp_path):
    gan = _model(tmp_path, "phase", msssim_freq=1, test_num=1)
    gan.test()
    path = os.path.join(str(tmp_path / "phase" / "results"), gan.model_dir, "msssim.txt")
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert [r[0] for r in rows] == ["msssim", "msssim_real"] and all(0.0 <= float(r[1]) <= 1.0 + 1e-6 for r in rows)
