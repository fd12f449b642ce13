"""The sliced Wasserstein kernels (csrc/swd.hip) and the metric on the device against the float64 restatement of
tests/swd_ref.py.  Every output sits between guard bands that must stay untouched; every launch is repeated once and
must be bit-identical.  Bounds: swd_ref.py derives them from the fp32 unit round-off; nothing here is fitted."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import functional as Fn, metrics, model, scope as S
from tests import swd_ref as R, trainlog_ref as TR
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


@pytest.fixture(scope="module")
def e2e():
    return R.end_to_end_case(0)


# ---------------------------------------------------------------- pyramid
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("B,H", [(2, 32), (1, 128)], ids=["2x32", "1x128"])
def test_pyramid(B, H, C, dtype):
    g = torch.Generator(device="cuda").manual_seed(100 * H + 10 * C + B)
    x = (torch.rand(B, H, H, C, device="cuda", generator=g) * 2.0 - 1.0).to(dtype)
    x64 = _n64(x)
    buf, y = _guarded((B, H // 2, H // 2, C))
    Fn.swd_pyr_down(x, out=y)
    first = y.clone()
    Fn.swd_pyr_down(x, out=y)
    assert torch.equal(first, y) and _bands_untouched(buf)
    err, bound = np.abs(_n64(y) - R.down(x64)), R.down_bound(x64)
    print("down %s C=%d %dx%d: worst error / bound %.3f" % (dtype, C, B, H, (err / bound).max()))
    assert (err <= bound).all()
    # the Laplacian level from the kernel's own coarse level: the reference is fed the same fp32 values
    g1 = first
    buf, lap = _guarded((B, H, H, C))
    Fn.swd_pyr_lap(x, g1, out=lap)
    first = lap.clone()
    Fn.swd_pyr_lap(x, g1, out=lap)
    assert torch.equal(first, lap) and _bands_untouched(buf)
    err, bound = np.abs(_n64(lap) - (x64 - R.up(_n64(g1)))), R.lap_bound(x64, _n64(g1))
    print("lap  %s C=%d %dx%d: worst error / bound %.3f" % (dtype, C, B, H, (err / bound).max()))
    assert (err <= bound).all()


def test_pyramid_wrappers_reject_what_they_cannot_run():
    x = torch.zeros(1, 32, 32, 3, device="cuda")
    with pytest.raises(RuntimeError):
        Fn.swd_pyr_down(x.half())
    with pytest.raises(RuntimeError):
        Fn.swd_pyr_down(x[:, :, :16])
    with pytest.raises(RuntimeError):
        Fn.swd_pyr_down(torch.zeros(1, 16, 16, 3, device="cuda"))
    with pytest.raises(RuntimeError):
        Fn.swd_pyr_lap(x, torch.zeros(1, 16, 16, 3, device="cuda", dtype=torch.bfloat16))


# ---------------------------------------------------------------- descriptors
@pytest.mark.parametrize("C,H", [(1, 16), (3, 32), (4, 16)], ids=["1x16", "3x32", "4x16"])
def test_descriptors(C, H):
    rng = np.random.RandomState(7 * C + H)
    B, K = 4, 49 * C
    level = (rng.uniform(-1, 1, size=(B, H, H, C)) + 0.5).astype(np.float32)
    if C == 4:
        level[..., 3] = 1.0                                        # a constant alpha plane: no deviation
    pos = R.draw_positions(rng, B, H)
    pos[0, 0], pos[0, 1], pos[3, 127] = (3, 3), (H - 4, H - 4), (H - 4, 3)
    if C != 4:                                                     # (zero rows would give the constant plane a deviation)
        pos[1, 2], pos[1, 3], pos[2, 4], pos[2, 5], pos[3, 6] = (2, 8), (8, H - 3), (-1, 8), (8, 1 << 20), (H, H)
    want = R.descriptors(level, pos)
    assert want.dtype == np.float32 and want[0].any() and (C == 4 or not want[128 + 2].any())
    x, p = torch.from_numpy(level).cuda(), torch.from_numpy(pos).cuda()
    buf, desc = _guarded((B * 128, K))
    pbuf, part = _guarded((B, C, 2), torch.float64)
    # two calls fill one buffer: images 0-1 at row 0, images 2-3 at row 256
    for _ in range(2):
        Fn.swd_descriptors(x[:2], p[:2], desc, 0, part)
        Fn.swd_descriptors(x[2:], p[2:], desc, 256, part)
        got = desc.cpu().numpy()
        assert got.tobytes() == want.tobytes()
        assert _bands_untouched(buf) and _bands_untouched(pbuf)
    sbuf, stats = _guarded((C, 2), torch.float64)
    Fn.swd_stats(part, out=stats)
    first = stats.clone()
    Fn.swd_stats(part, out=stats)
    assert torch.equal(first, stats) and _bands_untouched(sbuf)
    mean, std = R.channel_stats(want)
    got = stats.cpu().numpy()
    live = std > 0
    assert (np.abs(got[:, 0] - mean) <= 1e-12 * np.abs(mean)).all()
    assert (np.abs(got[live, 1] - 1.0 / std[live]) <= 1e-12 / std[live]).all()
    assert (got[~live, 1] == 0).all() and int((~live).sum()) == (1 if C == 4 else 0)


# ---------------------------------------------------------------- sort
def _sort_inputs(rng, n_seg, seg_len):
    n = n_seg * seg_len
    normal = rng.randn(n_seg, seg_len).astype(np.float32)
    inf = normal.copy()
    inf.reshape(-1)[rng.randint(0, n, size=max(2, n // 16))] = np.inf
    inf.reshape(-1)[rng.randint(0, n, size=max(2, n // 16))] = -np.inf
    inf[0, 0], inf[-1, -1] = np.inf, -np.inf
    asc = np.sort(normal, axis=1)
    return {"normal": normal, "equal": np.full((n_seg, seg_len), 0.25, np.float32), "ascending": asc,
            "descending": asc[:, ::-1].copy(), "duplicates": rng.randint(-3, 4, size=(n_seg, seg_len)).astype(np.float32),
            "inf": inf}


@pytest.mark.parametrize("n_seg", [1, 3, 16])
@pytest.mark.parametrize("tiles", [0, 0.5, 1, 2, 8], ids=["len2", "len64", "tile", "2tiles", "8tiles"])
def test_sort_segments(tiles, n_seg):
    tile = Fn.swd_sort_tile()
    seg_len = {0: 2, 0.5: 64}.get(tiles, int(tiles * tile))
    rng = np.random.RandomState(seg_len % 1000 + n_seg)
    for kind, x in _sort_inputs(rng, n_seg, seg_len).items():
        want = np.sort(x, axis=1)
        buf, data = _guarded((n_seg, seg_len))
        runs = []
        for _ in range(2):
            data.copy_(torch.from_numpy(x))
            Fn.swd_sort_segments(data, seg_len)
            runs.append(data.cpu().numpy())
            assert _bands_untouched(buf), kind
        assert np.array_equal(runs[0], want), kind
        assert runs[0].tobytes() == runs[1].tobytes(), kind


def test_sort_wrapper_rejects_what_it_cannot_run():
    x = torch.zeros(96, device="cuda")
    with pytest.raises(RuntimeError):
        Fn.swd_sort_segments(x, 96)
    with pytest.raises(RuntimeError):
        Fn.swd_sort_segments(x, 64)
    with pytest.raises(RuntimeError):
        Fn.swd_sort_segments(x.double(), 32)


# ---------------------------------------------------------------- L1
@pytest.mark.parametrize("n,n_out", [(5001, 3), (8192, 4), (1 << 20, 1)], ids=["scalar", "vector", "many-blocks"])
def test_l1(n, n_out):
    rng = np.random.RandomState(n % 97)
    a, b = rng.randn(n_out, n).astype(np.float32), rng.randn(n_out, n).astype(np.float32)
    want = np.abs(a.astype(np.float64) - b.astype(np.float64)).sum(axis=1)
    buf, out = _guarded((n_out,), torch.float64)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    Fn.swd_l1(ta, tb, n_out, out=out)
    first = out.clone()
    Fn.swd_l1(ta, tb, n_out, out=out)
    assert torch.equal(first, out) and _bands_untouched(buf)
    assert (np.abs(out.cpu().numpy() - want) <= 1e-12 * want).all()


# ---------------------------------------------------------------- projection and end to end
def test_projection_within_the_dot_product_bound(e2e):
    lv = e2e["levels"][0]
    da, db = lv["da"].astype(np.float32), lv["db"].astype(np.float32)
    ta, tb, dirs = torch.from_numpy(da).cuda(), torch.from_numpy(db).cuda(), torch.from_numpy(lv["dirs"]).cuda()
    stats = []
    for d in (da, db):                                   # the per-image partial rows, as the gather writes them
        d = d.astype(np.float64).reshape(d.shape[0] // 128, 128, 3, 49)
        part = np.stack([d.sum(axis=(1, 3)), (d * d).sum(axis=(1, 3))], axis=-1)
        stats.append(Fn.swd_stats(torch.from_numpy(np.ascontiguousarray(part)).cuda()))
    N, S_ = da.shape[0], lv["dirs"].shape[1]
    buf, out = _guarded((2 * S_, N))
    Fn.swd_project(ta, stats[0], dirs, out, tb, stats[1])
    first = out.clone()
    Fn.swd_project(ta, stats[0], dirs, out, tb, stats[1])
    assert torch.equal(first, out) and _bands_untouched(buf)
    got = _n64(out)
    for k, d in enumerate((da, db)):
        want = (R.normalise(d) @ lv["dirs"].astype(np.float64)).T
        bound = R.projection_bound(d, lv["dirs"])
        err = np.abs(got[k * S_:(k + 1) * S_] - want).max()
        print("projection set %d: worst error %.3g, bound %.3g" % (k, err, bound))
        assert err <= bound
    # one set alone writes the first S segments only
    buf, one = _guarded((S_, N))
    Fn.swd_project(ta, stats[0], dirs, one)
    assert torch.equal(one, first[:S_]) and _bands_untouched(buf)


def _device_metric(case, seed=1):
    B, side, C = case["real"].shape[0], case["real"].shape[1], case["real"].shape[3]
    plan = metrics.SwdPlan(side, C, B, B, seed, repeats=case["repeats"], n_dirs=case["n_dirs"])
    m = metrics.Swd(plan, "cuda")
    m.dirs = [torch.from_numpy(d).cuda() for d in case["dirs"]]
    m.pos = {"real": [torch.from_numpy(p).cuda() for p in case["pos_real"]],
             "fake": [torch.from_numpy(p).cuda() for p in case["pos_fake"]]}
    return m


def test_end_to_end_against_the_reference(e2e):
    """B = 4 images of 32 x 32 x 3 (N = 512), 2 repeats x 16 directions; real = one pass of the blur over uniform noise,
    fake = two.  The gate is the sum of the two sets' worst-case projection errors (swd_ref.distance_gate)."""
    m = _device_metric(e2e)
    real, fake = torch.from_numpy(e2e["real"]).cuda(), torch.from_numpy(e2e["fake"]).cuda()
    runs = []
    for _ in range(2):
        m.begin("real")
        m.add(real[:3])                                 # the images arrive in batches
        m.add(real[3:])
        m.real = m.finish()
        m.begin("fake")
        m.add(fake)
        runs.append(m.scores(m.finish()))
    assert runs[0] == runs[1]
    assert list(runs[0]) == ["swd_32", "swd_16", "swd_avg"]
    for side, lv in zip(e2e["sides"], e2e["levels"]):
        got = runs[0]["swd_%d" % side] / 1e3
        print("level %d: device %.9g reference %.9g gate %.3g" % (side, got, lv["dist"], lv["gate"]))
        assert lv["dist"] >= 100 * lv["gate"]
        assert abs(got - lv["dist"]) <= lv["gate"]
    assert abs(runs[0]["swd_avg"] - np.mean([runs[0]["swd_32"], runs[0]["swd_16"]])) < 1e-9


# ---------------------------------------------------------------- model level
def _model(tmp_path, tag, **kw):
    d = tmp_path / tag
    flags = dict(img_size=64, ch=8, batch_size=4, swd_images=8, log_dir=str(d / "logs"), checkpoint_dir=str(d / "ckpt"),
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


def test_model_scores_agree_with_the_reference_and_leave_the_run_alone(tmp_path):
    gan = _model(tmp_path, "swd")
    gan.train_step(gan.synthetic_batch())                  # the moving averages now differ from the live weights
    snap = _snapshot(gan)
    np_state = np.random.get_state()[1].copy()
    first = gan.swd()
    second = gan.swd()
    _same_state(gan, snap)
    assert np.array_equal(np.random.get_state()[1], np_state)
    assert list(first) == ["swd_64", "swd_32", "swd_16", "swd_avg"] and all(np.isfinite(v) for v in first.values())
    assert first == second
    # the same images, positions and directions through the float64 restatement
    plan = gan.monitor_plan("swd")
    assert plan.n_images == 8 and not plan.from_files
    z, cls_z = gan.monitor_fake_inputs(plan)
    fake = _n64(gan.generate(z, cls_z, ema=True))
    real = _n64(torch.cat(list(gan.monitor_real_batches(plan))))
    _same_state(gan, snap)
    pos_r, pos_f, dirs = plan.draw_positions("real"), plan.draw_positions("fake"), plan.draw_directions()
    lr, lf = R.laplacian_pyramid(real), R.laplacian_pyramid(fake)
    er, ef = R.laplacian_pyramid_bounds(real), R.laplacian_pyramid_bounds(fake)
    for i, side in enumerate(plan.sides):
        da, db = R.descriptors(lr[i], pos_r[i]), R.descriptors(lf[i], pos_f[i])
        want = 1e3 * R.distance(da, db, dirs[i], plan.repeats)
        gate = 1e3 * R.distance_gate(da, db, dirs[i], R.descriptors(er[i], pos_r[i]), R.descriptors(ef[i], pos_f[i]))
        print("swd_%d: device %.9g reference %.9g gate %.3g" % (side, first["swd_%d" % side], want, gate))
        assert abs(first["swd_%d" % side] - want) <= gate
    # --sample_ema both: the live weights under their own tags, and they differ from the moving averages'
    gan.generate_noema_samples = True
    both = gan.swd()
    assert list(both) == list(first) + ["swd_noema_64", "swd_noema_32", "swd_noema_16", "swd_noema_avg"]
    assert {k: both[k] for k in first} == first and both["swd_noema_64"] != both["swd_64"]
    _same_state(gan, snap)


def test_the_real_set_is_the_first_files_of_the_dataset_without_flips(tmp_path):
    from biggan_tensorflow_amd import data as D, utils
    root = tmp_path / "dataset"
    (root / "toy").mkdir(parents=True)
    rng = np.random.RandomState(9)
    for i in range(5):
        utils.write_png(rng.randint(0, 256, size=(70, 80, 3)).astype(np.uint8), str(root / "toy" / ("%02d.png" % i)))
    gan = _model(tmp_path, "files", dataset="toy")
    plan = gan.monitor_plan("swd", str(root))
    assert plan.from_files and plan.n_images == 4                   # min(8 asked, 5 files) rounded down to a power of two
    files = gan._dataset_files(str(root))
    assert [os.path.basename(f) for f in files] == ["%02d.png" % i for i in range(5)]
    real = torch.cat(list(gan.monitor_real_batches(plan, str(root))))
    want = np.stack([D.ImageData(64, 3, True, False).image_processing(f) for f in files[:4]])
    assert np.array_equal(real.cpu().numpy(), want)
    scores = gan.swd(str(root))
    assert list(scores) == ["swd_64", "swd_32", "swd_16", "swd_avg"] and all(np.isfinite(v) for v in scores.values())
    assert gan._monitors["swd"].plan.n_images == 4 and gan.swd(str(root)) == scores


def _train(tmp_path, tag, swd_freq, **kw):
    gan = _model(tmp_path, tag, swd_freq=swd_freq, **kw)
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
    """Three training steps with --swd_freq 1 and with --swd_freq 0 from the same seed, run once per precision."""
    tmp_path = tmp_path_factory.mktemp("pair_" + request.param)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        scored, seen = _train(tmp_path, "scored", 1, precision=request.param)
    lines = [l for l in out.getvalue().splitlines() if l.startswith("SWD: ")]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        plain, seen2 = _train(tmp_path, "plain", 0, precision=request.param)
    assert "SWD: " not in out.getvalue()
    return dict(scored=scored, plain=plain, seen=seen, seen2=seen2, lines=lines, tmp_path=tmp_path)


def test_training_state_with_the_score_is_bit_identical(run_pair):
    """Every parameter, moving average, Adam slot, u, statistic, the training generator and the counter (under bf16 the
    images that the metric reads are bf16)."""
    scored, plain = run_pair["scored"], run_pair["plain"]
    a, b = scored.state_tensors(), plain.state_tensors()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(k.endswith("/u") for k in a) and any(k.endswith("/Adam_1") for k in a)
    assert any(k.endswith("/ExponentialMovingAverage") for k in a)
    assert torch.equal(scored.gen.get_state(), plain.gen.get_state()) and scored.counter == plain.counter == 3
    assert plain._monitors.get("swd") is None and scored._monitors.get("swd") is not None


def test_training_losses_with_the_score_are_bit_identical(run_pair):
    """The losses of all three steps, bit for bit.  (This needs a loss that is the same from run to run in the first
    place: the regulariser's loss terms are added in a fixed order, tests/test_gpu_loss_order.py.)"""
    assert len(run_pair["seen"]) == 3
    assert run_pair["seen"] == run_pair["seen2"]


def test_training_logs_the_scores(run_pair):
    scored, lines = run_pair["scored"], run_pair["lines"]
    d = os.path.join(str(run_pair["tmp_path"] / "scored" / "logs"), scored.model_dir)
    ev = TR.read_events(os.path.join(d, os.listdir(d)[0]))
    tags = ["swd_64", "swd_32", "swd_16", "swd_avg"]
    swd_events = [e for e in ev[1:] if e["values"][0][0].startswith("swd")]
    # the losses of every step, and the scores at the same steps
    assert [e["step"] for e in swd_events] == [e["step"] for e in ev[1:] if "d_loss" in [t for t, _, _ in e["values"]]]
    assert len(swd_events) == 3 == len(lines)
    for e, line in zip(swd_events, lines):
        assert [t for t, _, _ in e["values"]] == tags and all(k == "scalar" and np.isfinite(v) for _, k, v in e["values"])
        assert [f.split(": ")[0] for f in line[len("SWD: "):].split(", ")] == tags
        avg = float(e["values"][3][2])
        assert abs(float(line.split("swd_avg: ")[1]) - avg) <= 1e-4 * max(1.0, abs(avg))
    # the weights moved between the events, the scores with them
    assert swd_events[0]["values"] != swd_events[2]["values"]


def test_phase_test_writes_the_scores(tmp_path):
    gan = _model(tmp_path, "phase", swd_freq=1, test_num=1)
    gan.test()
    path = os.path.join(str(tmp_path / "phase" / "results"), gan.model_dir, "swd.txt")
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert [r[0] for r in rows] == ["swd_64", "swd_32", "swd_16", "swd_avg"] and all(np.isfinite(float(r[1])) for r in rows)
