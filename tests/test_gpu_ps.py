"""The power-spectrum kernels (csrc/powerspec.hip) and the frequency check on the device against the float64 restatement of
tests/ps_ref.py.  Every output sits between guard bands that must stay untouched; every launch is repeated once and must
be bit-identical.  Gates: per coefficient the bound that ps_ref.py derives from the fp32 unit round-off, per profile bin
16 x the distance of the NumPy fp32 restatement from float64 that ps_ref.py records; nothing is fitted to the device."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import functional as Fn, metrics, model, scope as S
from tests import ps_ref as R, trainlog_ref as TR
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


def _on_device(k, dtype="fp32"):
    x = torch.tensor(k["x"]).cuda().to(torch.float32 if dtype == "fp32" else torch.bfloat16)
    assert np.array_equal(x.float().cpu().numpy(), k["x"])               # (the bf16 cases hold bf16-exact values)
    return x


def _run(x, with_sum=True):
    """Both launches, each twice, between guard bands: (power, profiles, sum2d) as float64 / fp32 NumPy arrays."""
    n, S_, _, C = x.shape
    W, nb = S_ // 2 + 1, R.n_bins(S_)
    wbuf, ws = _guarded((Fn.ps_workspace(n, S_, "cuda").numel(),), torch.float64)
    pbuf, power = _guarded((n, S_, W))
    Fn.ps_power(x, power, ws)
    first = power.clone()
    power.fill_(FILL)
    Fn.ps_power(x, power, ws)
    assert torch.equal(first, power) and not bool((power == FILL).any())
    fbuf, prof = _guarded((n, nb), torch.float64)
    sbuf, sum2d = _guarded((S_, W), torch.float64)
    sum2d.zero_()
    Fn.ps_profile(power, prof, sum2d if with_sum else None)
    first_prof, first_sum = prof.clone(), sum2d.clone()
    prof.fill_(FILL)
    sum2d.zero_()
    Fn.ps_profile(power, prof, sum2d if with_sum else None)
    assert torch.equal(first_prof, prof) and torch.equal(first_sum, sum2d) and not bool((prof == FILL).any())
    assert all(_bands_untouched(b) for b in (wbuf, pbuf, fbuf, sbuf))
    return power.cpu().numpy(), prof.cpu().numpy(), sum2d.cpu().numpy()


def _check(label, got, ref):
    power, prof, sum2d = got
    frac = R.check_power(power, ref)
    rel, pfrac = R.check_profiles(prof, ref)
    print("%s: worst |P^ - P| / bound %.3g; profile: worst relative gap %.3g (gate %.3g), worst gap / bound %.3g"
          % (label, frac, rel, R.PROFILE_GATE, pfrac))
    assert frac <= 1.0, label
    assert rel <= R.PROFILE_GATE and pfrac <= 1.0, label
    # the 2-D sum: the fp64 sum of the fp32 powers in image order
    want = np.zeros(power.shape[1:], dtype=np.float64)
    for p in power:
        want += p.astype(np.float64)
    assert np.array_equal(sum2d, want), label
    return frac, rel


# ---------------------------------------------------------------- the launches against float64
@pytest.mark.parametrize("S_,n,C", R.STRUCTURE_CASES, ids=["%dpx" % c[0] for c in R.STRUCTURE_CASES])
def test_every_side_against_the_reference(S_, n, C):
    """Radix-4 passes plus a leftover radix-2 pass for odd log2 S; 1024 / S row pairs a block; 512 has the largest LDS
    footprint and four columns a block."""
    k = R.case(S_, n, C)
    _check("S=%d" % S_, _run(_on_device(k)), k["ref"])


@pytest.mark.parametrize("S_,n,C", R.CONTENT_CASES, ids=["%dpx-n%d-C%d" % c for c in R.CONTENT_CASES])
def test_content_kinds_channels_and_dtypes(S_, n, C):
    """White, 1/f and DC-heavy inputs; odd image counts (a partly filled block at 16 px); 1, 3 and 4 channels; fp32 and bf16."""
    for dtype in R.DTYPES:
        for kind in R.KINDS:
            k = R.case(S_, n, C, kind, dtype)
            _check("S=%d n=%d C=%d %s %s" % (S_, n, C, dtype, kind), _run(_on_device(k, dtype)), k["ref"])
    if C == 4:                                                           # alpha is ignored
        k = R.case(S_, n, C)
        x = _on_device(k)
        y = x.clone()
        y[..., 3] = 0.25
        assert torch.equal(Fn.ps_power(x), Fn.ps_power(y))


def test_bin_boundaries():
    """Single cosines at the eight frequencies whose radius lies nearest a half-integer: each lands in its own bin."""
    b = R.boundary_case()
    power, prof, sum2d = got = _run(_on_device(b))
    _check("boundary", got, b["ref"])
    counts = R.counts(R.BOUNDARY_SIDE)
    for i, (ky, kx) in enumerate(b["freqs"]):
        r = R.bin_of(ky, kx)
        assert abs(power[i, ky % R.BOUNDARY_SIDE, kx] - 0.25) < 1e-6
        assert abs(prof[i, r] * counts[r] - 0.5) < 1e-6 and np.delete(prof[i], r).max() < 1e-12, (ky, kx, r)


def test_sum2d_accumulates_in_image_order_and_may_be_absent():
    k = R.case(64, 5, 3, "pink")
    x = _on_device(k)
    power = Fn.ps_power(x)
    whole = torch.zeros(64, 33, dtype=torch.float64, device="cuda")
    prof_whole = Fn.ps_profile(power, None, whole)
    parts = torch.zeros(64, 33, dtype=torch.float64, device="cuda")
    prof_a = Fn.ps_profile(power[:2], None, parts)
    prof_b = Fn.ps_profile(power[2:], None, parts)                       # added to what the first call left
    assert torch.equal(parts, whole) and torch.equal(torch.cat([prof_a, prof_b]), prof_whole)
    assert torch.equal(Fn.ps_profile(power, None, None), prof_whole)     # no 2-D sum
    again = torch.zeros(64, 33, dtype=torch.float64, device="cuda")
    assert torch.equal(Fn.ps_profile(Fn.ps_power(x), None, again), prof_whole) and torch.equal(again, whole)
    # a batch is the images one at a time
    single = torch.cat([Fn.ps_power(x[i:i + 1]) for i in range(5)])
    assert torch.equal(single, power)
    got = _run(x, with_sum=False)
    assert (got[2] == 0).all()


def test_wrappers_reject_what_they_cannot_run():
    x = torch.zeros(2, 32, 32, 3, device="cuda")
    with pytest.raises(RuntimeError):
        Fn.ps_power(x.half())
    with pytest.raises(RuntimeError):
        Fn.ps_power(x.cpu())                                             # no CPU fallback
    with pytest.raises(RuntimeError):
        Fn.ps_power(torch.zeros(2, 48, 48, 3, device="cuda"), torch.zeros(2, 48, 25, device="cuda"),
                    torch.zeros(1 << 16, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError):
        Fn.ps_power(torch.zeros(2, 32, 32, 2, device="cuda"))
    with pytest.raises(RuntimeError):
        Fn.ps_power(x, torch.zeros(2, 32, 16, device="cuda"))
    with pytest.raises(RuntimeError):
        Fn.ps_power(x, None, Fn.ps_workspace(1, 32, "cuda"))             # workspace too small
    with pytest.raises(RuntimeError):
        Fn.ps_workspace(2, 48, "cuda")
    with pytest.raises(RuntimeError):
        Fn.ps_profile(torch.zeros(2, 32, 17, device="cuda"), torch.zeros(2, 23, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError):
        Fn.ps_profile(torch.zeros(2, 32, 16, device="cuda"))


# ---------------------------------------------------------------- metrics.PowerSpectrum end to end
def test_runner_in_ragged_batches():
    k = R.case(64, 5, 3, "pink")
    x = _on_device(k)
    plan = metrics.PowerSpectrumPlan(64, 3, 4, 5, 1)
    m = metrics.PowerSpectrum(plan, "cuda")
    runs = []
    for size in (2, 3, 5):
        m.begin()
        for lo in range(0, 5, size):
            m.add(x[lo:lo + size])
        m.add(x[:2])                                                     # padding past n_images is dropped
        runs.append(m.finish())
    for r in runs[1:]:
        assert r["profile"].tobytes() == runs[0]["profile"].tobytes() and r["sum2d"].tobytes() == runs[0]["sum2d"].tobytes()
    want = R.set_profile(k["ref"]["profiles"])
    assert np.abs(runs[0]["profile"] / want - 1.0).max() <= R.PROFILE_GATE
    assert np.abs(runs[0]["sum2d"] - k["ref"]["power"].sum(axis=0)).max() <= R.power_bound(k["ref"]).sum(axis=0).max()
    # a blurred and a checkerboarded copy against the set itself
    real = runs[0]
    xs = k["x"].astype(np.float64)
    blur = 0.1 * xs + 0.9 * 0.25 * (xs + np.roll(xs, 1, 1) + np.roll(xs, 1, 2) + np.roll(np.roll(xs, 1, 1), 1, 2))
    yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    board = xs + 0.05 * np.where((xx + yy) % 2 == 0, 1.0, -1.0)[None, :, :, None]
    for name, fake in (("blur", blur), ("board", board)):
        f32 = fake.astype(np.float32)
        m.begin()
        m.add(torch.from_numpy(f32).cuda())
        got = m.scores(real, m.finish())
        want = R.image_scores(k["x"], f32)
        print(name, got, want)
        assert got["ps_peak_at"] == want["ps_peak_at"]
        assert all(abs(got[key] - want[key]) <= 2 * np.log10(1 + R.PROFILE_GATE) for key in got)
        assert (got["ps_hf"] < -0.3) if name == "blur" else (got["ps_peak"] > 1.0 and got["ps_peak_at"] == 45 / 64.0)
    assert m.scores(real, real) == {"ps_dist": 0.0, "ps_hf": 0.0, "ps_peak": 0.0, "ps_peak_at": 0.25}


# ---------------------------------------------------------------- model level
def _model(tmp_path, tag, **kw):
    d = tmp_path / tag
    flags = dict(img_size=64, ch=8, batch_size=4, ps_images=8, log_dir=str(d / "logs"), checkpoint_dir=str(d / "ckpt"),
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


def _reference_with_its_own_gate(real, fake):
    """float64 scores of two image sets and, per score, 16 x the distance of the fp32 restatement from them on these very
    images (at least 16 u): the rule of ps_ref.py applied to inputs that are not among its cases."""
    S_ = real.shape[1]
    want = R.image_scores(real, fake)
    emul = R.scores(R.set_profile(R.emulate(real)[1]), R.set_profile(R.emulate(fake)[1]), S_)
    return want, {k: 16 * max(abs(emul[k] - want[k]), R.U32) for k in want}


def test_model_scores_agree_with_the_reference_and_leave_the_run_alone(tmp_path):
    gan = _model(tmp_path, "ps")
    gan.train_step(gan.synthetic_batch())                  # the moving averages now differ from the live weights
    snap = _snapshot(gan)
    np_state = np.random.get_state()[1].copy()
    first = gan.power_spectrum()
    second = gan.power_spectrum()
    _same_state(gan, snap)
    assert np.array_equal(np.random.get_state()[1], np_state)
    assert list(first) == ["ps_dist", "ps_hf", "ps_peak", "ps_peak_at"] and second == first
    # the same images through the float64 restatement: 8 images in batches of 4
    plan = gan.monitor_plan("ps")
    assert plan.n_images == 8 and not plan.from_files and plan.n_real == 8
    z, cls_z = gan.monitor_fake_inputs(plan)
    assert z.shape[0] == 8 and cls_z is None
    fake = gan.generate(z, cls_z, ema=True).float().cpu().numpy()
    real = torch.cat(list(gan.monitor_real_batches(plan))).cpu().numpy()
    want, gate = _reference_with_its_own_gate(real, fake)
    print("device %s\nreference %s\ngates %s" % (first, want, gate))
    assert first["ps_peak_at"] == want["ps_peak_at"]
    assert all(abs(first[k] - want[k]) <= gate[k] for k in want)
    _same_state(gan, snap)
    # --sample_ema both: the live weights under their own tags
    gan.generate_noema_samples = True
    both = gan.power_spectrum()
    assert list(both) == ["ps_dist", "ps_hf", "ps_peak", "ps_peak_at", "ps_dist_noema", "ps_hf_noema", "ps_peak_noema",
                          "ps_peak_at_noema"]
    assert all(both[k] == first[k] for k in first)
    live = gan.generate(z, cls_z, ema=False).float().cpu().numpy()
    want, gate = _reference_with_its_own_gate(real, live)
    assert all(abs(both[k + "_noema"] - want[k]) <= gate[k] for k in want)
    _same_state(gan, snap)


def test_the_real_set_is_the_first_files_without_flips(tmp_path):
    from biggan_tensorflow_amd import data as D, utils
    root = tmp_path / "dataset"
    (root / "toy").mkdir(parents=True)
    rng = np.random.RandomState(9)
    for i in range(5):
        utils.write_png(rng.randint(0, 256, size=(70, 80, 3)).astype(np.uint8), str(root / "toy" / ("%02d.png" % i)))
    gan = _model(tmp_path, "files", dataset="toy")
    plan = gan.monitor_plan("ps", str(root))
    assert plan.from_files and plan.n_real == 5 and plan.n_images == 8
    files = gan._dataset_files(str(root))
    real = torch.cat(list(gan.monitor_real_batches(plan, str(root))))
    want = np.stack([D.ImageData(64, 3, True, False).image_processing(f) for f in files[:5]])
    assert np.array_equal(real.cpu().numpy(), want)
    scores = gan.power_spectrum(str(root))
    assert gan._monitors["ps"].real["n"] == 5
    ref = R.reference(want)
    assert np.abs(gan._monitors["ps"].real["profile"] / R.set_profile(ref["profiles"]) - 1.0)[R.significant(ref).all(axis=0)].max() \
        <= R.PROFILE_GATE
    assert set(scores) == {"ps_dist", "ps_hf", "ps_peak", "ps_peak_at"}


def _train(tmp_path, tag, ps_freq, **kw):
    gan = _model(tmp_path, tag, ps_freq=ps_freq, **kw)
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
    """Three training steps with --ps_freq 1 and with --ps_freq 0 from the same seed, run once per precision."""
    tmp_path = tmp_path_factory.mktemp("pair_" + request.param)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        scored, seen = _train(tmp_path, "scored", 1, precision=request.param)
    lines = [l for l in out.getvalue().splitlines() if l.startswith("PS: ")]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        plain, seen2 = _train(tmp_path, "plain", 0, precision=request.param)
    assert "PS: " not in out.getvalue()
    return dict(scored=scored, plain=plain, seen=seen, seen2=seen2, lines=lines, tmp_path=tmp_path)


def test_training_state_and_losses_with_the_check_are_bit_identical(run_pair):
    scored, plain = run_pair["scored"], run_pair["plain"]
    a, b = scored.state_tensors(), plain.state_tensors()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(k.endswith("/u") for k in a) and any(k.endswith("/Adam_1") for k in a)
    assert torch.equal(scored.gen.get_state(), plain.gen.get_state()) and scored.counter == plain.counter == 3
    assert plain._monitors.get("ps") is None and scored._monitors.get("ps") is not None
    assert len(run_pair["seen"]) == 3 and run_pair["seen"] == run_pair["seen2"]


def test_training_logs_the_scores(run_pair):
    scored, lines = run_pair["scored"], run_pair["lines"]
    d = os.path.join(str(run_pair["tmp_path"] / "scored" / "logs"), scored.model_dir)
    ev = TR.read_events(os.path.join(d, os.listdir(d)[0]))
    events = [e for e in ev[1:] if e["values"][0][0].startswith("ps_")]
    assert [e["step"] for e in events] == [e["step"] for e in ev[1:] if "d_loss" in [t for t, _, _ in e["values"]]]
    assert len(events) == 3 == len(lines)
    for e, line in zip(events, lines):
        assert [t for t, _, _ in e["values"]] == ["ps_dist", "ps_hf", "ps_peak", "ps_peak_at"]
        assert all(kind == "scalar" and np.isfinite(v) for _, kind, v in e["values"])
        assert [f.split(": ")[0] for f in line[len("PS: "):].split(", ")] == [t for t, _, _ in e["values"]]
        assert abs(float(line.split("ps_dist: ")[1].split(",")[0]) - float(e["values"][0][2])) <= 1e-4
    assert events[0]["values"][0] != events[2]["values"][0]           # the weights moved between the events


def test_phase_test_writes_the_table_and_the_image(tmp_path):
    gan = _model(tmp_path, "phase", ps_freq=1, test_num=1)
    paths = gan.test()
    folder = os.path.join(str(tmp_path / "phase" / "results"), gan.model_dir)
    lines = open(os.path.join(folder, "ps.txt")).read().splitlines()
    assert lines[0] == "# r\tr/S\tn_r\tL_real\tL_fake\tD_fake" and len(lines) == 1 + R.n_bins(64)
    rows = [l.split("\t") for l in lines[1:]]
    assert [int(r[2]) for r in rows] == R.counts(64).tolist()
    assert all(abs(float(r[5]) - (float(r[4]) - float(r[3]))) < 2e-6 for r in rows)
    png = os.path.join(folder, "ps.png")
    assert png in paths and open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
