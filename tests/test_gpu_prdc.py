"""The precision / recall / density / coverage kernels (csrc/prdc.hip), the runner (metrics.Prdc) and the model's event
against the float64 restatement of tests/prdc_ref.py.  Every output sits between guard bands that must stay untouched;
every launch is repeated once and must be bit-identical.  Exact operands are compared bit for bit; generic ones within
the bound derived in nn_ref.py from the fp32 unit round-off, counts up to the pairs that the bound leaves undecided."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import functional as Fn, metrics, model, scope as S, utils
from tests import prdc_ref as R, trainlog_ref as TR
from tests.common import make_args

pytestmark = pytest.mark.gpu

BAND = 4096
FILL = {torch.float32: 12345.0, torch.int32: 12345, torch.int64: 12345}


def _guarded(n, dtype=torch.float32):
    """(buffer, view): the view of n elements sits between two bands of FILL."""
    buf = torch.full((BAND + n + BAND,), FILL[dtype], dtype=dtype, device="cuda")
    return buf, buf[BAND:BAND + n]


def _bands_untouched(buf):
    fill = FILL[buf.dtype]
    return bool((buf[:BAND] == fill).all()) and bool((buf[-BAND:] == fill).all())


def _bf16(a):
    """float64 array of bf16-representable values -> bf16 tensor on the device, exactly."""
    t = torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda().to(torch.bfloat16)
    assert np.array_equal(t.float().cpu().numpy().astype(np.float64), a)
    return t


def _radii_twice(x, k):
    buf, out = _guarded(len(x))
    tx = _bf16(x)
    Fn.prdc_radii(tx, k, out=out)
    first = out.clone()
    Fn.prdc_radii(tx, k, out=out)
    assert torch.equal(first, out) and _bands_untouched(buf)
    return first.cpu().numpy()


def _cover_twice(q, rad, s, count=True, dmin=True):
    """(count, dmin) as numpy, None for an output that was not asked for; ``rad`` float64 of fp32-representable values, a
    device tensor, or None (then no count)."""
    tq, ts = _bf16(q), _bf16(s)
    tr = rad if rad is None or torch.is_tensor(rad) else torch.from_numpy(np.asarray(rad, dtype=np.float32)).cuda()
    cb, cv = _guarded(len(s), torch.int32)
    db, dv = _guarded(len(s))
    Fn.prdc_cover(tq, tr, ts, count=cv if count else None, dmin=dv if dmin else None)
    first = (cb.clone(), db.clone())
    Fn.prdc_cover(tq, tr, ts, count=cv if count else None, dmin=dv if dmin else None)
    assert torch.equal(first[0], cb) and torch.equal(first[1], db) and _bands_untouched(cb) and _bands_untouched(db)
    if not count:
        assert bool((cv == FILL[torch.int32]).all())                    # an output that is NULL is not written
    if not dmin:
        assert bool((dv == FILL[torch.float32]).all())
    return (cv.cpu().numpy() if count else None), (dv.cpu().numpy() if dmin else None)


# ---------------------------------------------------------------- exact operands, bit for bit
@pytest.mark.parametrize("case", range(len(R.RADII_CASES)), ids=["%dx%d-k%d" % c for c in R.RADII_CASES])
def test_radii_of_exact_operands_bit_for_bit(case):
    N, D, k = R.RADII_CASES[case]
    x = R.radii_operands(case)
    got, want = _radii_twice(x, k), R.radii(x, k, R.distances_exact)
    assert np.array_equal(got.astype(np.float64), want)
    if N > 40:                                             # the three equal rows: neighbours of each other at distance 0
        for kk, zero in ((1, True), (2, True), (3, False)):
            r = _radii_twice(x, kk)
            assert np.array_equal(r.astype(np.float64), R.radii(x, kk, R.distances_exact))
            assert ((r[[5, 6, 40]] == 0.0).all()) == zero


@pytest.mark.parametrize("k", range(1, 9))
def test_every_k_on_one_set(k):
    x = R.radii_operands(2)[:, :64]                        # 17 rows: one past a block
    assert np.array_equal(_radii_twice(x, k).astype(np.float64), R.radii(x, k, R.distances_exact))


@pytest.mark.parametrize("case", range(len(R.COVER_CASES)), ids=["%dx%dx%d" % c for c in R.COVER_CASES])
def test_cover_of_exact_operands_bit_for_bit(case):
    Q, N, D = R.COVER_CASES[case]
    q, rad, s = R.cover_operands(case)
    want_count, want_dmin = R.cover(q, rad, s, R.distances_exact)
    count, dmin = _cover_twice(q, rad, s)
    assert np.array_equal(count.astype(np.int64), want_count)
    assert np.array_equal(dmin.astype(np.float64), want_dmin)
    d = R.distances_exact(q, s)
    assert d[0, N // 2] == rad[0] and count[N // 2] >= 1               # the pair at exactly its radius is counted
    if Q > 2:
        assert count.min() >= 1 and dmin[3] == 0.0                      # the query of radius +inf; the planted equal row
    if N > 7:
        assert dmin[7] > 0 and dmin[7] == d[:, 7].min()                 # the all-zero row: no padded query reaches it
    only_count, none = _cover_twice(q, rad, s, dmin=False)
    assert none is None and np.array_equal(only_count, count)
    none, only_dmin = _cover_twice(q, rad, s, count=False)
    assert none is None and np.array_equal(only_dmin, dmin)
    none, no_radius = Fn.prdc_cover(_bf16(q), None, _bf16(s), count=None)
    assert none is None and np.array_equal(no_radius.cpu().numpy(), dmin)


def test_reduce_counts_what_it_should():
    rng = np.random.default_rng(3)
    for M, N in ((1, 1), (255, 257), (5000, 3001)):
        count_f = rng.integers(0, 3, size=M).astype(np.int32) * rng.integers(0, 1 << 20, size=M).astype(np.int32)
        count_r = rng.integers(0, 3, size=N).astype(np.int32)
        dmin_r = rng.integers(0, 8, size=N).astype(np.float32)
        radius_r = rng.integers(0, 8, size=N).astype(np.float32)
        radius_r[0] = np.inf
        buf, out = _guarded(4, torch.int64)
        args = [torch.from_numpy(a).cuda() for a in (count_f, count_r, dmin_r, radius_r)]
        Fn.prdc_reduce(*args, out=out)
        first = out.clone()
        Fn.prdc_reduce(*args, out=out)
        assert torch.equal(first, out) and _bands_untouched(buf)
        assert first.cpu().tolist() == R.reduce4(count_f, count_r, dmin_r, radius_r)
    big = torch.full((3000,), 2 ** 31 - 1, dtype=torch.int32, device="cuda")          # the sum is an int64
    got = Fn.prdc_reduce(big, big[:5], torch.zeros(5, device="cuda"), torch.zeros(5, device="cuda")).cpu().tolist()
    assert got == [3000, 3000 * (2 ** 31 - 1), 5, 5]


# ---------------------------------------------------------------- symmetry
def test_distances_are_symmetric_bit_for_bit():
    rng = np.random.default_rng(77)
    x, y = R.bf16_round(rng.uniform(-1, 1, size=(20, 576))), R.bf16_round(rng.uniform(-1, 1, size=(20, 576)))
    want = R.distances(x, y)
    xy = np.stack([_cover_twice(x[i:i + 1], None, y, count=False)[1] for i in range(20)])          # [i, n] = d(x_i, y_n)
    yx = np.stack([_cover_twice(y[n:n + 1], None, x, count=False)[1] for n in range(20)])          # [n, i] = d(y_n, x_i)
    assert np.array_equal(xy, yx.T)
    err = np.abs(xy.astype(np.float64) - want)
    print("symmetry: worst error / bound %.3f" % (err / (R.gamma(576) * want)).max())
    assert (err <= R.gamma(576) * want).all()


# ---------------------------------------------------------------- generic operands against float64
@functools.lru_cache(maxsize=None)
def _generic(case):
    """The case, its float64 radii and the bands of its two cover passes: computed once, read by the tests below."""
    real, fake, k = R.generic_operands(case)
    rr, rf = R.radii(real, k), R.radii(fake, k)
    return dict(real=real, fake=fake, k=k, rr=rr, rf=rf, on_fake=R.cover_bands(real, rr, fake),
                on_real=R.cover_bands(fake, rf, real), bands=R.score_bands(real, fake, k))


@pytest.mark.parametrize("case", range(len(R.GENERIC_CASES)), ids=["%dx%dx%d-k%d" % c for c in R.GENERIC_CASES])
def test_generic_operands_within_the_bound(case):
    """Measured on an MI355X, worst error / bound: see DESIGN.md ("precision / recall / density / coverage")."""
    g = _generic(case)
    D, k = g["real"].shape[1], g["k"]
    assert g["on_fake"][3] <= R.UNDECIDED_SHARE and g["on_real"][3] <= R.UNDECIDED_SHARE          # the condition
    dev = {}
    for name, x, want in (("real", g["real"], g["rr"]), ("fake", g["fake"], g["rf"])):
        got = _radii_twice(x, k)
        err = np.abs(got.astype(np.float64) - want)
        print("case %d radii of %s: worst error / bound %.3f" % (case, name, (err / (R.gamma(D) * want)).max()))
        assert (err <= R.gamma(D) * want).all()
        dev[name] = torch.from_numpy(got).cuda()
    for tag, q, rad, s, ref in (("q=real", g["real"], dev["real"], g["fake"], g["on_fake"]),
                                ("q=fake", g["fake"], dev["fake"], g["real"], g["on_real"])):
        sure, open_, dmin64, _ = ref
        count, dmin = _cover_twice(q, rad, s)
        err = np.abs(dmin.astype(np.float64) - dmin64)
        print("case %d cover %s: %d undecided pairs, dmin worst error / bound %.3f"
              % (case, tag, open_.sum(), (err / (R.gamma(D) * dmin64)).max()))
        assert (count >= sure).all() and (count <= sure + open_).all()
        assert (err <= R.gamma(D) * dmin64).all()


@pytest.mark.parametrize("case", range(len(R.GENERIC_CASES)), ids=["%dx%dx%d-k%d" % c for c in R.GENERIC_CASES])
def test_composed_scores_equal_the_reference_up_to_undecided_rows(case):
    g = _generic(case)
    N, M, D, k = R.GENERIC_CASES[case]
    plan = metrics.PrdcPlan(8, 3, 64, pr_images=M, pr_k=k, pr_size=8, n_files=N)       # k; the sets bring their sizes
    runs = []
    for _ in range(2):
        m = metrics.Prdc(plan, "cuda")
        sets = {}
        for name, x in (("real", g["real"]), ("fake", g["fake"])):
            desc = _bf16(x)
            sets[name] = {"desc": desc, "radius": Fn.prdc_radii(desc, k), "n": len(x)}
        runs.append(m.scores(sets["real"], sets["fake"]))
    assert runs[0] == runs[1] and list(runs[0]) == ["pr_precision", "pr_recall", "pr_density", "pr_coverage"]
    print("case %d: device %s\nreference bands %s" % (case, runs[0], g["bands"]))
    for name, (lo, hi) in g["bands"].items():
        assert lo <= runs[0]["pr_" + name] <= hi, name


# ---------------------------------------------------------------- rejections
def test_wrappers_reject_what_they_cannot_run():
    x = torch.zeros(20, 192, device="cuda", dtype=torch.bfloat16)
    rad = torch.zeros(20, device="cuda")
    flat = torch.zeros(20 * 192 + 8, device="cuda", dtype=torch.bfloat16)
    off = flat[1:1 + 20 * 192].view(20, 192)                                 # contiguous, 2 bytes off a 16-byte boundary
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        Fn.prdc_radii(x[:, :96].contiguous(), 3)                             # D is no multiple of 64
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x[:, :96].contiguous(), rad, x[:, :96].contiguous())
    for k in (0, 9):
        with pytest.raises(RuntimeError):
            Fn.prdc_radii(x, k)
    with pytest.raises(RuntimeError):
        Fn.prdc_radii(x[:3], 3)                                              # N <= k
    with pytest.raises(RuntimeError):
        Fn.prdc_radii(x[:8], 8)
    with pytest.raises(RuntimeError):
        Fn.prdc_radii(off, 3)
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(off, rad, x)
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x, rad, off)
    with pytest.raises(RuntimeError):
        Fn.prdc_radii(x.float(), 3)                                          # fp32 rows
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x.float(), rad, x)
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x, rad, x.float())
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x, rad, x, count=None, dmin=None)                      # both outputs NULL
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x, None, x)                                            # a count without radii
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x, rad[:5], x)
    with pytest.raises(RuntimeError):
        Fn.prdc_cover(x, rad, x[:, :128])                                    # not contiguous, another D
    with pytest.raises(RuntimeError):
        Fn.prdc_reduce(torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda", dtype=torch.int32), rad[:4], rad[:4])


# ---------------------------------------------------------------- the runner
def test_runner_in_ragged_batches():
    """16 real and 16 generated images of 16 px, box 2: batches of 5, 5, 6 and one batch of 20 (padding dropped) give
    the same set; the scores are the reference's on the packed descriptors."""
    rng = np.random.default_rng(11)
    plan = metrics.PrdcPlan(16, 3, 8, pr_images=16, pr_k=2, pr_size=8)
    assert (plan.D, plan.f, plan.N, plan.M) == (192, 2, 16, 16)
    imgs = torch.from_numpy(rng.uniform(-1, 1, size=(20, 16, 16, 3)).astype(np.float32)).cuda()
    fakes = torch.from_numpy(np.clip(imgs[:16].cpu().numpy() + rng.normal(0, 0.3, size=(16, 16, 16, 3)), -1, 1)
                             .astype(np.float32)).cuda()
    m = metrics.Prdc(plan, "cuda")
    m.begin()
    for lo, hi in ((0, 5), (5, 10), (10, 16)):
        m.add(imgs[lo:hi])
    a = m.finish()
    m.begin()
    m.add(imgs)
    b = m.finish()
    assert torch.equal(a["desc"], b["desc"]) and torch.equal(a["radius"], b["radius"]) and a["n"] == 16
    assert torch.equal(a["desc"], Fn.nn_pack(imgs[:16], 2))
    m.begin()
    m.add(fakes.to(torch.bfloat16))
    f = m.finish()
    m.begin()
    m.add(imgs[:3])
    with pytest.raises(RuntimeError):
        m.finish()
    with pytest.raises(ValueError):
        m.add(imgs[:, :8, :8])
    got = m.scores(a, f)
    bands = R.score_bands(a["desc"].float().cpu().numpy().astype(np.float64),
                          f["desc"].float().cpu().numpy().astype(np.float64), 2)
    print("runner: %s, bands %s" % (got, bands))
    assert all(lo <= got["pr_" + name] <= hi for name, (lo, hi) in bands.items())
    assert m.scores(a, a) == {"pr_precision": 1.0, "pr_recall": 1.0, "pr_density": 1.5, "pr_coverage": 1.0}


# ---------------------------------------------------------------- model level
def _model(tmp_path, tag, **kw):
    d = tmp_path / tag
    flags = dict(img_size=64, ch=8, batch_size=4, pr_images=16, pr_k=3, log_dir=str(d / "logs"),
                 checkpoint_dir=str(d / "ckpt"), sample_dir=str(d / "samples"), result_dir=str(d / "results"))
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


def _within_bands(scores, suffix, real, fake, k):
    as64 = lambda t: t.float().cpu().numpy().astype(np.float64)         # noqa: E731
    bands = R.score_bands(as64(real["desc"]), as64(fake["desc"]), k)
    print("device %s\nreference bands %s" % (scores, bands))
    return all(lo <= scores["pr_" + name + suffix] <= hi for name, (lo, hi) in bands.items())


KEYS = ["pr_precision", "pr_recall", "pr_density", "pr_coverage"]


def test_model_scores_agree_with_the_reference_and_leave_the_run_alone(tmp_path):
    gan = _model(tmp_path, "prdc")
    gan.train_step(gan.synthetic_batch())                  # the moving averages now differ from the live weights
    snap = _snapshot(gan)
    np_state = np.random.get_state()[1].copy()
    first, runner, sets = gan.prdc(details=True)
    second = gan.prdc()
    _same_state(gan, snap)
    assert np.array_equal(np.random.get_state()[1], np_state)
    assert list(first) == KEYS and second == first and list(sets) == ["pr"]
    plan = runner.plan
    assert (plan.N, plan.M, plan.k, plan.D, plan.f) == (16, 16, 3, 64 * 64 * 3, 1) and not plan.from_files
    real = runner.real
    assert real["n"] == 16 and tuple(real["desc"].shape) == (16, plan.D) and tuple(real["radius"].shape) == (16,)
    # the descriptors are those of the plan's draws through the generator and the pack
    z, cls_z = gan.monitor_fake_inputs(plan)
    assert z.shape[0] == 16 and cls_z is None
    assert torch.equal(sets["pr"]["desc"], Fn.nn_pack(gan.generate(z, cls_z, ema=True), plan.f))
    assert torch.equal(real["desc"], Fn.nn_pack(torch.cat(list(gan.monitor_real_batches(plan))), plan.f))
    assert _within_bands(first, "", real, sets["pr"], 3)
    # --sample_ema both: the live weights under their own tags
    gan.generate_noema_samples = True
    both, _, sets = gan.prdc(details=True)
    assert list(both) == KEYS + [k + "_noema" for k in KEYS] and list(sets) == ["pr", "pr_noema"]
    assert all(both[k] == first[k] for k in first)
    assert torch.equal(sets["pr_noema"]["desc"], Fn.nn_pack(gan.generate(z, cls_z, ema=False), plan.f))
    assert _within_bands(both, "_noema", real, sets["pr_noema"], 3)
    assert gan._monitors["prdc"].real is real                 # the real set is measured once
    _same_state(gan, snap)


def test_the_real_set_is_the_first_files_without_flips(tmp_path):
    from biggan_tensorflow_amd import data as D
    root = tmp_path / "dataset"
    (root / "toy").mkdir(parents=True)
    rng = np.random.RandomState(9)
    for i in range(9):
        utils.write_png(rng.randint(0, 256, size=(70, 80, 3)).astype(np.uint8), str(root / "toy" / ("%02d.png" % i)))
    gan = _model(tmp_path, "files", dataset="toy", pr_size=32)
    plan = gan.monitor_plan("prdc", str(root))
    assert plan.from_files and (plan.N, plan.M, plan.f, plan.D) == (9, 16, 2, 32 * 32 * 3)
    files = gan._dataset_files(str(root))
    want = np.stack([D.ImageData(64, 3, True, False).image_processing(f) for f in files[:9]])
    scores, runner, sets = gan.prdc(str(root), details=True)
    assert torch.equal(runner.real["desc"], Fn.nn_pack(torch.from_numpy(want).cuda(), 2))
    assert list(scores) == KEYS and _within_bands(scores, "", runner.real, sets["pr"], 3)


def _train(tmp_path, tag, pr_freq, **kw):
    gan = _model(tmp_path, tag, pr_freq=pr_freq, **kw)
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
    """Three training steps with --pr_freq 1 and with --pr_freq 0 from the same seed, run once per precision."""
    tmp_path = tmp_path_factory.mktemp("pair_" + request.param)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        scored, seen = _train(tmp_path, "scored", 1, precision=request.param)
    lines = [l for l in out.getvalue().splitlines() if l.startswith("PRDC: ")]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        plain, seen2 = _train(tmp_path, "plain", 0, precision=request.param)
    assert "PRDC: " not in out.getvalue()
    return dict(scored=scored, plain=plain, seen=seen, seen2=seen2, lines=lines, tmp_path=tmp_path)


def test_training_state_and_losses_with_the_check_are_bit_identical(run_pair):
    scored, plain = run_pair["scored"], run_pair["plain"]
    a, b = scored.state_tensors(), plain.state_tensors()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(k.endswith("/u") for k in a) and any(k.endswith("/Adam_1") for k in a)
    assert torch.equal(scored.gen.get_state(), plain.gen.get_state()) and scored.counter == plain.counter == 3
    assert plain._monitors.get("prdc") is None and scored._monitors.get("prdc") is not None
    assert len(run_pair["seen"]) == 3 and run_pair["seen"] == run_pair["seen2"]


def test_training_logs_the_scores(run_pair):
    scored, lines = run_pair["scored"], run_pair["lines"]
    d = os.path.join(str(run_pair["tmp_path"] / "scored" / "logs"), scored.model_dir)
    ev = TR.read_events(os.path.join(d, os.listdir(d)[0]))
    events = [e for e in ev[1:] if e["values"][0][0].startswith("pr_")]
    assert [e["step"] for e in events] == [e["step"] for e in ev[1:] if "d_loss" in [t for t, _, _ in e["values"]]]
    assert len(events) == 3 == len(lines)
    for e, line in zip(events, lines):
        assert [t for t, _, _ in e["values"]] == KEYS
        assert all(kind == "scalar" and np.isfinite(v) and 0.0 <= v <= 16.0 / 3 for _, kind, v in e["values"])
        assert [f.split(": ")[0] for f in line[len("PRDC: "):].split(", ")] == KEYS
        assert abs(float(line.split("pr_density: ")[1].split(",")[0]) - float(e["values"][2][2])) <= 1e-4


def test_phase_test_writes_the_scores(tmp_path):
    gan = _model(tmp_path, "phase", pr_freq=1, test_num=1)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        gan.test()
    folder = os.path.join(str(tmp_path / "phase" / "results"), gan.model_dir)
    rows = [l.split("\t") for l in open(os.path.join(folder, "prdc.txt")).read().splitlines()]
    assert [r[0] for r in rows] == KEYS + ["k", "N", "M", "D"]
    assert [int(r[1]) for r in rows[4:]] == [3, 16, 16, 64 * 64 * 3]
    line = [l for l in out.getvalue().splitlines() if l.startswith("PRDC: ")]
    assert len(line) == 1
    for r in rows[:4]:
        assert abs(float(r[1]) - float(line[0].split(r[0] + ": ")[1].split(",")[0])) <= 1e-4
