"""The nearest-training-image kernels (csrc/nearest.hip) and the search on the device against the float64 restatement of
tests/nn_ref.py.  Every output sits between guard bands that must stay untouched; every launch is repeated once and must
be bit-identical.  The distance bound is derived in nn_ref.py from the fp32 unit round-off; the selection and the packing
of exact inputs are compared bit for bit."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data as D, functional as Fn, model, neighbours as NB, scope as S, utils
from tests import nn_ref as R, trainlog_ref as TR
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


def _bf16(a):
    """float64 array of bf16-representable values -> bf16 tensor on the device, exactly."""
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda().to(torch.bfloat16)


def _distances_twice(q, s):
    buf, out = _guarded((len(q), len(s)))
    tq, ts = _bf16(q), _bf16(s)
    Fn.nn_distances(tq, ts, out=out)
    first = out.clone()
    Fn.nn_distances(tq, ts, out=out)
    assert torch.equal(first, out) and _bands_untouched(buf)
    return first.cpu().numpy()


# ---------------------------------------------------------------- distances
@pytest.mark.parametrize("Q,N,D", R.SHAPES)
def test_distances_within_the_bound(Q, N, D):
    q, s = R.random_operands(np.random.RandomState(Q + N + D), Q, N, D)
    got, want = _distances_twice(q, s), R.distances(q, s)
    err, bound = np.abs(got.astype(np.float64) - want), R.bound(D, want)
    print("distances %s: worst error / bound %.3f" % ((Q, N, D), (err[want > 0] / bound[want > 0]).max()))
    assert (err <= bound).all()
    eq = R.planted_equal(Q, N)
    if eq is not None:
        assert want[eq] == 0.0 and got[eq] == 0.0 and np.signbit(got[eq]) == 0


@pytest.mark.parametrize("Q,N,D", R.SHAPES)
def test_distances_of_exact_operands_bit_for_bit(Q, N, D):
    q, s = R.exact_operands(np.random.RandomState(Q * N + D), Q, N, D)
    q[Q - 1] = s[N // 2]                                           # a query equal to a set row: exactly 0
    got, want = _distances_twice(q, s), R.distances(q, s)
    assert np.array_equal(got.astype(np.float64), want)
    assert got[Q - 1, N // 2] == 0.0


def test_distance_wrapper_rejects_what_it_cannot_run():
    q, s = torch.zeros(2, 192, device="cuda", dtype=torch.bfloat16), torch.zeros(5, 192, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        Fn.nn_distances(q.float(), s)
    with pytest.raises(RuntimeError):
        Fn.nn_distances(q[:, :128], s)
    with pytest.raises(RuntimeError):
        Fn.nn_distances(q[:, :96].contiguous(), s[:, :96].contiguous())      # D is no multiple of 64
    with pytest.raises(RuntimeError):
        Fn.nn_topk(torch.zeros(2, 5, device="cuda"), 17)


# ---------------------------------------------------------------- selection
@pytest.mark.parametrize("Q", [1, 40])
@pytest.mark.parametrize("k", [1, 3, 8, 16])
@pytest.mark.parametrize("N", [1, 5, 257, 100000])
def test_topk_is_exact(N, k, Q):
    rng = np.random.RandomState(N + 16 * k + Q)
    rows = {"random": rng.uniform(0, 100, size=(Q, N)).astype(np.float32),
            "ties": rng.randint(0, 4, size=(Q, N)).astype(np.float32)}
    for kind, x in rows.items():
        tx = torch.from_numpy(x).cuda()
        v1, i1 = Fn.nn_topk(tx, k)
        v2, i2 = Fn.nn_topk(tx, k)
        assert torch.equal(v1, v2) and torch.equal(i1, i2), kind
        wv, wi = R.topk(x, k)
        assert np.array_equal(v1.cpu().numpy(), wv) and np.array_equal(i1.cpu().numpy(), wi), kind
        assert N >= k or (wi[:, N:] == -1).all()


# ---------------------------------------------------------------- pack
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("f", [1, 2, 4])
def test_pack(f, C, mirror, dtype):
    for S_ in (16, 32):
        if S_ // f < 8:
            continue
        rng = np.random.RandomState(100 * S_ + 10 * f + C)
        B, D_ = 3, (S_ // f) ** 2 * C
        # bytes as the loader normalises them: every value and every sum of up to 256 of them is exact in fp32
        x = ((rng.randint(0, 256, size=(B, S_, S_, C)) - 128) / 128.0).astype(np.float32)
        tx = torch.from_numpy(x).cuda().to(dtype)                   # (v - 128) / 128 has 8 bits: exact in bf16 too
        buf, out = _guarded((B, D_), torch.bfloat16)
        Fn.nn_pack(tx, f, mirror, out=out)
        first = out.clone()
        Fn.nn_pack(tx, f, mirror, out=out)
        assert torch.equal(first, out) and _bands_untouched(buf)
        want = R.bf16_bits(R.box_mean(x, f, mirror))
        assert np.array_equal(first.view(torch.int16).cpu().numpy().view(np.uint16), want)
        assert torch.equal(first, Fn.nn_pack(tx.flip(2).contiguous(), f, not mirror))   # mirror = packing x.flip(2)
        # random inputs: within one bf16 ulp of the float64 box mean
        y = rng.uniform(-1, 1, size=(B, S_, S_, C)).astype(np.float32)
        ty = torch.from_numpy(y).cuda().to(dtype)
        got = R.bf16_value(Fn.nn_pack(ty, f, mirror).view(torch.int16).cpu().numpy().view(np.uint16))
        mean = R.box_mean(ty.float().cpu().numpy(), f, mirror)
        assert (np.abs(got - mean) <= R.bf16_ulp(mean)).all()


# ---------------------------------------------------------------- composed
def test_composed_search_on_the_planted_case():
    case = R.planted_case()
    Dn = case["side"] ** 2 * case["C"]
    plan = NB.NnPlan(case["side"], case["C"], 64, nn_size=case["side"], nn_images=case["N"], budget=1 << 30)
    assert (plan.f, plan.D, plan.N) == (1, Dn, case["N"])
    images, queries = torch.from_numpy(case["images"]).cuda(), torch.from_numpy(case["queries"]).cuda()
    runs = []
    for _ in range(2):
        s = NB.NearestSet(plan, "cuda")
        for lo in range(0, case["N"], 64):
            s.add(images[lo:lo + 64])
        runs.append(s.finish().search(queries, case["k"], True))
    for key in ("dist", "index", "mirrored"):
        assert np.array_equal(runs[0][key], runs[1][key])
    want, _ = R.nearest(case["queries"].reshape(case["Q"], Dn), case["images"].reshape(case["N"], Dn), case["side"],
                        case["C"], case["k"], True)
    got = runs[0]
    for i, row in enumerate(want):
        assert got["index"][i].tolist() == [r[1] for r in row]
        assert got["mirrored"][i].tolist() == [r[2] for r in row]
        rms = np.sqrt(np.array([r[0] for r in row]) / Dn)
        assert (np.abs(got["dist"][i] - rms) <= R.gamma(Dn) * rms).all()   # sqrt(1 + g) <= 1 + g
        assert got["files"][i] == ["synthetic:%d" % r[1] for r in row]


# ---------------------------------------------------------------- model level
def _model(tmp_path, tag, **kw):
    d = tmp_path / tag
    flags = dict(img_size=64, ch=8, batch_size=4, log_dir=str(d / "logs"), checkpoint_dir=str(d / "ckpt"),
                 sample_dir=str(d / "samples"), result_dir=str(d / "results"))
    flags.update(kw)
    return model.BigGAN(make_args(**flags), store=S.VariableStore("cuda", seed=5)).build_model()


def _write_dataset(root, n=24):
    (root / "toy").mkdir(parents=True)
    rng = np.random.RandomState(9)
    for i in range(n):
        utils.write_png(rng.randint(0, 256, size=(40, 48, 3)).astype(np.uint8), str(root / "toy" / ("%02d.png" % i)))
    return str(root)


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


def test_nearest_finds_a_training_image_and_its_mirror_image(tmp_path):
    root = _write_dataset(tmp_path / "dataset")
    files = sorted(os.listdir(os.path.join(root, "toy")))
    loader = D.ImageData(64, 3, True, False)
    five = loader.image_processing(os.path.join(root, "toy", files[5]))
    seven = loader.image_processing(os.path.join(root, "toy", files[7]))
    queries = torch.from_numpy(np.stack([five, seven[:, ::-1]])).cuda()
    gan = _model(tmp_path, "flip", dataset="toy", random_flip="true")
    snap = _snapshot(gan)
    res = gan.nearest(images=queries, root=root)
    _same_state(gan, snap)
    assert gan._nn.plan.N == 24 and gan._nn.plan.from_files and res["dist"].shape == (2, 3)
    assert (res["index"][0, 0], res["dist"][0, 0], bool(res["mirrored"][0, 0])) == (5, 0.0, False)
    assert (res["index"][1, 0], res["dist"][1, 0], bool(res["mirrored"][1, 0])) == (7, 0.0, True)
    assert os.path.basename(res["files"][0][0]) == files[5] and os.path.basename(res["files"][1][0]) == files[7]
    assert res["dist"][0, 1] > 0 and np.array_equal(gan._nn_fetch(5), five)
    # the set is the listing through the loader's own path, device or host: the same descriptors either way
    want = Fn.nn_pack(torch.from_numpy(np.stack([loader.image_processing(os.path.join(root, "toy", f)) for f in files])).cuda(), 1)
    assert torch.equal(gan._nn.arena, want)
    # a run that never flips does not search mirror images
    plain = _model(tmp_path, "noflip", dataset="toy", random_flip="false")
    res = plain.nearest(images=queries, root=root, k=2)
    assert res["dist"].shape == (2, 2) and (res["index"][0, 0], res["dist"][0, 0]) == (5, 0.0)
    assert res["dist"][1, 0] > 0 and not res["mirrored"].any()


def _train(tmp_path, tag, nn_freq, **kw):
    gan = _model(tmp_path, tag, nn_freq=nn_freq, **kw)
    gan.log_events = True
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        gan.train(iterations=2, resume=False)
    return gan, [l for l in out.getvalue().splitlines() if l.startswith("NN: ")]


@pytest.mark.parametrize("with_files", [False, True], ids=["synthetic", "files"])
def test_training_with_the_search_writes_its_files_and_leaves_the_run_alone(tmp_path, monkeypatch, with_files):
    monkeypatch.chdir(tmp_path)
    kw = dict(nn_images=24)
    if with_files:
        _write_dataset(tmp_path / "dataset")
        kw["dataset"] = "toy"
    searched, lines = _train(tmp_path, "searched", 2, **kw)
    plain, none = _train(tmp_path, "plain", 0, **kw)
    assert not none and plain._nn is None and searched._nn is not None and searched._nn.plan.from_files == with_files
    assert len(lines) == 2 and lines[0].startswith("NN: set of 24 images") and "nn_dist_min" in lines[1]
    a, b = searched.state_tensors(), plain.state_tensors()
    assert a.keys() == b.keys()
    for key in a:
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(searched.gen.get_state(), plain.gen.get_state()) and searched.counter == plain.counter == 2
    # the grid: rows x (k + 1) tiles; the table: rows of the queries x k
    names = NB.event_names(searched.model_name, 0, 2)
    folder = str(tmp_path / "searched" / "samples")
    assert sorted(os.listdir(folder)) == [names["png"], names["txt"]]
    n_q, k = min(searched.sample_num, 4), 3
    png = D.decode_png(open(os.path.join(folder, names["png"]), "rb").read())
    assert png.shape == (min(n_q, 8) * 64, (k + 1) * 64, 3)
    rows = [l.split("\t") for l in open(os.path.join(folder, names["txt"])).read().splitlines()]
    assert len(rows) == n_q * k and [r[:2] for r in rows] == [[str(q), str(r + 1)] for q in range(n_q) for r in range(k)]
    for r in rows:
        assert os.path.isfile(r[4]) if with_files else r[4] in ["synthetic:%d" % i for i in range(24)]
    first = [float(r[2]) for r in rows if r[1] == "1"]
    # the scalars, at the step of the second iteration
    d = os.path.join(str(tmp_path / "searched" / "logs"), searched.model_dir)
    ev = TR.read_events(os.path.join(d, os.listdir(d)[0]))
    nn_events = [e for e in ev[1:] if e["values"][0][0].startswith("nn_")]
    assert len(nn_events) == 1 and nn_events[0]["step"] == 1
    assert [t for t, _, _ in nn_events[0]["values"]] == ["nn_dist_min", "nn_dist_mean"]
    assert abs(nn_events[0]["values"][0][2] - min(first)) <= 1e-5 and abs(nn_events[0]["values"][1][2] - np.mean(first)) <= 1e-5


def test_phase_test_writes_the_neighbours(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    gan = _model(tmp_path, "phase", nn_freq=1, nn_images=16, nn_k=2, test_num=1)
    with contextlib.redirect_stdout(io.StringIO()):
        gan.test()
    folder = os.path.join(str(tmp_path / "phase" / "results"), gan.model_dir)
    rows = open(os.path.join(folder, "nn.txt")).read().splitlines()
    assert len(rows) == min(gan.sample_num, 4) * 2
    assert D.decode_png(open(os.path.join(folder, "nn.png"), "rb").read()).shape == (4 * 64, 3 * 64, 3)
