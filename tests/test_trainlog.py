"""Training logs, the part that needs no GPU: the bucket table and rule, the run-collapsed encoding, CRC-32C (library helper
and Python fallback), the event file read back by the independent reader of tests/trainlog_ref.py, the list of histogrammed
variables, VariableHistograms' host path against the reference, and the wiring of the training loop (train_step patched
to return fixed losses)."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, model, scope as S, trainlog as T
from tests import trainlog_ref as R


# ---------------------------------------------------------------- table and bucket rule
def test_the_table():
    lim = T.bucket_limits()
    assert lim.shape == (1551,) and lim.dtype == np.float64
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[-2] == 9.920775621859783e+19
    assert lim[0] == -R.DBL_MAX and lim[-1] == R.DBL_MAX
    assert np.array_equal(lim, R.LIMITS) and np.all(np.diff(lim) > 0)
    assert np.array_equal(lim[1:775], -lim[776:1550][::-1])
    # no positive limit is a float32: a float32 never sits exactly on one
    pos = lim[776:1550]
    assert not np.any(pos.astype(np.float32).astype(np.float64) == pos)


def test_zeros_and_denormals():
    x = np.array([0.0, -0.0, 1.4e-45, -1.4e-45], dtype=np.float32)
    for i, want in enumerate([776, 776, 776, 775]):
        counts, stats = T.host_histogram(x[i:i + 1])
        assert counts[want] == 1 and counts.sum() == 1 and stats[2] == 1.0, (x[i], want)


# ---------------------------------------------------------------- collapse
def _vec(**at):
    c = np.zeros(1551, dtype=np.int64)
    for k, v in at.items():
        c[int(k[1:])] = v
    return c


COLLAPSE_CASES = {
    "empty": (_vec(), [(R.DBL_MAX, 0.0)]),
    "one_in_the_middle": (_vec(b800=7), [(R.LIMITS[799], 0.0), (R.LIMITS[800], 7.0), (R.DBL_MAX, 0.0)]),
    "first_bucket": (_vec(b0=2), [(-R.DBL_MAX, 2.0), (R.DBL_MAX, 0.0)]),
    "last_bucket": (_vec(b1550=3), [(R.LIMITS[1549], 0.0), (R.DBL_MAX, 3.0)]),
    "adjacent_then_gap": (_vec(b10=1, b11=2, b13=4),
                          [(R.LIMITS[9], 0.0), (R.LIMITS[10], 1.0), (R.LIMITS[11], 2.0), (R.LIMITS[12], 0.0),
                           (R.LIMITS[13], 4.0), (R.DBL_MAX, 0.0)]),
    "first_and_last": (_vec(b0=1, b1550=1), [(-R.DBL_MAX, 1.0), (R.LIMITS[1549], 0.0), (R.DBL_MAX, 1.0)]),
}


@pytest.mark.parametrize("name", sorted(COLLAPSE_CASES))
def test_collapse(name):
    counts, want = COLLAPSE_CASES[name]
    assert R.collapse(counts) == want                         # the reference's loop gives the hand-written answer
    lim, cnt = T.collapse(counts)
    assert list(zip(lim.tolist(), cnt.tolist())) == want
    assert lim.dtype == np.float64 and cnt.dtype == np.float64


def test_collapse_of_a_matrix_equals_row_by_row():
    rng = np.random.default_rng(0)
    m = rng.integers(0, 3, size=(7, 1551)) * (rng.random((7, 1551)) < 0.1)
    m[3] = 0
    for row, (lim, cnt) in zip(m, T.collapse(m.astype(np.uint32))):
        assert list(zip(lim.tolist(), cnt.tolist())) == R.collapse(row)


# ---------------------------------------------------------------- CRC-32C
def _lib_crc(data, crc=0):
    return int(hip.lib().bg_crc32c(bytes(data), len(data), crc))


@pytest.mark.parametrize("fn", [_lib_crc, T.crc32c_py, T.crc32c, R.crc32c], ids=["library", "python", "writer", "ref"])
def test_crc32c_known_answers(fn):
    assert fn(b"123456789") == 0xE3069283
    assert fn(bytes(32)) == 0x8A9136AA
    assert fn(b"") == 0
    assert fn(b"6789", fn(b"12345")) == 0xE3069283            # fed in pieces


def test_crc32c_library_and_python_agree():
    rng = np.random.default_rng(1)
    for n in list(range(0, 70)) + [255, 256, 257, 1023, 4095, 4096, 4097, 4098, 4099]:
        buf = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert _lib_crc(buf) == T.crc32c_py(buf), n
    for n in (5, 64, 300):
        buf = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert _lib_crc(buf) == R.crc32c(buf), n


def test_the_writer_uses_the_library_helper():
    T.crc32c(b"x")
    assert T._crc_native and T._crc_native.restype is ctypes.c_uint32


# ---------------------------------------------------------------- file format
def _hist_of(x):
    counts, s = T.host_histogram(x)
    lim, cnt = T.collapse(counts)
    return (float(s[0]), float(s[1]), float(s[2]), float(s[3]), float(s[4]), lim, cnt)


def test_event_file_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(1000) * 0.02).astype(np.float32)
    zeros = np.zeros(5, dtype=np.float32)
    scalars = {"d_loss": 1.2345678, "g_loss": -0.25, "zero": 0.0, "big": 3.0e38}
    w = T.EventWriter(str(tmp_path / "logs" / "run"))
    w.add_scalars(0, scalars)
    w.add_scalars(7, {"d_loss": 0.5})
    w.add_histograms(250, [("a/kernel_0/hist", _hist_of(x)), ("a/bias_0/hist", _hist_of(zeros))])
    w.add_scalars(-1, {"neg": 1.0})
    w.flush()
    name = os.path.basename(w.path)
    assert name.startswith("events.out.tfevents.") and int(name.split(".")[3]) > 0
    mid = R.read_events(w.path)                               # readable after a flush, before the close
    assert len(mid) == 5
    w.close()
    w.close()
    ev = R.read_events(w.path)                                # (verifies the length CRC and the data CRC of every record)
    assert len(ev) == 5
    assert ev[0]["file_version"] == "brain.Event:2" and ev[0]["values"] is None and ev[0]["wall_time"] > 0
    assert [e["step"] for e in ev] == [0, 0, 7, 250, -1]
    assert [(t, k) for t, k, _ in ev[1]["values"]] == [(k, "scalar") for k in scalars]
    for (tag, _, got), want in zip(ev[1]["values"], scalars.values()):
        assert got.dtype == np.float32 and got == np.float32(want), tag
    assert ev[2]["values"] == [("d_loss", "scalar", np.float32(0.5))]
    (t0, k0, h0), (t1, k1, h1) = ev[3]["values"]
    assert (t0, k0, t1, k1) == ("a/kernel_0/hist", "histo", "a/bias_0/hist", "histo")
    for h, arr in ((h0, x), (h1, zeros)):
        ref = R.histogram(arr)
        ds, dq = R.sum_bounds(ref)
        assert (h["min"], h["max"], h["num"]) == (ref["min"], ref["max"], ref["num"])
        assert abs(h["sum"] - ref["sum"]) <= ds and abs(h["sum_squares"] - ref["sum_squares"]) <= dq
        assert list(zip(h["bucket_limit"], h["bucket"])) == R.collapse(ref["counts"])
    assert h1["bucket_limit"] == [R.LIMITS[775], R.LIMITS[776], R.DBL_MAX] and h1["bucket"] == [0.0, 5.0, 0.0]


def test_a_second_writer_gets_a_file_of_its_own(tmp_path):
    a = T.EventWriter(str(tmp_path))
    b = T.EventWriter(str(tmp_path))
    a.close(), b.close()
    assert a.path != b.path and len(os.listdir(str(tmp_path))) == 2


def test_a_damaged_record_is_caught_by_the_reader(tmp_path):
    w = T.EventWriter(str(tmp_path))
    w.add_scalars(1, {"x": 1.0})
    w.close()
    raw = bytearray(open(w.path, "rb").read())
    raw[-6] ^= 1
    open(w.path, "wb").write(bytes(raw))
    with pytest.raises(AssertionError):
        R.read_records(w.path)


def test_record_frame_by_hand():
    rec = T.tfrecord(b"abc")
    assert rec[:8] == struct.pack("<Q", 3) and rec[12:15] == b"abc" and len(rec) == 19
    assert struct.unpack("<I", rec[8:12])[0] == R.masked(rec[:8])
    assert struct.unpack("<I", rec[15:])[0] == R.masked(b"abc")


# ---------------------------------------------------------------- the model's variables
def _model(tmp_path, *extra, seed=42):
    argv = ["--gan_type", "hinge", "--img_size", "64", "--ch", "8", "--batch_size", "2", "--z_dim", "64",
            "--log_dir", str(tmp_path / "logs"), "--checkpoint_dir", str(tmp_path / "ckpt"),
            "--sample_dir", str(tmp_path / "samples")] + list(extra)
    args = M.parse_args(argv, make_dirs=False)
    return model.BigGAN(args, device="cpu", store=S.VariableStore("cpu", seed)).build_model()


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("trainlog"))


def test_histogram_tags_are_the_variables_of_the_store(cpu_model):
    vh = T.VariableHistograms(cpu_model.store)
    assert not vh.device_path
    assert vh.tags == [n + "_0/hist" for n in cpu_model.store.vars]
    assert len(set(vh.tags)) == len(vh.tags) > 50
    assert any(t.endswith("/u_0/hist") for t in vh.tags) and any(t.endswith("/pop_mean_0/hist") for t in vh.tags)
    assert not any("/Adam" in t or "ExponentialMovingAverage" in t for t in vh.tags)
    got = vh.compute()
    assert [t for t, _ in got] == vh.tags


def test_host_path_equals_the_reference(cpu_model):
    vh = T.VariableHistograms(cpu_model.store)
    got = dict(vh.compute())
    assert vh.nonfinite == {}
    for name, t in cpu_model.store.vars.items():
        ref = R.histogram(t.detach().numpy())
        mn, mx, num, s, sq, lim, cnt = got[name + "_0/hist"]
        ds, dq = R.sum_bounds(ref)
        assert (mn, mx, num) == (ref["min"], ref["max"], ref["num"]) and num == t.numel(), name
        assert abs(s - ref["sum"]) <= ds and abs(sq - ref["sum_squares"]) <= dq, name
        assert list(zip(lim.tolist(), cnt.tolist())) == R.collapse(ref["counts"]), name


def test_a_variable_with_a_nan_is_skipped_with_a_warning(tmp_path, capsys):
    gan = _model(tmp_path)
    name = next(n for n, t in gan.store.vars.items() if t.numel() > 10)
    with torch.no_grad():
        gan.store.vars[name].view(-1)[3] = float("nan")
    vh = T.VariableHistograms(gan.store)
    got = vh.compute()
    out = capsys.readouterr().out
    assert [t for t, _ in got] == [t for t in vh.tags if t != name + "_0/hist"]
    assert vh.nonfinite == {name: 1}
    assert out.count("warning") == 1 and name in out and "1 non-finite" in out


def test_bg_device_hist_0_selects_the_host_path(monkeypatch, cpu_model):
    monkeypatch.setenv("BG_DEVICE_HIST", "0")
    assert not T.VariableHistograms(cpu_model.store, device="cuda").device_path


# ---------------------------------------------------------------- ABI
def test_abi_of_the_histogram_entry_points():
    L = hip.lib()
    header = open(os.path.join(os.path.dirname(hip.LIB_PATH), "..", "include", "biggan_hip.h")).read()
    for name in ("bg_crc32c", "bg_var_hist_plan_chunks", "bg_var_hist_plan_bytes", "bg_var_hist_plan",
                 "bg_var_hist_workspace_bytes", "bg_var_hist"):
        assert name in hip.SIGNATURES and name + "(" in header
    items = (hip.BgHistItem * 3)()
    for it, (p, n) in zip(items, [(4096, 1), (4100, 16384), (8192, 16385)]):
        it.x, it.n = p, n
    nc = ctypes.c_int(-1)
    assert L.bg_var_hist_plan_chunks(items, 3, ctypes.byref(nc)) == 0 and nc.value == 4
    nb = L.bg_var_hist_plan_bytes(3, 4)
    plan = np.zeros(nb // 8, dtype=np.int64)
    assert L.bg_var_hist_plan(items, 3, plan.ctypes.data_as(ctypes.c_void_p), nb) == 0
    chunks = plan.view(np.uint32)[3 * 6:].reshape(4, 4)
    assert chunks[:, :3].tolist() == [[0, 0, 1], [1, 0, 16384], [2, 0, 16384], [2, 16384, 1]]
    assert L.bg_var_hist_workspace_bytes(3, 4) >= 4 * 6 * 8
    # errors: a message, and nothing written
    assert L.bg_var_hist_plan(items, 3, plan.ctypes.data_as(ctypes.c_void_p), nb - 1) == 1
    assert b"plan_bytes" in L.bg_last_error()
    items[1].n = 1 << 32
    assert L.bg_var_hist_plan_chunks(items, 3, ctypes.byref(nc)) == 1 and b"2^32" in L.bg_last_error()
    items[1].n, items[1].x = 8, 4098
    assert L.bg_var_hist_plan_chunks(items, 3, ctypes.byref(nc)) == 1 and b"aligned" in L.bg_last_error()
    assert L.bg_var_hist_plan_chunks(items, 0, ctypes.byref(nc)) == 1
    assert L.bg_var_hist(None, 3, 4, None, 1551, None, None, None, 1 << 20, None) == 1
    assert b"bg_var_hist" in L.bg_last_error()


# ---------------------------------------------------------------- wiring of the training loop
LOSSES = [{"d_loss": 1.5, "g_loss": -0.75}, {"d_loss": 1.25, "g_loss": 0.1}, {"d_loss": 0.3333333, "g_loss": 2.0}]


def _run(tmp_path, monkeypatch, *extra, log=True, rank=0, iterations=3):
    gan = _model(tmp_path, *extra)
    gan.rank = rank
    seen = []

    def fake_step(real, labels=None, real_g=None):
        out = {k: torch.tensor(v, dtype=torch.float32) for k, v in LOSSES[len(seen) % 3].items()}
        seen.append(out)
        gan.counter += 1
        return out

    monkeypatch.setattr(gan, "train_step", fake_step)
    monkeypatch.setattr(gan, "save", lambda *a, **k: None)
    gan.log_events = log
    gan.train(data_fn=lambda: torch.zeros(2, 64, 64, 3), iterations=iterations, resume=False)
    return gan, os.path.join(str(tmp_path / "logs"), gan.model_dir)


def _events(d):
    files = os.listdir(d)
    assert len(files) == 1 and files[0].startswith("events.out.tfevents.")
    ev = R.read_events(os.path.join(d, files[0]))
    assert ev[0]["file_version"] == "brain.Event:2"
    scalars = [e for e in ev[1:] if e["values"][0][1] == "scalar"]
    hists = [e for e in ev[1:] if e["values"][0][1] == "histo"]
    assert len(scalars) + len(hists) == len(ev) - 1
    return scalars, hists


def test_scalars_every_iteration_histograms_every_histogram_freq(tmp_path, monkeypatch):
    gan, d = _run(tmp_path, monkeypatch, "--histogram_freq", "2")
    scalars, hists = _events(d)
    assert [e["step"] for e in scalars] == [0, 1, 2] and [e["step"] for e in hists] == [0, 2]
    for e, want in zip(scalars, LOSSES):
        assert [(t, v) for t, _, v in e["values"]] == [(k, np.float32(v)) for k, v in want.items()]
    for e in hists:
        assert [t for t, _, _ in e["values"]] == [n + "_0/hist" for n in gan.store.vars]
    assert gan._log_writer is None                            # closed at the end of train()


def test_histogram_freq_0_writes_no_histogram(tmp_path, monkeypatch):
    _, d = _run(tmp_path, monkeypatch, "--histogram_freq", "0")
    scalars, hists = _events(d)
    assert [e["step"] for e in scalars] == [0, 1, 2] and hists == []


def test_the_step_continues_from_the_counter(tmp_path, monkeypatch):
    gan = _model(tmp_path, "--histogram_freq", "125")
    gan.counter = 250                                         # as after a resume: the iteration that runs has step 249
    monkeypatch.setattr(gan, "save", lambda *a, **k: None)

    def fake_step(real, labels=None, real_g=None):
        gan.counter += 1
        return {"d_loss": torch.tensor(1.0)}

    monkeypatch.setattr(gan, "train_step", fake_step)
    gan.log_events = True
    gan.train(data_fn=lambda: torch.zeros(2, 64, 64, 3), iterations=2, resume=False)
    scalars, hists = _events(os.path.join(str(tmp_path / "logs"), gan.model_dir))
    assert [e["step"] for e in scalars] == [250, 251] and [e["step"] for e in hists] == [250]


def test_another_rank_creates_no_file(tmp_path, monkeypatch):
    _, d = _run(tmp_path, monkeypatch, "--histogram_freq", "2", rank=1)
    assert not os.path.exists(str(tmp_path / "logs"))


def test_without_the_opt_in_nothing_is_created(tmp_path, monkeypatch):
    gan, d = _run(tmp_path, monkeypatch, "--histogram_freq", "2", log=False)
    assert not os.path.exists(str(tmp_path / "logs"))
    assert model.BigGAN(gan.args, device="cpu", store=S.VariableStore("cpu")).log_events is False


def test_the_file_is_closed_when_training_raises(tmp_path, monkeypatch):
    gan = _model(tmp_path)

    def boom(real, labels=None, real_g=None):
        raise RuntimeError("boom")

    monkeypatch.setattr(gan, "train_step", boom)
    gan.log_events = True
    with pytest.raises(RuntimeError):
        gan.train(data_fn=lambda: torch.zeros(2, 64, 64, 3), iterations=1, resume=False)
    assert gan._log_writer is None
    scalars, hists = _events(os.path.join(str(tmp_path / "logs"), gan.model_dir))
    assert scalars == [] and hists == []


def test_the_command_line_opts_in(monkeypatch):
    made = []

    class Stub:
        log_events = False

        def __init__(self, args):
            made.append(self)

        def build_model(self):
            pass

        def train(self, *a, **kw):
            self.at_train = self.log_events

    monkeypatch.setattr(model, "BigGAN", Stub)
    monkeypatch.setattr(M, "check_folder", lambda d: d)
    M.main(["--phase", "train"])
    assert made[0].at_train is True
