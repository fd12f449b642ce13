"""bg_var_hist on the GPU against tests/trainlog_ref.py: counts, min, max, num and the non-finite count exactly, sum and
sum_squares within 2 n 2^-53 sum|x| (sum x^2) of math.fsum (any order of double additions meets (n-1) 2^-53 sum|x|, so the
bound allows a factor of two); then the training loop's event file end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, model, scope as S, trainlog as T
from tests import trainlog_ref as R
from tests.common import make_args

pytestmark = pytest.mark.gpu

N_LIMITS = 1551
FLT_MAX = float(np.finfo(np.float32).max)


class Hist:
    """One plan over a list of CUDA fp32 views, and the buffers of a call."""

    def __init__(self, views):
        L = hip.lib()
        self.views = views
        n = self.n = len(views)
        items = (hip.BgHistItem * n)()
        for it, v in zip(items, views):
            assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
            it.x, it.n = v.data_ptr(), v.numel()
        nc = ctypes.c_int(0)
        assert L.bg_var_hist_plan_chunks(items, n, ctypes.byref(nc)) == 0, L.bg_last_error()
        self.n_chunks = nc.value
        plan = np.zeros(L.bg_var_hist_plan_bytes(n, self.n_chunks) // 8, dtype=np.int64)
        assert L.bg_var_hist_plan(items, n, plan.ctypes.data_as(ctypes.c_void_p), plan.nbytes) == 0, L.bg_last_error()
        self.plan = torch.from_numpy(plan).cuda()
        self.limits = torch.from_numpy(np.array(R.LIMITS)).cuda()
        self.ws_bytes = L.bg_var_hist_workspace_bytes(n, self.n_chunks)
        self.ws = torch.empty(self.ws_bytes // 8 + 1, dtype=torch.float64, device="cuda")

    def call(self, **over):
        a = dict(plan=hip.ptr(self.plan), n_items=self.n, n_chunks=self.n_chunks, limits=hip.ptr(self.limits),
                 n_limits=N_LIMITS, ws=hip.ptr(self.ws), ws_bytes=self.ws_bytes)
        a.update(over)
        counts = torch.full((self.n, N_LIMITS), -7, dtype=torch.int32, device="cuda")       # (the call zeroes them)
        stats = torch.full((self.n, 6), -7.0, dtype=torch.float64, device="cuda")
        rc = hip.lib().bg_var_hist(a["plan"], a["n_items"], a["n_chunks"], a["limits"], a["n_limits"], hip.ptr(counts),
                                   hip.ptr(stats), a["ws"], a["ws_bytes"], hip.stream())
        torch.cuda.synchronize()
        return rc, counts, stats


def check_item(counts, stats, x, what=""):
    """counts [1551] / stats [6] of one item (numpy) against the reference on the host copy x; returns the reference."""
    ref = R.histogram(x)
    ds, dq = R.sum_bounds(ref)
    print("%s n=%d: sum %.17g (ref %.17g, bound %.3g)  sum_squares %.17g (ref %.17g, bound %.3g)  counts differ in %d buckets"
          % (what, x.size, stats[3], ref["sum"], ds, stats[4], ref["sum_squares"], dq,
             int((counts.astype(np.int64) != ref["counts"]).sum())))
    assert np.array_equal(counts.astype(np.int64), ref["counts"]), what
    assert stats[0] == ref["min"] and stats[1] == ref["max"] and stats[2] == ref["num"], (what, stats, ref["min"], ref["max"])
    assert stats[5] == ref["nonfinite"], what
    assert abs(stats[3] - ref["sum"]) <= ds, what
    assert abs(stats[4] - ref["sum_squares"]) <= dq, what
    return ref


def run_and_check(views, what=""):
    h = Hist(views)
    rc, counts, stats = h.call()
    assert rc == 0, hip.lib().bg_last_error()
    c, s = counts.cpu().numpy().view(np.uint32), stats.cpu().numpy()
    for i, v in enumerate(views):
        check_item(c[i], s[i], v.cpu().numpy().ravel(), "%s item %d" % (what, i))
    return c, s


def normal(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.02).cuda()


# ---------------------------------------------------------------- edge lengths and alignments
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_edge_lengths_at_every_alignment(off):
    for n in (1, 3, 5, 63, 64, 65, 4099):
        buf = normal(4099 + 64, 100 + n)
        assert buf.data_ptr() % 16 == 0
        lo = 16 + off                                   # 16 floats = 64 bytes past the start: `off` floats past a 16-byte boundary
        buf[lo - 1] = 1e30                              # a read past either end lands in the last bucket
        buf[lo + n] = 1e30
        view = buf[lo:lo + n]
        assert (view.data_ptr() % 16) // 4 == off
        c, _ = run_and_check([view], "off=%d n=%d" % (off, n))
        assert c[0, 1550] == 0 and c[0].sum() == n


# ---------------------------------------------------------------- a real manifest
def test_every_variable_of_a_model_in_one_call():
    args = make_args(img_size=64, ch=8, batch_size=2, z_dim=64, n_labels=3)
    gan = model.BigGAN(args, store=S.VariableStore("cuda", seed=3)).build_model()
    vh = T.VariableHistograms(gan.store)
    assert vh.device_path and vh._n == len(gan.store.vars) > 100
    sizes = [t.numel() for t in gan.store.vars.values()]
    assert min(sizes) == 1 and max(sizes) > 1000
    vh.launch()
    counts, stats = vh.fetch()
    for i, (name, t) in enumerate(gan.store.vars.items()):
        check_item(counts[i], stats[i], t.detach().cpu().numpy().ravel(), name)
        assert stats[i, 2] == t.numel() and counts[i].sum() == t.numel(), name
    # and through compute(): the collapsed encoding of the same counts, tag by tag
    got = vh.compute()
    assert [t for t, _ in got] == [n + "_0/hist" for n in gan.store.vars]
    for (tag, h), (name, t) in zip(got, gan.store.vars.items()):
        ref = R.histogram(t.detach().cpu().numpy())
        assert list(zip(h[5].tolist(), h[6].tolist())) == R.collapse(ref["counts"]), name
    # BG_DEVICE_HIST=0: the host path gives the same histograms
    host = T.VariableHistograms(gan.store, device_path=False).compute()
    for (tag, h), (tag2, h2) in zip(got, host):
        assert tag == tag2 and h[:3] == h2[:3] and np.array_equal(h[5], h2[5]) and np.array_equal(h[6], h2[6]), tag


# ---------------------------------------------------------------- large items
def test_an_item_of_many_chunks():
    buf = normal(3 * 2 ** 20 + 5 + 8, 7)
    buf[0] = 1e30
    buf[-1] = 1e30
    view = buf[1:1 + 3 * 2 ** 20 + 5]                   # one float past a 16-byte boundary
    h = Hist([view])
    assert h.n_chunks > 100
    c, _ = run_and_check([view], "3*2^20+5")
    assert c[0, 1550] == 0


def test_an_all_zero_item():
    z = torch.zeros(2 ** 20 + 1, device="cuda")
    h = Hist([z])
    rc, counts, stats = h.call()
    assert rc == 0
    c, s = counts.cpu().numpy().view(np.uint32), stats.cpu().numpy()
    want = np.zeros(N_LIMITS, dtype=np.uint32)
    want[776] = 2 ** 20 + 1
    assert np.array_equal(c[0], want)
    assert s[0].tolist() == [0.0, 0.0, float(2 ** 20 + 1), 0.0, 0.0, 0.0]


# ---------------------------------------------------------------- boundary values
def boundary_values():
    lim = R.LIMITS
    pos = [776 + int(round(i * 773 / 39)) for i in range(40)]              # 40 limits spread over the positive half
    picks = sorted(set(pos + [776, 1549])) + sorted(set([775 - (p - 775) for p in pos] + [774, 1]))
    vals = []
    for i in picks:
        f = np.float32(lim[i])
        if not np.isfinite(f):
            continue
        vals += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    vals += [0.0, -0.0, 1.4e-45, -1.4e-45, FLT_MAX, -FLT_MAX, 1e-12, -1e-12, 9.92e19, -9.92e19]
    out = np.array(vals, dtype=np.float32)
    assert np.isfinite(out).all() and len(picks) >= 80
    return out


def test_boundary_values_one_item_each_and_all_together():
    vals = boundary_values()
    buf = torch.from_numpy(vals).cuda()
    views = [buf[i:i + 1] for i in range(len(vals))] + [buf]
    c, s = run_and_check(views, "boundary")
    for i, v in enumerate(vals):                         # exactly one element, in upper_bound's bucket
        assert c[i].sum() == 1 and c[i, np.searchsorted(R.LIMITS, np.float64(v), side="right")] == 1, v
    z = {float(v): int(np.argmax(c[i])) for i, v in enumerate(vals) if abs(v) < 1e-40}
    assert z[0.0] == 776 and z[1.401298464324817e-45] == 776 and z[-1.401298464324817e-45] == 775


# ---------------------------------------------------------------- non-finite values
def test_non_finite_values_are_counted_apart():
    buf = normal(3 * 1000, 11)
    buf[1000 + 5] = float("nan")
    buf[1000 + 64] = float("nan")
    buf[1000 + 500] = float("inf")
    buf[1000 + 999] = float("-inf")
    views = [buf[0:1000], buf[1000:2000], buf[2000:3000]]
    c, s = run_and_check(views, "nonfinite")
    assert s[:, 5].tolist() == [0.0, 4.0, 0.0] and s[:, 2].tolist() == [1000.0, 996.0, 1000.0]
    assert c.sum(axis=1).tolist() == [1000, 996, 1000]
    only = torch.full((7,), float("nan"), device="cuda")
    rc, counts, stats = Hist([only]).call()
    assert rc == 0 and int(counts.abs().sum()) == 0
    assert stats.cpu().numpy()[0].tolist() == [R.DBL_MAX, -R.DBL_MAX, 0.0, 0.0, 0.0, 7.0]


# ---------------------------------------------------------------- determinism and ABI
def test_two_calls_give_the_same_bits():
    buf = normal(2 ** 20 + 300, 13)
    h = Hist([buf[3:2 ** 20 + 3], buf[2 ** 20 + 3:2 ** 20 + 203], buf[2 ** 20 + 203:]])
    rc1, c1, s1 = h.call()
    rc2, c2, s2 = h.call()
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(c1, c2) and torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    assert int(c1.sum()) == 2 ** 20 + 297                 # (the three views leave out the first 3 elements)


def test_bad_arguments_return_an_error_and_launch_nothing():
    L = hip.lib()
    h = Hist([normal(100, 17)])
    for over, word in ((dict(n_items=0), b"n_items"), (dict(limits=None), b"NULL"),
                       (dict(ws_bytes=h.ws_bytes - 1), b"ws_bytes"), (dict(n_limits=4096), b"n_limits")):
        rc, counts, stats = h.call(**over)
        assert rc == 1 and word in L.bg_last_error(), (over, L.bg_last_error())
        assert bool((counts == -7).all()) and bool((stats == -7.0).all())            # nothing ran
    big = (hip.BgHistItem * 1)()
    big[0].x, big[0].n = h.views[0].data_ptr(), 1 << 32
    nc = ctypes.c_int(0)
    assert L.bg_var_hist_plan_chunks(big, 1, ctypes.byref(nc)) == 1 and b"2^32" in L.bg_last_error()
    rc, counts, stats = h.call()
    assert rc == 0 and int(counts.sum()) == 100


# ---------------------------------------------------------------- end to end
def _train(tmp_path, tag, log):
    d = tmp_path / tag
    args = make_args(img_size=64, ch=8, batch_size=4, z_dim=64, histogram_freq=2, log_dir=str(d / "logs"),
                     checkpoint_dir=str(d / "ckpt"), sample_dir=str(d / "samples"))
    gan = model.BigGAN(args, store=S.VariableStore("cuda", seed=5)).build_model()
    seen = []
    step = gan.train_step

    def recording_step(*a, **k):
        out = step(*a, **k)
        seen.append({name: np.float32(v.item()) for name, v in out.items()})
        return out

    gan.train_step = recording_step
    gan.log_events = log
    gan.train(iterations=3, resume=False)
    return gan, seen, str(d / "logs")


def test_training_writes_the_losses_and_the_histograms_and_changes_nothing(tmp_path):
    gan, seen, logs = _train(tmp_path, "logged", True)
    d = os.path.join(logs, gan.model_dir)
    files = os.listdir(d)
    assert len(files) == 1
    ev = R.read_events(os.path.join(d, files[0]))
    assert ev[0]["file_version"] == "brain.Event:2"
    scalars = [e for e in ev[1:] if e["values"][0][1] == "scalar"]
    hists = [e for e in ev[1:] if e["values"][0][1] == "histo"]
    assert [e["step"] for e in scalars] == [0, 1, 2] and [e["step"] for e in hists] == [0, 2]
    assert len(seen) == 3 and "d_loss" in seen[0] and "g_loss" in seen[0]
    for e, want in zip(scalars, seen):
        assert [(t, v) for t, _, v in e["values"]] == list(want.items())
    # the histograms of step 2 were taken after the last update: they describe the variables as they are now
    names = list(gan.store.vars)
    assert [t for t, _, _ in hists[1]["values"]] == [n + "_0/hist" for n in names]
    for (tag, _, h), name in zip(hists[1]["values"], names):
        ref = R.histogram(gan.store.vars[name].detach().cpu().numpy())
        ds, dq = R.sum_bounds(ref)
        assert (h["min"], h["max"], h["num"]) == (ref["min"], ref["max"], ref["num"]), name
        assert abs(h["sum"] - ref["sum"]) <= ds and abs(h["sum_squares"] - ref["sum_squares"]) <= dq, name
        assert list(zip(h["bucket_limit"], h["bucket"])) == R.collapse(ref["counts"]), name
    # logging leaves the run bit-identical
    plain, seen2, logs2 = _train(tmp_path, "plain", False)
    assert not os.path.exists(logs2)
    assert seen2 == seen
    a, b = gan.state_tensors(), plain.state_tensors()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
