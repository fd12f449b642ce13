"""What the four quality monitors share (metrics.MonitorPlan, metrics.Monitor), without a GPU: the seed tables and the draws
of every plan against literals, the event driver on recording stand-ins for the runners, and the bookkeeping of ``add``
and ``finish`` of the runners that take stand-ins for the launch wrappers."""
import weakref

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import metrics, sampling

KINDS = ("swd", "msssim", "ps", "prdc")


def _plan(kind, seed=0, n_files=None):
    """The tiny plans of this file: 8 SWD images, 3 MS-SSIM pairs, 5 spectrum images, 8 PRDC images with k = 3."""
    if kind == "swd":
        return metrics.SwdPlan(32, 3, 4, 8, seed, n_files=n_files)
    if kind == "msssim":
        return metrics.MsssimPlan(32, 3, 4, 3, seed, n_files=n_files)
    if kind == "ps":
        return metrics.PowerSpectrumPlan(32, 3, 4, 5, seed, n_files=n_files)
    return metrics.PrdcPlan(32, 3, 4, pr_images=8, pr_k=3, pr_size=32, static_sample_seed=seed, n_files=n_files)


# ---------------------------------------------------------------- seeds: (base + stride * (i + 1)) % 2^32, by hand
SEEDS_AT_0 = {
    "swd": {"directions": 7919, "pos_real": 15838, "pos_fake": 23757, "latents": 31676, "labels": 39595, "real": 47514},
    "msssim": {"latents": 15485863, "labels": 30971726, "real": 46457589, "real_pairs": 61943452},
    "ps": {"latents": 32452843, "labels": 64905686, "real": 97358529},
    "prdc": {"latents": 49979687, "labels": 99959374, "real": 149939061},
}
# 4294967295 = 2^32 - 1: (2^32 - 1 + x) % 2^32 = x - 1 for every 0 < x < 2^32
SEEDS_AT_MAX = {
    "swd": {"directions": 7918, "pos_real": 15837, "pos_fake": 23756, "latents": 31675, "labels": 39594, "real": 47513},
    "msssim": {"latents": 15485862, "labels": 30971725, "real": 46457588, "real_pairs": 61943451},
    "ps": {"latents": 32452842, "labels": 64905685, "real": 97358528},
    "prdc": {"latents": 49979686, "labels": 99959373, "real": 149939060},
}


@pytest.mark.parametrize("kind", KINDS)
def test_seed_tables_are_the_literals(kind):
    for seed, want in ((0, SEEDS_AT_0), (4294967295, SEEDS_AT_MAX)):
        seeds = _plan(kind, seed).seeds
        assert seeds == want[kind] and list(seeds) == list(want[kind])             # values and order


# ---------------------------------------------------------------- draws
# kind -> (generated images without a dataset, with a 5-file dataset, label rows drawn per image count)
COUNTS = {"swd": (8, 4, 1), "msssim": (6, 6, 2), "ps": (5, 5, 1), "prdc": (8, 8, 1)}
# kind -> real images streamed (without a dataset, with 5 files)
STREAMED = {"swd": (8, 4), "msssim": (6, 4), "ps": (5, 5), "prdc": (8, 5)}


@pytest.mark.parametrize("n_files", [None, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_draws_are_those_of_the_sampler_from_the_literal_seeds(kind, n_files):
    plan = _plan(kind, 0, n_files)
    count = COUNTS[kind][0 if n_files is None else 1]
    per_label = COUNTS[kind][2]
    assert plan.n_fake == count and plan.n_stream == STREAMED[kind][0 if n_files is None else 1]
    assert plan.from_files == (n_files is not None)
    for trunc in (True, False):
        g = torch.Generator(device="cpu")
        g.manual_seed(SEEDS_AT_0[kind]["latents"])
        z = plan.draw_latents(16, trunc)
        assert tuple(z.shape) == (count, 1, 1, 16) and torch.equal(z, sampling.draw_z(count, 16, g, trunc))
    table = np.eye(7, dtype=np.float32)[[0, 3, 6, 2, 5]]
    rows = sampling.draw_n_tags(table, count // per_label, np.random.RandomState(SEEDS_AT_0[kind]["labels"]))
    tags = plan.draw_labels(table)
    assert tags.dtype == np.float32 and tags.shape == (count, 7)
    assert np.array_equal(tags[0::per_label], rows)
    if kind == "msssim":
        assert np.array_equal(tags[0::2], tags[1::2])                              # rows 2 p and 2 p + 1: one class vector
        assert sorted(plan.real_order().tolist()) == list(range(plan.n_stream))    # a matching of the first files
        assert np.array_equal(plan.real_order(), plan.draw_real_pairs().reshape(-1))
    else:
        assert plan.real_order() is None


# ---------------------------------------------------------------- the event driver on recording stand-ins
class _Set:
    """What a stand-in's ``finish`` returns: an object that a weak reference can watch."""


def _recording(kind):
    """The runner class of ``kind`` with ``begin`` / ``add`` / ``finish`` / ``scores`` replaced by recorders; ``begin_set``,
    ``name_scores``, ``real_scores`` and ``event`` are the class's own."""
    base = metrics.MONITORS[kind][1]

    class Recording(base):
        def __init__(self, plan):
            metrics.Monitor.__init__(self, plan, "cpu", ops=object())
            self.calls, self.finished = [], []

        def begin(self, *args):
            self.calls.append(("begin",) + args)

        def add(self, batch):
            self.calls.append(("add", batch))

        def finish(self):
            self.calls.append(("finish",))
            if kind == "msssim":                               # (its finished set is the score itself)
                return 0.25 * len([c for c in self.calls if c == ("finish",)])
            out = _Set()
            self.finished.append(weakref.ref(out))
            return out

        def scores(self, *args):
            prefix = args[-1] if isinstance(args[-1], str) else self.prefix
            assert all(isinstance(a, _Set) for a in args if not isinstance(a, str))
            return {prefix + "_a": 1.0, prefix + "_b": 2.0}

    return Recording(_plan(kind))


# kind -> (the begin of the real set, the begin of a fake set, the ema keys, the noema keys)
EVENTS = {
    "swd": (("begin", "real"), ("begin", "fake"), ["swd_a", "swd_b"], ["swd_noema_a", "swd_noema_b"]),
    "msssim": (("begin", 3), ("begin", None), ["msssim"], ["msssim_noema"]),
    "ps": (("begin", 5), ("begin", None), ["ps_a", "ps_b"], ["ps_a_noema", "ps_b_noema"]),
    "prdc": (("begin", 8), ("begin", None), ["pr_a", "pr_b"], ["pr_a_noema", "pr_b_noema"]),
}


def _drive(m, ema, noema, details=False):
    """One event on stand-ins: the real set is the batches "r0", "r1", "r2"; ``generate`` records itself and checks that no
    finished fake set is alive while the next one is generated (the real set's is the first of ``m.finished``)."""
    def generate(from_ema, consume):
        assert consume == m.add
        if not details:
            assert all(ref() is None for ref in m.finished[1:])
        m.calls.append(("generate", from_ema))

    streams = []

    def real_batches():
        streams.append(1)
        return iter(["r0", "r1", "r2"])

    out, sets = m.event(real_batches, generate, ema, noema, details)
    return out, sets, len(streams)


@pytest.mark.parametrize("kind", KINDS)
def test_the_driver_measures_the_real_set_once_then_ema_then_noema(kind):
    real_begin, fake_begin, ema_keys, noema_keys = EVENTS[kind]
    m = _recording(kind)
    out, sets, streamed = _drive(m, True, True)
    one_set = lambda from_ema: [fake_begin, ("generate", from_ema), ("finish",)]      # noqa: E731
    assert m.calls == [real_begin, ("add", "r0"), ("add", "r1"), ("add", "r2"), ("finish",)] + one_set(True) + one_set(False)
    assert streamed == 1 and sets == {}
    assert list(out) == ema_keys + noema_keys + (["msssim_real"] if kind == "msssim" else [])
    real = m.real
    assert real is not None
    if kind == "msssim":
        assert out == {"msssim": 0.5, "msssim_noema": 0.75, "msssim_real": 0.25}
    else:
        assert m.finished[0]() is real and all(ref() is None for ref in m.finished[1:])   # no fake set is held
    # the second event leaves the real set alone
    del m.calls[:]
    out2, _, streamed = _drive(m, True, True)
    assert m.calls == one_set(True) + one_set(False) and streamed == 0 and m.real is real
    assert list(out2) == ema_keys + noema_keys
    if kind != "msssim":
        assert out2 == {k: out[k] for k in out2} and all(ref() is None for ref in m.finished[1:])


@pytest.mark.parametrize("kind", KINDS)
def test_the_driver_generates_only_what_sample_ema_asks_for(kind):
    _, fake_begin, ema_keys, noema_keys = EVENTS[kind]
    m = _recording(kind)
    out, _, _ = _drive(m, False, True)
    assert [c for c in m.calls if c[0] == "generate"] == [("generate", False)]
    assert m.calls[-3:] == [fake_begin, ("generate", False), ("finish",)]
    assert list(out) == noema_keys + (["msssim_real"] if kind == "msssim" else [])
    m = _recording(kind)
    out, _, _ = _drive(m, True, False)
    assert [c for c in m.calls if c[0] == "generate"] == [("generate", True)]
    assert list(out) == ema_keys + (["msssim_real"] if kind == "msssim" else [])


@pytest.mark.parametrize("kind", ["swd", "ps", "prdc"])
def test_details_keep_the_finished_sets_under_their_tags(kind):
    m = _recording(kind)
    out, sets, _ = _drive(m, True, True, details=True)
    assert list(sets) == [m.prefix, m.prefix + "_noema"] and m.prefix == {"swd": "swd", "ps": "ps", "prdc": "pr"}[kind]
    assert [ref() for ref in m.finished] == [m.real, sets[m.prefix], sets[m.prefix + "_noema"]]
    assert list(out) == EVENTS[kind][2] + EVENTS[kind][3]


# ---------------------------------------------------------------- add / finish of the runners that take ops= stand-ins
class _Ops:
    """Stands in for the launch wrappers of all three runners: records the rows every launch was given."""

    def __init__(self):
        self.rows = []

    def ps_power(self, x):
        self.rows.append(int(x.shape[0]))
        return x

    def ps_profile(self, power, profiles, sum2d):
        assert profiles.shape[0] == power.shape[0]

    def nn_pack(self, x, f, mirrored, out):
        assert out.shape[0] == x.shape[0]
        self.rows.append(int(x.shape[0]))

    def prdc_radii(self, desc, k):
        return torch.zeros(desc.shape[0])

    def msssim_workspace(self, P, H, C, device):
        self.rows.append(2 * P)

    def msssim_level(self, a, b, H, level, ws, pool):
        pass

    def msssim_finish(self, ws, P, H, C, scores, row_offset):
        pass


# kind -> images a fake set takes
RUNNERS = {"msssim": 6, "ps": 5, "prdc": 8}


def _runner(kind):
    ops = _Ops()
    return metrics.MONITORS[kind][1](_plan(kind), "cpu", ops=ops), ops


@pytest.mark.parametrize("kind", list(RUNNERS))
def test_a_last_batch_longer_than_the_rows_still_missing_is_truncated(kind):
    n = RUNNERS[kind]
    m, ops = _runner(kind)
    m.begin()
    m.add(torch.zeros(4, 32, 32, 3))
    m.add(torch.zeros(4, 32, 32, 3))                       # 4 + 4 > 5, 6; = 8
    m.add(torch.zeros(4, 32, 32, 3))                       # nothing is missing any more: no launch
    assert ops.rows == [4, n - 4] and sum(ops.rows) == n
    m.finish()
    # the real set's count is begin's argument
    m.begin(1 if kind == "msssim" else 2)
    m.add(torch.zeros(4, 32, 32, 3))
    assert ops.rows[2:] == [2]
    m.finish()


@pytest.mark.parametrize("kind", list(RUNNERS))
def test_a_wrong_image_shape_raises_the_same_text(kind):
    m, ops = _runner(kind)
    m.begin()
    with pytest.raises(ValueError) as e:
        m.add(torch.zeros(2, 16, 16, 3))
    assert str(e.value) == "%s: images of (16, 16, 3), the plan is for (32, 32, 3)" % kind
    with pytest.raises(ValueError) as e:
        m.add(torch.zeros(2, 32, 32, 4))
    assert str(e.value) == "%s: images of (32, 32, 4), the plan is for (32, 32, 3)" % kind
    assert ops.rows == []


@pytest.mark.parametrize("kind", list(RUNNERS))
def test_finish_one_image_short_raises_the_same_text(kind):
    n = RUNNERS[kind]
    m, _ = _runner(kind)
    m.begin()
    m.add(torch.zeros(n - 1, 32, 32, 3))
    with pytest.raises(RuntimeError) as e:
        m.finish()
    assert str(e.value) == "%s: %d of %d images arrived" % (kind, n - 1, n)


def test_bad_channel_counts_name_their_monitor():
    for kind in KINDS:
        with pytest.raises(ValueError) as e:
            metrics.MONITORS[kind][0](32, 2, 4, 8, 0) if kind != "prdc" else metrics.PrdcPlan(32, 2, 4, pr_images=8)
        assert str(e.value) == "%s: c_dim 2 (1, 3 or 4)" % kind
