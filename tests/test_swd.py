"""The sliced Wasserstein score without a GPU: the float64 restatement (tests/swd_ref.py) against scipy, its invariances,
the mutation tests of the gates that tests/test_gpu_swd.py uses, the host plan (metrics.SwdPlan), the flags, the C ABI
and the event-file scalars."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import scipy.stats
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, metrics, trainlog
from tests import swd_ref as R, trainlog_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bg_swd_pyr_down", "bg_swd_pyr_lap", "bg_swd_stats_workspace_bytes", "bg_swd_descriptors",
               "bg_swd_stats_finish", "bg_swd_project", "bg_swd_sort_tile", "bg_swd_sort_segments",
               "bg_swd_l1_workspace_bytes", "bg_swd_l1")


@pytest.fixture(scope="module")
def e2e():
    """The end-to-end case of the GPU test: its inputs, draws, descriptors, reference distances and gates, computed once."""
    return R.end_to_end_case(0)


# ---------------------------------------------------------------- reference self-checks
def test_pyramid_agrees_with_scipy_mirror():
    rng = np.random.RandomState(1)
    x = rng.uniform(-1, 1, size=(2, 32, 32, 3))
    want = np.stack([np.stack([scipy.ndimage.convolve(x[b, :, :, c], R.W25, mode="mirror") for c in range(3)], axis=-1)
                     for b in range(2)])
    assert np.abs(R.blur(x) - want).max() < 1e-15
    assert np.array_equal(R.down(x), R.blur(x)[:, ::2, ::2])
    u = np.zeros((2, 64, 64, 3))
    u[:, ::2, ::2] = x
    want_up = np.stack([np.stack([scipy.ndimage.convolve(u[b, :, :, c], 4 * R.W25, mode="mirror") for c in range(3)], axis=-1)
                        for b in range(2)])
    assert np.abs(R.up(x) - want_up).max() < 1e-15
    # a constant image is a fixed point of both operators, so its Laplacian levels vanish
    lap = R.laplacian_pyramid(np.full((1, 64, 64, 1), 0.75))
    assert [l.shape[1] for l in lap] == [64, 32, 16] == R.level_sides(64)
    assert max(np.abs(l).max() for l in lap[:-1]) < 1e-15 and np.abs(lap[-1] - 0.75).max() < 1e-15


def test_levels():
    assert [len(R.level_sides(s)) for s in (64, 128, 256, 512)] == [3, 4, 5, 6]
    assert [len(metrics.level_sides(s)) for s in (64, 128, 256, 512)] == [3, 4, 5, 6]
    assert metrics.level_sides(128) == R.level_sides(128) == [128, 64, 32, 16]


def test_column_distance_agrees_with_scipy(e2e):
    lv = e2e["levels"][0]
    pa, pb = R.normalise(lv["da"]) @ lv["dirs"].astype(np.float64), R.normalise(lv["db"]) @ lv["dirs"].astype(np.float64)
    want = np.mean([scipy.stats.wasserstein_distance(pa[:, s], pb[:, s]) for s in range(pa.shape[1])])
    assert abs(lv["dist"] - want) < 1e-15


def test_identical_sets_shuffles_and_affine_maps(e2e):
    lv = e2e["levels"][0]
    assert R.distance(lv["da"], lv["da"], lv["dirs"], 2) == 0.0
    perm = np.random.RandomState(2).permutation(lv["db"].shape[0])
    assert abs(R.distance(lv["da"], lv["db"][perm], lv["dirs"], 2) - lv["dist"]) < 1e-15
    assert abs(R.distance(lv["da"], 0.3 * lv["db"].astype(np.float64) + 0.2, lv["dirs"], 2) - lv["dist"]) < 1e-12


def test_a_constant_channel_gives_zero_descriptors_and_a_finite_score():
    rng = np.random.RandomState(3)
    img = rng.uniform(-1, 1, size=(2, 2, 16, 16, 4))
    img[..., 3] = 1.0                                   # a constant alpha plane
    pos = R.draw_positions(rng, 2, 16)
    da, db = R.descriptors(img[0], pos), R.descriptors(img[1], pos)
    n = R.normalise(da)
    assert not n[:, 3 * 49:].any() and n[:, :3 * 49].std() > 0.9
    assert np.isfinite(R.distance(da, db, R.draw_directions(rng, 196, 2, 16), 2))


def test_descriptor_layout_and_out_of_range_centres():
    level = np.arange(2 * 16 * 16 * 3, dtype=np.float64).reshape(2, 16, 16, 3)
    pos = np.full((2, 128, 2), 8, np.int32)
    pos[0, 0], pos[0, 1], pos[1, 5], pos[1, 6] = (3, 3), (12, 12), (2, 8), (8, 13)
    d = R.descriptors(level, pos)
    assert d.shape == (256, 147)
    assert d[0, 0] == level[0, 0, 0, 0] and d[0, 1] == level[0, 0, 1, 0] and d[0, 7] == level[0, 1, 0, 0]
    assert d[0, 49] == level[0, 0, 0, 1] and d[1, 146] == level[0, 15, 15, 2]
    assert not d[128 + 5].any() and not d[128 + 6].any() and d[128 + 7].any()


# ---------------------------------------------------------------- the gates catch what they are for
def test_the_end_to_end_inputs_separate_the_sets_by_100_gates(e2e):
    for side, lv in zip(e2e["sides"], e2e["levels"]):
        print("level %d: distance %.6g gate %.3g ratio %.1f" % (side, lv["dist"], lv["gate"], lv["dist"] / lv["gate"]))
        assert lv["dist"] >= 100 * lv["gate"], side


def test_pyramid_gate_catches_ten_bounds():
    rng = np.random.RandomState(4)
    x = rng.uniform(-1, 1, size=(1, 32, 32, 3)).astype(np.float32)
    ref, bound = R.down(x), R.down_bound(x)
    assert (np.abs(ref.astype(np.float32) - ref) <= bound).all()            # fp32 rounding of the exact value passes
    bad = ref.copy()
    bad[0, 5, 7, 1] += 10 * bound[0, 5, 7, 1]
    assert not (np.abs(bad - ref) <= bound).all()
    g1 = ref.astype(np.float32)
    lap, lb = x - R.up(g1), R.lap_bound(x, g1)
    assert (np.abs(lap.astype(np.float32) - lap) <= lb).all()
    bad = lap.copy()
    bad[0, 0, 31, 2] -= 10 * lb[0, 0, 31, 2]
    assert not (np.abs(bad - lap) <= lb).all()


def test_distance_gate_catches_ten_bounds(e2e):
    """A projection error of 10 gates in one set, on every entry, moves the distance by more than the gate."""
    lv = e2e["levels"][0]
    pa = np.sort(R.normalise(lv["da"]) @ lv["dirs"].astype(np.float64), axis=0)
    pb = np.sort(R.normalise(lv["db"]) @ lv["dirs"].astype(np.float64), axis=0)
    base = np.abs(pa - pb).mean()
    sign = np.where(pa >= pb, 1.0, -1.0)
    moved = np.abs(pa + 10 * lv["gate"] * sign - pb).mean()
    assert abs(base - lv["dist"]) < 1e-15 and abs(moved - base) > lv["gate"]


def test_stats_and_l1_gates_catch_ten_bounds(e2e):
    mean, std = R.channel_stats(e2e["levels"][1]["da"])
    for v in (mean, 1.0 / std):
        assert not (np.abs(v * (1 + 1e-11) - v) <= 1e-12 * np.abs(v)).all()


def test_sort_check_catches_one_swapped_pair():
    x = np.random.RandomState(5).randn(3, 64).astype(np.float32)
    want = np.sort(x, axis=1)
    assert np.array_equal(np.sort(x, axis=1), want)
    bad = want.copy()
    bad[1, [10, 11]] = bad[1, [11, 10]]
    assert not np.array_equal(bad, want)


# ---------------------------------------------------------------- the plan
PLAN_CASES = [   # img_size, c_dim, swd_images, n_files -> n_images
    (64, 3, 2048, None, 2048), (128, 3, 2047, None, 1024), (256, 4, 8, None, 8), (512, 1, 3000, None, 2048),
    (64, 3, 2048, 100, 64), (64, 3, 16, 100, 16), (64, 3, 9, 8, 8), (128, 3, 1, 5, 1), (64, 3, 64, 64, 64)]


@pytest.mark.parametrize("case", PLAN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_plan_invariants(case):
    img_size, c_dim, swd_images, n_files, want = case
    p = metrics.SwdPlan(img_size, c_dim, 4, swd_images, 123456789, n_files=n_files)
    assert p.n_images == want and p.n_images & (p.n_images - 1) == 0
    assert p.n_images <= swd_images and (n_files is None or p.n_images <= n_files)
    assert 2 * p.n_images > min(swd_images, n_files or swd_images)                # the largest such power of two
    assert p.sides == R.level_sides(img_size) and p.sides[-1] == 16
    assert p.n_rows == 128 * p.n_images and p.K == 49 * c_dim and p.S == 512
    assert p.n_rows & (p.n_rows - 1) == 0                                          # the sort's segment length
    assert p.desc_bytes == p.n_rows * p.K * 4 and p.real_bytes == len(p.sides) * p.desc_bytes
    assert p.projection_bytes == 2 * 512 * p.n_rows * 4
    assert p.peak_bytes == 2 * p.real_bytes + p.projection_bytes
    assert len(set(p.seeds.values())) == len(p.seeds) == 6


def test_plan_budget_at_512px_and_2048_images():
    p = metrics.SwdPlan(512, 3, 256, 2048, 1)
    assert p.real_bytes <= 0.95e9 and p.projection_bytes == 1 << 30


def test_plan_rejects_what_it_cannot_measure():
    with pytest.raises(ValueError):
        metrics.SwdPlan(64, 3, 4, 0, 1)
    with pytest.raises(ValueError):
        metrics.SwdPlan(64, 3, 4, 8, 1, n_files=0)
    with pytest.raises(ValueError):
        metrics.SwdPlan(16, 3, 4, 8, 1)
    with pytest.raises(ValueError):
        metrics.SwdPlan(96, 3, 4, 8, 1)
    with pytest.raises(ValueError):
        metrics.SwdPlan(64, 2, 4, 8, 1)


def test_the_same_seeds_give_the_same_draws_and_touch_no_other_generator():
    np_state = np.random.get_state()[1].copy()
    torch_state = torch.get_rng_state().clone()

    def draws(seed):
        p = metrics.SwdPlan(64, 3, 4, 8, seed)
        return (p.draw_directions(), p.draw_positions("real"), p.draw_positions("fake"),
                [p.draw_latents(32, True).numpy()], [p.draw_labels(np.eye(5, dtype=np.float32))])
    a, b, c = draws(7), draws(7), draws(8)
    for xa, xb, xc in zip(a, b, c):
        assert all(np.array_equal(u, v) for u, v in zip(xa, xb))
        assert not all(np.array_equal(u, v) for u, v in zip(xa, xc))
    dirs, pos_r, pos_f, z, cls = a
    assert [d.shape for d in dirs] == [(147, 512)] * 3 and dirs[0].dtype == np.float32
    assert np.abs(np.sqrt((dirs[0].astype(np.float64) ** 2).sum(axis=0)) - 1).max() < 1e-6
    assert not np.array_equal(dirs[0], dirs[1]) and not np.array_equal(pos_r[0], pos_f[0])
    for side, p in zip((64, 32, 16), pos_r):
        assert p.shape == (8, 128, 2) and p.dtype == np.int32 and p.min() == 3 and p.max() == side - 4
    assert z[0].shape == (8, 1, 1, 32) and np.abs(z[0]).max() <= 2.0
    assert cls[0].shape == (8, 5) and (cls[0].sum(axis=1) == 1).all()
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


# ---------------------------------------------------------------- flags, ABI, event file
def test_flags_parse_with_their_defaults():
    args = M.parse_args(["--gan_type", "hinge"], make_dirs=False)
    assert args.swd_freq == 0 and args.swd_images == 2048
    args = M.parse_args(["--swd_freq", "500", "--swd_images", "256"], make_dirs=False)
    assert args.swd_freq == 500 and args.swd_images == 256
    assert ("swd_freq", int, 0) in M.EXTRA_FLAGS and ("swd_images", int, 2048) in M.EXTRA_FLAGS
    assert len(M.FLAGS) == 119 and not any(n.startswith("swd") for n, _, _ in M.FLAGS)


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "biggan_hip.h")).read()
    assert re.search(r"#define BG_ABI_VERSION 10\b", header) and hip.ABI_VERSION == 10
    for name in NEW_SYMBOLS:
        res, args = hip.SIGNATURES[name]
        decl = re.search(r"\b(int|size_t)\s+%s\(([^)]*)\)" % name, header)
        assert decl, name
        assert res is (ctypes.c_int if decl.group(1) == "int" else ctypes.c_size_t), name
        params = [p for p in decl.group(2).split(",") if p.strip() != "void"]
        assert len(params) == len(args), name
        for text, ctype in zip(params, args):
            want = ctypes.c_void_p if "*" in text else ctypes.c_int64 if "int64_t" in text else \
                ctypes.c_size_t if "size_t" in text else ctypes.c_int
            assert ctype is want, (name, text)
    assert "swd.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    L = hip.lib()
    assert L.bg_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    tile = L.bg_swd_sort_tile()
    assert tile >= 1024 and tile & (tile - 1) == 0
    assert L.bg_swd_stats_workspace_bytes(8, 3) == 8 * 3 * 2 * 8 and L.bg_swd_l1_workspace_bytes(1 << 20, 4) % 8 == 0


def test_the_entry_points_check_their_arguments_before_any_launch():
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails validation
    assert L.bg_swd_pyr_down(None, 0, fake, 2, 32, 3, None) == 1 and b"NULL" in L.bg_last_error()
    assert L.bg_swd_pyr_down(fake, 2, fake, 2, 32, 3, None) == 1 and b"dtype" in L.bg_last_error()
    assert L.bg_swd_pyr_down(fake, 0, fake, 2, 16, 3, None) == 1 and L.bg_swd_pyr_down(fake, 0, fake, 2, 48, 3, None) == 1
    assert L.bg_swd_pyr_down(fake, 0, fake, 2, 32, 2, None) == 1
    assert L.bg_swd_pyr_lap(fake, 1, None, fake, 2, 32, 3, None) == 1
    assert L.bg_swd_pyr_lap(fake, 7, fake, fake, 2, 32, 3, None) == 1
    assert L.bg_swd_descriptors(fake, fake, 2, 16, 3, fake, 256, 128, fake, 1 << 20, None) == 1      # rows 128 + 256 > 256
    assert L.bg_swd_descriptors(fake, fake, 2, 16, 3, fake, 256, 64, fake, 1 << 20, None) == 1       # offset not x 128
    assert L.bg_swd_descriptors(fake, fake, 2, 16, 3, fake, 256, 0, fake, 8, None) == 1              # partials too small
    assert L.bg_swd_stats_finish(fake, 8, 2, 3, fake, None) == 1
    assert L.bg_swd_project(fake, fake, fake, None, fake, fake, 128, 3, 32, None) == 1               # half a second set
    assert L.bg_swd_project(fake, fake, None, None, fake, fake, 100, 3, 32, None) == 1               # N not x 64
    assert L.bg_swd_project(fake, fake, None, None, fake, fake, 128, 2, 32, None) == 1
    for seg_len in (0, 1, 3, 96, 1 << 25):
        assert L.bg_swd_sort_segments(fake, 1, seg_len, None) == 1, seg_len
    assert L.bg_swd_sort_segments(fake, 0, 64, None) == 1
    assert L.bg_swd_sort_segments(ctypes.c_void_p(4100), 1, 8192, None) == 1 and b"aligned" in L.bg_last_error()
    assert L.bg_swd_l1(fake, fake, 1024, 2, fake, fake, 8, None) == 1
    assert L.bg_swd_l1(fake, fake, 0, 2, fake, fake, 1 << 20, None) == 1


def test_event_file_holds_the_scores(tmp_path):
    scores = {"swd_64": 12.5, "swd_32": 3.25, "swd_16": 0.125, "swd_avg": 5.291666507720947}
    w = trainlog.EventWriter(str(tmp_path))
    w.add_scalars(41, scores)
    w.close()
    ev = TR.read_events(w.path)
    assert ev[1]["step"] == 41
    assert [(t, kind, float(v)) for t, kind, v in ev[1]["values"]] == [(k, "scalar", float(np.float32(v)))
                                                                       for k, v in scores.items()]
    assert metrics.format_scores(scores).startswith("swd_64: 12.5000, swd_32: 3.2500")
