"""Host side of the nearest-training-image search (neighbours.py): flags, the plan, the merge of the plain and mirrored
lists, the table and the grid; and the float64 reference of tests/nn_ref.py checking itself, with the precondition of the
composed GPU test, so that nothing there has to be skipped."""
import numpy as np
import pytest

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import main as M, neighbours as NB
from tests import nn_ref as R
from tests.common import make_args


# ---------------------------------------------------------------- flags
def test_flags_are_extensions_with_their_defaults():
    for flag in (("nn_freq", int, 0), ("nn_k", int, 3), ("nn_size", int, 64), ("nn_images", int, 0)):
        assert flag in M.EXTRA_FLAGS and flag[0] not in [f[0] for f in M.FLAGS]
    assert len(M.FLAGS) == 119
    a = make_args()
    assert (a.nn_freq, a.nn_k, a.nn_size, a.nn_images) == (0, 3, 64, 0)
    a = make_args(nn_freq=500, nn_k=5, nn_size=32, nn_images=1000)
    assert (a.nn_freq, a.nn_k, a.nn_size, a.nn_images) == (500, 5, 32, 1000)


def test_k_range():
    assert [NB.check_k(k) for k in (1, 3, 8)] == [1, 3, 8]
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            NB.check_k(k)


# ---------------------------------------------------------------- plan
@pytest.mark.parametrize("c_dim", [1, 3, 4])
@pytest.mark.parametrize("img_size", [32, 64, 128, 256, 512])
def test_plan_geometry(img_size, c_dim):
    p = NB.NnPlan(img_size, c_dim, 8, nn_size=64, n_files=100, budget=1 << 30)
    side = min(img_size, 64)
    assert (p.side, p.f, p.D) == (side, img_size // side, side * side * c_dim)
    assert p.D % 64 == 0 and p.N == 100 and p.bytes == 100 * p.D * 2 and not p.truncated and p.from_files


def test_plan_clamps_and_rejects_sides():
    assert NB.NnPlan(32, 3, 8, nn_size=128, n_files=10).side == 32           # larger than the image: clamped
    assert NB.NnPlan(256, 3, 8, nn_size=8, n_files=10).f == 32
    for bad in (48, 4, 0, 100):
        with pytest.raises(ValueError):
            NB.NnPlan(64, 3, 8, nn_size=bad, n_files=10)
    with pytest.raises(ValueError):
        NB.NnPlan(64, 2, 8, n_files=10)


def test_plan_truncation_and_the_image_cut(monkeypatch):
    D = 64 * 64 * 3
    p = NB.NnPlan(64, 3, 8, n_files=1000, budget=100 * D * 2 + 5)
    assert (p.N, p.listed, p.truncated, p.bytes) == (100, 1000, True, 100 * D * 2) and "first 100 of 1000" in p.describe()
    p = NB.NnPlan(64, 3, 8, nn_images=40, n_files=1000, budget=1 << 30)
    assert (p.N, p.listed, p.truncated) == (40, 40, False) and "first" not in p.describe()
    assert NB.NnPlan(64, 3, 8, nn_images=4000, n_files=1000, budget=1 << 30).N == 1000
    # the environment variable is the default budget, in GiB
    monkeypatch.setenv("BG_NN_GB", str(50 * D * 2 / float(1 << 30)))
    assert NB.NnPlan(64, 3, 8, n_files=1000).N == 50
    monkeypatch.delenv("BG_NN_GB")
    assert NB.NnPlan(64, 3, 8, n_files=10).budget == 8 << 30
    # without a dataset: 2048 synthetic images, or --nn_images
    p = NB.NnPlan(64, 3, 8)
    assert (p.N, p.from_files) == (2048, False) and NB.NnPlan(64, 3, 8, nn_images=24).N == 24
    with pytest.raises(ValueError):
        NB.NnPlan(64, 3, 8, n_files=10, budget=100)


# ---------------------------------------------------------------- merge
def test_merge_of_the_plain_and_mirrored_lists():
    plain = [(0.5, 7), (1.0, 3), (2.0, 9)]
    mirrored = [(0.25, 4), (1.0, 3), (1.5, 7), (2.0, 1)]
    got = NB.merge_lists(plain, mirrored, 3)
    assert got == [(0.25, 4, True), (0.5, 7, False), (1.0, 3, False)]        # 7 once, at its smaller distance; 3: plain wins
    assert got == R.merge(plain, mirrored, 3)
    # ordering by (distance, index) across the lists, and a k past the union
    full = NB.merge_lists(plain, mirrored, 8)
    assert full == [(0.25, 4, True), (0.5, 7, False), (1.0, 3, False), (2.0, 1, True), (2.0, 9, False)] == R.merge(plain, mirrored, 8)
    # a mirrored entry that is strictly closer replaces the plain one
    assert NB.merge_lists([(1.0, 3)], [(0.5, 3)], 2) == [(0.5, 3, True)]
    # padding entries are dropped; no mirrored list at all
    assert NB.merge_lists([(0.5, 2), (np.inf, -1)], None, 2) == [(0.5, 2, False)]


def test_merge_agrees_with_the_reference_on_random_lists():
    rng = np.random.RandomState(0)
    for _ in range(50):
        lists = []
        for _ in range(2):
            idx = rng.permutation(12)[:6]
            lists.append(sorted(zip(rng.randint(0, 4, size=6) / 4.0, idx)))
        k = int(rng.randint(1, 9))
        assert NB.merge_lists(lists[0], lists[1], k) == R.merge(lists[0], lists[1], k)


# ---------------------------------------------------------------- table and grid
def _result():
    return {"dist": np.array([[0.30, 0.40], [0.10, 0.50], [0.20, np.inf]]), "index": np.array([[4, 1], [2, 4], [0, -1]]),
            "mirrored": np.array([[False, True], [True, False], [False, False]]),
            "files": [["d/4.png", "d/1.png"], ["d/2.png", "d/4.png"], ["d/0.png", ""]]}


def test_names_table_and_scalars():
    assert NB.event_names("BigGAN", 3, 250) == {"png": "BigGAN_nn_03_00250.png", "txt": "BigGAN_nn_03_00250.txt"}
    assert NB.event_names("BigGAN", 3, 250, "nn_noema")["png"] == "BigGAN_nn_noema_03_00250.png"
    assert NB.tsv_lines(_result()) == ["0\t1\t0.300000\t0\td/4.png", "0\t2\t0.400000\t1\td/1.png",
                                       "1\t1\t0.100000\t1\td/2.png", "1\t2\t0.500000\t0\td/4.png",
                                       "2\t1\t0.200000\t0\td/0.png"]
    s = NB.scalars(_result())
    assert s["nn_dist_min"] == 0.1 and abs(s["nn_dist_mean"] - 0.2) < 1e-12 and list(s) == ["nn_dist_min", "nn_dist_mean"]
    assert list(NB.scalars(_result(), "nn_noema")) == ["nn_noema_dist_min", "nn_noema_dist_mean"]


def test_grid_rows_are_the_most_suspicious_first_and_mirrored_hits_are_flipped(tmp_path):
    res = _result()
    assert NB.grid_queries(res) == [1, 2, 0] and NB.grid_queries(res, 2) == [1, 2]
    many = {"dist": np.arange(12, 0, -1.0)[:, None]}
    assert NB.grid_queries(many) == [11, 10, 9, 8, 7, 6, 5, 4]               # at most 8 rows
    rng = np.random.RandomState(1)
    samples = rng.uniform(-1, 1, size=(3, 8, 8, 3)).astype(np.float32)
    train = rng.uniform(-1, 1, size=(5, 8, 8, 3)).astype(np.float32)
    asked = []

    def fetch(i):
        asked.append(i)
        return train[i]

    g = NB.grid_images(res, [1, 2, 0], samples, fetch)
    assert g.shape == (9, 8, 8, 3)
    assert np.array_equal(g[0], samples[1]) and np.array_equal(g[1], train[2][:, ::-1]) and np.array_equal(g[2], train[4])
    assert np.array_equal(g[3], samples[2]) and np.array_equal(g[4], train[0]) and (g[5] == -1).all()
    assert np.array_equal(g[6], samples[0]) and np.array_equal(g[7], train[4]) and np.array_equal(g[8], train[1][:, ::-1])
    assert -1 not in asked
    # the files: a grid of rows x (k + 1) tiles and the table
    from biggan_tensorflow_amd import data as D
    paths = NB.write_event(res, samples, fetch, str(tmp_path), NB.event_names("m", 0, 2))
    assert [p.split("/")[-1] for p in paths] == ["m_nn_00_00002.png", "m_nn_00_00002.txt"]
    png = D.decode_png(open(paths[0], "rb").read())
    assert png.shape == (3 * 8, 3 * 8, 3)
    assert open(paths[1]).read().splitlines() == NB.tsv_lines(res)


# ---------------------------------------------------------------- the reference checks itself
def test_reference_distances_agree_with_the_definition():
    rng = np.random.RandomState(2)
    q, s = R.random_operands(rng, 3, 5, 192)
    a, b = R.distances(q, s), R.distances_loop(q, s)
    assert np.abs(a - b).max() <= 1e-12 * b.max() and R.planted_equal(3, 5) == (2, 3) and a[2, 3] == 0.0
    x = rng.uniform(-1, 1, size=(2, 16, 16, 3))
    m = R.box_mean(x, 4)
    assert m.shape == (2, 48) and abs(m[1, (2 * 4 + 3) * 3 + 1] - x[1, 8:12, 12:16, 1].mean()) < 1e-15
    assert np.array_equal(R.box_mean(x, 2, mirror=True), R.box_mean(x[:, :, ::-1], 2))
    assert np.array_equal(R.bf16_bits(np.array([1.0, 1.00390625, 1.01171875, -0.5])), [0x3F80, 0x3F80, 0x3F82, 0xBF00])
    v, i = R.topk(np.array([[3.0, 1.0, 1.0, 0.5]]), 3)
    assert v.tolist() == [[0.5, 1.0, 1.0]] and i.tolist() == [[3, 1, 2]]
    v, i = R.topk(np.array([[3.0, 1.0]]), 3)
    assert v.tolist() == [[1.0, 3.0, np.inf]] and i.tolist() == [[1, 0, -1]]


@pytest.mark.parametrize("Q,N,D", R.SMALL_SHAPES)
def test_sequential_fp32_stays_inside_the_bound_and_mutations_leave_it(Q, N, D):
    rng = np.random.RandomState(D + N)
    q, s = R.random_operands(rng, Q, N, D)
    want = R.distances(q, s)
    b = R.bound(D, want)
    assert (np.abs(R.distances_fp32_sequential(q, s) - want) <= b).all()
    assert (np.abs(R.distances_fp32_sequential(q, s, drop_last=8) - want) > b).any()
    side = {192: 8, 1024: 16, 3072: 32}[D]
    assert (np.abs(R.distances_fp32_sequential(q, s, mirror_cols=(side, D // side ** 2)) - want) > b).any()
    if N > 1:
        assert (np.abs(R.distances_fp32_sequential(q, s, row_shift=1) - want) > b).any()
    if Q > 8:
        assert (np.abs(R.distances_fp32_sequential(q, s, reuse_tile=8) - want) > b).any()
    # the exact operands: fp32 in any order equals float64
    q, s = R.exact_operands(rng, Q, N, D)
    assert np.array_equal(R.distances_fp32_sequential(q, s).astype(np.float64), R.distances(q, s))


def test_the_planted_case_is_decided_by_the_reference_alone():
    case = R.planted_case()
    ok, worst = R.gaps_are_decided(case)
    print("smallest non-zero gap / bound among the first k + 1: %.1f" % worst)
    assert ok
    D = case["side"] ** 2 * case["C"]
    want, _ = R.nearest(case["queries"].reshape(case["Q"], D), case["images"].reshape(case["N"], D), case["side"], case["C"],
                        case["k"], True)
    for i, row in enumerate(want):
        slots = case["slots"][i]
        # j = 0, 1, then the tie of j = 2 by index, then 3 .. 6; odd j only through the mirrored search
        tie = sorted([slots[2], slots[8]])
        assert [r[1] for r in row] == [slots[0], slots[1]] + tie + [slots[j] for j in (3, 4, 5, 6)]
        assert [r[2] for r in row] == [False, True, False, False, True, False, True, False]
        assert row[2][0] == row[3][0]
    # uniformly random sets do not meet the condition, which is why the case is planted
    rng = np.random.RandomState(0)
    loose = dict(case, images=R.bf16_round(rng.uniform(-1, 1, size=(20000,) + case["images"].shape[1:])).astype(np.float32), N=20000)
    assert not R.gaps_are_decided(loose)[0]
