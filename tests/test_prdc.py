"""Precision / recall / density / coverage (metrics.PrdcPlan / Prdc, csrc/prdc.hip): flags, the ABI, the plan's arithmetic,
the float64 reference of tests/prdc_ref.py against itself, and its mutations against the case tables.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, metrics
from tests import prdc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bg_prdc_radii", "bg_prdc_cover", "bg_prdc_reduce")


# ---------------------------------------------------------------- flags and ABI
def test_flags_parse_with_their_defaults():
    args = M.parse_args(["--gan_type", "hinge"], make_dirs=False)
    assert (args.pr_freq, args.pr_images, args.pr_k, args.pr_size) == (0, 4096, 3, 64)
    args = M.parse_args(["--pr_freq", "500", "--pr_images", "64", "--pr_k", "5", "--pr_size", "32"], make_dirs=False)
    assert (args.pr_freq, args.pr_images, args.pr_k, args.pr_size) == (500, 64, 5, 32)
    for flag in (("pr_freq", int, 0), ("pr_images", int, 4096), ("pr_k", int, 3), ("pr_size", int, 64)):
        assert flag in M.EXTRA_FLAGS
    assert len(M.FLAGS) == 119 and not any(n.startswith("pr_") for n, _, _ in M.FLAGS)


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "biggan_hip.h")).read()
    assert re.search(r"#define BG_ABI_VERSION 10\b", header) and hip.ABI_VERSION == 10
    for name in NEW_SYMBOLS:
        res, args = hip.SIGNATURES[name]
        decl = re.search(r"\bint\s+%s\(([^)]*)\)" % name, header)
        assert decl and res is ctypes.c_int, name
        params = decl.group(1).split(",")
        assert len(params) == len(args), name
        for text, ctype in zip(params, args):
            want = ctypes.c_void_p if "*" in text else ctypes.c_int64 if "int64_t" in text else ctypes.c_int
            assert ctype is want, (name, text)
    assert "prdc.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    L = hip.lib()
    assert L.bg_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None


def test_the_entry_points_check_their_arguments_before_any_launch():
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails validation

    def radii(x=fake, N=20, D=192, k=3, out=fake):
        return L.bg_prdc_radii(x, N, D, k, out, None)

    def cover(q=fake, rad=fake, Q=20, s=fake, N=20, D=192, count=fake, dmin=fake):
        return L.bg_prdc_cover(q, rad, Q, s, N, D, count, dmin, None)

    def reduce(cf=fake, M_=20, cr=fake, dm=fake, rr=fake, N=20, out=fake):
        return L.bg_prdc_reduce(cf, M_, cr, dm, rr, N, out, None)

    def rejected(rc, word):
        return rc == 1 and word in L.bg_last_error()

    assert rejected(radii(x=None), b"NULL") and rejected(radii(out=None), b"NULL")
    assert rejected(cover(q=None), b"NULL") and rejected(cover(s=None), b"NULL")
    assert rejected(cover(count=None, dmin=None), b"both NULL") and rejected(cover(rad=None), b"radius_q")
    for name in ("cf", "cr", "dm", "rr", "out"):
        assert rejected(reduce(**{name: None}), b"NULL"), name
    for D in (0, 32, 96, 200, -64):
        assert rejected(radii(D=D), b"D=") and rejected(cover(D=D), b"D="), D
    for k in (0, 9, -1):
        assert rejected(radii(k=k), b"k="), k
    for N, k in ((3, 3), (1, 1), (8, 8), (0, 1), (-5, 1)):
        assert rejected(radii(N=N, k=k), b"N="), (N, k)
    assert rejected(cover(Q=0), b"Q=") and rejected(cover(N=0), b"N=") and rejected(cover(Q=1 << 31), b"Q=")
    assert rejected(reduce(M_=0), b"M=") and rejected(reduce(N=0), b"N=")
    odd, half = ctypes.c_void_p(4104), ctypes.c_void_p(4098)
    assert rejected(radii(x=odd), b"aligned") and rejected(radii(out=half), b"aligned")
    assert rejected(cover(q=odd), b"aligned") and rejected(cover(s=odd), b"aligned")
    assert rejected(cover(rad=half), b"aligned") and rejected(cover(count=half), b"aligned")
    assert rejected(cover(dmin=half), b"aligned")
    assert rejected(reduce(cf=half), b"aligned") and rejected(reduce(out=ctypes.c_void_p(4100)), b"aligned")


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("c_dim", [1, 3, 4])
def test_plan_arithmetic(c_dim):
    p = metrics.PrdcPlan(128, c_dim, 8, pr_images=100, pr_k=3, pr_size=64, static_sample_seed=7, n_files=1000)
    assert (p.side, p.f, p.D, p.k, p.N, p.M) == (64, 2, 64 * 64 * c_dim, 3, 100, 100) and p.D % 64 == 0 and p.from_files
    assert metrics.PrdcPlan(32, c_dim, 8, pr_images=100, pr_size=64).side == 32          # larger than the image: clamped
    assert metrics.PrdcPlan(256, c_dim, 8, pr_images=100, pr_size=8).D == 64 * c_dim
    capped = metrics.PrdcPlan(64, c_dim, 8, pr_images=100, pr_k=3, n_files=24)
    assert (capped.N, capped.M, capped.n_real, capped.n_images) == (24, 100, 24, 100)
    synthetic = metrics.PrdcPlan(64, c_dim, 8, pr_images=100)
    assert (synthetic.N, synthetic.M, synthetic.from_files) == (100, 100, False)
    # two descriptor sets and O(N) vectors
    sets = capped.N * capped.D * 2 + capped.M * capped.D * 2
    assert capped.peak_bytes - sets == capped.vector_bytes == 8 * (24 + 100) + 4 * 24 + 32
    assert capped.set_bytes == 100 * capped.D * 2
    default = metrics.PrdcPlan(128, 3, 256)
    assert (default.N, default.M, default.D, default.k) == (4096, 4096, 12288, 3)
    assert default.peak_bytes == 2 * 4096 * 12288 * 2 + 20 * 4096 + 32


def test_bad_flags_raise():
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            metrics.PrdcPlan(64, 3, 8, pr_images=100, pr_k=k)
    for images, k in ((3, 3), (1, 1), (0, 1), (8, 8)):
        with pytest.raises(ValueError):
            metrics.PrdcPlan(64, 3, 8, pr_images=images, pr_k=k)
    with pytest.raises(ValueError):
        metrics.PrdcPlan(64, 3, 8, pr_images=100, pr_k=3, n_files=3)           # the dataset is too small for k
    for size in (0, 4, 48):
        with pytest.raises(ValueError):
            metrics.PrdcPlan(64, 3, 8, pr_images=100, pr_size=size)
    with pytest.raises(ValueError):
        metrics.PrdcPlan(64, 2, 8, pr_images=100)
    with pytest.raises(ValueError):
        metrics.PrdcPlan(48, 3, 8, pr_images=100)


def test_seeds_and_draws():
    p, q = metrics.PrdcPlan(64, 3, 8, pr_images=20, static_sample_seed=7), metrics.PrdcPlan(64, 3, 8, pr_images=20, static_sample_seed=8)
    assert len(set(p.seeds.values())) == 3 and set(p.seeds.values()).isdisjoint(q.seeds.values())
    other = metrics.PowerSpectrumPlan(64, 3, 8, 20, 7)
    assert set(p.seeds.values()).isdisjoint(other.seeds.values())
    z = p.draw_latents(16, True)
    assert tuple(z.shape) == (20, 1, 1, 16) and np.array_equal(z.numpy(), p.draw_latents(16, True).numpy())
    assert not np.array_equal(z.numpy(), q.draw_latents(16, True).numpy())
    table = np.eye(5, dtype=np.float32)
    tags = p.draw_labels(table)
    assert tuple(tags.shape) == (20, 5) and np.array_equal(np.asarray(tags), np.asarray(p.draw_labels(table)))


def test_ratios_come_from_the_four_integers():
    got = metrics.Prdc.ratios([3, 7, 5, 2], 3, 10, 4)
    assert got == {"pr_precision": 0.75, "pr_recall": 0.5, "pr_density": 7 / 12.0, "pr_coverage": 0.2}
    assert list(got) == ["pr_precision", "pr_recall", "pr_density", "pr_coverage"]
    assert metrics.Prdc.ratios([3, 7, 5, 2], 3, 10, 4, prefix="x") == {"x_" + k[3:]: v for k, v in got.items()}
    assert R.ratios([3, 7, 5, 2], 3, 10, 4) == {k[3:]: v for k, v in got.items()}


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("k", [1, 3, 8])
def test_identical_sets_without_ties(k):
    x = R.bf16_round(np.random.default_rng(k).uniform(-1, 1, size=(40, 64)))
    d = R.distances(x, x)
    assert len(np.unique(d[np.triu_indices(40, 1)])) == 40 * 39 // 2               # no ties
    s = R.scores(x, x, k)
    assert s["precision"] == 1.0 and s["recall"] == 1.0 and s["coverage"] == 1.0
    # row i holds f_j within rad_k(r_i) for itself and its k nearest others: k + 1 per ball
    assert s["density"] == (k + 1) / float(k)


def test_a_far_away_fake_set_scores_nothing():
    rng = np.random.default_rng(5)
    real = R.bf16_round(rng.uniform(-0.1, 0.1, size=(30, 64)))                 # radii at most 64 * 0.2^2
    fake = R.bf16_round(rng.uniform(-0.1, 0.1, size=(25, 64)) + 0.875)         # every d(f, r) at least 64 * 0.65^2
    assert R.scores(real, fake, 3) == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}


def test_radius_is_by_index_and_ties_count_with_multiplicity():
    x = np.array([[0.0], [0.0], [1.0], [1.0], [3.0]]) * np.ones((1, 64))
    # row 0: others at 0, 64, 64, 576
    assert R.radii(x, 1).tolist() == [0.0, 0.0, 0.0, 0.0, 256.0]
    assert R.radii(x, 2).tolist() == [64.0, 64.0, 64.0, 64.0, 256.0]
    assert R.radii(x, 3).tolist() == [64.0, 64.0, 64.0, 64.0, 576.0]
    assert np.array_equal(R.radii(x, 2, R.distances_exact), R.radii(x, 2))
    count, dmin = R.cover(x[:2], [0.0, 64.0], x[2:])
    assert count.tolist() == [1, 1, 0] and dmin.tolist() == [64.0, 64.0, 576.0]    # <= is inclusive


def test_the_exact_matrix_equals_the_float64_one():
    for case in range(len(R.COVER_CASES)):
        q, _, s = R.cover_operands(case)
        assert np.array_equal(R.distances_exact(q, s), R.distances(q, s))
    assert R.distances_exact(np.ones((1, 2112)), -np.ones((1, 2112)))[0, 0] == 4.0 * 2112   # the largest sum there is


# ---------------------------------------------------------------- the case tables
def test_the_case_tables_cover_what_they_should():
    assert R.RADII_CASES == [(9, 64, 8), (16, 64, 1), (17, 192, 3), (61, 2112, 3), (203, 576, 5)]
    assert R.COVER_CASES == [(1, 1, 64), (8, 16, 64), (13, 17, 192), (197, 203, 2112), (75, 130, 576)]
    assert R.GENERIC_CASES == [(203, 197, 192, 3), (203, 197, 2112, 5), (130, 75, 576, 1)]
    x = R.radii_operands(3)
    assert np.array_equal(x[5], x[40]) and np.array_equal(x[6], x[40])
    rad = R.radii(x, 3, R.distances_exact)
    assert rad[5] == rad[6] == rad[40] > 0 and R.radii(x, 2, R.distances_exact)[[5, 6, 40]].tolist() == [0.0, 0.0, 0.0]
    for case, (Q, N, D) in enumerate(R.COVER_CASES):
        q, rad, s = R.cover_operands(case)
        assert q.shape == (Q, D) and s.shape == (N, D) and np.array_equal(rad.astype(np.float32), rad)
        assert np.abs(q).max() <= 1 and np.array_equal(np.rint(q * 8), q * 8)
        d = R.distances_exact(q, s)
        assert rad[0] == d[0, N // 2]                                   # a radius equal to an attained distance
        if Q > 2:
            assert rad[1] == 0.0 and d[1, 3] == 0.0 and rad[2] == np.inf
        if N > 7:
            count, dmin = R.cover(q, rad, s, R.distances_exact)
            assert not s[7].any() and dmin[7] > 0 and q.any(axis=1).all()


@pytest.mark.parametrize("case", range(len(R.GENERIC_CASES)))
def test_the_generic_cases_are_decided_and_not_trivial(case):
    """The condition of the device test: at most 0.2 % of the pairs of either cover pass are undecided.  Recorded from this
    reference (undecided pairs of cover(q = real) / cover(q = fake) of all pairs): 0 / 1 of 39991, 29 / 24 of 39991,
    0 / 1 of 9750; scores P .640 R .764 D .829 C .483, P .716 R .842 D .761 C .507, P .240 R .823 D .400 C .177."""
    real, fake, k = R.generic_operands(case)
    N, M, D, _ = R.GENERIC_CASES[case]
    assert real.shape == (N, D) and fake.shape == (M, D)
    assert np.array_equal(R.bf16_round(real), real) and np.array_equal(R.bf16_round(fake), fake)
    rr, rf = R.radii(real, k), R.radii(fake, k)
    for q, rad, s in ((real, rr, fake), (fake, rf, real)):
        _, open_, _, share = R.cover_bands(q, rad, s)
        print("case %d: %d undecided of %d" % (case, open_.sum(), len(q) * len(s)))
        assert share <= R.UNDECIDED_SHARE
    s = R.scores(real, fake, k)
    print("case %d: %s" % (case, s))
    assert all(0.1 < v < 0.95 for v in s.values())
    for name, (lo, hi) in R.score_bands(real, fake, k).items():
        assert lo <= s[name] <= hi and hi - lo <= 0.05


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_reference_is_caught_by_the_case_tables(mutation):
    caught = []
    for case, (N, D, k) in enumerate(R.RADII_CASES):
        x = R.radii_operands(case)
        if not np.array_equal(R.radii(x, k, R.distances_exact), R.radii(x, k, R.distances_exact, mutation)):
            caught.append(("radii", case))
    for case in range(len(R.COVER_CASES)):
        q, rad, s = R.cover_operands(case)
        want, got = R.cover(q, rad, s, R.distances_exact), R.cover(q, rad, s, R.distances_exact, mutation)
        if not (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])):
            caught.append(("cover", case))
    assert caught, mutation
    if mutation == "padded_query":                      # the all-zero set row is where a padded query shows in dmin
        assert ("cover", 2) in caught
        q, rad, s = R.cover_operands(2)
        assert R.cover(q, rad, s, R.distances_exact, mutation)[1][7] == 0.0
