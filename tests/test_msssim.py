"""The diversity score (mean MS-SSIM of pairs) without a GPU: the float64 restatement (tests/msssim_ref.py) on known
answers, the gap that sizes the gates of tests/test_gpu_msssim.py, the host plan (metrics.MsssimPlan), the carry logic of
metrics.Msssim on a stand-in for the launch wrappers, the flags and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, metrics, neighbours
from tests import msssim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bg_msssim_workspace_bytes", "bg_msssim_level", "bg_msssim_finish")


# ---------------------------------------------------------------- flags and ABI
def test_flags_parse_with_their_defaults():
    args = M.parse_args(["--gan_type", "hinge"], make_dirs=False)
    assert args.msssim_freq == 0 and args.msssim_pairs == 1024
    args = M.parse_args(["--msssim_freq", "500", "--msssim_pairs", "64"], make_dirs=False)
    assert args.msssim_freq == 500 and args.msssim_pairs == 64
    assert ("msssim_freq", int, 0) in M.EXTRA_FLAGS and ("msssim_pairs", int, 1024) in M.EXTRA_FLAGS
    assert len(M.FLAGS) == 119 and not any(n.startswith("msssim") for n, _, _ in M.FLAGS)


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
    assert "msssim.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    L = hip.lib()
    assert L.bg_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    # fp64 (cs, ssim) per pair, tile of 16 x 16 positions, channel and level
    for S, tiles in ((16, 1), (32, 4 + 1), (64, 16 + 4 + 1), (128, 64 + 16 + 4 + 1), (256, 256 + 64 + 16 + 4 + 1),
                     (512, 1024 + 256 + 64 + 16 + 4)):
        assert L.bg_msssim_workspace_bytes(3, S, 4) == 3 * tiles * 4 * 2 * 8, S
        assert metrics.MsssimPlan(S, 4, 5, 8, 1).workspace_bytes == L.bg_msssim_workspace_bytes(3, S, 4)
    assert L.bg_msssim_workspace_bytes(0, 64, 3) == 0 and L.bg_msssim_workspace_bytes(1, 48, 3) == 0
    assert L.bg_msssim_workspace_bytes(1, 8, 3) == 0 and L.bg_msssim_workspace_bytes(1, 64, 2) == 0


def test_the_entry_points_check_their_arguments_before_any_launch():
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails validation
    big = 1 << 24

    def level(a=fake, b=fake, dtype=0, stride=1, P=2, H=64, lv=0, C=3, pa=fake, pb=fake, ws=fake, nb=big):
        return L.bg_msssim_level(a, b, dtype, stride, P, H, lv, C, pa, pb, ws, nb, None)

    def finish(ws=fake, nb=big, P=2, H=64, C=3, scores=fake, n=8, off=0):
        return L.bg_msssim_finish(ws, nb, P, H, C, scores, n, off, None)

    def rejected(rc, word):
        return rc == 1 and word in L.bg_last_error()

    assert rejected(level(a=None), b"NULL") and rejected(level(b=None), b"NULL") and rejected(level(ws=None), b"NULL")
    assert rejected(level(pa=None), b"pool") and rejected(level(pb=None), b"pool")      # not the last level
    for H in (8, 48, 96, 0, -64):
        assert rejected(level(H=H), b"H="), H
        assert rejected(finish(H=H), b"H="), H
    for C in (0, 2, 5):
        assert rejected(level(C=C), b"C="), C
        assert rejected(finish(C=C), b"C="), C
    assert rejected(level(dtype=2), b"dtype") and rejected(level(dtype=-1), b"dtype")
    assert rejected(level(dtype=1, lv=1), b"fp32")                                      # bf16 at level 0 only
    assert rejected(level(P=0), b"P=") and rejected(level(P=-3), b"P=") and rejected(finish(P=0), b"P=")
    assert rejected(level(stride=0), b"pair_stride")
    assert rejected(level(lv=3), b"level") and rejected(level(lv=-1), b"level")         # 64 px has 3 levels
    need = L.bg_msssim_workspace_bytes(2, 64, 3)
    assert rejected(level(nb=need - 8), b"workspace") and rejected(finish(nb=need - 8), b"workspace")
    assert rejected(level(ws=ctypes.c_void_p(4100)), b"aligned")
    assert rejected(level(pa=ctypes.c_void_p(4098)), b"aligned")
    assert rejected(finish(ws=None), b"NULL") and rejected(finish(scores=None), b"NULL")
    assert rejected(finish(n=8, off=7), b"fit") and rejected(finish(off=-1), b"fit") and rejected(finish(n=1), b"fit")


# ---------------------------------------------------------------- the plan
def test_levels_and_weights_for_every_allowed_side():
    table = {16: 1, 32: 2, 64: 3, 128: 4, 256: 5, 512: 5, 1024: 5}
    for S, L in table.items():
        assert metrics.msssim_sides(S) == R.sides(S) == [S >> i for i in range(L)]
        assert metrics.msssim_sides(S)[-1] >= 16
        p = metrics.MsssimPlan(S, 3, 4, 8, 1)
        assert p.sides == R.sides(S) and len(p.weights) == L
        assert abs(p.weights.sum() - 1.0) < 1e-15 and np.array_equal(p.weights, R.weights(L))
        assert np.allclose(p.weights * sum(metrics.MS_WEIGHTS[:L]), metrics.MS_WEIGHTS[:L], rtol=1e-15)
    assert metrics.MS_WEIGHTS == R.WEIGHTS5
    for bad in (8, 48, 96, 0):
        with pytest.raises(ValueError):
            metrics.msssim_sides(bad)
    with pytest.raises(ValueError):
        metrics.MsssimPlan(64, 2, 4, 8, 1)
    with pytest.raises(ValueError):
        metrics.MsssimPlan(64, 3, 4, 0, 1)
    with pytest.raises(ValueError):
        metrics.MsssimPlan(64, 3, 4, 8, 1, n_files=1)


def test_plan_sizes_hold_nothing_of_p_times_s_squared():
    p = metrics.MsssimPlan(128, 3, 256, 1024, 1)
    assert p.batch_pairs == 128 and p.tiles_per_pair == 64 + 16 + 4 + 1
    assert p.pyramid_bytes == 2 * 128 * (64 * 64 + 32 * 32 + 16 * 16) * 3 * 4
    assert p.score_bytes == 1024 * 8
    assert p.peak_bytes == p.workspace_bytes + p.pyramid_bytes + p.score_bytes
    big = metrics.MsssimPlan(128, 3, 256, 1 << 20, 1)                 # more pairs cost 8 bytes each
    assert big.peak_bytes - p.peak_bytes == ((1 << 20) - 1024) * 8
    assert metrics.MsssimPlan(64, 3, 5, 8, 1).batch_pairs == 3       # an odd batch and the carried image
    assert metrics.MsssimPlan(64, 3, 4, 8, 1, n_files=10).n_real_pairs == 5
    assert metrics.MsssimPlan(64, 3, 4, 8, 1, n_files=100).n_real_pairs == 8


def test_seeds_and_draws():
    np_state = np.random.get_state()[1].copy()
    torch_state = torch.get_rng_state().clone()
    seed = 123456789
    p = metrics.MsssimPlan(64, 3, 4, 8, seed)
    swd = metrics.SwdPlan(64, 3, 4, 8, seed)
    nn = neighbours.NnPlan(64, 3, 4, 64, 0, seed)
    assert len(set(p.seeds.values())) == len(p.seeds) == 4
    assert not set(p.seeds.values()) & (set(swd.seeds.values()) | {nn.seed})

    def draws(s):
        q = metrics.MsssimPlan(64, 3, 4, 8, s, n_files=40)
        return q.draw_latents(32, True).numpy(), q.draw_labels(np.eye(5, dtype=np.float32)), q.draw_real_pairs()
    a, b, c = draws(7), draws(7), draws(8)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and not any(np.array_equal(u, v) for u, v in zip(a, c))
    z, cls, pairs = a
    assert z.shape == (16, 1, 1, 32) and np.abs(z).max() <= 2.0 and not np.array_equal(z[0], z[1])
    assert not np.array_equal(z, swd.draw_latents(32, True).numpy()[:16])
    assert cls.shape == (16, 5) and (cls.sum(axis=1) == 1).all()
    assert np.array_equal(cls[0::2], cls[1::2]) and len({tuple(r) for r in cls}) > 1      # one class per pair
    assert pairs.shape == (8, 2) and sorted(pairs.reshape(-1)) == list(range(16))         # the first 2 P files, each once
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


# ---------------------------------------------------------------- the carry logic on a stand-in for the launches
class _Recorder:
    """Stands in for functional.msssim_*: a pair's "score" is 1000 * id(first image) + id(second image), where an image's
    id is its value at [0, 0, 0]."""

    def __init__(self):
        self.launches = []

    def msssim_workspace(self, P, H, C, device):
        return {"P": P, "rows": None}

    def msssim_level(self, a, b, H, level, ws, pool):
        if level == 0:
            assert b is None and a.shape[0] == 2 * ws["P"]
            ids = a[:, 0, 0, 0].double()
            ws["rows"] = 1000.0 * ids[0::2] + ids[1::2]
            self.launches.append(int(a.shape[0]))
        assert (pool is None) == (level == 2)
        return pool

    def msssim_finish(self, ws, P, H, C, scores, row_offset):
        scores[row_offset:row_offset + P] = ws["rows"]


def _feed(batches, n_pairs=3):
    plan = metrics.MsssimPlan(64, 3, 4, n_pairs, 1)
    rec = _Recorder()
    m = metrics.Msssim(plan, "cpu", ops=rec)
    m.begin()
    for ids in batches:
        m.add(torch.tensor(ids, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 64, 64, 3).contiguous())
    mean = m.finish()
    return m.per_pair.tolist(), mean, rec.launches


def test_a_pair_that_straddles_two_batches_is_carried():
    want = [1002.0, 3004.0, 5006.0]
    one, mean1, launches1 = _feed([[1, 2, 3, 4, 5, 6]])
    two, mean2, launches2 = _feed([[1, 2, 3], [4, 5, 6]])
    assert one == want == two and mean1 == mean2 == sum(want) / 3
    assert launches1 == [6] and launches2 == [2, 2, 2]              # (1,2) | carried (3,4) | (5,6)
    # padding past 2 P is dropped, also when it arrives in a batch of its own; batches of one image work
    assert _feed([[1, 2, 3, 4], [5, 6, 9, 9], [9, 9]])[0] == want
    assert _feed([[1], [2], [3], [4], [5], [6], [9]])[0] == want
    assert _feed([[1, 2, 3, 4, 5], [6, 9, 9, 9, 9]])[0] == want
    with pytest.raises(RuntimeError):
        _feed([[1, 2, 3, 4, 5]])                                     # an image is missing
    with pytest.raises(ValueError):
        m = metrics.Msssim(metrics.MsssimPlan(64, 3, 4, 3, 1), "cpu", ops=_Recorder())
        m.begin()
        m.add(torch.zeros(2, 32, 32, 3))


# ---------------------------------------------------------------- known answers of the reference
def test_identical_images_score_exactly_one_and_the_score_is_symmetric():
    a, b = R.make_pairs(64, 3, 5, seed=3)
    assert (R.pair_scores(a, a)["scores"] == 1.0).all()
    ab, ba = R.pair_scores(a, b), R.pair_scores(b, a)
    assert np.array_equal(ab["scores"], ba["scores"])
    assert ab["scores"][1] == 1.0 and 0.0 < ab["scores"][0] < 0.5      # the identical pair; two independent images
    assert [x[0].shape[1] for x in ab["pyramid"]] == [64, 32, 16] and len(ab["cs"]) == 3


@pytest.mark.parametrize("S", [16, 32, 64, 256])
def test_constant_images_have_the_closed_form(S):
    p, q = 0.25, -0.5
    a, b = np.full((1, S, S, 3), p), np.full((1, S, S, 3), q)
    up, uq = (p + 1) / 2, (q + 1) / 2
    L = len(R.sides(S))
    want = ((2 * up * uq + R.C1) / (up * up + uq * uq + R.C1)) ** R.weights(L)[-1]
    got = R.pair_scores(a, b)
    # float64 rounding of the 121-term sums, at most 121 x 2^-53 x E[u^2], against C2 = 9e-4 in cs: below 1e-11
    assert abs(got["scores"][0] - want) < 1e-11
    assert all(np.abs(cs - 1.0).max() < 1e-11 for cs in got["cs"])    # no variance: cs = C2 / C2


def test_a_negated_image_scores_exactly_zero():
    for S, C in ((16, 1), (64, 3), (128, 4)):
        a, _ = R.make_pairs(S, C, 1, seed=S + C)
        got = R.pair_scores(a, -a)
        # the clamp fires at every level: each level's spatial mean of cs (and of ssim) is negative
        assert all((cs < -0.5).all() for cs in got["cs"]) and all((ss < 0).all() for ss in got["ssim"])
        assert got["scores"][0] == 0.0


def test_the_pooled_pyramid_and_its_bound():
    x = np.arange(2 * 4 * 4 * 1, dtype=np.float64).reshape(2, 4, 4, 1)
    assert np.array_equal(R.pool(x)[0, :, :, 0], [[2.5, 4.5], [10.5, 12.5]])
    rng = np.random.RandomState(5)
    x32 = rng.uniform(-1, 1, size=(1, 32, 32, 3)).astype(np.float32)
    f = np.float32
    got = ((x32[:, 0::2, 0::2] + x32[:, 0::2, 1::2]) + (x32[:, 1::2, 0::2] + x32[:, 1::2, 1::2])) * f(0.25)
    err, bound = np.abs(got.astype(np.float64) - R.pool(x32.astype(np.float64))), R.pool_bound(x32)
    assert (err <= bound).all() and bound.max() < 4 * R.U32
    bad = got.astype(np.float64)
    bad[0, 3, 5, 1] += 10 * bound[0, 3, 5, 1]
    assert not (np.abs(bad - R.pool(x32.astype(np.float64))) <= bound).all()


# ---------------------------------------------------------------- the gates of the GPU tests
def test_the_measured_gap_stays_within_the_recorded_constants():
    """The fp32 emulation against float64 over exactly the inputs of tests/test_gpu_msssim.py."""
    mean_gap, score_gap = R.measure_gaps()
    print("largest gap of a mean: %.4g (recorded %.4g); of a score: %.4g (recorded %.4g)"
          % (mean_gap, R.MEAN_GAP, score_gap, R.SCORE_GAP))
    assert 0 < mean_gap <= R.MEAN_GAP and 0 < score_gap <= R.SCORE_GAP
    assert R.MEAN_GATE == 4 * R.MEAN_GAP and R.SCORE_GATE == 4 * R.SCORE_GAP
    assert R.MEAN_GAP <= 1.25 * mean_gap and R.SCORE_GAP <= 1.25 * score_gap      # recorded, not padded


def test_the_inputs_hold_every_kind_of_pair_and_the_gates_catch_a_wrong_tap():
    kinds = set()
    for S, C, P in R.LEVEL_CASES:
        kinds |= set(R.case(S, C, P)["kinds"])
    assert kinds == set(R.KINDS)
    assert {S for S, _, _ in R.LEVEL_CASES} == {16, 32, 64, 128} and {P for _, _, P in R.LEVEL_CASES} == {1, 3, 5}
    for S in (16, 32, 64, 128):
        assert {P for s, _, P in R.LEVEL_CASES if s == S} == {1, 3, 5}
    k = R.case(64, 3, 5)
    neg, ident = k["kinds"].index("negated"), k["kinds"].index("identical")
    assert k["ref"]["scores"][neg] == 0.0 and k["ref"]["scores"][ident] == 1.0
    assert all((cs[neg] < 0).all() for cs in k["ref"]["cs"])
    # an image shifted by one pixel (a wrong tap or stride) moves the means by far more than the gate
    moved = R.pair_scores(k["a"], np.roll(k["b"], 1, axis=2))
    assert np.abs(moved["cs"][0][0] - k["ref"]["cs"][0][0]).min() > 10 * R.MEAN_GATE
    assert abs(moved["scores"][0] - k["ref"]["scores"][0]) > 10 * R.SCORE_GATE
    assert R.bf16_round(np.array([1.0, 1.00390625, 1.01171875], dtype=np.float32)).tolist() == [1.0, 1.0, 1.015625]
    x = np.random.RandomState(6).uniform(-1, 1, size=4096).astype(np.float32)
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
