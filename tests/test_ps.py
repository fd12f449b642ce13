"""The radial power spectrum without a GPU: the float64 restatement (tests/ps_ref.py) on known answers, the gates of
tests/test_gpu_ps.py and the mutations they must catch, the host plan (metrics.PowerSpectrumPlan), the batch logic and the
host tail of metrics.PowerSpectrum on a stand-in for the launch wrappers, the flags and the C ABI."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, metrics, neighbours
from tests import ps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bg_ps_workspace_bytes", "bg_ps_power", "bg_ps_profile")


# ---------------------------------------------------------------- flags and ABI
def test_flags_parse_with_their_defaults():
    args = M.parse_args(["--gan_type", "hinge"], make_dirs=False)
    assert args.ps_freq == 0 and args.ps_images == 1024
    args = M.parse_args(["--ps_freq", "500", "--ps_images", "64"], make_dirs=False)
    assert args.ps_freq == 500 and args.ps_images == 64
    assert ("ps_freq", int, 0) in M.EXTRA_FLAGS and ("ps_images", int, 1024) in M.EXTRA_FLAGS
    assert len(M.FLAGS) == 119 and not any(n.startswith("ps_") for n, _, _ in M.FLAGS)


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
    assert "powerspec.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    L = hip.lib()
    assert L.bg_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    # the twiddle table and fp32 complex [n, S, S/2 + 1]
    for S in R.SIDES:
        assert L.bg_ps_workspace_bytes(3, S) == 4096 + 3 * S * (S // 2 + 1) * 8, S
        assert metrics.PowerSpectrumPlan(S, 3, 3, 8, 1).workspace_bytes == L.bg_ps_workspace_bytes(3, S)
    for n, S in ((0, 64), (-1, 64), (1, 8), (1, 48), (1, 1024), (1, 0), (1, -64)):
        assert L.bg_ps_workspace_bytes(n, S) == 0, (n, S)


def test_the_entry_points_check_their_arguments_before_any_launch():
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails validation
    big = 1 << 24

    def power(x=fake, dtype=0, n=2, S=64, C=3, out=fake, ws=fake, nb=big):
        return L.bg_ps_power(x, dtype, n, S, C, out, ws, nb, None)

    def profile(p=fake, n=2, S=64, prof=fake, sum2d=fake):
        return L.bg_ps_profile(p, n, S, prof, sum2d, None)

    def rejected(rc, word):
        return rc == 1 and word in L.bg_last_error()

    assert rejected(power(x=None), b"NULL") and rejected(power(out=None), b"NULL") and rejected(power(ws=None), b"NULL")
    assert rejected(profile(p=None), b"NULL") and rejected(profile(prof=None), b"NULL")
    for S in (8, 48, 96, 1024, 0, -64):
        assert rejected(power(S=S), b"S="), S
        assert rejected(profile(S=S), b"S="), S
    for C in (0, 2, 5):
        assert rejected(power(C=C), b"C="), C
    assert rejected(power(dtype=2), b"dtype") and rejected(power(dtype=-1), b"dtype")
    assert rejected(power(n=0), b"n=") and rejected(power(n=-3), b"n=") and rejected(profile(n=0), b"n=")
    need = L.bg_ps_workspace_bytes(2, 64)
    assert rejected(power(nb=need - 8), b"workspace")
    assert rejected(power(ws=ctypes.c_void_p(4100)), b"aligned")
    assert rejected(power(out=ctypes.c_void_p(4098)), b"aligned")
    assert rejected(power(x=ctypes.c_void_p(4098)), b"aligned")
    assert rejected(power(x=ctypes.c_void_p(4097), dtype=1), b"aligned")
    assert rejected(profile(p=ctypes.c_void_p(4098)), b"aligned")
    assert rejected(profile(prof=ctypes.c_void_p(4100)), b"aligned")
    assert rejected(profile(sum2d=ctypes.c_void_p(4100)), b"aligned")


# ---------------------------------------------------------------- the plan
def test_bins_and_counts_for_every_allowed_side():
    for S in R.SIDES:
        p = metrics.PowerSpectrumPlan(S, 3, 4, 8, 1)
        assert p.n_bins == metrics.ps_bins(S) == R.n_bins(S) == R.NB_TABLE[S]
        assert np.array_equal(p.counts, R.counts(S)) and p.counts.sum() == S * S and p.counts[0] == 1
        table = metrics.ps_bin_table(S)
        assert np.array_equal(table, R.full_bins(S)[:, :S // 2 + 1])
        assert table[S // 2, S // 2] == p.n_bins - 1 and table.max() == p.n_bins - 1       # the corner is the last bin
        assert p.first_hf == S // 4
        # round(sqrt) in integers equals floor(sqrt + 0.5) for every coefficient
        f = np.arange(S)
        f = np.where(f < S // 2, f, f - S)
        m = (f[:, None] ** 2 + f[None, :S // 2 + 1] ** 2).astype(np.float64)
        assert np.array_equal(table, np.floor(np.sqrt(m) + 0.5).astype(np.int64))
    assert R.full_bins(32)[16, 16] == 23 == R.n_bins(32) - 1                                # where a checkerboard lands
    for bad in (8, 48, 1024, 0):
        with pytest.raises(ValueError):
            metrics.PowerSpectrumPlan(bad, 3, 4, 8, 1)
    with pytest.raises(ValueError):
        metrics.PowerSpectrumPlan(64, 2, 4, 8, 1)
    with pytest.raises(ValueError):
        metrics.PowerSpectrumPlan(64, 3, 4, 0, 1)
    with pytest.raises(ValueError):
        metrics.PowerSpectrumPlan(64, 3, 4, 8, 1, n_files=0)
    assert metrics.PowerSpectrumPlan(64, 3, 4, 8, 1, n_files=5).n_real == 5
    assert metrics.PowerSpectrumPlan(64, 3, 4, 8, 1, n_files=50).n_real == 8
    p = metrics.PowerSpectrumPlan(128, 3, 256, 1024, 1)
    assert p.power_bytes == 256 * 128 * 65 * 4 and p.kept_bytes == 1024 * 92 * 8 + 128 * 65 * 8
    assert p.peak_bytes == p.workspace_bytes + p.power_bytes + p.kept_bytes


def test_seeds_and_draws():
    np_state = np.random.get_state()[1].copy()
    torch_state = torch.get_rng_state().clone()
    seed = 123456789
    p = metrics.PowerSpectrumPlan(64, 3, 4, 8, seed)
    others = set(metrics.SwdPlan(64, 3, 4, 8, seed).seeds.values()) | set(metrics.MsssimPlan(64, 3, 4, 8, seed).seeds.values())
    others |= {neighbours.NnPlan(64, 3, 4, 64, 0, seed).seed}
    assert len(set(p.seeds.values())) == len(p.seeds) == 3 and not set(p.seeds.values()) & others

    def draws(s):
        q = metrics.PowerSpectrumPlan(64, 3, 4, 8, s)
        return q.draw_latents(32, True).numpy(), q.draw_labels(np.eye(5, dtype=np.float32))
    a, b, c = draws(7), draws(7), draws(8)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and not any(np.array_equal(u, v) for u, v in zip(a, c))
    assert a[0].shape == (8, 1, 1, 32) and np.abs(a[0]).max() <= 2.0
    assert a[1].shape == (8, 5) and (a[1].sum(axis=1) == 1).all()
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


# ---------------------------------------------------------------- known answers
def test_a_plane_wave_puts_a_quarter_at_its_frequency_and_at_the_mirror():
    S = 32
    x = R.cosine_images(S, [(3, 4)], np.float64)
    P = R.power_full(x)[0]
    assert abs(P[3, 4] - 0.25) < 1e-14 and abs(P[S - 3, S - 4] - 0.25) < 1e-14
    rest = P.copy()
    rest[3, 4] = rest[S - 3, S - 4] = 0.0
    assert rest.max() < 1e-28
    ref = R.reference(x)
    assert abs(ref["power"][0, 3, 4] - 0.25) < 1e-14 and ref["power"][0, S - 3, 4] < 1e-28      # the half plane holds one
    prof = ref["profiles"][0]
    assert abs(prof[5] * R.counts(S)[5] - 0.5) < 1e-14 and np.delete(prof, 5).max() < 1e-28      # sqrt(9 + 16) = 5
    # the restatement of the kernel finds the same through the half plane and the doubled columns
    x = x.astype(np.float32)
    power, eprof = R.emulate(x)
    ref = R.reference(x)
    assert abs(power[0, 3, 4] - 0.25) < 1e-6 and abs(eprof[0, 5] * R.counts(S)[5] - 0.5) < 1e-6
    assert R.passes(power, eprof, ref)


def test_a_checkerboard_lands_in_the_last_bin_and_a_constant_in_bin_zero():
    S = 32
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    board = np.where((x + y) % 2 == 0, 1.0, -1.0)[None, :, :, None].astype(np.float32)
    ref = R.reference(board)
    nb = R.n_bins(S)
    assert R.counts(S)[nb - 1] == 1 and nb - 1 == 23
    assert abs(ref["profiles"][0, nb - 1] - 1.0) < 1e-14 and ref["profiles"][0, :nb - 1].max() < 1e-28
    power, prof = R.emulate(np.repeat(board, 3, axis=3))
    assert abs(prof[0, nb - 1] - 1.0) < 1e-6 and prof[0, :nb - 1].max() < 1e-12
    const = np.full((1, S, S, 3), 0.5, dtype=np.float32)
    ref = R.reference(const)
    assert abs(ref["profiles"][0, 0] - 0.25) < 1e-15 and ref["profiles"][0, 1:].max() < 1e-28
    assert abs(ref["profiles"].sum() - 0.25) < 1e-15                                    # sum P = mean(Y^2)
    # Parseval on noise: the full-plane sum, and the half plane with its doubled columns
    k = R.case(64, 3, 3)
    total = (k["ref"]["profiles"] * R.counts(64)).sum(axis=1)
    assert np.allclose(total, (k["ref"]["Y"] ** 2).mean(axis=(1, 2)), rtol=1e-12)
    half = (k["ref"]["power"] * R.half_weights(64)).sum(axis=(1, 2))
    assert np.allclose(half, total, rtol=1e-12)


def test_alpha_is_ignored_and_one_channel_is_used_as_it_is():
    x = R.make_images(16, 2, 4, "white")
    y = x.copy()
    y[..., 3] = 0.25
    assert np.array_equal(R.reference(x)["power"], R.reference(y)["power"])
    assert np.array_equal(R.emulate(x)[0], R.emulate(y)[0])
    g = R.make_images(16, 2, 1, "white")
    assert np.array_equal(R.luminance(g), g[..., 0].astype(np.float64))
    assert abs(sum(R.LUMA) - 1.0) < 1e-15


# ---------------------------------------------------------------- scores
def _blur(x):
    """A tenth of the image plus nine tenths of its 2 x 2 box mean: no frequency is removed entirely."""
    box = 0.25 * (x + np.roll(x, 1, axis=1) + np.roll(x, 1, axis=2) + np.roll(np.roll(x, 1, axis=1), 1, axis=2))
    return 0.1 * x + 0.9 * box


def _checker(x, amp=0.05):
    S = x.shape[1]
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    return x + amp * np.where((xx + yy) % 2 == 0, 1.0, -1.0)[None, :, :, None]


def test_scores_are_zero_for_equal_sets_and_signed_for_blur_and_checkerboard():
    S = 64
    real = R.make_images(S, 5, 3, "pink").astype(np.float64)
    plan = metrics.PowerSpectrumPlan(S, 3, 4, 5, 1)
    runner = metrics.PowerSpectrum(plan, "cpu", ops=object())

    def as_set(x):
        ref = R.reference(x)
        return {"profile": R.set_profile(ref["profiles"]), "sum2d": ref["power"].sum(axis=0), "n": x.shape[0]}
    same = runner.scores(as_set(real), as_set(real))
    assert same == {"ps_dist": 0.0, "ps_hf": 0.0, "ps_peak": 0.0, "ps_peak_at": 0.25}
    blurred = runner.scores(as_set(real), as_set(_blur(real)))
    assert blurred["ps_hf"] < -0.3 and blurred["ps_dist"] > 0.1 and blurred["ps_peak"] <= 0.0
    board = runner.scores(as_set(real), as_set(_checker(real)))
    assert board["ps_peak"] > 1.0 and board["ps_peak_at"] == (R.n_bins(S) - 1) / float(S) and board["ps_hf"] > 0.0
    assert board["ps_dist"] > 0.0
    for got, fake in ((blurred, _blur(real)), (board, _checker(real))):
        want = R.image_scores(real, fake)
        assert got.keys() == want.keys() and all(abs(got[k] - want[k]) < 1e-12 for k in got)
    assert runner.scores(as_set(real), as_set(real), prefix="x").keys() == {"x_dist", "x_hf", "x_peak", "x_peak_at"}


# ---------------------------------------------------------------- batches on a stand-in for the launches
class _HostOps:
    """Stands in for functional.ps_power / ps_profile with the float64 reference on host tensors."""

    def __init__(self):
        self.batches = []

    def ps_power(self, x):
        self.batches.append(int(x.shape[0]))
        return torch.from_numpy(R.reference(x.numpy())["power"].copy())

    def ps_profile(self, power, profiles, sum2d):
        P = power.numpy()
        n, S, W = P.shape
        b, w = R.full_bins(S)[:, :W].reshape(-1), np.tile(R.half_weights(S), S)
        for i in range(n):
            profiles[i] = torch.from_numpy(np.bincount(b, weights=w * P[i].reshape(-1), minlength=R.n_bins(S)) / R.counts(S))
            sum2d += torch.from_numpy(P[i])
        return profiles


def _feed(x, sizes, n_images, extra=0):
    plan = metrics.PowerSpectrumPlan(x.shape[1], x.shape[3], 4, n_images, 1)
    ops = _HostOps()
    m = metrics.PowerSpectrum(plan, "cpu", ops=ops)
    m.begin()
    lo = 0
    for size in sizes:
        m.add(torch.from_numpy(x[lo:lo + size]))
        lo += size
    for _ in range(extra):
        m.add(torch.from_numpy(x[:2]))
    return m, m.finish(), ops.batches


def test_ragged_batches_give_the_same_set_and_padding_is_dropped():
    x = R.make_images(16, 7, 3, "pink")
    ref = R.reference(x[:5])
    _, one, b1 = _feed(x, [5], 5)
    _, two, b2 = _feed(x, [3, 4], 5, extra=1)                  # the second batch holds two images of padding
    _, three, b3 = _feed(x, [1, 1, 1, 1, 1], 5)
    assert b1 == [5] and b2 == [3, 2] and b3 == [1] * 5
    for got in (one, two, three):
        assert got["n"] == 5 and got["profile"].tobytes() == one["profile"].tobytes()
        assert got["sum2d"].tobytes() == one["sum2d"].tobytes()
    assert np.allclose(one["profile"], R.set_profile(ref["profiles"]), rtol=1e-12)
    assert np.allclose(one["sum2d"], ref["power"].sum(axis=0), rtol=1e-12)
    with pytest.raises(RuntimeError):
        _feed(x, [4], 5)                                       # an image is missing
    with pytest.raises(ValueError):
        m = metrics.PowerSpectrum(metrics.PowerSpectrumPlan(16, 3, 4, 5, 1), "cpu", ops=_HostOps())
        m.begin()
        m.add(torch.zeros(2, 32, 32, 3))
    m, real, _ = _feed(x, [2], 2)                              # begin(n) for a set of another size
    m.begin(3)
    m.add(torch.from_numpy(x[:3]))
    assert m.finish()["n"] == 3


def _read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, depth, ctype = struct.unpack(">IIBB", data[16:26])
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT" and (depth, ctype) == (8, 0)
    return np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(h, 1 + w)[:, 1:]


def test_ps_txt_and_ps_png_are_written(tmp_path):
    S = 32
    real = R.make_images(S, 4, 1, "pink")
    wave = R.cosine_images(S, [(3, 4)] * 4, np.float64)
    m, real_set, _ = _feed(real, [4], 4)
    _, fake_set, _ = _feed(wave, [4], 4)
    _, live_set, _ = _feed(real, [4], 4)
    txt, png = m.save(str(tmp_path), real_set, {"ps": fake_set, "ps_noema": live_set})
    assert os.path.basename(txt) == "ps.txt" and os.path.basename(png) == "ps.png"
    lines = open(txt).read().splitlines()
    assert lines[0] == "# r\tr/S\tn_r\tL_real\tL_fake\tL_fake_noema\tD_fake\tD_fake_noema"
    rows = [l.split("\t") for l in lines[1:]]
    assert len(rows) == R.n_bins(S) and [int(r[0]) for r in rows] == list(range(R.n_bins(S)))
    assert [int(r[2]) for r in rows] == R.counts(S).tolist() and all(len(r) == 8 for r in rows)
    assert float(rows[8][1]) == 0.25 and all(abs(float(r[7])) == 0.0 for r in rows)          # the live set is the real set
    Lr = R.log_profile(real_set["profile"])
    assert all(abs(float(r[3]) - Lr[i]) < 1e-6 for i, r in enumerate(rows))
    assert float(rows[5][4]) == pytest.approx(np.log10(0.5 / R.counts(S)[5]), abs=1e-6)      # the wave's bin
    assert float(rows[6][4]) == -30.0                                                        # an empty bin: the floor
    # the image: real beside fake, DC at (S/2, S/2); the wave is two mirrored bright pixels
    img = _read_png(png)
    assert img.shape == (S, 2 * S)
    fake = img[:, S:]
    bright = sorted(zip(*np.nonzero(fake == 255)))
    assert bright == [(S // 2 - 3, S // 2 - 4), (S // 2 + 3, S // 2 + 4)] and np.count_nonzero(fake) == 2
    left = img[:, :S]
    assert left.max() == 255 and left.min() > 0 and len(np.unique(left)) > 16      # the largest non-DC value is white
    assert np.array_equal(left[1:, 1:], left[1:, 1:][::-1, ::-1])                            # a real image: Hermitian
    # only the live weights: their set is shown
    m.save(str(tmp_path), real_set, {"ps_noema": fake_set})
    assert np.array_equal(_read_png(png)[:, S:], fake)
    assert open(txt).read().splitlines()[0] == "# r\tr/S\tn_r\tL_real\tL_fake_noema\tD_fake_noema"


# ---------------------------------------------------------------- the gates of the GPU tests
def test_the_measured_gap_stays_within_the_recorded_constant():
    """The fp32 restatement against float64 over exactly the inputs of tests/test_gpu_ps.py."""
    gap, where, power_frac, profile_frac = R.measure_profile_gap()
    print("largest relative gap of a profile bin: %.4g at %s (recorded %.4g); worst |P^ - P| / bound %.4g; worst profile "
          "gap / bound %.4g" % (gap, where, R.PROFILE_GAP, power_frac, profile_frac))
    assert 0 < gap <= R.PROFILE_GAP and R.PROFILE_GAP <= 1.25 * gap            # recorded, not padded
    assert R.PROFILE_GATE == 16 * R.PROFILE_GAP
    assert power_frac <= 0.05 and profile_frac <= 0.05                          # the derived bound is rigorous, not tight
    for S, n, C in R.STRUCTURE_CASES:                                           # white noise uses at most 0.004 of it
        k = R.case(S, n, C)
        assert R.check_power(R.emulate(k["x"])[0], k["ref"]) <= 0.004


def test_the_case_table_covers_what_it_should():
    assert [S for S, _, _ in R.STRUCTURE_CASES] == list(R.SIDES)
    assert {(S, n, C) for S, n, C in R.CONTENT_CASES} == {(S, n, C) for S in (16, 64) for n in (1, 3, 5) for C in (1, 3, 4)}
    k = R.case(64, 3, 3, "dc", "bf16")
    assert np.array_equal(R.bf16_round(k["x"]), k["x"]) and k["x"].mean() > 0.85
    x = np.random.RandomState(6).uniform(-1, 1, size=4096).astype(np.float32)
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    # white noise gives the coefficient bound teeth: every |F_k| is far above the bound on its error
    for S in (16, 64, 128):
        ref = R.case(S, 2, 3)["ref"]
        assert (np.sqrt(ref["power"]) * S * S > 10 * np.sqrt(R.power_bound(ref) * float(S) ** 4)).mean() > 0.9
    # the boundary frequencies: four round down, four up, all within 0.02 of a half-integer
    freqs = R.boundary_frequencies()
    assert len(freqs) == 8 and len(set(freqs)) == 8
    rho = np.array([np.sqrt(ky * ky + kx * kx) for ky, kx in freqs])
    frac = rho - np.floor(rho)
    assert (frac[:4] < 0.5).all() and (frac[4:] > 0.5).all() and np.abs(frac - 0.5).max() < 0.02
    b = R.boundary_case()
    for i, (ky, kx) in enumerate(freqs):
        r = R.bin_of(ky, kx)
        assert r == int(np.floor(rho[i] + 0.5))
        assert abs(b["ref"]["profiles"][i, r] * R.counts(64)[r] - 0.5) < 1e-7          # (the cosines are stored in fp32)
        assert R.significant(b["ref"])[i].sum() == 1


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_restatement_fails_a_gate(mutation):
    caught = 0
    for label, k in R.all_cases():
        power, prof = R.emulate(k["x"], mutation)
        caught += not R.passes(power, prof, k["ref"])
    clean = all(R.passes(*R.emulate(k["x"]), k["ref"]) for _, k in R.all_cases()) if mutation == R.MUTATIONS[0] else True
    print("%s: caught on %d cases" % (mutation, caught))
    assert clean and caught >= 60          # R and B swapped cannot show on one channel; everything else shows everywhere
