"""The singular-value monitor without a GPU: flags, the C ABI and its argument checks, the monitored set and the layout
of the plumbing model, the float64 restatement (tests/sv_ref.py) against LAPACK, the design conditions of the cases, the
convergence of a fresh Gaussian weight, and mutations of the simulated kernel that the gate of tests/test_gpu_sv.py must
catch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, model, scope as S, spectrum
from tests import sv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bg_sv_workspace_bytes", "bg_sv_batch")
NAMES = [c[0] for c in R.CASES]


# ---------------------------------------------------------------- flags and ABI
def test_flags_parse_with_their_defaults():
    args = M.parse_args(["--gan_type", "hinge"], make_dirs=False)
    assert (args.sv_freq, args.sv_k, args.sv_iters, args.sv_tol) == (0, 3, 8, 1e-2)
    args = M.parse_args(["--sv_freq", "500", "--sv_k", "4", "--sv_iters", "3", "--sv_tol", "1e-3"], make_dirs=False)
    assert (args.sv_freq, args.sv_k, args.sv_iters, args.sv_tol) == (500, 4, 3, 1e-3)
    for flag in (("sv_freq", int, 0), ("sv_k", int, 3), ("sv_iters", int, 8), ("sv_tol", float, 1e-2)):
        assert flag in M.EXTRA_FLAGS
    assert len(M.FLAGS) == 119 and not any(n.startswith("sv_") for n, _, _ in M.FLAGS)


def _cpu_model(*extra):
    argv = ["--gan_type", "hinge", "--img_size", "64", "--ch", "8"] + list(extra)
    return model.BigGAN(M.parse_args(argv, make_dirs=False), device="cpu", store=S.VariableStore("cpu"))


@pytest.mark.parametrize("flag,value", [("--sv_k", "0"), ("--sv_k", "5"), ("--sv_iters", "0"), ("--sv_iters", "257"),
                                        ("--sv_tol", "0")])
def test_values_out_of_range_are_value_errors(flag, value):
    with pytest.raises(ValueError, match=flag):
        _cpu_model(flag, value)


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "biggan_hip.h")).read()
    assert re.search(r"#define BG_ABI_VERSION 10\b", header) and hip.ABI_VERSION == 10
    assert re.search(r"#define BG_SV_BLOCK 8\b", header) and hip.SV_BLOCK == 8 == R.BLOCK
    for name in NEW_SYMBOLS:
        res, args = hip.SIGNATURES[name]
        decl = re.search(r"\b(int|size_t)\s+%s\(([^)]*)\)" % name, header)
        assert decl, name
        assert res is (ctypes.c_int if decl.group(1) == "int" else ctypes.c_size_t), name
        params = decl.group(2).split(",")
        assert len(params) == len(args), name
        for text, ctype in zip(params, args):
            want = ctypes.c_void_p if "*" in text else ctypes.c_size_t if "size_t" in text else ctypes.c_int
            assert ctype is want, (name, text)
    # the struct: the same fields in the same order, pointers first, 48 bytes
    body = re.search(r"typedef struct BgSvItem \{(.*?)\} BgSvItem;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if "int64_t" in decl else ctypes.c_int32
        for name in decl.split("*")[-1].replace("int64_t", "").replace("int32_t", "").split(","):
            fields.append((name.strip(), ctype))
    assert fields == list(hip.BgSvItem._fields_)
    assert ctypes.sizeof(hip.BgSvItem) == 48 and hip.BgSvItem.ws_offset.offset == 32 and hip.BgSvItem.cols.offset == 44
    assert "spectrum.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    L = hip.lib()
    assert L.bg_abi_version() == 10
    # per item: a header of 80 doubles, Z [cols][8] and Y [rows][8] in fp64
    for rows, cols in ((1, 1), (3, 1), (2, 7), (1030, 24), (184, 24576), (24576, 1536)):
        assert L.bg_sv_workspace_bytes(rows, cols) == 8 * (80 + 8 * cols + 8 * rows)
    assert L.bg_sv_workspace_bytes(0, 4) == 0 and L.bg_sv_workspace_bytes(4, 0) == 0 and L.bg_sv_workspace_bytes(-1, 4) == 0


def rejections(L, table, ws, big):
    """(return code, message) of every bad-argument case of bg_sv_batch; ``table`` and ``ws`` are good pointers."""
    small = L.bg_sv_workspace_bytes(1, 1)
    calls = {
        "NULL item table": (None, 2, 3, ws, big),
        "NULL workspace": (table, 2, 3, None, big),
        "n_items=0": (table, 0, 3, ws, big),
        "n_items=257": (table, 257, 3, ws, big),
        "n_items=-1": (table, -1, 3, ws, big),
        "iters=-1": (table, 2, -1, ws, big),
        "iters=257": (table, 2, 257, ws, big),
        "too small": (table, 2, 3, ws, 2 * small - 8),
        "aligned": (table, 2, 3, ctypes.c_void_p(ws.value + 4), big),
    }
    return {word: (L.bg_sv_batch(a[0], a[1], a[2], a[3], a[4], None), L.bg_last_error().decode()) for word, a in calls.items()}


def test_bad_arguments_are_rejected_before_any_launch():
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call fails validation
    for word, (rc, msg) in rejections(L, fake, fake, 1 << 24).items():
        assert rc == 1 and word in msg and "bg_sv_batch" in msg, (word, rc, msg)


# ---------------------------------------------------------------- the plan of the plumbing model
def test_monitored_set_and_layout_of_the_plumbing_model():
    gan = _cpu_model().build_model()
    store = gan.store
    plan = spectrum.SvPlan(store)
    want = [n for n in store.vars if n.endswith("/kernel") and store.trainable[n]]
    assert plan.names == want and plan.n == len(want) > 20
    assert all(n.startswith(("generator/", "discriminator/")) for n in plan.names)
    assert not any("ExponentialMovingAverage" in n or n.endswith("/u") for n in plan.names)
    assert {n.split("/")[0] for n in plan.names} == {"generator", "discriminator"}
    for n, rows, cols, b in zip(plan.names, plan.rows, plan.cols, plan.beff):
        v = store.vars[n]
        assert cols == v.shape[-1] and rows * cols == v.numel() and b == min(8, rows, cols)
        if n in store.sn_pairs:                                     # the reshape of spectral norm: u is [1, cols]
            assert store.vars[store.sn_pairs[n]].numel() == cols
    assert len(store.sn_pairs) > 10 and set(store.sn_pairs) <= set(plan.names)
    # scratch: 16-byte aligned, disjoint, in order; the basis: one [cols, 8] block per weight
    L = hip.lib()
    end = 0
    for off, rows, cols in zip(plan.ws_offsets, plan.rows, plan.cols):
        assert off % 16 == 0 and off >= end
        end = off + L.bg_sv_workspace_bytes(rows, cols)
    assert plan.ws_bytes >= end
    assert plan.q_offsets == list(np.cumsum([0] + [8 * c for c in plan.cols[:-1]])) and plan.q_floats == 8 * sum(plan.cols)
    assert plan.weight_bytes == 4 * sum(store.vars[n].numel() for n in want)
    for bad in (dict(k=0), dict(k=5), dict(iters=0), dict(tol=0.0)):
        with pytest.raises(ValueError):
            spectrum.SvPlan(store, **bad)


def test_the_basis_draws_are_the_monitors_own():
    np_state, torch_state = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
    gen = torch.Generator().manual_seed(spectrum.SEED)
    q = spectrum.draw_basis(37, 5, gen)
    assert q.shape == (37, 8) and q.dtype == torch.float32 and not q[:, 5:].any()
    assert R.defect_of(q.numpy())[0] <= 2 * R.U32 + R.U32 ** 2 + R.EPS64
    assert torch.equal(q, spectrum.draw_basis(37, 5, torch.Generator().manual_seed(spectrum.SEED)))
    assert spectrum.refill_basis(q, 5, gen) is None
    holed = q.clone()
    holed[:, 1] = 0
    holed[:, 4] = 0
    new = spectrum.refill_basis(holed, 5, gen)
    assert torch.equal(new[:, [0, 2, 3]], q[:, [0, 2, 3]]) and not new[:, 5:].any()
    assert new[:, 1].any() and new[:, 4].any() and R.defect_of(new.numpy())[0] <= 2 * R.U32 + R.U32 ** 2 + R.EPS64
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


def test_scalars_and_the_printed_line():
    result = dict(weights=[dict(name="generator/a/kernel", rows=4, cols=3, sv=np.array([2.0, 1.0]), resid=np.zeros(2)),
                           dict(name="generator/b/kernel", rows=4, cols=3, sv=np.array([3.0, 0.5]), resid=np.zeros(2)),
                           dict(name="discriminator/c/kernel", rows=4, cols=3, sv=np.array([0.25, 0.125]),
                                resid=np.array([4e-3, 1e-3]))], rounds=2, resid_max=4e-3)
    sigma = {"generator/a/kernel": 1.0, "discriminator/c/kernel": 0.5, "generator/b/kernel": 0.0}
    vals, top = spectrum.scalars(result, 2, sigma.get)
    assert list(vals) == ["sv/generator/a/kernel/s0", "sv/generator/a/kernel/s1", "sv/generator/b/kernel/s0",
                          "sv/generator/b/kernel/s1", "sv/discriminator/c/kernel/s0", "sv/discriminator/c/kernel/s1",
                          "sv_g_max", "sv_d_max", "sv_resid_max", "sv_sn_ratio_min", "sv_sn_ratio_max"]
    assert (vals["sv_g_max"], vals["sv_d_max"], vals["sv_resid_max"]) == (3.0, 0.25, 4e-3)
    assert (vals["sv_sn_ratio_min"], vals["sv_sn_ratio_max"]) == (0.5, 2.0)          # a zero sigma slot is left out
    assert "sv_sn_ratio_min" not in spectrum.scalars(result, 2)[0]
    assert spectrum.format_line(result, top) == \
        "SV: G max s0 3 (generator/b/kernel), D max s0 0.25 (discriminator/c/kernel), resid 0.004, rounds 2"


# ---------------------------------------------------------------- the float64 run, the cases, the stand-in
@pytest.mark.parametrize("name", NAMES)
def test_float64_run_meets_lapack_within_the_theorem(name):
    k = R.case(name)
    b = min(8, k["rows"], k["cols"])
    ref = k["ref"]
    miss = R.theorem_miss(ref["sv"], ref["resid"], k["truth"], R.EPS64)
    print(name, "sv", ref["sv"][:b], "resid", ref["resid"][:b])
    assert (miss[:b] <= 0).all(), miss
    assert (ref["sv"][b:] == 0).all() and (ref["resid"][b:] == 0).all() and not ref["q"][:, b:].any()
    assert np.abs(ref["resid"] - R.pair_resid(R.apply_gram(k["w"]), ref["q"], ref["sv"]))[:b].max() <= R.EPS64
    assert R.defect_of(ref["q"])[0] <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_every_case_keeps_the_check_from_being_vacuous(name):
    """The float64 residual of the first K values is at least 100 times below the fp32 floor, the caps of the first K
    values stay below the gaps of the spectrum, and the caps are not the trivial 2.01 where the value is not at the
    rounding level."""
    k = R.case(name)
    bd, kk = k["bounds"], min(R.K, 8, k["rows"], k["cols"])
    assert (k["ref"]["resid"][:kk] <= bd["floor"] / 100).all(), (k["ref"]["resid"][:kk], bd["floor"])
    lam = np.concatenate([k["truth"] ** 2, [0.0]]) / bd["s0"] ** 2
    for i in range(kk):
        if lam[i] < 1e-6:                                       # (rank 1: sv[1..] sit at the rounding level of sigma_0)
            assert name == "rank1_8x8" and i >= 1
            continue
        others = np.abs(lam - lam[i])
        others = others[others > 1e-6]                          # (sigma_0 = sigma_1 up to the fp32 rounding: one value)
        assert bd["cap"][i] < 2.0 and bd["gap"][i] < 0.25 * others.min(), (i, bd["gap"][i], others.min())
    assert bd["floor"] < 1e-4 and bd["defect"] < 1.1e-6


@pytest.mark.parametrize("name", NAMES)
def test_fp32_stand_in_passes_the_gate(name):
    k = R.case(name)
    kk = min(R.K, 8, k["rows"], k["cols"])
    print(name, "resid fp32", k["sim"]["resid"][:kk], "float64", k["ref"]["resid"][:kk], "cap", k["bounds"]["cap"][:kk])
    assert R.gate(k, k["sim"]) == []


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_of_the_stand_in_are_caught(mutation):
    caught = [n for n in NAMES if R.gate(R.case(n), R.run(R.case(n)["w"], R.case(n)["q0"], R.case(n)["iters"], np.float32,
                                                          mutate=mutation))]
    print(mutation, "caught on", caught)
    assert len(caught) >= 4
    assert "1030x24" in caught                   # rows % 256 != 0, 24 values, more than one row unit


def test_a_fresh_gaussian_weight_converges_within_eight_rounds():
    """1152 x 128, std 0.02: a flat spectrum, the slowest kind.  Recorded: the iterations that the float64 run needs for
    resid <= 1e-2 on the first three values; asserted: 8 rounds of 8 iterations reach it."""
    rng = np.random.RandomState(7)
    w = (rng.standard_normal((1152, 128)) * 0.02).astype(np.float32)
    q = R.make_basis(128, 8)
    needed, rounds = None, None
    for t in range(1, 65):
        out = R.run(w, q, 1, np.float64)
        q = out["q"]
        if needed is None and out["resid"][:3].max() <= 1e-2:
            needed = t
        if rounds is None and t % 8 == 0 and out["resid"][:3].max() <= 1e-2:
            rounds = t // 8
    print("iterations needed: %s, rounds of 8: %s, resid after 64: %s" % (needed, rounds, out["resid"][:3]))
    assert needed is not None and rounds is not None and rounds <= 8
    assert (R.theorem_miss(out["sv"], out["resid"], R.truth(w), R.EPS64) <= 0).all()
