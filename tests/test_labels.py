"""Labelled datasets on the host: the --cls_loss_type grammar (reference utils.py:339-375), the float64 restatement
of the sliced label loss in tests/label_ref.py against a NumPy loop, autograd and finite differences, a mutation check of
the kernel gate's bounds, the label-table validation of open_dataset, and the new C entry points.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, main as M, model, scope as S, utils
from tests import label_ref as LR
from tests import launch_replay as R

NEW_SYMBOLS = {
    "bg_label_loss_sums": (ctypes.c_int, [hip._P] * 6 + [ctypes.c_int] * 3 + [hip._P]),
    "bg_label_loss_finish": (ctypes.c_int, [hip._P] * 6 + [ctypes.c_double, ctypes.c_float, hip._P, hip._P]
                             + [ctypes.c_int] * 3 + [hip._P]),
    "bg_gather_rows": (ctypes.c_int, [hip._P] * 3 + [ctypes.c_int] * 3 + [hip._P]),
}


def _model(*extra):
    argv = ["--gan_type", "hinge", "--img_size", "64", "--ch", "8"] + list(extra)
    return model.BigGAN(M.parse_args(argv, make_dirs=False), device="cpu", store=S.VariableStore("cpu"))


# ---------------------------------------------------------------- the grammar
@pytest.mark.parametrize("spec,n,want", [
    ("logistic", 10, [("logistic", 10)]),
    ("euclidean", 7, [("euclidean", 7)]),
    ("6-logistic,4-euclidean", 10, [("logistic", 6), ("euclidean", 4)]),
    ("1-euclidean,997-logistic,2-euclidean", 1000, [("euclidean", 1), ("logistic", 997), ("euclidean", 2)]),
    ("3-logistic,3-logistic", 6, [("logistic", 3), ("logistic", 3)]),
])
def test_accepted_specs_and_their_slice_tables(spec, n, want):
    assert utils.parse_cls_loss_type(spec, n) == want
    assert LR.parse(spec, n) == want
    slices, cols = LR.table(spec, n)
    assert slices.tolist() == [[utils.CLS_LOSS_KINDS[k], s] for k, s in want]
    assert cols.numel() == n and cols.tolist() == sorted(cols.tolist())
    assert [int((cols == i).sum()) for i in range(len(want))] == [s for _, s in want]


@pytest.mark.parametrize("spec,n", [
    ("6-logistic,3-euclidean", 10),          # sizes do not sum to n_labels: the reference's tf.split fails
    ("6-logistic,4-hinge", 10),              # unknown type
    ("10-logistic", 10),                     # size-type without a comma: the reference's "Invalid label loss type"
    ("hinge", 10), ("6-logistic,4", 10), ("x-logistic,4-euclidean", 10), ("0-logistic,10-euclidean", 10),
])
def test_rejected_specs_are_value_errors_naming_the_spec(spec, n):
    for parse in (utils.parse_cls_loss_type, LR.parse):
        with pytest.raises(ValueError, match="Invalid label loss type.*" + spec.split(",")[0]):
            parse(spec, n)
    with pytest.raises(ValueError, match="Invalid label loss type"):
        utils.cls_loss_fn(spec, torch.ones(n))
    with pytest.raises(ValueError, match="Invalid label loss type"):       # at construction, not at first use
        _model("--n_labels", str(n), "--cls_loss_type", spec)


def test_cls_loss_fn_builds_every_type_on_the_host():
    """'euclidean' and the sliced form used to raise NotImplementedError."""
    w = torch.ones(10)
    for spec in ("logistic", "euclidean", "6-logistic,4-euclidean"):
        fn = utils.cls_loss_fn(spec, w)
        assert callable(fn)
    assert utils.cls_loss_fn("6-logistic,4-euclidean", w).slices == [("logistic", 6), ("euclidean", 4)]
    gan = _model("--n_labels", "10", "--cls_loss_type", "6-logistic,4-euclidean")
    assert gan.cls_loss_type == "6-logistic,4-euclidean" and gan.label_table is None


@pytest.mark.parametrize("flag", ["g_final_layer", "multi_head", "z_reconstruct", "d_final_conv"])
def test_neighbouring_flags_stay_rejected(flag):
    with pytest.raises(NotImplementedError):
        _model("--n_labels", "10", "--cls_loss_type", "euclidean", "--" + flag, "true")


# ---------------------------------------------------------------- the restatement
def _numpy_loss(t, x, w, spec):
    t, x, w = (np.asarray(a, np.float64) for a in (t, x, w))
    B, n = x.shape
    total, a = 0.0, 0
    for kind, size in LR.parse(spec, n):
        if kind == "logistic":
            s = 0.0
            for b in range(B):
                for j in range(a, a + size):
                    s += (max(x[b, j], 0.0) - x[b, j] * t[b, j] + math.log1p(math.exp(-abs(x[b, j])))) * w[j]
            total += s / (B * size)
        else:
            s = 0.0
            for b in range(B):
                for j in range(a, a + size):
                    s += ((x[b, j] - t[b, j]) * w[j]) ** 2
            total += math.sqrt(s)
        a += size
    return total


SPECS = [("logistic", 5), ("euclidean", 5), ("2-logistic,3-euclidean", 5), ("6-logistic,4-euclidean", 10)]


@pytest.mark.parametrize("spec,n", SPECS)
def test_restatement_against_numpy_autograd_and_finite_differences(spec, n):
    t, x, w = LR.inputs(3, n, 7, "random")
    t, x, w = t.double(), x.double().requires_grad_(True), w.double()
    loss = LR.label_loss(t, x, w, spec)
    assert abs(loss.item() - _numpy_loss(t, x.detach(), w, spec)) <= 1e-12 * abs(loss.item())
    g, = torch.autograd.grad(loss, x)
    closed = LR.dlogits(t, x.detach(), w, spec)
    assert float((g - closed).abs().max()) <= 1e-13
    xd, h = x.detach(), 1e-6
    for b, j in ((0, 0), (1, n // 2), (2, n - 1)):
        e = torch.zeros_like(xd)
        e[b, j] = h
        fd = (float(LR.label_loss(t, xd + e, w, spec)) - float(LR.label_loss(t, xd - e, w, spec))) / (2 * h)
        assert abs(fd - float(g[b, j])) <= 1e-7 * max(1.0, abs(fd)), (spec, b, j)


def test_logistic_restatement_is_the_oracles():
    from oracle import ref_ops
    t, x, w = LR.inputs(4, 10, 3, "random")
    a = ref_ops.cls_loss_logistic(t.double(), x.double(), w.double())
    assert abs(float(a) - float(LR.label_loss(t, x.double(), w, "logistic"))) <= 1e-14


def test_zero_norm_slice_has_loss_0_and_gradient_0():
    t, x, w = LR.inputs(3, 5, 11, "zero-slice", "2-logistic,3-euclidean")
    assert float(w[2:].abs().max()) == 0.0
    x = x.double().requires_grad_(True)
    loss = LR.label_loss(t, x, w, "2-logistic,3-euclidean")
    g, = torch.autograd.grad(loss, x)
    assert bool(torch.isfinite(g).all()) and float(g[:, 2:].abs().max()) == 0.0 and float(g[:, :2].abs().max()) > 0
    assert abs(loss.item() - float(LR.label_loss(t[:, :2], x[:, :2].detach(), w[:2], "logistic"))) <= 1e-15
    x0 = t.double().clone().requires_grad_(True)              # logits == truth: zero norm with weights of one
    loss = LR.label_loss(t, x0, torch.ones(5), "euclidean")
    g, = torch.autograd.grad(loss, x0)
    assert loss.item() == 0.0 and float(g.abs().max()) == 0.0
    assert float(LR.dlogits(t, t, torch.ones(5), "euclidean").abs().max()) == 0.0
    sim_loss, sim_dx = LR.simulate(t, t, torch.ones(5), "euclidean")
    assert float(sim_loss) == 0.0 and float(sim_dx.abs().max()) == 0.0


# ---------------------------------------------------------------- the gate's bounds: what passes, what must not
def _gate_both(t, x, w, spec, lw, loss, dx):
    ref, E = LR.grad_bound(t, x, w, spec, lw)
    ok_g = R.gate(dx, ref, E)[0]
    lref, lE = LR.loss_bound(t, x, w, spec, lw)
    ok_l = R.gate(loss.reshape(1), lref.reshape(1), lE.reshape(1))[0]
    return ok_l, ok_g


@pytest.mark.parametrize("spec,n,B", [("euclidean", 1, 1), ("2-logistic,3-euclidean", 5, 3),
                                      ("6-logistic,4-euclidean", 10, 4),
                                      ("1-euclidean,997-logistic,2-euclidean", 1000, 32)])
@pytest.mark.parametrize("weights", ["ones", "random", "zero-slice"])
def test_fp32_evaluation_of_the_formula_passes_the_gate(spec, n, B, weights):
    t, x, w = LR.inputs(B, n, 5, weights, spec)
    loss, dx = LR.simulate(t, x, w, spec, 5.0)
    assert _gate_both(t, x, w, spec, 5.0, loss, dx) == (True, True)


def test_mutants_leave_the_gate():
    """Stated input: B = 4, n = 10, '6-logistic,4-euclidean', seed 5, weights U[0, 2], loss weight 5."""
    spec, lw = "6-logistic,4-euclidean", 5.0
    t, x, w = LR.inputs(4, 10, 5, "random", spec)
    td, xd, wd = t.double(), x.double(), w.double()
    B, n = x.shape
    good = LR.dlogits(td, xd, wd, spec, lw)
    good_loss = lw * LR.label_loss(td, xd, wd, spec)
    assert _gate_both(t, x, w, spec, lw, good_loss.float(), good.float()) == (True, True)
    # wrong divisor: B * n instead of B * size on the logistic slice
    m = good.clone()
    m[:, :6] = lw * wd[:6] * (torch.sigmoid(xd[:, :6]) - td[:, :6]) / (B * n)
    m_loss = lw * ((LR._sce(td[:, :6], xd[:, :6]) * wd[:6]).sum() / (B * n)
                   + LR.label_loss(td[:, 6:], xd[:, 6:], wd[6:], "euclidean"))
    assert _gate_both(t, x, w, spec, lw, m_loss.float(), m.float()) == (False, False)
    # w instead of w^2 on the euclidean slice
    m = good.clone()
    nrm = (((xd[:, 6:] - td[:, 6:]) * wd[6:]) ** 2).sum().sqrt()
    m[:, 6:] = lw * wd[6:] * (xd[:, 6:] - td[:, 6:]) / nrm
    assert _gate_both(t, x, w, spec, lw, good_loss.float(), m.float()) == (True, False)
    # the norm taken per rank (2 x 2 rows) instead of over the whole batch
    m = good.clone()
    for rows in (slice(0, 2), slice(2, 4)):
        nr = (((xd[rows, 6:] - td[rows, 6:]) * wd[6:]) ** 2).sum().sqrt()
        m[rows, 6:] = lw * wd[6:] ** 2 * (xd[rows, 6:] - td[rows, 6:]) / nr
    assert _gate_both(t, x, w, spec, lw, good_loss.float(), m.float()) == (True, False)


# ---------------------------------------------------------------- the label table
def _toy_dataset(tmp_path, rows):
    folder = tmp_path / "dataset" / "toy"
    folder.mkdir(parents=True)
    lines = []
    for i, row in enumerate(rows):
        utils.save_images(np.zeros((1, 8, 8, 3), np.float32), [1, 1], str(folder / ("%d.png" % i)))
        lines.append("\t".join(["%d.png" % i] + ["%g" % v for v in row]))
    label_file = tmp_path / "labels.tsv"
    label_file.write_text("\n".join(lines) + "\n")
    return label_file


def test_label_row_of_the_wrong_width_is_a_value_error_naming_the_file(tmp_path):
    label_file = _toy_dataset(tmp_path, [[1, 0, 0], [0, 1, 1], [1, 1], [0, 0, 1, 1]])
    gan = _model("--n_labels", "3", "--dataset", "toy", "--label_file", str(label_file))
    with pytest.raises(ValueError, match=r"2\.png has 2 labels.*3"):
        gan.open_dataset(root=str(tmp_path / "dataset"))
    assert gan.label_table is None


def test_open_dataset_uploads_the_label_table(tmp_path):
    rows = [[1, 0, 0.5], [0, 1, 1], [1, 1, 0]]
    label_file = _toy_dataset(tmp_path, rows)
    gan = _model("--n_labels", "3", "--dataset", "toy", "--label_file", str(label_file), "--batch_size", "2")
    loader = gan.open_dataset(root=str(tmp_path / "dataset"))
    try:
        assert gan.labels == [list(map(float, r)) for r in rows]
        assert gan.label_table.dtype == torch.float32 and gan.label_table.tolist() == gan.labels
    finally:
        loader.close()


# ---------------------------------------------------------------- the C ABI
def test_library_exports_the_new_entry_points():
    L = hip.lib()
    assert L.bg_abi_version() == hip.ABI_VERSION == 10
    for name, (res, args) in NEW_SYMBOLS.items():
        assert hip.SIGNATURES[name] == (res, args), name
        assert getattr(L, name) is not None
    # argument validation happens before any launch: NULL tensors are BG_ERR_ARG (1)
    assert L.bg_label_loss_sums(None, None, None, None, None, None, 4, 10, 2, None) == 1
    assert b"NULL" in L.bg_last_error()
    assert L.bg_label_loss_finish(None, None, None, None, None, None, 4.0, 1.0, None, None, 4, 10, 2, None) == 1
    assert L.bg_gather_rows(None, None, None, 5, 6, 4, None) == 1
    assert b"NULL" in L.bg_last_error()


def test_header_declares_the_new_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "biggan_hip.h")).read()
    assert "#define BG_ABI_VERSION 10" in text
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in text
