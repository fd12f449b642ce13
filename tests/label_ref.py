"""float64 restatement of the label loss of --cls_loss_type (reference utils.py:339-375) and the error bounds of the
gate on csrc/labels.hip.

Test helper, not product code.  Four parts:

* ``parse`` - the grammar, restated: 'logistic' / 'euclidean' are one slice of every column, a spec containing ',' is a
  list of ``size-type`` parts whose sizes sum to the number of labels; anything else is a ValueError.
* ``label_loss(truth, logits, weights, spec)`` - the loss in the dtype of ``logits`` (float64 for the reference),
  differentiable: the sum over the slices of mean(sigmoid_ce * w) over the slice's own B * size elements (logistic) or
  of ||(logits - truth) * w||_2 over the slice (euclidean: one norm, not a mean).  Where a slice's sum of squares is
  exactly 0 its loss is 0 and its gradient is 0 (the product's stated deviation; TensorFlow's sqrt gradient gives NaN).
  ``dlogits`` is the same gradient in closed form.
* bounds - ``grad_bound`` / ``loss_bound`` return (ref, E) for ``launch_replay.gate``.  E is built from the counted fp32
  roundings of the formulas in include/biggan_hip.h times 2^-24 and, for the sums, ``launch_replay.bound`` over the
  element count: never from anything a kernel returned.  ``simulate`` is the same formula evaluated in float32 in the
  kernel's order of operations (tests/test_labels.py: it must pass the gate, the mutants must not).
* ``install(monkeypatch, spec, weights)`` - makes the whole-step oracle follow the configured loss: ``ref_model.Trainer``
  computes both label losses through ``oracle.ref_ops.cls_loss_logistic``.
"""
import torch

from tests import launch_replay as R

U32 = R.U32
D64 = torch.float64
KINDS = ("logistic", "euclidean")


def parse(spec, n):
    """-> [(kind, size), ...] with sizes summing to n; ValueError naming the spec otherwise."""
    spec = str(spec)
    if "," not in spec:
        if spec not in KINDS:
            raise ValueError("Invalid label loss type: " + spec)
        return [(spec, int(n))]
    out = []
    for part in spec.split(","):
        bits = part.split("-")
        if len(bits) != 2 or not bits[0].isdigit() or int(bits[0]) < 1 or bits[1] not in KINDS:
            raise ValueError("Invalid label loss type: %s (part %r)" % (spec, part))
        out.append((bits[1], int(bits[0])))
    if sum(s for _, s in out) != int(n):
        raise ValueError("Invalid label loss type: %s does not cover %d labels" % (spec, n))
    return out


def table(spec, n):
    """The device-side description of include/biggan_hip.h: (slices int32 [S, 2] = (kind, size), col_slice int32 [n])."""
    sl = parse(spec, n)
    slices = torch.tensor([[KINDS.index(k), s] for k, s in sl], dtype=torch.int32)
    cols = torch.tensor([i for i, (_, s) in enumerate(sl) for _ in range(s)], dtype=torch.int32)
    return slices, cols


def _sce(t, x):
    """tf.nn.sigmoid_cross_entropy_with_logits: max(x, 0) - x t + log(1 + exp(-|x|))."""
    return x.clamp_min(0) - x * t + torch.log1p(torch.exp(-x.abs()))


def _norm(ss):
    """sqrt with value 0 and gradient 0 at exactly 0."""
    pos = ss > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, ss, torch.ones_like(ss))), torch.zeros_like(ss))


def _columns(spec, n):
    a = 0
    for kind, size in parse(spec, n):
        yield kind, size, a, a + size
        a += size


def label_loss(truth, logits, weights, spec):
    """truth, logits [B, n] (the GLOBAL batch), weights [n] -> scalar, in logits' dtype, differentiable."""
    t, w = truth.to(logits.dtype), weights.to(logits.dtype)
    total = logits.new_zeros(())
    for kind, size, a, b in _columns(spec, logits.shape[1]):
        x, ts, ws = logits[:, a:b], t[:, a:b], w[a:b]
        if kind == "logistic":
            total = total + (_sce(ts, x) * ws).mean()
        else:
            d = (x - ts) * ws
            total = total + _norm((d * d).sum())
    return total


def dlogits(truth, logits, weights, spec, loss_weight=1.0):
    """d(loss_weight * label_loss)/d logits in closed form, float64."""
    t, x, w = truth.to(D64), logits.to(D64), weights.to(D64)
    B, n = x.shape
    out = torch.zeros_like(x)
    for kind, size, a, b in _columns(spec, n):
        xs, ts, ws = x[:, a:b], t[:, a:b], w[a:b]
        if kind == "logistic":
            out[:, a:b] = loss_weight * ws * (torch.sigmoid(xs) - ts) / (B * size)
        else:
            nrm = _norm((((xs - ts) * ws) ** 2).sum())
            if float(nrm) > 0:
                out[:, a:b] = loss_weight * ws * ws * (xs - ts) / nrm
    return out


# ------------------------------------------------------------------------------------------
# bounds.  Counted fp32 roundings (unit 2^-24) of the formulas in include/biggan_hip.h; the per-slice sums are fp64.
# ------------------------------------------------------------------------------------------
SIG_M = 5       # sigmoid(x) = 1 / (1 + e) or e / (1 + e), e = expf(-|x|): expf within 1 ulp = 2 units (2); 1 + e (3);
#                 the division (4); + 1 for the second-order terms.  Relative to sigmoid(x).
DIFF_M = 4      # c = loss_weight / (B size) rounded to fp32 (1); w c (2); sigmoid - t (3); their product (4).  Relative to
#                 |w c (sigmoid - t)|; the output's own rounding is the gate's 2^-24 |ref|.
EUC_M = 8       # x - t (1); * w (2); * w (3); c = loss_weight / norm rounded to fp32 (4); * c (5); the norm itself: every
#                 square carries 4 units of its two-rounding factor, so does their fp64 sum, the root halves it (6, 7);
#                 + 1 second-order.  Relative to |ref|.
SCE_TERM_M = 7  # one logistic term (max(x, 0) - x t + log1p(e)) * w: x t (1); the subtraction (2); e = expf within 1 ulp
#                 = 2 units, which log1p passes on at no more than its own size (3, 4); log1pf within 1 ulp (5, 6); the
#                 sum (7).  Relative to the term's absolute-value form; the * w is covered by bound()'s "+ 2".
EUC_LOSS_M = 3  # the norm from fp32 terms: 2 units (above) + 1 second-order


def grad_bound(truth, logits, weights, spec, loss_weight=1.0):
    """-> (ref, E) float64 [B, n] for the dlogits of bg_label_loss_finish (B = the global batch)."""
    t, x, w = truth.to(D64), logits.to(D64), weights.to(D64)
    B, n = x.shape
    ref = dlogits(t, x, w, spec, loss_weight)
    E = torch.zeros_like(ref)
    for kind, size, a, b in _columns(spec, n):
        if kind == "logistic":
            sig = torch.sigmoid(x[:, a:b])
            cw = abs(loss_weight) * w[a:b].abs() / (B * size)
            E[:, a:b] = U32 * cw * (SIG_M * sig + DIFF_M * (sig - t[:, a:b]).abs())
        else:
            E[:, a:b] = EUC_M * U32 * ref[:, a:b].abs()
    return ref, E


def loss_bound(truth, logits, weights, spec, loss_weight=1.0):
    """-> (ref, E) float64 scalars for the loss of bg_label_loss_finish: ``launch_replay.bound`` over the B n elements on
    the absolute-value form of the sum, plus the roundings inside a term."""
    t, x, w = truth.to(D64), logits.to(D64), weights.to(D64)
    B, n = x.shape
    ref = loss_weight * label_loss(t, x, w, spec)
    A_log = x.new_zeros(())
    A_euc = x.new_zeros(())
    for kind, size, a, b in _columns(spec, n):
        xs, ts, ws = x[:, a:b], t[:, a:b], w[a:b]
        if kind == "logistic":
            terms = (xs.clamp_min(0) + (xs * ts).abs() + torch.log1p(torch.exp(-xs.abs()))) * ws.abs()
            A_log = A_log + terms.mean()
        else:
            A_euc = A_euc + _norm((((xs - ts) * ws) ** 2).sum())
    lw = abs(loss_weight)
    A = lw * (A_log + A_euc)
    E = R.bound(A, B * n, lw * U32 * (SCE_TERM_M * A_log + EUC_LOSS_M * A_euc))
    return ref, E


def simulate(truth, logits, weights, spec, loss_weight=1.0, rows_global=None):
    """The two kernels' arithmetic on the CPU: fp32 terms in the kernel's order of operations, float64 sums.
    -> (loss float32 scalar, dlogits float32 [B, n])."""
    f = torch.float32
    t, x, w = truth.to(f), logits.to(f), weights.to(f)
    B, n = x.shape
    rows = float(rows_global if rows_global is not None else B)
    total = torch.zeros((), dtype=D64)
    dx = torch.zeros_like(x)
    for kind, size, a, b in _columns(spec, n):
        xs, ts, ws = x[:, a:b], t[:, a:b], w[a:b]
        if kind == "logistic":
            e = torch.exp(-xs.abs())
            s = ((xs.clamp_min(0) - xs * ts + torch.log1p(e)) * ws).to(D64).sum()
            total = total + s / (rows * size)
            c = torch.tensor(loss_weight / (rows * size), dtype=D64).to(f)
            sig = torch.where(xs >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
            dx[:, a:b] = (sig - ts) * (ws * c)
        else:
            d = (xs - ts) * ws
            ss = (d.to(D64) ** 2).sum()
            total = total + torch.sqrt(ss)
            c = (loss_weight / torch.sqrt(ss)).to(f) if float(ss) > 0 else torch.zeros((), dtype=f)
            dx[:, a:b] = d * ws * c
    return (loss_weight * total).to(f), dx


# ------------------------------------------------------------------------------------------
# inputs of the gate
# ------------------------------------------------------------------------------------------
def inputs(B, n, seed, weights="ones", spec=None, device="cpu"):
    """Logits N(0, 3^2), truth multi-hot (each label set with probability 0.3), weights 'ones', 'random' (U[0, 2]) or
    'zero-slice' (random, with every weight of the spec's LAST euclidean slice exactly 0: a zero norm)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, n, generator=g) * 3.0
    t = (torch.rand(B, n, generator=g) < 0.3).float()
    if weights == "ones":
        w = torch.ones(n)
    else:
        w = torch.rand(n, generator=g) * 2.0
        if weights == "zero-slice":
            euc = [(a, b) for kind, _, a, b in _columns(spec, n) if kind == "euclidean"]
            a, b = euc[-1]
            w[a:b] = 0.0
    return t.to(device), x.to(device), w.to(device)


def install(monkeypatch, spec, weights):
    """``oracle.ref_ops.cls_loss_logistic`` := the configured loss (the trainer passes weights of ones: ignored)."""
    from oracle import ref_ops
    wt = torch.as_tensor(weights, dtype=D64)

    def configured(truth, answer, cls_weights):
        return label_loss(truth, answer, wt.to(answer.dtype), spec)
    monkeypatch.setattr(ref_ops, "cls_loss_logistic", configured)
