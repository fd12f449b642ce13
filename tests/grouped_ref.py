"""float64 references, error bounds, case tables and simulated kernels of the multi-branch convolution
(csrc/mixconv.hip: bg_mixconv_fwd / _dgrad / _wgrad), the grouped dense projections and the latent routing
(csrc/dense_group.hip: bg_dense_group_fwd / _wgrad / _dgrad, bg_latent_fanout / _fanin).

Test helper, not product code.  The pattern of tests/weight_ref.py:

* references - plain float64 restatements of the comments of ``include/biggan_hip.h`` (BgMixBranch, BgDenseItem,
  BgLatentTarget / BgLatentSeg): explicit tf.pad-style padding per branch, one matmul per tap, the transposed branch as a
  correlation with the flipped [k,k,cb,Cin] kernel, the reflect fold as the adjoint of the padding.  Device-agnostic, no
  convolution library call; ``tests/test_grouped_gate.py`` checks them against float64 autograd.
* bounds - never anything a kernel returned.  Operands are bf16-representable, so every product is exact in fp32 and
  what is left is the fp32 accumulation and the store: ``E = (8 sqrt(K) + 2) 2^-24 A`` (launch_replay.bound) with ``A``
  the same reference on absolute values (|bias| and, when the call accumulates, the prior included) and ``K`` the number
  of products that reach the element - k^2 Cin forward, counted with all-ones operands for the two gradients (the
  reflect fold makes it vary per pixel, zero padding per tap), K / B / sum of N_i for the dense group, the number of
  covering segments for the fan-in - plus ``2^-24 A`` for every further rounding the code visibly has: each slab partial
  of the split-K finish, the ``acc_w`` / ``accumulate`` / ``acc_b`` add, the bias add.  Acceptance is launch_replay.gate.
  fp32 tensors under BG_COMPUTE_BF16 are the exception to the operands: they are NOT bf16-representable and the reference
  reads their RNE-rounded values, so a kernel that forgets to round misses by 2^-9 per product.
* case tables - fixed functions of their index; each row names the edge it exists for.
* simulated kernels - the same formulas in fp32 with the bf16 store (and the weight gradient slab by slab), with the
  mutations that ``tests/test_grouped_gate.py`` requires the gate to reject.
"""
import math

import torch

from tests.launch_replay import U32, bound, gate, bf16_exact

D64 = torch.float64
F32T, BF16T = torch.float32, torch.bfloat16
REFLECT, ZERO = 0, 1
EDGE = 2                       # edge replication: a mutation, no mode of the library
F32, BF16 = 0, 1
COMPUTE_F32, COMPUTE_BF16 = 0, 1
MIX_MAX_BRANCHES, DENSE_GROUP_MAX, LATENT_MAX_TARGETS, LATENT_MAX_SEGS = 8, 8, 8, 48
NAN = float("nan")


def bound_t(A, K):
    """launch_replay.bound with a reduction length that varies per element (K a tensor shaped like A)."""
    return (8.0 * K.sqrt() + 2.0) * U32 * A


def _dt(code):
    return BF16T if code == BF16 else F32T


# ------------------------------------------------------------------------------------------
# padding and its adjoint
# ------------------------------------------------------------------------------------------
def pad_idx(n, lo, npad, mode):
    """Source index of each of the npad padded coordinates of an axis (the first is -lo); n = the zero row."""
    idx = []
    for u in range(npad):
        j = u - lo
        if j < 0 or j >= n:
            if mode == ZERO:
                j = n
            elif mode == EDGE:
                j = min(max(j, 0), n - 1)
            else:                          # tf.pad REFLECT: mirrored at the border without repeating it
                j = -j if j < 0 else 2 * (n - 1) - j
                assert 0 <= j < n, (n, lo, npad)
        idx.append(j)
    return torch.tensor(idx, dtype=torch.long)


def pad2d(x, lo, Hp, Wp, mode):
    N, H, W, C = x.shape
    xe = torch.zeros((N, H + 1, W + 1, C), dtype=x.dtype, device=x.device)
    xe[:, :H, :W] = x
    xe = xe.index_select(1, pad_idx(H, lo, Hp, mode).to(x.device))
    return xe.index_select(2, pad_idx(W, lo, Wp, mode).to(x.device))


def fold2d(gp, lo, H, W, mode):
    """Adjoint of pad2d: every padded row / column adds into its source."""
    N, Hp, Wp, C = gp.shape
    t = torch.zeros((N, H + 1, Wp, C), dtype=gp.dtype, device=gp.device).index_add_(
        1, pad_idx(H, lo, Hp, mode).to(gp.device), gp)
    t = torch.zeros((N, H + 1, W + 1, C), dtype=gp.dtype, device=gp.device).index_add_(
        2, pad_idx(W, lo, Wp, mode).to(gp.device), t)
    return t[:, :H, :W]


# ------------------------------------------------------------------------------------------
# multi-branch convolution: one branch, any float dtype (float64 = the reference, float32 = the simulated kernel)
# ------------------------------------------------------------------------------------------
def corr_kernel(w, br, flip=True):
    """W(i,j,ci,c) [k,k,Cin,cb]: w itself, or for a transposed branch w[k-1-i][k-1-j][c][ci]."""
    if not br["tr"]:
        return w
    return (w.flip(0, 1) if flip else w).permute(0, 1, 3, 2)


def var_layout(Wc, br):
    """The inverse of corr_kernel: a [k,k,Cin,cb] tensor in the variable's layout."""
    return Wc.permute(0, 1, 3, 2).flip(0, 1) if br["tr"] else Wc


def _taps(br):
    return [(i, j) for i in range(br["k"]) for j in range(br["k"])]


def fwd_branch(x, w, br, mode=None, flip=True):
    """y[n,p,q,c] = sum_{i,j} sum_ci x[n, P(p - lo + i dil), P(q - lo + j dil), ci] W(i,j,ci,c)"""
    N, H, W, Cin = x.shape
    dil, span = br["dil"], (br["k"] - 1) * br["dil"]
    xp = pad2d(x, br["lo"], H + span, W + span, br["mode"] if mode is None else mode)
    Wc = corr_kernel(w, br, flip)
    y = torch.zeros((N, H, W, br["cb"]), dtype=x.dtype, device=x.device)
    for i, j in _taps(br):
        y += xp[:, i * dil:i * dil + H, j * dil:j * dil + W] @ Wc[i, j]
    return y


def dgrad_branch(dyb, w, br, mode=None):
    """The adjoint of fwd_branch in x: the gradient on the padded grid, folded back onto the image."""
    N, H, W, _ = dyb.shape
    dil, span = br["dil"], (br["k"] - 1) * br["dil"]
    Wc = corr_kernel(w, br)
    gp = torch.zeros((N, H + span, W + span, Wc.shape[2]), dtype=dyb.dtype, device=dyb.device)
    for i, j in _taps(br):
        gp[:, i * dil:i * dil + H, j * dil:j * dil + W] += dyb @ Wc[i, j].t()
    return fold2d(gp, br["lo"], H, W, br["mode"] if mode is None else mode)


def wgrad_branch(x, dyb, br, p0=0, p1=None):
    """dw in the variable's layout from the output pixels [p0, p1) (all of them by default)."""
    N, H, W, Cin = x.shape
    dil, span = br["dil"], (br["k"] - 1) * br["dil"]
    xp = pad2d(x, br["lo"], H + span, W + span, br["mode"])
    g = dyb.reshape(N * H * W, -1)[p0:p1]
    dWc = torch.zeros((br["k"], br["k"], Cin, br["cb"]), dtype=x.dtype, device=x.device)
    for i, j in _taps(br):
        dWc[i, j] = xp[:, i * dil:i * dil + H, j * dil:j * dil + W].reshape(N * H * W, Cin)[p0:p1].t() @ g
    return var_layout(dWc, br)


# ------------------------------------------------------------------------------------------
# multi-branch convolution: case table
# ------------------------------------------------------------------------------------------
def branch(kind, cb, k, dil=1, mode=REFLECT):
    """A clown-style branch (ops.py:403-436): stride-1 conv2d_transpose SAME (always zero-padded), or a conv whose
    padding centres the effective kernel."""
    if kind == "deconv":
        return dict(cb=cb, k=k, dil=1, lo=k - 1 - (k - 1) // 2, mode=ZERO, tr=1)
    return dict(cb=cb, k=k, dil=dil, lo=(k - 1) * dil // 2, mode=mode, tr=0)


def clown_table(inner, mode=REFLECT, no_deconv2=False):
    """ops.py:405-417: deconv4, deconv3, (deconv2,) conv3, conv5, dilated conv5 and their widths."""
    s = inner // 8
    d4, c5 = s + inner - 7 * s, s
    if no_deconv2:
        d4 += s // 2
        c5 += s - s // 2
    t = [branch("deconv", d4, 4), branch("deconv", 2 * s, 3)]
    if not no_deconv2:
        t.append(branch("deconv", s, 2))
    return t + [branch("conv", s, 3, 1, mode), branch("conv", c5, 5, 1, mode), branch("conv", s, 5, 2, mode)]


def _mix_case(name, why, table, N, H, W, Cin, xdt, ydt, compute=COMPUTE_BF16, ldy=None, c_off=0, x_off=0,
              unrounded=False):
    table = [dict(b) for b in table]
    off = c_off
    for b in table:
        b["c_off"] = off
        off += b["cb"]
    return dict(name=name, why=why, table=table, N=N, H=H, W=W, Cin=Cin, xdt=xdt, ydt=ydt, compute=compute,
                ldy=off if ldy is None else ldy, x_off=x_off, unrounded=unrounded)


def _mix_cases():
    M4T = [branch("conv", 3, 5, 2), branch("conv", 5, 1), branch("conv", 8, 3)]
    D2T = [branch("conv", 5, 3), branch("conv", 6, 5)]
    cases = [
        _mix_case("M1", "585 pixels: a 9-row partial tile, tiles straddling images, 2 slabs with boundary 292, the 8-pixel "
                  "fragment wraps rows and images", clown_table(8), 3, 15, 13, 32, BF16, BF16),
        _mix_case("M2", "cb 34 / 17: partial third wave, partial second K step of the input gradient; Cin % 64 != 0",
                  clown_table(136, ZERO), 2, 8, 8, 96, BF16, BF16),
        _mix_case("M3", "branches wider than a 64-column block, 30 pixels < one tile, foreign columns on both sides",
                  [branch("conv", 72, 3), branch("deconv", 80, 4)], 1, 5, 6, 64, BF16, BF16, ldy=160, c_off=3),
        _mix_case("M4", "reflection at its limit lo = H - 1, three sources per axis", M4T, 2, 5, 5, 32, BF16, BF16),
        _mix_case("M5", "the five-branch no_deconv2 table, 5 aligned slabs", clown_table(16, REFLECT, True), 5, 16, 16, 32,
                  BF16, BF16),
        _mix_case("D1", "direct <bf16,bf16>", clown_table(8), 3, 15, 13, 24, BF16, BF16),
        _mix_case("D2", "direct <bf16,float>", D2T, 2, 6, 7, 32, BF16, F32),
        _mix_case("D3", "direct <float,bf16>", D2T, 2, 6, 7, 32, F32, BF16),
        _mix_case("D4a", "direct <float,float>, exact fp32 chain", M4T, 2, 5, 5, 32, F32, F32, compute=COMPUTE_F32),
        _mix_case("D4b", "direct <float,float>, BG_COMPUTE_BF16 on unrounded operands", M4T, 2, 5, 5, 32, F32, F32,
                  unrounded=True),
        _mix_case("D5", "x / dx 8 bytes off a 16-byte boundary: forward and input gradient fall back to the direct "
                  "kernel, the weight gradient stays on the MFMA", clown_table(8), 3, 15, 13, 32, BF16, BF16, x_off=8),
    ]
    return [_mix_flags(c, idx) for idx, c in enumerate(cases)]


def _mix_flags(c, idx):
    c["idx"] = idx
    c["accumulate"] = idx % 2                              # the input gradient accumulates on odd cases
    n = len(c["table"])
    for j, b in enumerate(c["table"]):
        b["bias"] = j % 2 == 0                             # bias on the even branches
        b["acc_w"] = j % 2                                 # the gradient slot of a variable on the odd ones
        b["dw"] = j != idx % n                             # one branch per case has dw = NULL
    return c


MIX_CASES = _mix_cases()
MIX = {c["name"]: c for c in MIX_CASES}


def gap_case():
    """The largest map of tests/test_gpu_mixed.test_bf16_mfma_path_against_float64, where a whole-tensor norm hides a
    wrong pixel (tests/test_grouped_gate.py writes the figures down); no case of the GPU table."""
    return _mix_flags(_mix_case("GAP", "N 2, 32 x 32, Cin 96, inner 48", clown_table(48), 2, 32, 32, 96, BF16, BF16), 100)


def composed_case(fork):
    """The case of the composed run through functional.MixConvFn in bf16-resident mode: every kernel is a variable whose
    gradient slot was already written this step (acc_w = 1 on every branch); ``fork``: the input is a forked tensor whose
    other branch has delivered its gradient (dx accumulates).  No case of the raw table."""
    c = _mix_flags(_mix_case("C-fork" if fork else "C-var", "MixConvFn forward + backward", clown_table(16), 2, 8, 8, 32,
                             BF16, BF16), 200 + int(fork))
    c["accumulate"] = int(fork)
    for b in c["table"]:
        b["acc_w"], b["dw"] = 1, True
    return c


def mfma_shape(c):
    return c["xdt"] == BF16 and c["ydt"] == BF16 and c["Cin"] % 32 == 0


def mfma_ok(c):
    """mx_mfma_ok: the shape rule and a 16-byte aligned x / dx."""
    return mfma_shape(c) and c["x_off"] % 16 == 0


def mix_prepare_ok(c):
    """mix_prepare's preconditions."""
    ok = 1 <= len(c["table"]) <= MIX_MAX_BRANCHES and min(c["N"], c["H"], c["W"], c["Cin"]) > 0
    for b in c["table"]:
        ok = ok and b["cb"] > 0 and b["k"] >= 1 and b["dil"] >= 1 and b["lo"] >= 0 and b["c_off"] >= 0
        ok = ok and b["c_off"] + b["cb"] <= c["ldy"] and b["mode"] in (REFLECT, ZERO)
        if b["mode"] == REFLECT:
            hi = (b["k"] - 1) * b["dil"] - b["lo"]
            ok = ok and max(b["lo"], hi) <= min(c["H"], c["W"]) - 1
    return bool(ok)


def mix_elements(c):
    return sum(b["k"] * b["k"] * c["Cin"] * b["cb"] for b in c["table"])


def mix_slabs(c):
    """mix_slabs of csrc/mixconv.hip: the MFMA form wants >= 2048 blocks in all and >= 256 pixels per slab, the direct
    form splits the image rows while slabs x elements stays within 2^21."""
    if mfma_shape(c):
        P = c["N"] * c["H"] * c["W"]
        blocks = sum(b["k"] * b["k"] * ((c["Cin"] + 63) // 64) * ((b["cb"] + 63) // 64) for b in c["table"])
        return max(1, min((2048 + blocks - 1) // blocks, P // 256, 1024))
    return min(max(1, (1 << 21) // mix_elements(c)), c["N"] * c["H"], 1024)


def slab_ranges(c):
    """Pixel range of every slab: pixel slabs in the MFMA form, slabs of whole image rows in the direct form."""
    s = mix_slabs(c)
    if mfma_shape(c):
        P = c["N"] * c["H"] * c["W"]
        return [(P * i // s, P * (i + 1) // s) for i in range(s)]
    rows = c["N"] * c["H"]
    return [(rows * i // s * c["W"], rows * (i + 1) // s * c["W"]) for i in range(s)]


def mix_cols(c):
    """(first, past-last) channel the branches write in a row of y."""
    return min(b["c_off"] for b in c["table"]), max(b["c_off"] + b["cb"] for b in c["table"])


def mix_inputs(c):
    """Deterministic operands (CPU): x, dy (NaN in the foreign columns: a kernel that reads them shows it), branch
    kernels, biases, and the bf16-exact priors of dx and dw."""
    g = torch.Generator().manual_seed(4000 + c["idx"])
    N, H, W, Cin, ldy = c["N"], c["H"], c["W"], c["Cin"], c["ldy"]

    def draw(shape, scale=1.0, dtype=F32T):
        if c["unrounded"]:
            return (torch.randn(shape, generator=g) * scale).to(dtype)
        return bf16_exact(shape, g, "cpu", scale, dtype)

    inp = dict(x=draw((N, H, W, Cin), 1.0, _dt(c["xdt"])))
    dy = torch.full((N, H, W, ldy), NAN, dtype=_dt(c["ydt"]))
    lo, hi = mix_cols(c)
    dy[..., lo:hi] = draw((N, H, W, hi - lo), 1.0, _dt(c["ydt"]))
    inp["dy"] = dy
    inp["w"], inp["bias"], inp["dw0"] = [], [], []
    for b in c["table"]:
        shape = (b["k"], b["k"], b["cb"], Cin) if b["tr"] else (b["k"], b["k"], Cin, b["cb"])
        inp["w"].append(draw(shape, 1.0 / math.sqrt(b["k"] * b["k"] * Cin)))
        inp["bias"].append(bf16_exact((b["cb"],), g, "cpu") if b["bias"] else None)
        inp["dw0"].append(bf16_exact(shape, g, "cpu") if b["dw"] and b["acc_w"] else None)
    inp["dx0"] = bf16_exact((N, H, W, Cin), g, "cpu", 1.0, _dt(c["xdt"])) if c["accumulate"] else None
    return inp


def _rounds(c):
    return not (c["xdt"] == F32 and c["ydt"] == F32 and c["compute"] == COMPUTE_F32)


def _operand(c, t, dtype, rounded=True):
    """A multiplied operand as the arithmetic sees it: RNE-rounded to bf16 unless the call is the exact fp32 chain."""
    t = t.to(BF16T) if (_rounds(c) and rounded) else t
    return t.to(dtype)


def mix_expect(c, inp):
    """-> [(entry point, label, output key, channel slice or None, ref, E)] for every output of the three passes."""
    out = []
    x = _operand(c, inp["x"], D64)
    ws = [_operand(c, w, D64) for w in inp["w"]]
    ones_x = torch.ones_like(x)
    slabs = mix_slabs(c)
    dref = dA = dK = 0.0
    for j, (b, w) in enumerate(zip(c["table"], ws)):
        sl = slice(b["c_off"], b["c_off"] + b["cb"])
        dyb = _operand(c, inp["dy"][..., sl], D64)
        # forward: K = k^2 Cin; the bias is one more rounding (the direct chain starts from it, the MFMA form adds it)
        ref, A = fwd_branch(x, w, b), fwd_branch(x.abs(), w.abs(), b)
        E = bound(A, b["k"] * b["k"] * c["Cin"])
        if b["bias"]:
            ref, A = ref + inp["bias"][j].double(), A + inp["bias"][j].double().abs()
            E = bound(A, b["k"] * b["k"] * c["Cin"]) + U32 * A
        out.append(("bg_mixconv_fwd", "y[branch %d]" % j, "y", sl, ref, E))
        dref = dref + dgrad_branch(dyb, w, b)
        dA = dA + dgrad_branch(dyb.abs(), w.abs(), b)
        dK = dK + dgrad_branch(torch.ones_like(dyb), torch.ones_like(w), b)
        if b["dw"]:
            ref, A = wgrad_branch(x, dyb, b), wgrad_branch(x.abs(), dyb.abs(), b)
            K = wgrad_branch(ones_x, torch.ones_like(dyb), b)          # pixels that contribute (zero padding: per tap)
            extra = float(slabs)                                       # v += ws[s][e], once per slab
            if b["acc_w"]:
                ref, A = ref + inp["dw0"][j].double(), A + inp["dw0"][j].double().abs()
                extra += 1.0                                           # dw[el] + v
            out.append(("bg_mixconv_wgrad", "dw[branch %d]" % j, "dw%d" % j, None, ref, bound_t(A, K) + extra * U32 * A))
    E = bound_t(dA, dK)
    if c["accumulate"]:
        dref, dA = dref + inp["dx0"].double(), dA + inp["dx0"].double().abs()
        E = bound_t(dA, dK) + U32 * dA                                 # dx + acc
    out.append(("bg_mixconv_dgrad", "dx", "dx", None, dref, E))
    return out


def mix_sim(c, inp, mut=None, slabwise=False):
    """The simulated kernels: the formulas above in fp32, stored in the outputs' types; outputs as the launches leave
    them (NaN where nothing was written).  ``mut``: one of the mutations of tests/test_grouped_gate.py."""
    mut = mut or ("none",)
    rounded = mut[0] != "unrounded"
    N, H, W, Cin, ldy = c["N"], c["H"], c["W"], c["Cin"], c["ldy"]
    P = N * H * W
    x = _operand(c, inp["x"], F32T, rounded)
    ws = [_operand(c, w, F32T, rounded) for w in inp["w"]]
    outs = {"y": torch.full((N, H, W, ldy), NAN, dtype=_dt(c["ydt"]))}
    dx = torch.zeros((N, H, W, Cin), dtype=F32T)
    for j, (b, w) in enumerate(zip(c["table"], ws)):
        sl = slice(b["c_off"], b["c_off"] + b["cb"])
        dyb = _operand(c, inp["dy"][..., sl], F32T, rounded)
        y = fwd_branch(x, w, b, mode=EDGE if mut == ("edge", j) else None, flip=mut != ("noflip", j))
        if b["bias"]:
            y = y + inp["bias"][j]
        if mut == ("shift", j):
            sl = slice(sl.start + 1, sl.stop + 1)
        if mut[0] == "tile":                               # the last, partial 64-pixel tile stays unwritten
            y.view(P, -1)[P // 64 * 64:] = NAN
        outs["y"][..., sl] = y.to(outs["y"].dtype)
        g = dgrad_branch(dyb, w, b)
        if mut[0] == "nofold" and mut[1] == j:             # the mirrored sources of one pixel (of image 0) are not visited
            p, q = mut[2], mut[3]
            g[0, p, q] = dgrad_branch(dyb, w, b, mode=ZERO)[0, p, q]
        dx = dx + g
        if not b["dw"]:
            continue
        if slabwise or mut[0] == "slab_drop":
            dw = torch.zeros_like(w)
            for s, (p0, p1) in enumerate(slab_ranges(c)):
                if mut[0] == "slab_drop" and s == 0:
                    p1 -= 1                                # the last pixel before the first slab boundary is lost
                dw = dw + wgrad_branch(x, dyb, b, p0, p1)
        else:
            dw = wgrad_branch(x, dyb, b)
        if b["acc_w"] and mut[0] != "no_acc_w":
            dw = inp["dw0"][j] + dw
        outs["dw%d" % j] = dw
    if c["accumulate"] and mut[0] != "no_acc":
        dx = inp["dx0"].float() + dx
    outs["dx"] = dx.to(_dt(c["xdt"]))
    return outs


# ------------------------------------------------------------------------------------------
# grouped dense projections
# ------------------------------------------------------------------------------------------
def dense_fwd(x, w, bias=None):
    y = x @ w
    return y if bias is None else y + bias


def dense_wgrad(x, dy, rows=None):
    """(dw, db) from the first ``rows`` batch rows (all by default)."""
    return x[:rows].t() @ dy[:rows], dy[:rows].sum(0)


def dense_dgrad(dys, ws):
    return sum(dy @ w.t() for dy, w in zip(dys, ws))


def _dense_case(name, why, B, items):
    its = []
    for j, (K, N) in enumerate(items):
        its.append(dict(K=K, N=N, ldx=K + 3 if j % 2 else K, x_col=2 if j % 2 else 0,      # odd items: a column slice
                        bias=j % 3 != 2, db=j % 4 != 3, acc_w=j % 2, acc_b=(j // 2) % 2))
    return dict(name=name, why=why, B=B, items=its)


DENSE_CASES = [
    _dense_case("G1", "a group of one, K = N = 1, B = 3 (< one 8-row strip)", 3, [(1, 1)]),
    _dense_case("G4", "four items of different K in one group, B = 13 (a partial strip), N = 300 (two column tiles)", 13,
                [(20, 17), (37, 300), (1, 17), (20, 1)]),
    _dense_case("G8", "BG_DENSE_GROUP_MAX items, B = 130: two full 64-row chunks plus 2 rows", 130,
                [(37, 300), (20, 17), (1, 1), (37, 17), (20, 300), (37, 1), (1, 300), (20, 17)]),
]
DENSE_DGRAD_CASES = [
    dict(name="DG1", why="K = N = 1", B=3, K=1, Ns=(1,), acc=0),
    dict(name="DG2", why="N at, one past and far past the 64-column chunk, accumulate", B=13, K=37, Ns=(64, 65, 300, 1),
         acc=1),
    dict(name="DG3", why="K = 65: a third 32-column tile of one column, B = 130", B=130, K=65, Ns=(300, 65, 64), acc=0),
    dict(name="DG4", why="BG_DENSE_GROUP_MAX items, accumulate", B=13, K=65, Ns=(1, 64) * 4, acc=1),
]
for _i, _c in enumerate(DENSE_CASES + DENSE_DGRAD_CASES):
    _c["idx"] = _i
DENSE = {c["name"]: c for c in DENSE_CASES + DENSE_DGRAD_CASES}


def dense_inputs(c):
    """Per item: x_full [B, ldx] (NaN outside the item's K columns), w, bias, dy and the priors of dw / db."""
    g = torch.Generator().manual_seed(5000 + c["idx"])
    B, out = c["B"], []
    for it in c["items"]:
        K, N = it["K"], it["N"]
        xf = torch.full((B, it["ldx"]), NAN)
        xf[:, it["x_col"]:it["x_col"] + K] = bf16_exact((B, K), g, "cpu")
        out.append(dict(x_full=xf, x=xf[:, it["x_col"]:it["x_col"] + K], w=bf16_exact((K, N), g, "cpu", K ** -0.5),
                        bias=bf16_exact((N,), g, "cpu") if it["bias"] else None, dy=bf16_exact((B, N), g, "cpu"),
                        dw0=bf16_exact((K, N), g, "cpu") if it["acc_w"] else None,
                        db0=bf16_exact((N,), g, "cpu") if it["db"] and it["acc_b"] else None))
    return out


def dense_expect(c, inp):
    out = []
    for j, (it, i) in enumerate(zip(c["items"], inp)):
        x, w, dy = i["x"].double(), i["w"].double(), i["dy"].double()
        b = None if i["bias"] is None else i["bias"].double()
        ref, A = dense_fwd(x, w, b), dense_fwd(x.abs(), w.abs(), None if b is None else b.abs())
        out.append(("bg_dense_group_fwd", "y[item %d]" % j, "y%d" % j, ref,
                    bound(A, it["K"]) + (U32 * A if b is not None else 0.0)))
        (rw, rb), (Aw, Ab) = dense_wgrad(x, dy), dense_wgrad(x.abs(), dy.abs())
        extra = 0.0
        if it["acc_w"]:
            rw, Aw, extra = rw + i["dw0"].double(), Aw + i["dw0"].double().abs(), 1.0
        out.append(("bg_dense_group_wgrad", "dw[item %d]" % j, "dw%d" % j, rw, bound(Aw, c["B"]) + extra * U32 * Aw))
        if it["db"]:
            extra = 0.0
            if it["acc_b"]:
                rb, Ab, extra = rb + i["db0"].double(), Ab + i["db0"].double().abs(), 1.0
            out.append(("bg_dense_group_wgrad", "db[item %d]" % j, "db%d" % j, rb, bound(Ab, c["B"]) + extra * U32 * Ab))
    return out


def dense_sim(c, inp, mut=None):
    mut = mut or ("none",)
    outs = {}
    for j, (it, i) in enumerate(zip(c["items"], inp)):
        outs["y%d" % j] = dense_fwd(i["x"], i["w"], i["bias"])
        dw, db = dense_wgrad(i["x"], i["dy"])
        if mut[0] == "db_rows":
            db = dense_wgrad(i["x"], i["dy"], c["B"] - 1)[1]
        outs["dw%d" % j] = i["dw0"] + dw if it["acc_w"] and mut[0] != "no_acc_w" else dw
        if it["db"]:
            outs["db%d" % j] = i["db0"] + db if it["acc_b"] else db
    return outs


def dense_dgrad_inputs(c):
    g = torch.Generator().manual_seed(5000 + c["idx"])
    B, K = c["B"], c["K"]
    dx0 = torch.full((B, K + 5), NAN)                       # rows K + 5 apart: the last 5 columns are foreign
    if c["acc"]:
        dx0[:, :K] = bf16_exact((B, K), g, "cpu")
    return dict(ws=[bf16_exact((K, n), g, "cpu", n ** -0.5) for n in c["Ns"]],
                dys=[bf16_exact((B, n), g, "cpu") for n in c["Ns"]], dx0=dx0)


def dense_dgrad_expect(c, inp):
    ws, dys = [w.double() for w in inp["ws"]], [d.double() for d in inp["dys"]]
    ref, A = dense_dgrad(dys, ws), dense_dgrad([d.abs() for d in dys], [w.abs() for w in ws])
    E = bound(A, sum(c["Ns"]))
    if c["acc"]:
        y0 = inp["dx0"][:, :c["K"]].double()
        ref, A = ref + y0, A + y0.abs()
        E = bound(A, sum(c["Ns"])) + U32 * A
    return [("bg_dense_group_dgrad", "dx", "dx", ref, E)]


def dense_dgrad_sim(c, inp, mut=None):
    dx = dense_dgrad(inp["dys"], inp["ws"])
    if c["acc"] and (mut or ("none",))[0] != "no_acc":
        dx = inp["dx0"][:, :c["K"]] + dx
    out = inp["dx0"].clone()
    out[:, :c["K"]] = dx
    return {"dx": out[:, :c["K"]]}


# ------------------------------------------------------------------------------------------
# latent fan-out / fan-in
# ------------------------------------------------------------------------------------------
def latent_route(targets, segs, srcs, priors, B, abs_=False, count=False, dtype=D64):
    """target t, element (b, c) (+)= sum over the segments with target == t that cover c, in array order, of
    src[b, src_col + c - dst_col]; an uncovered column becomes 0 or keeps its prior."""
    outs = []
    for t, tg in enumerate(targets):
        s = torch.zeros((B, tg["width"]), dtype=dtype)
        for sg in segs:
            if sg["target"] != t:
                continue
            v = srcs[sg["src"]][:, sg["src_col"]:sg["src_col"] + sg["width"]].to(dtype)
            v = torch.ones_like(v) if count else (v.abs() if abs_ else v)
            s[:, sg["dst_col"]:sg["dst_col"] + sg["width"]] += v
        if tg["accumulate"] and not count:
            p = priors[t][:, :tg["width"]].to(dtype)
            s = (p.abs() if abs_ else p) + s
        outs.append(s)
    return outs


def _latent_cases():
    fan_segs = [(0, 0, 0, 0, 10), (1, 0, 0, 10, 9), (2, 0, 0, 19, 1), (0, 10, 1, 0, 30), (1, 0, 1, 30, 9),
                (2, 0, 1, 39, 1), (1, 0, 2, 0, 9)]                  # (source, source column, level, level column, width)
    widths, off = [20, 40, 9], [0, 20, 60]
    cases = [
        dict(name="L1", why="the fan-out of LatentFanoutFn: the levels are column ranges of one packed target", fanout=True,
             B=13, src_widths=[40, 9, 1], targets=[dict(width=69, ldd=69, accumulate=0)],
             segs=[dict(src=s, src_col=sc, target=0, dst_col=off[o] + oc, width=w) for s, sc, o, oc, w in fan_segs]),
        dict(name="L2", why="the same routing onto one target per level, one of them with ldd > width", fanout=True, B=13,
             src_widths=[40, 9, 1], targets=[dict(width=w, ldd=w + (3 if i == 1 else 0), accumulate=0)
                                             for i, w in enumerate(widths)],
             segs=[dict(src=s, src_col=sc, target=o, dst_col=oc, width=w) for s, sc, o, oc, w in fan_segs]),
        dict(name="L3", why="the raw fan-in of test_latent_fanout_and_fanin: an accumulating target, an uncovered column "
             "that must become 0, ldd > width", fanout=False, B=13, src_widths=[20, 40, 9],
             targets=[dict(width=12, ldd=12, accumulate=1), dict(width=3, ldd=4, accumulate=0)],
             segs=[dict(src=1, src_col=0, target=0, dst_col=0, width=12), dict(src=0, src_col=5, target=0, dst_col=2, width=3),
                   dict(src=2, src_col=0, target=1, dst_col=0, width=2)]),
    ]
    # the maxima: 48 segments on 8 targets; the last column of every target is covered by no segment (it becomes 0 on the
    # overwriting targets and keeps its prior on the accumulating ones), odd targets accumulate and have ldd > width
    targets = [dict(width=5 + t, ldd=5 + t + t % 2, accumulate=t % 2) for t in range(LATENT_MAX_TARGETS)]
    segs = []
    for i in range(LATENT_MAX_SEGS):
        t, j = i % 8, i // 8
        segs.append(dict(src=i % 3, src_col=(3 * i) % 10, target=t, dst_col=(2 * j) % (targets[t]["width"] - 3),
                         width=1 + (j + t) % 3))
    cases.append(dict(name="L4", why="BG_LATENT_MAX_SEGS segments on BG_LATENT_MAX_TARGETS targets", fanout=False, B=13,
                      src_widths=[16, 16, 16], targets=targets, segs=segs))
    for idx, c in enumerate(cases):
        c["idx"] = idx
    return cases


LATENT_CASES = _latent_cases()
LATENT = {c["name"]: c for c in LATENT_CASES}


def latent_inputs(c):
    g = torch.Generator().manual_seed(6000 + c["idx"])
    srcs = [bf16_exact((c["B"], w), g, "cpu") for w in c["src_widths"]]
    priors = []
    for tg in c["targets"]:
        p = torch.full((c["B"], tg["ldd"]), NAN)
        if tg["accumulate"]:
            p[:, :tg["width"]] = bf16_exact((c["B"], tg["width"]), g, "cpu")
        priors.append(p)
    return dict(srcs=srcs, priors=priors)


def latent_expect(c, inp):
    a = (c["targets"], c["segs"], inp["srcs"], inp["priors"], c["B"])
    ref, A, K = latent_route(*a), latent_route(*a, abs_=True), latent_route(*a, count=True)
    entry = "bg_latent_fanout" if c["fanout"] else "bg_latent_fanin"
    out = []
    for t, tg in enumerate(c["targets"]):
        E = bound_t(A[t], K[t]) + (U32 * A[t] if tg["accumulate"] else 0.0)       # *o + s
        out.append((entry, "target %d" % t, "t%d" % t, ref[t], E))
    return out


def latent_sim(c, inp, mut=None):
    segs = c["segs"]
    if (mut or ("none",))[0] == "wrong_target":
        segs = [dict(s) for s in segs]
        segs[mut[1]]["target"] = mut[2]
    r = latent_route(c["targets"], segs, inp["srcs"], inp["priors"], c["B"], dtype=F32T)
    return {"t%d" % t: v for t, v in enumerate(r)}


# ------------------------------------------------------------------------------------------
# acceptance, reported like launch_replay.Replayer.record
# ------------------------------------------------------------------------------------------
def record(stats, failures, kernel, what, got, ref, E):
    """Gate one output; on failure append the count and the first three indices with got, ref and E."""
    if not torch.is_tensor(E):
        E = torch.full_like(ref, float(E))
    E = E.expand_as(ref)
    ok, ratio, above, below, nbad = gate(got, ref, E)
    if stats is not None:
        stats.add(kernel, ratio, above, below)
    if not ok:
        g = got.double()
        if got.dtype == BF16T:
            lo, hi = (ref - E).to(BF16T).double(), (ref + E).to(BF16T).double()
        else:
            lo, hi = ref - E - U32 * ref.abs(), ref + E + U32 * ref.abs()
        bad = ~((g >= lo) & (g <= hi))
        where = [tuple(int(i) for i in ix) for ix in bad.nonzero()[:3].tolist()]
        detail = "; ".join("at %s got %.9g ref %.9g E %.3g" % (ix, g[ix].item(), ref[ix].item(), E[ix].item())
                           for ix in where)
        failures.append("%s %s: %d of %d elements outside the bound (%s)" % (kernel, what, nbad, got.numel(), detail))
    return ok


def mix_check(c, exp, outs, stats=None, tag=None):
    """Gate every output of ``outs`` that ``exp`` (mix_expect) names -> list of failure messages.  ``tag``: a suffix
    per entry point for the rows of ``stats`` (the kernel form)."""
    failures = []
    for entry, label, key, sl, ref, E in exp:
        got = outs[key].cpu()
        got = got[..., sl] if sl is not None else got
        record(stats, failures, entry + (tag or {}).get(entry, ""), "%s %s" % (c["name"], label), got.reshape(ref.shape),
               ref, E)
    return failures


def flat_check(c, exp, outs, stats=None):
    """The same for the dense and latent tables (expectations without a channel slice)."""
    failures = []
    for entry, label, key, ref, E in exp:
        record(stats, failures, entry, "%s %s" % (c["name"], label), outs[key].cpu().reshape(ref.shape), ref, E)
    return failures
