"""The multi-branch convolution (bg_mixconv_fwd / _dgrad / _wgrad), the grouped dense projections (bg_dense_group_fwd /
_wgrad / _dgrad) and the latent routing (bg_latent_fanout / _fanin) against float64, element by element.

Every row of the case tables of tests/grouped_ref.py calls its entry point raw through ``hip.lib()``: outputs are
launch_replay.Buf buffers behind and before which sit guard bands, prefilled with NaN (or with their bf16-exact prior where
the call accumulates), foreign columns are the gaps of a strided view, every launch runs twice from the same prefill and
must return BG_OK and the same bits, and every output element must lie inside the derived bound of grouped_ref
(launch_replay.gate).  Operands the kernels must not read (the foreign columns of dy and of a column-sliced x) hold NaN.
The workspace query of the weight gradient must equal the restated slab count times 4 E.

One composed case per family runs through functional.py: MixConvFn forward and backward in bf16-resident mode on
variables whose gradient slots accumulate, the same on a forked input whose gradient accumulates, and LatentFanoutFn
followed by two groups of projections, backward through bg_dense_group_dgrad into bg_latent_fanin.

The last test prints the GateStats table: entry point (and kernel form), launches, worst err/bound, bf16 outputs whose
interval holds two values above / below the reference."""
import ctypes

import pytest
import torch

from tests import grouped_ref as G
from tests import launch_replay as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATS = R.GateStats()


def _hip():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip
    return Fn, hip


def _twice(what, run, outs):
    """Two runs from the same prefill: BG_OK, bit-identical outputs, guard bands and foreign columns untouched."""
    _, hip = _hip()
    first = None
    for rep in range(2):
        for o in outs:
            o.prefill()
        torch.cuda.synchronize()
        rc = run()
        assert rc == 0, "%s: %s" % (what, hip.lib().bg_last_error().decode())
        torch.cuda.synchronize()
        if rep == 0:
            first = [o.raw.clone() for o in outs]
    for o, f in zip(outs, first):
        if o.dtype != torch.uint8:                       # (scratch: guard bands only)
            assert torch.equal(o.raw, f), "%s: not bit-reproducible" % what
    for o in outs:
        assert o.guards_ok(), "%s: wrote outside its output (guard band / foreign columns)" % what


def _out(shape, dtype, y0=None, align=0):
    b = R.Buf(int(torch.Size(shape).numel()), dtype, DEV, align, shape=tuple(shape))
    b.y0 = y0
    return b


def _cols(rows, ld, width, dtype, y0=None):
    """[rows, width] inside rows ld apart: the other columns are foreign."""
    b = R.Buf(rows * ld, dtype, DEV, size=(rows, width), stride=(ld, 1))
    b.y0 = y0
    return b


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------
# multi-branch convolution
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in G.MIX_CASES])
def test_mixconv_case(name):
    Fn, hip = _hip()
    L = hip.lib()
    c = G.MIX[name]
    inp = G.mix_inputs(c)
    exp = G.mix_expect(c, inp)
    N, H, W, Cin, ldy = c["N"], c["H"], c["W"], c["Cin"], c["ldy"]
    P, n = N * H * W, len(c["table"])
    xdt, ydt = G._dt(c["xdt"]), G._dt(c["ydt"])
    lo, hi = G.mix_cols(c)
    es = torch.tensor([], dtype=ydt).element_size()

    xb = _out((N, H, W, Cin), xdt, align=c["x_off"])                 # (an input: at the case's byte offset)
    xb.prefill()
    xb.view.copy_(inp["x"])
    dy = inp["dy"].to(DEV)
    ws = [w.to(DEV) for w in inp["w"]]
    bs = [None if b is None else b.to(DEV) for b in inp["bias"]]
    # y: the branches' columns [lo, hi) of every row are the view, the rest of the row is foreign; the kernel's row
    # starts lo elements before the view's
    yb = _cols(P, ldy, hi - lo, ydt)
    y_ptr = ctypes.c_void_p(yb.ptr().value - lo * es)
    dxb = _out((N, H, W, Cin), xdt, y0=inp["dx0"], align=c["x_off"])
    dws = [_out(w.shape, torch.float32, y0=inp["dw0"][j]) if b["dw"] else None
           for j, (b, w) in enumerate(zip(c["table"], inp["w"]))]

    t = (hip.BgMixBranch * n)()
    for j, (e, b) in enumerate(zip(t, c["table"])):
        e.c_off, e.cb, e.k, e.dil, e.lo, e.pad_mode, e.transposed = b["c_off"], b["cb"], b["k"], b["dil"], b["lo"], \
            b["mode"], b["tr"]
        e.acc_w = b["acc_w"]
        e.w = ws[j].data_ptr()
        e.bias = None if bs[j] is None else bs[j].data_ptr()
        e.dw = None if dws[j] is None else dws[j].ptr().value
    tp = ctypes.cast(t, ctypes.c_void_p)
    d = hip.conv_desc(N, H, W, Cin, H, W, ldy, 1, 1, 0, G.ZERO, c["compute"], c["xdt"], c["ydt"])

    nb = int(L.bg_mixconv_wgrad_workspace_bytes(d, tp, n))
    assert nb == G.mix_slabs(c) * 4 * G.mix_elements(c), (nb, G.mix_slabs(c), G.mix_elements(c))
    wsb = R.Buf(nb, torch.uint8, DEV)

    form = {True: " [mfma]", False: " [direct]"}
    tag = {"bg_mixconv_fwd": form[G.mfma_ok(c)], "bg_mixconv_dgrad": form[G.mfma_ok(c)],
           "bg_mixconv_wgrad": form[G.mfma_shape(c)]}
    for k, v in tag.items():
        STATS.launch(k + v)
    st = hip.stream
    _twice(name + " forward", lambda: L.bg_mixconv_fwd(d, tp, n, xb.ptr(), y_ptr, ldy, st()), [yb])
    _twice(name + " input gradient",
           lambda: L.bg_mixconv_dgrad(d, tp, n, dy.data_ptr(), ldy, dxb.ptr(), c["accumulate"], st()), [dxb])
    # (a branch with dw = NULL has no buffer at all: whatever its blocks wrote would land in another branch's
    # gradient, a guard band or the workspace's)
    _twice(name + " weight gradient",
           lambda: L.bg_mixconv_wgrad(d, tp, n, xb.ptr(), dy.data_ptr(), ldy, wsb.ptr(), nb, st()),
           [b for b in dws if b is not None] + [wsb])
    assert xb.guards_ok() and torch.equal(xb.view.cpu(), inp["x"]), "x changed"
    assert _same_bits(dy.cpu(), inp["dy"]) and all(torch.equal(w.cpu(), w0) for w, w0 in zip(ws, inp["w"]))

    y = torch.full((P, ldy), G.NAN, dtype=ydt)
    y[:, lo:hi] = yb.view.cpu()
    outs = {"y": y.view(N, H, W, ldy), "dx": dxb.view.cpu()}
    for j, b in enumerate(dws):
        if b is not None:
            outs["dw%d" % j] = b.view.cpu()
    failures = G.mix_check(c, exp, outs, STATS, tag)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------
# grouped dense projections
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in G.DENSE_CASES])
def test_dense_group_case(name):
    Fn, hip = _hip()
    L = hip.lib()
    c = G.DENSE[name]
    inp = G.dense_inputs(c)
    exp = G.dense_expect(c, inp)
    B, n = c["B"], len(c["items"])
    dev = [{k: (None if v is None else v.to(DEV)) for k, v in i.items() if k != "x"} for i in inp]
    ys = [_out((B, it["N"]), torch.float32) for it in c["items"]]
    dws = [_out((it["K"], it["N"]), torch.float32, y0=i["dw0"]) for it, i in zip(c["items"], inp)]
    dbs = [_out((it["N"],), torch.float32, y0=i["db0"]) if it["db"] else None for it, i in zip(c["items"], inp)]

    def items(bwd):
        a = (hip.BgDenseItem * n)()
        for j, (e, it, dv) in enumerate(zip(a, c["items"], dev)):
            e.x, e.ldx = dv["x_full"].data_ptr() + 4 * it["x_col"], it["ldx"]
            e.K, e.N = it["K"], it["N"]
            if bwd:
                e.y, e.dw, e.acc_w, e.acc_b = dv["dy"].data_ptr(), dws[j].ptr().value, it["acc_w"], it["acc_b"]
                e.db = None if dbs[j] is None else dbs[j].ptr().value
            else:
                e.w, e.y = dv["w"].data_ptr(), ys[j].ptr().value
                e.bias = None if dv["bias"] is None else dv["bias"].data_ptr()
        return a

    fwd, bwd = items(False), items(True)
    STATS.launch("bg_dense_group_fwd")
    STATS.launch("bg_dense_group_wgrad")
    _twice(name + " forward", lambda: L.bg_dense_group_fwd(fwd, n, B, hip.stream()), ys)
    _twice(name + " weight gradient", lambda: L.bg_dense_group_wgrad(bwd, n, B, hip.stream()),
           dws + [b for b in dbs if b is not None])
    for dv, i in zip(dev, inp):
        assert _same_bits(dv["x_full"].cpu(), i["x_full"]) and torch.equal(dv["dy"].cpu(), i["dy"])
    outs = {}
    for j in range(n):
        outs["y%d" % j], outs["dw%d" % j] = ys[j].view.cpu(), dws[j].view.cpu()
        if dbs[j] is not None:
            outs["db%d" % j] = dbs[j].view.cpu()
    failures = G.flat_check(c, exp, outs, STATS)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", [c["name"] for c in G.DENSE_DGRAD_CASES])
def test_dense_group_input_gradient_case(name):
    Fn, hip = _hip()
    L = hip.lib()
    c = G.DENSE[name]
    inp = G.dense_dgrad_inputs(c)
    exp = G.dense_dgrad_expect(c, inp)
    B, K, n = c["B"], c["K"], len(c["Ns"])
    ws, dys = [w.to(DEV) for w in inp["ws"]], [g.to(DEV) for g in inp["dys"]]
    dx = _cols(B, K + 5, K, torch.float32, y0=inp["dx0"][:, :K] if c["acc"] else None)
    a = (hip.BgDenseItem * n)()
    for e, w, g in zip(a, ws, dys):
        e.w, e.y, e.K, e.N = w.data_ptr(), g.data_ptr(), K, w.shape[1]
    STATS.launch("bg_dense_group_dgrad")
    _twice(name, lambda: L.bg_dense_group_dgrad(a, n, B, dx.ptr(), K + 5, c["acc"], hip.stream()), [dx])
    failures = G.flat_check(c, exp, {"dx": dx.view.cpu()}, STATS)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------
# latent routing
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in G.LATENT_CASES])
def test_latent_case(name):
    Fn, hip = _hip()
    L = hip.lib()
    c = G.LATENT[name]
    inp = G.latent_inputs(c)
    exp = G.latent_expect(c, inp)
    B = c["B"]
    srcs = [s.to(DEV) for s in inp["srcs"]]
    tbs = [_cols(B, tg["ldd"], tg["width"], torch.float32, y0=p[:, :tg["width"]] if tg["accumulate"] else None)
           for tg, p in zip(c["targets"], inp["priors"])]
    tg = (hip.BgLatentTarget * len(tbs))()
    for e, t, b in zip(tg, c["targets"], tbs):
        e.dst, e.ldd, e.width, e.accumulate = b.ptr().value, t["ldd"], t["width"], t["accumulate"]
    sg = (hip.BgLatentSeg * len(c["segs"]))()
    for e, s in zip(sg, c["segs"]):
        e.src, e.lds = srcs[s["src"]].data_ptr(), c["src_widths"][s["src"]]
        e.src_col, e.dst_col, e.width, e.target = s["src_col"], s["dst_col"], s["width"], s["target"]
    fn = L.bg_latent_fanout if c["fanout"] else L.bg_latent_fanin
    entry = "bg_latent_fanout" if c["fanout"] else "bg_latent_fanin"
    STATS.launch(entry)
    _twice(name, lambda: fn(tg, len(tbs), sg, len(c["segs"]), B, hip.stream()), tbs)
    outs = {"t%d" % t: b.view.cpu() for t, b in enumerate(tbs)}
    failures = G.flat_check(c, exp, outs, STATS)
    assert not failures, "\n".join(failures)
    if c["fanout"]:                                      # a fan-out copies: the bits of the sources
        ref = G.latent_route(c["targets"], c["segs"], inp["srcs"], inp["priors"], B, dtype=torch.float32)
        assert all(torch.equal(outs["t%d" % t], r) for t, r in enumerate(ref))


# ------------------------------------------------------------------------------------------
# composed through functional.py
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fork", [False, True], ids=["variables", "forked-input"])
def test_composed_mixconv_fn(fork):
    """MixConvFn forward + backward in bf16-resident mode.  Every kernel is a store variable whose gradient slot has been
    written in this step, so the weight gradient adds into it (acc_w = 1); with ``fork`` the input is one output of a
    fork whose other branch has already left its gradient, so dx adds into that tensor.  The bounds are the raw ones:
    x, dy and the priors are given as bf16 tensors, so no intermediate bf16 store lies between the operands and the
    three gated outputs (y and dx are themselves stored in bf16, which the gate's interval covers)."""
    Fn, hip = _hip()
    c = G.composed_case(fork)
    inp = G.mix_inputs(c)
    exp = G.mix_expect(c, inp)
    Fn.set_precision("bf16")
    try:
        x = inp["x"].to(DEV).requires_grad_(True)
        prior = None
        if fork:
            prior = inp["dx0"].to(DEV).clone()
            x.bg_fork = Fn.ForkState()
            x.bg_fork.buf = prior
        params, slots = [], []
        for j, (w, b) in enumerate(zip(inp["w"], inp["bias"])):
            w = w.to(DEV).requires_grad_(True)
            w.bg_name, w.bg_grad, w.bg_touched = "mix/branch%d/kernel" % j, inp["dw0"][j].to(DEV).clone(), True
            slots.append(w.bg_grad)
            params += [w, None if b is None else b.to(DEV)]
        spec = tuple((b["c_off"], b["cb"], b["k"], b["dil"], b["lo"], b["mode"], b["tr"]) for b in c["table"])
        y = Fn.MixConvFn.apply(x, spec, *params)
        assert y.dtype == torch.bfloat16
        y.backward(inp["dy"].to(DEV))
        torch.cuda.synchronize()
        dx = x.grad
        assert dx.dtype == torch.bfloat16 and all(w.grad is None for w in params[0::2])
        assert not fork or _same_bits(dx, prior)         # (the launch added into the fork's tensor)
    finally:
        Fn.set_precision("fp32")
    outs = {"y": y.detach().cpu(), "dx": dx.cpu()}
    for j, s in enumerate(slots):
        outs["dw%d" % j] = s.cpu()
    tag = {k: " via MixConvFn" for k in ("bg_mixconv_fwd", "bg_mixconv_dgrad", "bg_mixconv_wgrad")}
    for k, v in tag.items():
        STATS.launch(k + v)
    failures = G.mix_check(c, exp, outs, STATS, tag)
    assert not failures, "\n".join(failures)


def test_composed_latent_fanout_and_grouped_projections():
    """LatentFanoutFn (the routing of case L1) followed by two GroupedDenseFn groups, one on level 0 and one on level 1,
    and their backward: the weight and bias gradients, bg_dense_group_dgrad per group and bg_latent_fanin, which sums the
    two levels' gradients of the class vector e and of the shared vector s.  Every intermediate tensor is fp32 (none is
    stored in bf16), so the rounding points added to the raw bounds are those of the chain: the fan-out copies exactly;
    each level gradient carries its own bound E_A / E_B into the fan-in, whose sum of two adds bound(|a| + |b|, 2)."""
    Fn, hip = _hip()
    c = G.LATENT["L1"]
    g = torch.Generator().manual_seed(77)
    B, widths = c["B"], [20, 40, 9]
    z, e, s = G.latent_inputs(c)["srcs"]
    segs, off = [], [0, 20, 60]
    for sg in c["segs"]:
        lvl = max(i for i in range(3) if off[i] <= sg["dst_col"])
        segs.append((sg["src"], sg["src_col"], lvl, sg["dst_col"] - off[lvl], sg["width"]))
    Ns = {0: (17, 24), 1: (24, 1)}
    w = {(l, i): R.bf16_exact((widths[l], n), g, "cpu", widths[l] ** -0.5) for l in Ns for i, n in enumerate(Ns[l])}
    b = {(l, 0): R.bf16_exact((Ns[l][0],), g, "cpu") for l in Ns}              # (the second item of a group: no bias)
    dy = {k: R.bf16_exact((B, v.shape[1]), g, "cpu") for k, v in w.items()}

    zt = z.to(DEV)
    et, st = e.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True)
    wt = {k: v.to(DEV).requires_grad_(True) for k, v in w.items()}
    bt = {k: v.to(DEV).requires_grad_(True) for k, v in b.items()}
    lev = Fn.LatentFanoutFn.apply(widths, segs, zt, et, st)
    ys = {}
    for l in Ns:
        ys[(l, 0)], ys[(l, 1)] = Fn.GroupedDenseFn.apply(2, lev[l], wt[(l, 0)], bt[(l, 0)], lev[l], wt[(l, 1)], None)
    keys = sorted(ys)
    leaves = [et, st] + [wt[k] for k in keys] + [bt[k] for k in sorted(bt)]
    grads = torch.autograd.grad([ys[k] for k in keys], leaves, [dy[k].to(DEV) for k in keys])
    torch.cuda.synchronize()
    got = dict(de=grads[0], ds=grads[1])
    for i, k in enumerate(keys):
        got["dw%d%d" % k] = grads[2 + i]
    for i, k in enumerate(sorted(bt)):
        got["db%d%d" % k] = grads[2 + len(keys) + i]

    D = torch.float64
    levels = [torch.cat([z[:, :10], e, s], 1).double(), torch.cat([z[:, 10:40], e, s], 1).double()]
    failures = []

    def check(entry, what, t, ref, E):
        G.record(STATS, failures, entry + " via functional", what, t.detach().cpu(), ref, E)

    for entry in ("bg_dense_group_fwd", "bg_dense_group_wgrad", "bg_dense_group_dgrad + bg_latent_fanin"):
        STATS.launch(entry + " via functional")
        STATS.launch(entry + " via functional")

    for l in Ns:
        assert torch.equal(lev[l].detach().cpu().double(), levels[l])            # the fan-out copies
    dl, El = {}, {}
    for l in Ns:
        x = levels[l]
        for i in (0, 1):
            wk, gk = w[(l, i)].double(), dy[(l, i)].double()
            bias = b[(l, i)].double() if (l, i) in b else None
            ref, A = G.dense_fwd(x, wk, bias), G.dense_fwd(x.abs(), wk.abs(), None if bias is None else bias.abs())
            check("bg_dense_group_fwd", "y%d%d" % (l, i), ys[(l, i)], ref,
                  R.bound(A, widths[l]) + (R.U32 * A if bias is not None else 0.0))
            (rw, rb), (Aw, Ab) = G.dense_wgrad(x, gk), G.dense_wgrad(x.abs(), gk.abs())
            check("bg_dense_group_wgrad", "dw%d%d" % (l, i), got["dw%d%d" % (l, i)], rw, R.bound(Aw, B))
            if bias is not None:
                check("bg_dense_group_wgrad", "db%d%d" % (l, i), got["db%d%d" % (l, i)], rb, R.bound(Ab, B))
        gs, wl = [dy[(l, i)].double() for i in (0, 1)], [w[(l, i)].double() for i in (0, 1)]
        dl[l] = G.dense_dgrad(gs, wl)
        El[l] = R.bound(G.dense_dgrad([t.abs() for t in gs], [t.abs() for t in wl]), sum(Ns[l]))
    for what, c0, c1, n in (("de", 10, 30, 9), ("ds", 19, 39, 1)):
        a, bb = dl[0][:, c0:c0 + n], dl[1][:, c1:c1 + n]
        Ea, Eb = El[0][:, c0:c0 + n], El[1][:, c1:c1 + n]
        E = Ea + Eb + R.bound(a.abs() + bb.abs() + Ea + Eb, 2)
        check("bg_dense_group_dgrad + bg_latent_fanin", what, got[what], (a + bb).to(D), E)
    assert not failures, "\n".join(failures)


def test_zz_gate_stats_table():
    """Not a check: prints how much of each bound the kernels used (the README quotes the worst ratios)."""
    print("\n" + STATS.table())
