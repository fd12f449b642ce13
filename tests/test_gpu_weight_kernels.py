"""The kernels that run once per weight per step - spectral norm (single and multi-tensor form, packed bf16 copies), the
orthogonal regularisers (Gram side and low-rank form) and the TF-Adam + EMA update - against float64.

Every row of the case table of tests/weight_ref.py calls its entry point raw through ``hip.lib()`` under the rules of
tests/test_gpu_elementwise16.Runner: guarded buffers (launch_replay.Buf) for every input, output and workspace, outputs
prefilled with NaN (or their initial value where the call accumulates or works in place: loss_accum, dw under the
accumulate mask, the in-place u, the Adam state), two runs that must agree bit for bit - the loss scalars excepted, which
several blocks add to with fp32 atomicAdd and which are gated after both runs instead - inputs left unchanged, and the
per-element gate of launch_replay against the float64 reference with the bounds of weight_ref.  One GateStats table per
entry point records how much of each bound is used.

One composed case per form runs functional.OrthoCosineRegFn's low-rank chain and the dense chain on the same weight at
the ``2 * rows <= c`` boundary against oracle/ref_ops.ortho_reg_loss and its autograd gradient."""
import ctypes
import math
import time

import pytest
import torch

from tests import launch_replay as R
from tests import weight_ref as W
from tests.test_gpu_elementwise16 import Runner, _lib

pytestmark = pytest.mark.gpu

class View:
    """An output that is a slice of a buffer another entry of ``outs`` guards."""

    def __init__(self, view):
        self.view = view


class WeightRunner(Runner):
    ref = W
    alt_label = "_dev entry"

    def key_of(self, c):
        return W.ENTRY[c["op"]]

    def wants_alt(self, c):
        return c["op"] == "adam"

    def gate(self, label, got, ref, Eb):
        entry = self.key
        self.key = "%s: %s" % (entry, label.split(" (")[0])
        try:
            super().gate(label, got, ref, Eb)
            self.stats.add(entry, self.stats.rows[self.key][1])
        finally:
            self.key = entry

    def exact(self, label, got, want):
        entry = self.key
        self.key = "%s: %s" % (entry, label)
        try:
            super().exact(label, got, want)
        finally:
            self.key = entry

    # -- buffers
    def buf(self, t, align=0, out=False, y0=None, shape=None, dtype=torch.float32):
        """A guarded buffer: an input holding t, or an output prefilled with y0 (None = NaN)."""
        if t is not None:
            shape, dtype = tuple(t.shape), t.dtype
        b = R.Buf(math.prod(shape), dtype, self.dev, align, shape=shape)
        if out:
            b.y0 = y0
            self.outs.append(b)
        else:
            b.view.copy_(t)
            b.src = t
            self.ins.append(b)
        return b

    def scratch(self, nbytes):
        b = R.Buf(max(int(nbytes), 16), torch.uint8, self.dev)
        self.outs.append(b)
        return b

    # -- the BgSnItem table of a multi-tensor case
    def table(self, c, i, bwd):
        """-> (device table, host items, {name: output}, workspace Buf, its byte count)."""
        hip, L = self.hip, self.L
        n = len(c["items"])
        items = (hip.BgSnItem * n)()
        out, groups, off = {}, {}, 0
        en = c.get("enable")
        acc = c.get("accumulate") or []
        for j, (it, ij) in enumerate(zip(c["items"], i["items"])):
            rows, cols, t = it["rows"], it["cols"], items[j]
            t.rows, t.cols, t.taps, t.pack_p_ld = rows, cols, max(it["taps"], 0), 0
            if bwd:
                b = {k: self.buf(ij[k]) for k in ("g", "wn", "u", "v", "sigma")}
                keep = j in acc or (en is not None and j not in en)
                dw = self.buf(None, out=True, y0=ij["dw0"] if keep else None, shape=(rows, cols))
                out["%d.dw" % j] = dw
                t.g_wnorm, t.w_norm, t.u, t.v, t.sigma = (b[k].ptr().value for k in ("g", "wn", "u", "v", "sigma"))
                t.dw = dw.ptr().value
                continue
            w = self.buf(ij["w"])
            u = self.buf(None, out=True, y0=ij["u0"], shape=(cols,))
            o = dict(u=u, v=self.buf(None, out=True, shape=(rows,)), sigma=self.buf(None, out=True, shape=(1,)),
                     wn=self.buf(None, out=True, shape=(rows, cols)))
            t.w, t.u, t.v, t.sigma, t.w_norm = (x.ptr().value for x in (w, o["u"], o["v"], o["sigma"], o["wn"]))
            t.ws_offset = off
            off += (int(L.bg_spectral_norm_workspace_bytes(rows, cols)) + 15) // 16 * 16
            if it["taps"]:
                taps, Rr = it["taps"], rows // it["taps"]
                if it["group"] is None:
                    pp = self.buf(None, out=True, shape=(taps, Rr, cols), dtype=torch.bfloat16)
                    pt = self.buf(None, out=True, shape=(taps, cols, Rr), dtype=torch.bfloat16)
                    t.pack_p, t.pack_t = pp.ptr().value, pt.ptr().value
                    o["pp"], o["pt"] = pp, pt
                else:                       # column slice of a common [R][ct] copy, row block of the common [ct][R]
                    gid, co, ct = it["group"]
                    if gid not in groups:
                        groups[gid] = (self.buf(None, out=True, shape=(1, Rr, ct), dtype=torch.bfloat16),
                                       self.buf(None, out=True, shape=(1, ct, Rr), dtype=torch.bfloat16))
                    gp, gt = groups[gid]
                    t.pack_p, t.pack_t = gp.ptr().value + 2 * co, gt.ptr().value + 2 * co * Rr
                    t.pack_p_ld = ct
                    o["pp"], o["pt"] = View(gp.view[:, :, co:co + cols]), View(gt.view[:, co:co + cols, :])
            for k, v in o.items():
                out["%d.%s" % (j, k)] = v
        ws = self.scratch(max(off, 8 * n))
        tab = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(self.dev)
        return tab, items, out, ws, max(off, 8 * n)

    # -- one case
    def launcher(self, c, i):
        L, hip, st = self.L, self.hip, self.hip.stream
        op = c["op"]
        P = lambda b: None if b is None else b.ptr()                # noqa: E731
        if op == "sn_fwd":
            rows, cols = c["rows"], c["cols"]
            w, u0 = self.buf(i["w"]), self.buf(i["u0"])
            o = dict(u=self.buf(None, out=True, shape=(cols,)), v=self.buf(None, out=True, shape=(rows,)),
                     sigma=self.buf(None, out=True, shape=(1,)), wn=self.buf(None, out=True, shape=(rows, cols)))
            nb = int(L.bg_spectral_norm_workspace_bytes(rows, cols))
            ws = self.scratch(nb)
            return (lambda: L.bg_spectral_norm_fwd(P(w), P(u0), P(o["u"]), P(o["v"]), P(o["sigma"]), P(o["wn"]), rows, cols,
                                                   P(ws), nb, st())), o
        if op == "sn_bwd":
            rows, cols = c["rows"], c["cols"]
            b = {k: self.buf(i[k]) for k in ("g", "wn", "u", "v", "sigma")}
            dw = self.buf(None, out=True, shape=(rows, cols))
            ws = self.scratch(16)
            return (lambda: L.bg_spectral_norm_bwd(P(b["g"]), P(b["wn"]), P(b["u"]), P(b["v"]), P(b["sigma"]), P(dw), rows,
                                                   cols, P(ws), 16, st())), {"dw": dw}
        if op == "sn_batch_fwd":
            tab, _, out, ws, nb = self.table(c, i, False)
            self.keep = tab
            return (lambda: L.bg_spectral_norm_batch_fwd(hip.ptr(tab), len(c["items"]), P(ws), nb, st())), out
        if op == "sn_batch_phase":
            return self.phase_launcher(c, i)
        if op == "sn_batch_bwd":
            tab, _, out, ws, nb = self.table(c, i, True)
            n = len(c["items"])
            words = (n + 63) // 64
            arr = ctypes.c_uint64 * words
            en, acc = W.mask_words(c, "enable"), W.mask_words(c, "accumulate")
            en = None if en is None else arr(*en)
            acc = None if acc is None else arr(*acc)
            self.keep = (tab, en, acc)
            return (lambda: L.bg_spectral_norm_batch_bwd(hip.ptr(tab), n, en, acc, P(ws), 8 * n, st())), out
        if op == "symmetrize":
            A = self.buf(i["A"])
            S = self.buf(None, out=True, shape=(c["c"], c["c"]))
            return (lambda: L.bg_symmetrize(P(A), P(S), c["c"], st())), {"S": S}
        if op in ("ortho_cosine", "ortho_identity"):
            A = self.buf(i["A"])
            loss = self.buf(None, out=True, y0=i["loss0"], shape=(1,))
            dA = self.buf(None, out=True, shape=(c["c"], c["c"])) if c["dA"] else None
            fn = L.bg_ortho_cosine_fwd_bwd if op == "ortho_cosine" else L.bg_ortho_identity_fwd_bwd
            out = {"loss": loss}
            if dA is not None:
                out["dA"] = dA
            return (lambda: fn(P(A), W.SCALE, P(loss), P(dA), c["c"], st())), out
        if op == "gemv_rows":
            w, v = self.buf(i["w"]), (self.buf(i["v"]) if i["v"] is not None else None)
            o = self.buf(None, out=True, shape=(c["rows"],))
            return (lambda: L.bg_gemv_rows(P(w), P(v), P(o), c["rows"], c["cols"], st())), {"out": o}
        if op == "lowrank_cols":
            rows, cc = c["rows"], c["c"]
            Wb_, Pb, sb = self.buf(i["W"]), self.buf(i["P"]), self.buf(i["s"])
            ab = self.buf(None, out=True, shape=(2 * cc,))
            Wb = self.buf(None, out=True, shape=(rows, cc))
            loss = self.buf(None, out=True, y0=i["loss0"], shape=(1,))
            return (lambda: L.bg_ortho_lowrank_cols(P(Wb_), P(Pb), P(sb), W.SCALE, P(ab), P(Wb), P(loss), rows, cc,
                                                    st())), {"loss": loss, "ab": ab, "Wb": Wb}
        if op == "lowrank_finish":
            rows, cc = c["rows"], c["c"]
            b = {k: self.buf(i[k]) for k in ("P", "s", "Wa", "ab")}
            dW = self.buf(None, out=True, y0=i["T"], shape=(rows, cc))
            return (lambda: L.bg_ortho_lowrank_finish(P(dW), P(b["P"]), P(b["s"]), P(b["Wa"]), P(b["ab"]), rows, cc,
                                                      st())), {"dW": dW}
        if op == "adam":
            n, al = c["n"], c["align"]
            g, lr = self.buf(i["g"], al), self.buf(i["lr"])
            o = {k: self.buf(None, al, out=True, y0=i[k], shape=(n,)) for k in ("p", "m", "v")}
            if c["ema"]:
                o["ema"] = self.buf(None, al, out=True, y0=i["ema"], shape=(n,))
            a = W.ADAM
            hp = (W.f32r(c["b1"]), a["b2"], a["eps"], W.f32r(c["decay"]), W.f32r(c["gscale"]), n)
            # (the _dev ABI carries no host step size at all: there is nothing to poison)
            self.call32 = lambda: L.bg_adam_tf_ema_step_dev(P(o["p"]), P(g), P(o["m"]), P(o["v"]), P(o.get("ema")), P(lr),
                                                            *hp, st())
            return (lambda: L.bg_adam_tf_ema_step(P(o["p"]), P(g), P(o["m"]), P(o["v"]), P(o.get("ema")), a["lr"], *hp,
                                                  st())), o
        raise KeyError(op)

    def phase_launcher(self, c, i):
        """BG_SN_ALL once for the bits to reproduce; then the case's call is BG_SN_POWER on the sub-table of the case's own
        items - which must write u, sigma and v of those items and nothing else -, the other items' sigma | u | v filled
        in from the BG_SN_ALL run (the all-gather's part), and BG_SN_NORMALIZE on the whole table."""
        L, hip, st = self.L, self.hip, self.hip.stream
        tab, items, out, ws, nb = self.table(c, i, False)
        n, own = len(c["items"]), c["own"]
        sub = (hip.BgSnItem * len(own))(*[items[j] for j in own])
        subtab = torch.frombuffer(bytearray(bytes(sub)), dtype=torch.uint8).to(self.dev)
        self.keep = (tab, subtab)
        for o in self.outs:
            o.prefill()
        torch.cuda.synchronize()
        rc = L.bg_spectral_norm_batch_phase(hip.ptr(tab), n, ws.ptr(), nb, hip.SN_ALL, st())
        torch.cuda.synchronize()
        if rc != 0:
            return (lambda: rc), out
        full = {k: o.view.clone() for k, o in out.items()}
        pre = {}

        def call():
            for k, o in out.items():
                pre[k] = o.view.clone()
            rc = L.bg_spectral_norm_batch_phase(hip.ptr(subtab), len(own), ws.ptr(), nb, hip.SN_POWER, st())
            if rc != 0:
                return rc
            torch.cuda.synchronize()
            for k, o in out.items():
                j, name = k.split(".")
                written = int(j) in own and name in ("u", "v", "sigma")
                same = torch.equal(o.view.contiguous().view(torch.uint8), pre[k].contiguous().view(torch.uint8))
                if written == same:
                    self.fail("BG_SN_POWER %s %s" % ("left unwritten" if written else "wrote", k))
                if not written and name in ("u", "v", "sigma"):
                    o.view.copy_(full[k])
            rc = L.bg_spectral_norm_batch_phase(hip.ptr(tab), n, ws.ptr(), nb, hip.SN_NORMALIZE, st())
            torch.cuda.synchronize()
            if rc == 0:
                for k, o in out.items():
                    self.exact("POWER + NORMALIZE == ALL", o.view, full[k])
            return rc
        return call, out


def _report(op, r, n, t0):
    print("\n[%s] %d cases in %.1f s" % (W.ENTRY[op], n, time.time() - t0))
    print(r.stats.table())


@pytest.mark.parametrize("op", W.OPS)
def test_entry_point_matches_float64(op):
    hip, L = _lib()
    r = WeightRunner(hip, L)
    t0 = time.time()
    todo = W.cases(op)
    left_out = 0
    for k, c in enumerate(todo):
        left_out += r.run(c, 2000 + k) or 0
        r.ins, r.outs = [], []
    _report(op, r, len(todo), t0)
    assert not r.failures, "%d failures:\n%s" % (len(r.failures), "\n".join(r.failures[:20]))
    assert left_out == 0
    assert all(row[1] <= 1.0 for row in r.stats.rows.values())


def test_rejected_calls_return_err_arg_and_launch_nothing():
    """n_items of 0 and 257 for the batch calls, a misaligned g_wnorm for bg_spectral_norm_bwd, an unknown phase, A == S
    for bg_symmetrize: BG_ERR_ARG, and no byte of any buffer involved changes."""
    hip, L = _lib()
    dev = torch.device("cuda")
    st = hip.stream
    gen = torch.Generator(device=dev).manual_seed(5)
    r = WeightRunner(hip, L)
    r.ins, r.outs = [], []
    c = W.cases("sn_batch_fwd")[0]
    i = W.make_inputs(c, dev, gen)
    tab, _, out, ws, nb = r.table(c, i, False)
    g = r.buf(None, 4, out=True, shape=(7, 33))                      # g_wnorm at +4 bytes
    wn, dw = r.buf(None, out=True, shape=(7, 33)), r.buf(None, out=True, shape=(7, 33))
    u, v, sg = r.buf(None, out=True, shape=(33,)), r.buf(None, out=True, shape=(7,)), r.buf(None, out=True, shape=(1,))
    A = r.buf(None, out=True, y0=torch.ones(5, 5, device=dev), shape=(5, 5))
    for o in r.outs:
        o.prefill()
    torch.cuda.synchronize()
    before = [o.raw.clone() for o in r.outs]
    P = lambda b: b.ptr()                                            # noqa: E731
    one = (ctypes.c_uint64 * 5)(*([2 ** 64 - 1] * 5))
    for n in (0, 257):
        assert L.bg_spectral_norm_batch_fwd(hip.ptr(tab), n, P(ws), nb, st()) == W.ERR_ARG
        assert L.bg_spectral_norm_batch_phase(hip.ptr(tab), n, P(ws), nb, hip.SN_POWER, st()) == W.ERR_ARG
        assert L.bg_spectral_norm_batch_phase(hip.ptr(tab), n, P(ws), nb, hip.SN_NORMALIZE, st()) == W.ERR_ARG
        assert L.bg_spectral_norm_batch_bwd(hip.ptr(tab), n, one, one, P(ws), nb, st()) == W.ERR_ARG
        assert b"items" in L.bg_last_error()
    assert L.bg_spectral_norm_batch_phase(hip.ptr(tab), 1, P(ws), nb, 3, st()) == W.ERR_ARG
    assert b"phase" in L.bg_last_error()
    assert L.bg_spectral_norm_batch_phase(hip.ptr(tab), 1, P(ws), nb, -1, st()) == W.ERR_ARG
    assert L.bg_spectral_norm_bwd(P(g), P(wn), P(u), P(v), P(sg), P(dw), 7, 33, P(ws), 16, st()) == W.ERR_ARG
    assert b"aligned" in L.bg_last_error()
    assert L.bg_symmetrize(P(A), P(A), 5, st()) == W.ERR_ARG
    assert b"bg_symmetrize" in L.bg_last_error()
    torch.cuda.synchronize()
    for o, b in zip(r.outs, before):
        assert torch.equal(o.raw, b)                                # a rejected call launches nothing


# ------------------------------------------------------------------------------------------
# the composed regulariser: both forms of OrthoCosineRegFn on one weight
# ------------------------------------------------------------------------------------------
def test_composed_regulariser_forms_agree_with_the_oracle():
    """functional.OrthoCosineRegFn on a [rows, c] weight with 2 * rows == c (its low-rank chain) and the dense chain of the
    same function on the same weight (its calls written out: gemm, bg_ortho_cosine_fwd_bwd, bg_symmetrize, gemm), both
    against the one float64 oracle/ref_ops.ortho_reg_loss and its autograd gradient.  One column is scaled so that its q
    lies in (0, 1e-12): the clamp on which the two forms used to disagree.  The bound is the sum of the stage bounds
    (weight_ref.composed_dense / composed_lowrank): worst case over four to eight stages, so a correct chain uses 0.2 - 0.5 %
    of it (the stage gates above are the sharp ones); the low-rank kernel that dropped the clamped column's q / 1e-12 missed
    it by a factor of 11 (loss) and 5454 (dW)."""
    from oracle import ref_ops
    hip, L = _lib()
    from biggan_tensorflow_amd import functional as Fn
    dev = torch.device("cuda")
    w = W.composed_weight(dev)
    rows, c = w.shape
    scale = W.SCALE
    w64 = w.double().cpu().requires_grad_(True)
    lref = ref_ops.ortho_reg_loss(w64, scale, "ortho_cosine")
    lref.backward()
    lref, gref = lref.detach().to(dev).reshape(1), w64.grad.to(dev)
    # the low-rank chain, as the product runs it
    wl = w.clone().requires_grad_(True)
    ll = Fn.OrthoCosineRegFn.apply(wl, scale, "ortho_cosine")
    ll.backward()
    # the dense chain, call by call
    A = torch.empty((c, c), dtype=torch.float32, device=dev)
    Fn.gemm(w, w, A, c, c, rows, c, c, c, transA=True)
    ld = torch.zeros(1, dtype=torch.float32, device=dev)
    dA, S, gd = torch.empty_like(A), torch.empty_like(A), torch.empty_like(w)
    hip.check(L.bg_ortho_cosine_fwd_bwd(hip.f32(A), scale, hip.f32(ld), hip.f32(dA), c, hip.stream()))
    hip.check(L.bg_symmetrize(hip.f32(dA), hip.f32(S), c, hip.stream()))
    Fn.gemm(w, S, gd, rows, c, c, c, c, c)
    torch.cuda.synchronize()
    stats = R.GateStats()
    bad = []
    for form, loss, grad, b in (("dense", ld, gd, W.composed_dense(w, scale)),
                                ("low-rank", ll.detach().reshape(1), wl.grad, W.composed_lowrank(w, scale))):
        for what, got, ref, Eb in (("loss", loss, lref, b["Eloss"]), ("dW", grad, gref, b["EdW"])):
            ok, ratio, _, _, nbad = R.gate(got, ref, Eb)
            key = "OrthoCosineRegFn %dx%d %s %s" % (rows, c, form, what)
            stats.launch(key)
            stats.add(key, ratio)
            if not ok:
                bad.append((key, nbad, ratio))
    print("\n" + stats.table())
    assert not bad, bad
    assert all(row[1] <= 1.0 for row in stats.rows.values())
