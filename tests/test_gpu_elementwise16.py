"""The bf16-resident elementwise and reduction kernels ("_t" entry points of csrc/elementwise.hip) against float64.

Every row of the case table of tests/elementwise_ref.py - the batch-norm, PReLU, residual-add, max-pool and bias-gradient
shapes of BASELINE config 3 at batch 256, and small shapes for each dispatch fallback - calls its entry point through
``hip.lib()`` on guarded buffers (launch_replay.Buf): outputs prefilled with NaN (or their initial value where the call
accumulates or aliases), two runs that must agree bit for bit, guard bands before and after every buffer, inputs left
unchanged, and the per-element gate of launch_replay against the float64 reference with a bound counted from the
formula's fp32 roundings.  One GateStats table per entry point records how much of each bound is used.

The fp32-only entry points of the family ("bg_X" next to "bg_X_t") forward to the "_t" ones: every fp32 / fp32 row without
dx_add then also calls the fp32 entry on the same buffers, and its outputs must equal the gated ones bit for bit."""
import ctypes
import time

import pytest
import torch

from tests import elementwise_ref as E
from tests import launch_replay as R

pytestmark = pytest.mark.gpu

BIG = 1 << 22          # elements from which a case's buffers are released before the next one


def _lib():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import hip
    return hip, hip.lib()


class Runner:
    """Runs the cases of one entry point; ``gate`` / ``exact`` / ``fail`` are the callbacks of ``ref.check``.  ``ref`` is the
    module with the case table's make_inputs / check / describe (tests/test_gpu_weight_kernels.py runs the same rules over
    tests/weight_ref.py); a case may name outputs that are ``exempt`` from the two-runs-equal-bits rule - those are gated
    after both runs instead."""
    ref = E
    alt_label = "fp32 entry"

    def __init__(self, hip, L):
        self.hip, self.L = hip, L
        self.dev = torch.device("cuda")
        self.stats = R.GateStats()
        self.failures = []
        self.key = self.case = None

    # -- buffers
    def inb(self, t, align=0):
        """A guarded copy of input tensor t (None -> None); only bf16 tensors are ever misaligned."""
        if t is None:
            return None
        b = R.Buf(t.numel(), t.dtype, self.dev, align if t.dtype == torch.bfloat16 else 0, shape=tuple(t.shape))
        b.view.copy_(t)
        b.src = t
        self.ins.append(b)
        return b

    def outb(self, shape, dtype, align=0, y0=None):
        n = 1
        for s in shape:
            n *= s
        b = R.Buf(n, dtype, self.dev, align if dtype == torch.bfloat16 else 0, shape=tuple(shape))
        b.y0 = y0
        self.outs.append(b)
        return b

    # -- callbacks
    def gate(self, label, got, ref, Eb):
        ok, ratio, above, below, nbad = R.gate(got, ref, Eb)
        self.stats.add(self.key, ratio, above, below)
        if not ok:
            g = got.double()
            if got.dtype == torch.bfloat16:
                lo, hi = (ref - Eb).to(got.dtype).double(), (ref + Eb).to(got.dtype).double()
            else:
                lo, hi = ref - Eb - R.U32 * ref.abs(), ref + Eb + R.U32 * ref.abs()
            bad = ~((g >= lo) & (g <= hi))
            where = [tuple(int(v) for v in ix) for ix in bad.nonzero()[:3].tolist()]
            detail = "; ".join("at %s got %.9g ref %.9g E %.3g" % (ix, g[ix].item(), ref[ix].item(), Eb[ix].item())
                               for ix in where)
            self.failures.append("%s %s: %d of %d elements outside the bound (%s)"
                                 % (self.ref.describe(self.case), label, nbad, got.numel(), detail))

    def exact(self, label, got, want):
        want = want.to(got.dtype)
        same = torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))
        self.stats.add(self.key, 0.0 if same else float("inf"))
        if not same:
            self.failures.append("%s %s: %d of %d elements differ from the exact result"
                                 % (self.ref.describe(self.case), label, int((got != want).sum()), got.numel()))

    def fail(self, msg):
        self.stats.add(self.key, float("inf"))
        self.failures.append("%s: %s" % (self.ref.describe(self.case), msg))

    def key_of(self, c):
        kind = "+8B" if c["align"] else ("edge" if c["small"] else "production")
        return "%-13s %s/%s %s" % (c["op"], "fb"[c["xdt"]], "fb"[c["ydt"]], kind)

    def wants_alt(self, c):
        """Whether the second entry point (``call32``) runs on the same buffers and must reproduce the gated bits."""
        return c["op"] in E.FP32_ENTRY and c["xdt"] == c["ydt"] == E.F32 and c["add"] in ("none", "null-dx")

    # -- one case
    def launcher(self, c, i):
        """-> (run(), {name: output Buf}) for case c on inputs i."""
        L, P = self.L, (lambda b: None if b is None else b.ptr())
        op, N, HW, C, al = c["op"], c["N"], c["HW"], c["C"], c["align"]
        xdt, ydt = E.tdt(c["xdt"]), E.tdt(c["ydt"])
        st = self.hip.stream
        b = {k: self.inb(v, al) for k, v in i.items() if torch.is_tensor(v) and k not in ("sums0", "dalpha0", "out0")}
        g = b.get
        if op == "bn_stats":
            o = self.outb((2 * C,), torch.float64, y0=i["sums0"])
            self.call32 = lambda: L.bg_bn_stats(P(b["x"]), o.ptr(), N * HW, C, st())
            return (lambda: L.bg_bn_stats_t(P(b["x"]), c["xdt"], o.ptr(), N * HW, C, st())), {"sums": o}
        if op == "bn_fwd":
            o = self.outb((N, HW, C), ydt, al)
            self.call32 = lambda: L.bg_bn_apply_act_fwd(P(b["x"]), P(b["mean"]), P(b["rstd"]), P(b["gamma"]), P(b["beta"]),
                                                        c["per_sample"], P(g("alpha")), o.ptr(), N, HW, C, st())
            return (lambda: L.bg_bn_apply_act_fwd_t(P(b["x"]), c["xdt"], P(b["mean"]), P(b["rstd"]), P(b["gamma"]),
                                                    P(b["beta"]), c["per_sample"], P(g("alpha")), o.ptr(), c["ydt"], N,
                                                    HW, C, st())), {"y": o}
        if op == "bn_bwd_reduce":
            o = self.outb((3, N, C), torch.float32)
            self.call32 = lambda: L.bg_bn_apply_act_bwd_reduce(P(b["x"]), P(b["dy"]), P(b["mean"]), P(b["rstd"]),
                                                               P(b["gamma"]), P(b["beta"]), c["per_sample"], P(g("alpha")),
                                                               o.ptr(), N, HW, C, st())
            return (lambda: L.bg_bn_apply_act_bwd_reduce_t(P(b["x"]), c["xdt"], P(b["dy"]), c["ydt"], P(b["mean"]),
                                                           P(b["rstd"]), P(b["gamma"]), P(b["beta"]), c["per_sample"],
                                                           P(g("alpha")), o.ptr(), N, HW, C, st())), {"part": o}
        if op in ("bn_bwd_dx", "prelu_bwd"):
            alias = c["add"] == "alias"
            if alias:                       # dx_add is dx itself: the output starts as the other branch's gradient
                self.ins.remove(b["add"])
            o = None
            if c["add"] != "null-dx":
                o = self.outb((N, HW, C), xdt, al, y0=i["add"] if alias else None)
            addp = (lambda: o.ptr()) if alias else (lambda: P(g("add")))
            if op == "bn_bwd_dx":
                self.call32 = lambda: L.bg_bn_apply_act_bwd_dx(P(b["x"]), P(b["dy"]), P(b["mean"]), P(b["rstd"]),
                                                               P(b["gamma"]), P(b["beta"]), c["per_sample"], P(g("alpha")),
                                                               P(b["cm"]), o.ptr(), N, HW, C, st())
                return (lambda: L.bg_bn_apply_act_bwd_dx_t(P(b["x"]), c["xdt"], P(b["dy"]), c["ydt"], P(b["mean"]),
                                                           P(b["rstd"]), P(b["gamma"]), P(b["beta"]), c["per_sample"],
                                                           P(g("alpha")), P(b["cm"]), o.ptr(), addp(), N, HW, C,
                                                           st())), {"dx": o}
            da = self.outb((C,), torch.float32, y0=i["dalpha0"]) if c["dalpha"] else None
            outs = {k: v for k, v in (("dx", o), ("dalpha", da)) if v is not None}
            self.call32 = lambda: L.bg_prelu_bwd(P(b["x"]), P(b["dy"]), P(b["alpha"]), P(o), P(da), N * HW, C, st())
            return (lambda: L.bg_prelu_bwd_t(P(b["x"]), c["xdt"], P(b["dy"]), c["ydt"], P(b["alpha"]), P(o), P(da),
                                             addp() if o is not None else None, N * HW, C, st())), outs
        if op == "prelu_fwd":
            o = self.outb((N, HW, C), ydt, al)
            self.call32 = lambda: L.bg_prelu_fwd(P(b["x"]), P(b["alpha"]), o.ptr(), N * HW, C, st())
            return (lambda: L.bg_prelu_fwd_t(P(b["x"]), c["xdt"], P(b["alpha"]), o.ptr(), c["ydt"], N * HW, C,
                                             st())), {"y": o}
        if op == "bias_grad":
            o = self.outb((C,), torch.float32)
            self.call32 = lambda: L.bg_bias_grad(P(b["x"]), o.ptr(), N * HW, C, st())
            return (lambda: L.bg_bias_grad_t(P(b["x"]), c["xdt"], o.ptr(), N * HW, C, st())), {"db": o}
        if op == "maxpool_fwd":
            o = self.outb((N, c["H"] // 2, c["W"] // 2, C), xdt, al)
            self.call32 = lambda: L.bg_maxpool2_fwd(P(b["x"]), o.ptr(), N, c["H"], c["W"], C, st())
            return (lambda: L.bg_maxpool2_fwd_t(P(b["x"]), o.ptr(), c["xdt"], N, c["H"], c["W"], C, st())), {"y": o}
        if op == "maxpool_bwd":
            o = self.outb((N, c["H"], c["W"], C), xdt, al)
            self.call32 = lambda: L.bg_maxpool2_bwd(P(b["x"]), P(b["dy"]), o.ptr(), N, c["H"], c["W"], C, st())
            return (lambda: L.bg_maxpool2_bwd_t(P(b["x"]), P(b["dy"]), o.ptr(), c["xdt"], N, c["H"], c["W"], C,
                                                st())), {"dx": o}
        if op == "sum_pool_fwd":
            o = self.outb((N, C), torch.float32)
            self.call32 = lambda: L.bg_sum_pool_fwd(P(b["x"]), o.ptr(), N, HW, C, st())
            return (lambda: L.bg_sum_pool_fwd_t(P(b["x"]), c["xdt"], o.ptr(), N, HW, C, st())), {"y": o}
        if op == "sum_pool_bwd":
            o = self.outb((N, HW, C), xdt, al)
            self.call32 = lambda: L.bg_sum_pool_bwd(P(b["dy"]), o.ptr(), N, HW, C, st())
            return (lambda: L.bg_sum_pool_bwd_t(P(b["dy"]), o.ptr(), c["xdt"], N, HW, C, st())), {"dx": o}
        if op == "lincomb":
            o = self.outb((c["n"],), xdt, al)
            s = float(i["s"])
            if c["sa_dev"]:                 # the device scalar counts; the host one is poison
                return (lambda: L.bg_lincomb_t(P(b["a"]), P(b["s"]), E.POISON, P(g("b")), i["sb"], o.ptr(), c["xdt"],
                                               c["n"], st())), {"y": o}
            return (lambda: L.bg_lincomb_t(P(b["a"]), None, s, P(g("b")), i["sb"], o.ptr(), c["xdt"], c["n"],
                                           st())), {"y": o}
        if op == "dot":
            o = self.outb((1,), torch.float32, y0=i["out0"])
            self.call32 = lambda: L.bg_dot(P(b["a"]), P(b["b"]), o.ptr(), c["n"], st())
            if c["n"] % 4:                  # bg_dot_t refuses these (test_bad_arguments_are_rejected): bg_dot is gated
                return self.call32, {"out": o}
            return (lambda: L.bg_dot_t(P(b["a"]), P(b["b"]), c["xdt"], o.ptr(), c["n"], st())), {"out": o}
        if op == "cast":
            o = self.outb((c["n"],), ydt)
            return (lambda: L.bg_cast(P(b["x"]), c["xdt"], o.ptr(), c["ydt"], c["n"], st())), {"y": o}
        raise KeyError(op)

    def run(self, c, seed):
        self.case = c
        self.key = self.key_of(c)
        self.ins, self.outs = [], []
        gen = torch.Generator(device=self.dev).manual_seed(seed)
        i = self.ref.make_inputs(c, self.dev, gen)
        self.call32 = None
        call, out = self.launcher(c, i)
        if not self.wants_alt(c):
            self.call32 = None
        exempt = [out[k] for k in c.get("exempt", ())]
        self.stats.launch(self.key)
        first = None
        for rep in range(2):
            for o in self.outs:
                o.prefill()
            torch.cuda.synchronize()
            rc = call()
            torch.cuda.synchronize()
            if rc != 0:
                self.failures.append("%s: return code %d (%s)" % (self.ref.describe(c), rc,
                                                                  self.L.bg_last_error().decode()))
                return
            if rep == 0:
                first = [o.raw.clone() for o in self.outs]
                snap = {k + " (first run)": out[k].view.clone() for k in c.get("exempt", ())}
        if not all(torch.equal(o.raw, f) for o, f in zip(self.outs, first)
                   if o.dtype != torch.uint8 and not any(o is x for x in exempt)):      # (scratch: guard bands only)
            self.failures.append("%s: two runs differ (not bit-reproducible)" % self.ref.describe(c))
        del first
        for bf in self.ins + self.outs:
            if not bf.guards_ok():
                self.failures.append("%s: wrote outside a buffer of %d elements (guard band)"
                                     % (self.ref.describe(c), bf.numel))
        for bf in self.ins:
            if not torch.equal(bf.view.view(torch.uint8), bf.src.view(torch.uint8)):
                self.failures.append("%s: an input buffer was modified" % self.ref.describe(c))
        res = {k: o.view for k, o in out.items()}
        res.update(snap)
        namb, nout = self.ref.check(c, i, res, self)
        if namb > self.ref.AMBIGUITY_CAP * nout:
            self.failures.append("%s: %d of %d elements are sign-ambiguous (cap %g)" % (self.ref.describe(c), namb, nout,
                                                                                        self.ref.AMBIGUITY_CAP))
        if self.call32 is not None and self.call32 is not call:
            want = [o.view.clone() for o in out.values()]
            for o in self.outs:
                o.prefill()
            torch.cuda.synchronize()
            rc = self.call32()
            torch.cuda.synchronize()
            if rc != 0:
                self.failures.append("%s: %s: return code %d (%s)" % (self.ref.describe(c), self.alt_label, rc,
                                                                      self.L.bg_last_error().decode()))
                return namb
            for (k, o), w in zip(out.items(), want):
                self.exact(self.alt_label + " " + k, o.view, w)
            if not all(bf.guards_ok() for bf in self.ins + self.outs):
                self.failures.append("%s: %s wrote outside a buffer (guard band)" % (self.ref.describe(c), self.alt_label))
        return namb


@pytest.mark.parametrize("op", E.OPS)
def test_entry_point_matches_float64(op):
    hip, L = _lib()
    r = Runner(hip, L)
    t0 = time.time()
    namb = 0
    todo = E.cases(op)
    for k, c in enumerate(todo):
        namb += r.run(c, 1000 + k) or 0
        if E.numel(c) >= BIG:
            r.ins, r.outs = [], []
            torch.cuda.empty_cache()
    print("\n[%s] %d cases (%d production shapes) in %.1f s, %d sign-ambiguous elements"
          % (op, len(todo), sum(not c["small"] for c in todo), time.time() - t0, namb))
    print(r.stats.table())
    assert not r.failures, "%d failures:\n%s" % (len(r.failures), "\n".join(r.failures[:20]))
    assert all(row[1] <= 1.0 for row in r.stats.rows.values())


def test_bad_arguments_are_rejected():
    """BG_ERR_ARG of this family beyond test_abi_rejects_bad_arguments_with_error_codes: odd H of the max pool,
    n % 4 != 0 of bg_lincomb_t / bg_dot_t, a dtype code that is neither BG_F32 nor BG_BF16."""
    hip, L = _lib()
    ERR_ARG = 1
    x = torch.zeros(4096, device="cuda", dtype=torch.bfloat16)
    y = torch.full((4096,), 3.0, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())                # noqa: E731
    st = hip.stream
    assert L.bg_maxpool2_fwd_t(P(x), P(y), E.BF16, 2, 3, 4, 8, st()) == ERR_ARG
    assert L.bg_maxpool2_bwd_t(P(x), P(x), P(y), E.BF16, 2, 3, 4, 8, st()) == ERR_ARG
    assert L.bg_maxpool2_fwd_t(P(x), P(y), E.BF16, 2, 4, 3, 8, st()) == ERR_ARG
    assert L.bg_lincomb_t(P(x), None, 1.0, P(x), 1.0, P(y), E.BF16, 6, st()) == ERR_ARG
    assert b"bg_lincomb_t" in L.bg_last_error()
    assert L.bg_dot_t(P(x), P(x), E.BF16, P(f), 6, st()) == ERR_ARG
    assert b"bg_dot_t" in L.bg_last_error()
    bad = 7
    assert L.bg_cast(P(x), bad, P(y), E.BF16, 64, st()) == ERR_ARG
    assert L.bg_cast(P(x), E.BF16, P(y), bad, 64, st()) == ERR_ARG
    assert L.bg_bn_stats_t(P(x), bad, P(f), 8, 8, st()) == ERR_ARG
    assert L.bg_bn_apply_act_fwd_t(P(x), bad, P(f), P(f), P(f), P(f), 0, None, P(y), E.BF16, 2, 4, 8, st()) == ERR_ARG
    assert L.bg_bn_apply_act_fwd_t(P(x), E.BF16, P(f), P(f), P(f), P(f), 0, None, P(y), bad, 2, 4, 8, st()) == ERR_ARG
    assert L.bg_bn_apply_act_bwd_reduce_t(P(x), E.BF16, P(x), bad, P(f), P(f), P(f), P(f), 0, None, P(f), 2, 4, 8,
                                          st()) == ERR_ARG
    assert L.bg_bn_apply_act_bwd_dx_t(P(x), bad, P(x), E.BF16, P(f), P(f), P(f), P(f), 0, None, P(f), P(y), None, 2, 4, 8,
                                      st()) == ERR_ARG
    assert L.bg_prelu_fwd_t(P(x), E.BF16, P(f), P(y), bad, 8, 8, st()) == ERR_ARG
    assert L.bg_prelu_bwd_t(P(x), bad, P(x), E.BF16, P(f), P(y), None, None, 8, 8, st()) == ERR_ARG
    assert L.bg_bias_grad_t(P(x), bad, P(f), 8, 8, st()) == ERR_ARG
    assert L.bg_maxpool2_fwd_t(P(x), P(y), bad, 2, 4, 4, 8, st()) == ERR_ARG
    assert L.bg_sum_pool_fwd_t(P(x), bad, P(f), 2, 4, 8, st()) == ERR_ARG
    assert L.bg_sum_pool_bwd_t(P(f), P(y), bad, 2, 4, 8, st()) == ERR_ARG
    assert L.bg_lincomb_t(P(x), None, 1.0, P(x), 1.0, P(y), bad, 64, st()) == ERR_ARG
    assert L.bg_dot_t(P(x), P(x), bad, P(f), 64, st()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((f == 0).all())      # a rejected call launches nothing
