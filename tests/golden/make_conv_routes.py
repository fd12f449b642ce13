"""Generates tests/golden/conv_route_traces.json: for every case of CASES - the smallest shapes at which each kernel route
of Conv2dFn / SubpixelConvFn / Deconv2dFn / ops.conv can be mis-chosen - the ordered list of every ``bg_*`` call made
through ``functional.lib()`` during one forward and backward (entry name, the fields of a BgConvDesc, every integer and
float argument, null / non-null for every pointer; the stream is left out), the element type and shape of every returned
tensor, and whether the result is the accumulator's own storage.

The file pins the launches of the commit it was produced at (recorded in it): tests/test_gpu_conv_routes.py replays the
table on the current code and tests/test_host.py checks ``conv_route`` against it.  It only uses ``Fn.*.apply`` and
``ops.conv``.  Run on an MI355X:

    python tests/golden/make_conv_routes.py tests/golden/conv_route_traces.json --commit <sha of the checkout>
    python tests/golden/make_conv_routes.py --bits FILE [--tree CHECKOUT]

``--bits``: instead of the traces, a SHA-256 of the bytes of y, dx, dw and db per case (inputs are seeded), for comparing
two checkouts against one built library; ``--tree`` imports the package from another checkout of this repository.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _case(mode, fn, x, cin, cout, k=3, stride=1, pad="reflect", bias=False, out=None, acc=None, acc_contig=True,
          fork=False, inputs_only=False, stats=False, env=None, hw=8):
    return dict(mode=mode, fn=fn, x=x, cin=cin, cout=cout, k=k, stride=stride, pad=pad, bias=bias, out=out, acc=acc,
                acc_contig=acc_contig, fork=fork, inputs_only=inputs_only, stats=stats, env=env or {}, hw=hw)


# N = 2, maps of ``hw`` x ``hw`` (8 unless noted).  ``acc``: element type of an accumulate_into tensor; ``out``: the out_dtype argument.
# subpixel: cout is C, the kernel has 4 C output channels (r = 2).  ops: ops.conv under a scratch variable store.
CASES = {
    "fp32/16-32-k3-bias": _case("fp32", "conv", "fp32", 16, 32, bias=True),
    "fp32/16-32-k3-bias-acc": _case("fp32", "conv", "fp32", 16, 32, bias=True, acc="fp32"),
    "fp32/16-3-k3-rgb": _case("fp32", "conv", "fp32", 16, 3),
    "fp32/16-3-k3-rgb-acc": _case("fp32", "conv", "fp32", 16, 3, acc="fp32"),
    "fp32/16-16-k1": _case("fp32", "conv", "fp32", 16, 16, k=1),
    "fp32/16-32-k4-s2-zero": _case("fp32", "conv", "fp32", 16, 32, k=4, stride=2, pad="zero"),
    "staged/64-64-k3": _case("bf16-staged", "conv", "fp32", 64, 64),
    "bf16/resident-8-8-k3-s2": _case("bf16", "conv", "bf16", 8, 8, stride=2),
    "bf16/resident-16-32-bias": _case("bf16", "conv", "bf16", 16, 32, bias=True),
    "bf16/resident-16-32-out-fp32": _case("bf16", "conv", "bf16", 16, 32, out="fp32"),
    "bf16/resident-16-32-acc": _case("bf16", "conv", "bf16", 16, 32, acc="bf16"),
    "bf16/resident-16-32-fork": _case("bf16", "conv", "bf16", 16, 32, fork=True),
    "bf16/resident-16-32-inputs-only": _case("bf16", "conv", "bf16", 16, 32, bias=True, inputs_only=True),
    "bf16/thin-in-fp32-3-16": _case("bf16", "conv", "fp32", 3, 16),
    "bf16/thin-in-bf16-3-16-s2": _case("bf16", "conv", "bf16", 3, 16, stride=2),
    "bf16/thin-in-4-16": _case("bf16", "conv", "fp32", 4, 16),
    "bf16/thin-in-1-16": _case("bf16", "conv", "fp32", 1, 16),
    "bf16/thin-out-16-3-bias": _case("bf16", "conv", "bf16", 16, 3, bias=True),
    "bf16/thin-out-16-4": _case("bf16", "conv", "bf16", 16, 4),
    "bf16/thin-out-16-1": _case("bf16", "conv", "bf16", 16, 1),
    "bf16/offgrid-20-12": _case("bf16", "conv", "bf16", 20, 12),
    "bf16/offgrid-5-16": _case("bf16", "conv", "bf16", 5, 16),
    "bf16/offgrid-8-8-k5": _case("bf16", "conv", "bf16", 8, 8, k=5),
    "bf16/offgrid-fp32-3-16-k7": _case("bf16", "conv", "fp32", 3, 16, k=7),
    "deconv/bf16-8-8-k4-s2": _case("bf16", "deconv", "bf16", 8, 8, k=4, stride=2, bias=True),
    "deconv/bf16-8-8-k4-s2-acc": _case("bf16", "deconv", "bf16", 8, 8, k=4, stride=2, acc="bf16"),
    "deconv/bf16-8-8-k4-s2-stats": _case("bf16", "deconv", "bf16", 8, 8, k=4, stride=2, stats=True),
    # (at 8 x 8 the library offers no statistics epilogue and the plain launch runs; at 16 x 16, 32 channels, it does)
    "deconv/bf16-32-32-k4-s2-stats-16x16": _case("bf16", "deconv", "bf16", 32, 32, k=4, stride=2, stats=True, hw=16),
    "deconv/bf16-8-8-k6-s2": _case("bf16", "deconv", "bf16", 8, 8, k=6, stride=2),
    "deconv/bf16-20-12-k4-s2": _case("bf16", "deconv", "bf16", 20, 12, k=4, stride=2),
    "deconv/fp32-16-16-k4-s2": _case("fp32", "deconv", "fp32", 16, 16, k=4, stride=2, bias=True),
    "subpixel/bf16-16-8": _case("bf16", "subpixel", "bf16", 16, 8, bias=True),
    "subpixel/bf16-16-4": _case("bf16", "subpixel", "bf16", 16, 4),
    "subpixel/fp32-16-8": _case("bf16", "subpixel", "fp32", 16, 8),
    "subpixel/bf16-16-8-unfused": _case("bf16", "subpixel", "bf16", 16, 8, bias=True, env={"BG_FUSE_D2S": "0"}),
    "ops/acc-wrong-dtype": _case("bf16", "ops", "bf16", 16, 32, bias=True, acc="fp32"),
    "ops/acc-non-contiguous": _case("bf16", "ops", "bf16", 16, 32, bias=True, acc="bf16", acc_contig=False),
    "ops/thin-acc": _case("bf16", "ops", "fp32", 3, 16, bias=True, acc="bf16"),
    "ops/resident-acc-fused": _case("bf16", "ops", "bf16", 16, 32, bias=True, acc="bf16"),
}
N = 2


def _addr(p):
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    return p.value or 0


def _record(hip, name, args):
    """One call as JSON: [name, args] - a BgConvDesc as a dict of its fields, a pointer as "ptr" / "null", numbers as
    they are; the trailing stream of a launch is dropped."""
    res, types = hip.SIGNATURES[name]
    if res is ctypes.c_int and types and types[-1] is ctypes.c_void_p:
        types, args = types[:-1], args[:len(types) - 1]
    out = []
    for t, v in zip(types, args):
        if isinstance(v, ctypes.Structure):
            out.append({f[0]: getattr(v, f[0]) for f in v._fields_})
        elif t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents"):
            out.append("ptr" if _addr(v) else "null")
        elif t in (ctypes.c_float, ctypes.c_double):
            out.append(float(v))
        else:
            out.append(int(v))
    return [name, out]


class _Proxy:
    def __init__(self, L, hip, calls):
        self._L, self._hip, self._calls = L, hip, calls

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("bg_"):
            return fn

        def wrapped(*a):
            self._calls.append(_record(self._hip, name, a))
            return fn(*a)
        return wrapped


class _Recording:
    """Every bg_* call made through functional.lib() / hip.lib(), looked up at call time, in order."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        from biggan_tensorflow_amd import functional as Fn, hip
        self._mods, self._saved = (Fn, hip), (Fn.lib, hip.lib)
        proxy = _Proxy(hip.lib(), hip, self.calls)
        Fn.lib = hip.lib = lambda: proxy
        return self

    def __exit__(self, *exc):
        Fn, hip = self._mods
        Fn.lib, hip.lib = self._saved
        return False


def run_case(name, c):
    """-> (calls, tensors): the recorded calls of one forward + backward and {"y", "dx", "dw", "db"} (None: not produced),
    plus tensors["acc"] = the accumulator (or None)."""
    import torch
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip, ops, scope as S
    DT = {"fp32": torch.float32, "bf16": torch.bfloat16, None: None}
    gen = torch.Generator(device="cuda").manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))

    def rnd(shape, dtype=torch.float32, scale=1.0):
        return (torch.randn(shape, generator=gen, device="cuda") * scale).to(dtype)

    cin, cout, k, s, HW = c["cin"], c["cout"], c["k"], c["stride"], c["hw"]
    saved_env = {e: os.environ.get(e) for e in c["env"]}
    os.environ.update(c["env"])
    Fn.set_precision(c["mode"])
    try:
        x = rnd((N, HW, HW, cin), DT[c["x"]]).requires_grad_(True)
        wc = 4 * cout if c["fn"] == "subpixel" else cout
        wshape = (k, k, cout, cin) if c["fn"] == "deconv" else (k, k, cin, wc)
        ws = [rnd(wshape, scale=(k * k * cin) ** -0.5).requires_grad_(True) for _ in range(2 if c["fork"] else 1)]
        bias = rnd((wc,)).requires_grad_(True) if c["bias"] else None
        lo = (k - s) // 2 if c["fn"] == "deconv" else (k - 1) // 2
        Ho = HW * s if c["fn"] == "deconv" else (HW + 2 * lo - k) // s + 1
        if c["fn"] == "subpixel":
            Ho = 2 * HW
        acc = None
        if c["acc"]:
            acc = rnd((N, Ho, Ho, cout if c["acc_contig"] else 2 * cout), DT[c["acc"]])
            acc = acc if c["acc_contig"] else acc[..., :cout]
        mode = hip.PAD_ZERO if c["pad"] == "zero" else hip.PAD_REFLECT
        ydt = DT[c["out"]]
        box = [None] if c["stats"] else None
        if c["fn"] == "ops":
            S.set_default_store(S.VariableStore("cuda", seed=11))
        with _Recording() as rec:
            if c["fn"] == "conv" and c["fork"]:
                state = Fn.ForkState()
                xs = Fn.ForkFn.apply(x, 2, state)
                for t in xs:
                    t.bg_fork = state
                ys = [Fn.Conv2dFn.apply(t, w, bias, s, lo, Ho, Ho, mode, ydt, None) for t, w in zip(xs, ws)]
            elif c["fn"] == "conv":
                ys = [Fn.Conv2dFn.apply(x, ws[0], bias, s, lo, Ho, Ho, mode, ydt, acc)]
            elif c["fn"] == "deconv":
                ys = [Fn.Deconv2dFn.apply(x, ws[0], bias, s, lo, acc, box)]
            elif c["fn"] == "subpixel":
                ys = [Fn.SubpixelConvFn.apply(x, ws[0], bias, lo, mode, 2, ydt)]
            else:
                opt = {"conv": {"sn": False, "padding_type": c["pad"]}}
                with S.variable_scope("discriminator"):
                    ys = [ops.conv(x, cout, opt, kernel=k, stride=s, pad=lo, use_bias=c["bias"], scope="c",
                                   _out_dtype=ydt, _accumulate_into=acc)]
                v = S.default_store().vars
                ws, bias = [v["discriminator/c/kernel"]], v.get("discriminator/c/bias")
            dys = [rnd(tuple(y.shape), y.dtype) for y in ys]
            if c["inputs_only"]:
                with Fn.inputs_only_backward():
                    torch.autograd.backward(ys, dys)
            else:
                torch.autograd.backward(ys, dys)
        torch.cuda.synchronize()
    finally:
        Fn.set_precision("fp32")
        S.set_default_store(None)
        for e, v in saved_env.items():
            if v is None:
                os.environ.pop(e, None)
            else:
                os.environ[e] = v
    tensors = {"y": ys[0], "dx": x.grad, "dw": ws[0].grad, "db": None if bias is None else bias.grad, "acc": acc}
    if c["fork"]:
        tensors.update(y2=ys[1], dw2=ws[1].grad)
    if box is not None:
        tensors["stats"] = box[0]
    return rec.calls, tensors


def trace(name, c):
    calls, t = run_case(name, c)
    acc = t.pop("acc")
    outs = {k: None if v is None else [str(v.dtype).replace("torch.", ""), list(v.shape)] for k, v in t.items()}
    same = acc is not None and t["y"].data_ptr() == acc.data_ptr()
    return {"case": c, "calls": calls, "outputs": outs, "y_is_accumulator": same}


def bits(name, c):
    import torch
    _, t = run_case(name, c)
    t.pop("acc")
    return {k: hashlib.sha256(v.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
            for k, v in t.items() if v is not None}


def write_traces(res, fh):
    """The traces as JSON with one call per line, so that a changed launch shows as a changed line."""
    js = lambda o: json.dumps(o, sort_keys=True)          # noqa: E731
    fh.write('{"commit": %s,\n"cases": {\n' % js(res["commit"]))
    for i, (name, t) in enumerate(sorted(res["cases"].items())):
        fh.write('%s: {"case": %s,\n "outputs": %s,\n "y_is_accumulator": %s,\n "calls": [\n' % (
            js(name), js(t["case"]), js(t["outputs"]), js(t["y_is_accumulator"])))
        fh.write(",\n".join("  " + js(c) for c in t["calls"]))
        fh.write("\n ]}%s\n" % ("," if i + 1 < len(res["cases"]) else ""))
    fh.write("}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="where conv_route_traces.json is written")
    ap.add_argument("--commit", default="", help="the commit of the checkout that is run, recorded in the file")
    ap.add_argument("--bits", default="", help="write SHA-256 digests of every case's tensors to this file instead")
    ap.add_argument("--tree", default=ROOT, help="checkout to import the package from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.bits:
        res = {name: bits(name, c) for name, c in CASES.items()}
        dst = a.bits
    else:
        if not a.out or not a.commit:
            raise SystemExit("usage: make_conv_routes.py OUT --commit SHA | --bits FILE [--tree PATH]")
        res = {"commit": a.commit, "cases": {name: trace(name, c) for name, c in CASES.items()}}
        dst = a.out
    with open(dst, "w") as fh:
        if a.bits:
            json.dump(res, fh, indent=0, sort_keys=True)
            fh.write("\n")
        else:
            write_traces(res, fh)
    print("wrote", dst, len(CASES), "cases")


if __name__ == "__main__":
    main()
