"""Every conv / transposed-conv / rgbconv / attention geometry the entry points accept, replayed against float64.

tests/geometry_sweep.py lists the calls (small and non-square maps, k = 1 .. 7, both strides, both splits of an odd padding,
both sides of every rung of the two attention ladders); each goes through launch_replay.replay_all exactly like a launch
recorded from a training iteration: float64 reference, the derived per-element bound of launch_replay.gate, NaN-prefilled
outputs behind guard bands, two runs that must agree bit for bit.  Every call must return BG_OK unless its geometry is in
geometry_sweep.NARROWED (one row: bf16-resident forward / input gradient with k > 4); a narrowed geometry must be rejected
by the forward entry as well, with a message.

29 cases of 64 .. 142 calls; each prints its wall time and per-kernel table.  The coverage test reads the union of the
replays' (tag, kernel symbol) sets, and the workspace queries where a form has no record of its own."""
import os
import re
import time

import pytest

from tests import geometry_sweep as G
from tests import launch_replay as R

pytestmark = pytest.mark.gpu

CASES = G.cases()
_DONE = {}


def _forward_of(c):
    """The forward call of the layer `c` belongs to (the call a training step makes first)."""
    if c.name.startswith("bg_attention"):
        return R.Call(c.name.replace("_bwd", "_fwd"), c.desc, {}, (0,) * 4)
    name = "bg_deconv2d_fwd" if "deconv" in c.name else ("bg_rgbconv_fwd" if "rgbconv" in c.name else "bg_conv2d_fwd")
    return R.Call(name, c.desc, dict(bias=False, alpha=False, acc=0, ws=0), (0, 0, 0))


def _run(case):
    """Replay one case (once per session) -> dict(stats, failures, prof, calls, rejected, seconds)."""
    if case in _DONE:
        return _DONE[case]
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import hip
    env, calls = CASES[case]
    L = hip.lib()
    t0 = time.time()
    try:
        for k, v in env.items():
            os.environ[k] = v
        calls = G.resolve(calls, L, hip.BgConvDesc)             # (workspace sizes depend on the form the variable picks)
        kept = [c for c in calls if G.narrowed(c) is None]
        rejected = [c for c in calls if G.narrowed(c) is not None]
        stats, failures, prof = R.replay_all(kept, L)
        for c in rejected:                                      # narrowed: the forward entry must say no, with a message
            r = R.Replayer(L)
            r.prof = set()
            try:
                r.replay(_forward_of(c))
                failures.append("%s %s is in NARROWED (%s) but its forward entry accepted it" % (c.name, c.desc,
                                                                                               G.narrowed(c)[0]))
            except R.Failure as e:
                assert len(str(e)) > len(c.name) + 2, "rejected without a message"
    finally:
        for k in env:
            os.environ.pop(k, None)
    out = dict(stats=stats, failures=failures, prof=prof, calls=calls, rejected=rejected, seconds=time.time() - t0)
    _DONE[case] = out
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_sweep_matches_float64(case):
    r = _run(case)
    print("\n[%s] %d calls replayed, %d narrowed, in %.1f s" % (case, len(r["calls"]) - len(r["rejected"]),
                                                               len(r["rejected"]), r["seconds"]))
    print(r["stats"].table())
    fam = [c for cid, (_, calls) in CASES.items() if G.family(cid) == G.family(case) for c in calls]
    share = sum(G.narrowed(c) is not None for c in fam) / len(fam)
    assert share <= G.MAX_REJECTED, "the %s sweep may not reject its way out (%.0f %%)" % (G.family(case), 100 * share)
    assert not r["failures"], "%d failures\n%s" % (len(r["failures"]), "\n".join(r["failures"][:40]))


def _kernels(*cases):
    return {k for c in cases for _, k in _run(c)["prof"]}


def test_sweep_covers_every_dispatch_path():
    """The sweep cannot quietly miss a path: every instantiation of both attention ladders, the fp32 mirrored-source input
    gradient, the padded-grid + fold form in both precisions, the ring form, and the three rgbconv entries."""
    a16 = sorted({G.a16_instance(d, dv) for d in G.A16_D for dv in G.A16_DV})
    assert len(a16) == 10
    for kind, sym in (("fwd", "attn16_fwd_kernel"), ("dq", "attn16_bwd_dq_kernel"), ("dkv", "attn16_bwd_dkv_kernel")):
        for Nk in (128, 256):
            got = _kernels("attention16_%s_Nk%d/bf16/-" % (kind, Nk))
            assert got == {"%s<%d, %d>" % (sym, a, b) for a, b in a16}, (kind, Nk, sorted(got))
    a2 = sorted({G.a2_instance(d, dv) for d in G.A2_D for dv in G.A2_DV})
    assert len(a2) == 8
    assert _kernels("attention2_fwd/fp32/-") == {"attn_fwd_kernel<%d, %d>" % i for i in a2}
    assert _kernels("attention2_bwd/fp32/-") == {"attn_bwd_dq_kernel + attn_bwd_dkv_kernel<%d, %d>" % i for i in a2}

    # fp32 input gradient of reflect padding: the mirrored-source kernels (template argument MIRROR = true) ...
    fp32 = _run("conv_dgrad_gemm/fp32/reflect")
    mirror = re.compile(r"nn_kernel<\d+, \d+, \d+, \d+, (true|false), \d+, true, (true|false)>")
    assert any(mirror.fullmatch(k) for _, k in fp32["prof"]), sorted(fp32["prof"])
    # ... and the padded grid + reflect_fold_kernel where a row mirrors both borders or only the high side is padded.  The
    # fold (like the ring launches) has no profile record of its own: the form shows in the workspace the call asks for
    folded = [c for c in fp32["calls"] if G.double_mirror(c.desc) or (c.desc[9] == 0 and c.desc[7] > c.desc[8])]
    plain = [c for c in fp32["calls"] if c not in folded]
    assert folded and plain
    assert all(c.flags["ws"] >= G.padded_grid_bytes(c.desc) for c in folded)
    assert any(c.flags["ws"] < G.padded_grid_bytes(c.desc) for c in plain)

    # bf16-resident: BG_DGRAD_RING=0 is the padded grid + fold everywhere, =1 the ring launches on the 3 x 3, pad 1 maps
    ring0, ring1 = _run("conv_dgrad_ring0/bf16/reflect"), _run("conv_dgrad_ring1/bf16/reflect")
    is_ring = lambda d: d[7] == 3 and d[9] == 1 and min(d[1], d[2]) >= 4                       # noqa: E731
    padded0 = [c for c in ring0["calls"] if c.desc[9] > 0 or c.desc[7] > c.desc[8]]
    assert padded0 and all(c.flags["ws"] >= G.padded_grid_bytes(c.desc) for c in padded0)
    nring = 0
    for c0, c1 in zip(ring0["calls"], ring1["calls"]):
        assert c0.desc == c1.desc
        if is_ring(c1.desc):          # whole fp32 split-K slabs of the H x W gradient (or nothing), no padded grid
            N, H, W, cin = c1.desc[:4]
            assert c1.flags["ws"] % (N * H * W * cin * 4) == 0 and c1.flags["ws"] != c0.flags["ws"], (c1.desc, c1.flags)
            nring += 1
        else:
            assert c1.flags["ws"] == c0.flags["ws"], (c1.desc, c0.flags, c1.flags)
    assert nring > 0

    for entry in ("fwd", "dgrad", "wgrad"):
        n = sum(_run("conv_%s_thin/fp32/%s" % (entry, p))["stats"].rows.get("bg_rgbconv_" + entry, [0])[0]
                for p in ("reflect", "zero"))
        assert n > 0, "no bg_rgbconv_%s launch in the sweep" % entry


@pytest.mark.parametrize("k,stride", [(5, 1), (7, 2)])
def test_wide_kernels_leave_the_resident_path(k, stride):
    """The NARROWED row is not reachable from the model: in bf16 mode functional.Conv2dFn sends a layer with more than
    4 x 4 taps to the fp32-tensor kernels (as it does a layer with an odd channel count).  Forward, input gradient and
    weight gradient against float64 autograd, EXACTLY: the operands are small integers, so every product and sum is exact."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, hip
    N, H, Cin, Cout = 2, 8, 8, 16
    rng = np.random.default_rng(k)
    x = torch.tensor(rng.integers(-2, 3, size=(N, H, H, Cin)), dtype=torch.float64, requires_grad=True)
    w = torch.tensor(rng.integers(-1, 2, size=(k, k, Cin, Cout)) * (rng.random((k, k, Cin, Cout)) < 0.3), dtype=torch.float64,
                     requires_grad=True)
    Ho = H // stride
    tot = (Ho - 1) * stride + k - H
    lo, hi = tot // 2, tot - tot // 2
    xp = F.pad(x.permute(0, 3, 1, 2), (lo, hi, lo, hi), mode="reflect")
    y = F.conv2d(xp, w.permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)
    g = torch.tensor(rng.integers(-1, 2, size=tuple(y.shape)) * (rng.random(tuple(y.shape)) < 0.25), dtype=torch.float64)
    y.backward(g)
    assert max(float(y.detach().abs().max()), float(x.grad.abs().max()), float(w.grad.abs().max())) <= 256   # exact in bf16
    Fn.set_precision("bf16")
    try:
        xc = x.detach().to("cuda", torch.bfloat16).requires_grad_(True)
        wc = w.detach().to("cuda", torch.float32).requires_grad_(True)
        yc = Fn.Conv2dFn.apply(xc, wc, None, stride, lo, Ho, Ho, hip.PAD_REFLECT)
        yc.backward(g.to("cuda", yc.dtype))
        assert torch.equal(yc.detach().double().cpu(), y.detach())
        assert torch.equal(xc.grad.double().cpu(), x.grad)
        wg = wc.grad if wc.grad is not None else wc.bg_grad
        assert torch.equal(wg.double().cpu(), w.grad)
    finally:
        Fn.set_precision("fp32")
