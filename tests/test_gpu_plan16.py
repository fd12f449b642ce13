"""The bf16 launch plans against what runs: one launch per kernel family of csrc/igemm16.hip.

bg_conv_plan_describe (csrc/igemm16_plan.hip, no GPU) says which instantiation a call takes and how much workspace; each
case launches the call with exactly that workspace through tests/launch_replay.py - float64 reference, derived bound,
NaN-prefilled outputs and workspace behind guard bands, two bit-identical runs - and the kernel bg_prof recorded must be
the one the plan named.  The shapes are the smallest that select each family."""
import os

import pytest

from tests import launch_replay as R

pytestmark = pytest.mark.gpu

Z, RF = R.PAD_ZERO, R.PAD_REFLECT


def _desc(N, H, Cin, Ho, Cout, k, s, lo, mode=Z):
    return (N, H, H, Cin, Ho, Ho, Cout, k, s, lo, mode, 1, R.BF16, R.BF16, 1)


TAP = _desc(2, 8, 16, 4, 32, 3, 2, 1)
CASES = [
    ("tap-image-major", "conv2d_fwd", TAP, {}, "nn16_kernel<1, 0, false>"),
    ("tap-position-major", "deconv2d_fwd", _desc(16, 4, 16, 4, 16, 3, 1, 1), {}, "nn16_kernel<1, 1, true>"),
    ("halo-nt3", "conv2d_fwd", _desc(1, 16, 32, 16, 32, 3, 1, 1), {}, "nn16h_kernel<3, 1, 0>"),
    ("halo-nt2", "deconv2d_fwd", _desc(1, 16, 32, 32, 32, 4, 2, 1), {}, "nn16h_kernel<2, 1, 1>"),
    ("wide", "conv2d_fwd", TAP, {"BG_NN16_PIPE": "2"}, "nn16_kernel<1, 0, false, false, 3, 4>"),
    ("phased", "conv2d_fwd", TAP, {"BG_NN16_PIPE": "3"}, "nn16_kernel<4, 0, false, false, 2, 4>"),
    ("ring-128", "conv2d_fwd", TAP, {"BG_NN16_PIPE": "1"}, "nn16_kernel<1, 0, false, false, 3, 2>"),
    ("thin-d2s", "conv2d_dgrad", _desc(2, 64, 8, 32, 96, 3, 2, 1), {}, "nn16h_kernel<2, 1, 0, d2s>"),
    ("mirrored-ring", "conv2d_dgrad", _desc(2, 8, 16, 8, 16, 3, 1, 1, RF), {"BG_DGRAD_RING": "1"}, None),
    ("tn16", "conv2d_wgrad", _desc(2, 8, 16, 8, 16, 1, 1, 0), {}, "tn16_kernel<0>"),
    ("tn16x", "conv2d_wgrad", _desc(2, 16, 32, 16, 32, 3, 1, 1), {}, "tn16x_kernel<0, 32>"),
    ("tn16x-phased", "conv2d_wgrad", _desc(2, 16, 32, 16, 192, 3, 1, 1), {"BG_TN16X_PHASED": "1"},
     "tn16x_phased_kernel<0, 192, 6>"),
]


@pytest.mark.parametrize("label,entry,desc,env,kernel", CASES, ids=[c[0] for c in CASES])
def test_launch_runs_the_described_plan(label, entry, desc, env, kernel):
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import hip
    L = hip.lib()
    d = hip.BgConvDesc(*desc)
    try:
        os.environ.update(env)
        plan = hip.plan_describe(d, entry)
        ws = int(plan["ws"])
        assert ws == int(getattr(L, "bg_%s_workspace_bytes" % entry)(d))
        # Handed what it asked for, the plan stands.  (Not so for the one known over-request: a launch that takes the
        # halo-tile form where the tap kernel would have split K is asked the tap kernel's slabs and uses none, so its
        # line says ws=0 once a size is given.  None of these shapes would split.)
        assert hip.plan_describe(d, entry, ws) == plan
        flags = dict(ws=ws) if entry.endswith("wgrad") else dict(alpha=False, acc=0, ws=ws)
        if entry.endswith("fwd"):
            flags["bias"] = True
        stats, failures, prof = R.replay_all([R.Call("bg_" + entry, desc, flags, (0, 0, 0))], L)
    finally:
        for k in env:
            os.environ.pop(k, None)
    print("\n[%s] %s" % (label, "; ".join("%s=%s" % kv for kv in plan.items())))
    print(stats.table())
    assert not failures, "\n".join(failures)
    assert {k for _, k in prof} == {plan["kernel"]}, (sorted(prof), plan)
    if kernel is not None:
        assert plan["kernel"] == kernel, plan
    else:                   # the mirrored-tap launch follows a plain launch and leaves that launch's name in the record
        assert plan["route"] == "BF16_RING" and plan["ring_kernel"] == "nn16_kernel<1, 1, true, true, 2>", plan
        assert plan["ring_form"] == "two" and plan["zfold"] == "0" and plan["splitk"] == "1", plan
