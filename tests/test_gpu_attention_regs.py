"""bf16 fused attention (csrc/attention16.hip) after the move of its MFMA accumulators into VGPRs:

  delta        the lane-group delta kernel (8-byte loads, rows that are 8- but not 16-byte aligned) against float64
  large logits q, k scaled by 3 (|logit| up to 85 / 120, lse 16 .. 107): forward and both backward calls stay finite and
               within tolerance where exp(S - lse) has a large S and a large lse
  repeat       two runs of the same call are bit-identical (no atomics, fixed-order reductions)

The main yardstick of these kernels stays tests/test_gpu_bf16.py::test_attention16_fwd_bwd_on_column_slices."""
import functools

import pytest
import torch

from tests.common import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(2, 256, 128, 12, 48), (2, 256, 128, 24, 96)]        # the discriminator's and the generator's <DQT, DVT>


def f64(t):
    return t.detach().double().cpu().numpy()


def _lib():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import hip
    return hip, hip.lib()


def _inputs(B, N, Nk, d, dv, scale):
    g = torch.Generator(device="cuda").manual_seed(B + N + d + dv)
    q = (torch.randn(B, N, d, device="cuda", generator=g) * 0.7 * scale).bfloat16()
    k = (torch.randn(B, Nk, d, device="cuda", generator=g) * 0.7 * scale).bfloat16()
    v = (torch.randn(B, Nk, dv, device="cuda", generator=g) * 0.7).bfloat16()
    do = torch.randn(B, N, dv, device="cuda", generator=g).bfloat16()
    return q, k, v, do


def _run(q, k, v, do, pad=0):
    """Forward, the dk / dv call and the dq call.  o and dO live in rows of dv + pad elements."""
    hip, L = _lib()
    from biggan_tensorflow_amd.hip import act, f32, stream, check
    (B, N, d), Nk, dv = q.shape, k.shape[1], v.shape[2]
    assert L.bg_attention16_supported(N, Nk, d, dv) == 1
    ld = dv + pad
    D = hip.BgAttn16Desc()
    D.B, D.N, D.Nk, D.d, D.dv = B, N, Nk, d, dv
    D.ldq, D.sq, D.ldk, D.sk, D.ldv, D.sv = d, N * d, d, Nk * d, dv, Nk * dv
    D.ldo, D.so, D.ldg, D.sg = ld, N * ld, ld, N * ld
    D.lddq, D.sdq, D.lddk, D.sdk, D.lddv, D.sdv = d, N * d, d, Nk * d, dv, Nk * dv
    o = torch.full((B, N, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    dop = torch.full((B, N, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    dop[..., :dv] = do
    lse = torch.empty(B, N, device="cuda")
    check(L.bg_attention16_fwd(D, act(q), act(k), act(v), act(o), f32(lse), stream()))
    dq, dk, dvo = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty(B, N, device="cuda")
    check(L.bg_attention16_bwd(D, act(q), act(k), act(v), act(o), act(dop), f32(lse), None, act(dk), act(dvo),
                               f32(delta), stream()))
    check(L.bg_attention16_bwd(D, act(q), act(k), act(v), act(o), act(dop), f32(lse), act(dq), None, None,
                               f32(delta), stream()))
    torch.cuda.synchronize()
    return {"o": o[..., :dv], "lse": lse, "dq": dq, "dk": dk, "dv": dvo, "delta": delta}


@functools.lru_cache(maxsize=None)
def _large_logit_case(shape):
    """(inputs, outputs of one run) of a SHAPES entry with q and k scaled by 3; shared and left unchanged."""
    inp = _inputs(*shape, scale=3.0)
    return inp, _run(*inp)


@pytest.mark.parametrize("dv,pad", [(8, 4), (48, 4), (96, 4), (100, 4), (256, 4), (48, 0)])
def test_attention16_delta(dv, pad):
    """delta_ws of the dk / dv call against sum(dO * O) in float64 on the same bf16 O and dO, with O / dO rows of
    dv + 4 elements (8-byte, not 16-byte aligned) and one contiguous case.  Bound 1e-6 relative L2: fp32 sums of these
    products in two different orders sit at 1e-8 .. 1e-7 from float64 for dv up to 256; ten times the worst."""
    q, k, v, do = _inputs(2, 128, 128, 12, dv, 1.0)
    r = _run(q, k, v, do, pad)
    ref = (f64(do) * f64(r["o"])).sum(-1)
    e = rel_err(f64(r["delta"]), ref)
    print("delta dv=%d ld=%d: rel L2 %.3e" % (dv, dv + pad, e))
    assert e < 1e-6, e


@pytest.mark.parametrize("shape", SHAPES)
def test_attention16_large_logits(shape):
    """q and k scaled by 3: finite outputs within the tolerances of test_attention16_fwd_bwd_on_column_slices against
    float64 (1e-2 forward, 2e-2 gradients, 1e-5 lse)."""
    (q, k, v, do), r = _large_logit_case(shape)
    qd, kd, vd = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    s_ = qd @ kd.transpose(1, 2)
    lse_ref = torch.logsumexp(s_, dim=-1).detach()
    ref = torch.softmax(s_, dim=-1) @ vd
    ref.backward(do.double().cpu())
    for name, t in r.items():
        assert bool(torch.isfinite(t.float()).all()), name
    e = {"o": rel_err(f64(r["o"]), ref.detach().numpy()), "lse": rel_err(f64(r["lse"]), lse_ref.numpy()),
         "dq": rel_err(f64(r["dq"]), qd.grad.numpy()), "dk": rel_err(f64(r["dk"]), kd.grad.numpy()),
         "dv": rel_err(f64(r["dv"]), vd.grad.numpy())}
    print("large logits %s: max |logit| %.1f, lse in [%.1f, %.1f], errors %s"
          % (shape, float(s_.detach().abs().max()), float(lse_ref.min()), float(lse_ref.max()),
             ", ".join("%s %.2e" % kv for kv in e.items())))
    assert e["o"] < 1e-2, e
    assert e["lse"] < 1e-5, e
    assert e["dq"] < 2e-2 and e["dk"] < 2e-2 and e["dv"] < 2e-2, e


@pytest.mark.parametrize("shape", SHAPES)
def test_attention16_repeat_is_bit_identical(shape):
    """A second run of the same forward + backward gives the same bits in every output."""
    inp, first = _large_logit_case(shape)
    second = _run(*inp)
    for name, t in first.items():
        assert torch.equal(t, second[name]), name
