"""Every GEMM-family launch of one D op and one G op of the benchmark's workloads, replayed against float64.

tests/launch_replay.py records the unique conv / deconv / rgbconv / attention16 / attention2 / gram16 / gemm calls of the
iteration and replays each through the same entry point on bf16-exact operands; the gate bounds every output element by
its fp32 accumulation error (or brackets it between the bf16 roundings of ref -/+ that bound).  The replay's (tag, kernel
symbol) set must equal the iteration's, so the check covers exactly the production dispatch.  The generator's RGB head
(bg_rgbconv_*, rows keyed by the entry name: those launches have no profile record) and the fp32 fused attention
(bg_attention2_*, float64 reference over launch_replay.image_subset) are part of the c2@64-fp32 replay; measured on an
MI355X: 6.9 s of replay for c3@256, 2.0 s for c2@64-fp32, 19 s for the two cases with their model builds."""
import time

import pytest
import torch

from tests import launch_replay as R

pytestmark = pytest.mark.gpu


def record_iteration(gan, B, img, d_and_g=None):
    """Record one D op and one G op (apply=False) of `gan`, or whatever `d_and_g()` runs."""
    from biggan_tensorflow_amd.DiffAugment import draw
    if d_and_g is None:
        real = gan.synthetic_batch(B)
        z = gan.sample_z(B)
        dr, df = draw(B, img, generator=gan.gen, device="cuda"), draw(B, img, generator=gan.gen, device="cuda")

        def d_and_g():
            gan.d_step(real, z, dr, df, apply=False)
            gan.g_step(B, gan.sample_z(B), draw(B, img, generator=gan.gen, device="cuda"), apply=False)
    with R.Recorder() as rec:
        d_and_g()
    return rec


def replay_and_check(rec, label):
    """Replay every recorded call (the model must already be freed); print the per-kernel table; assert."""
    from biggan_tensorflow_amd import hip
    t0 = time.time()
    stats, failures, prof = R.replay_all(list(rec.calls.values()), hip.lib())
    want = R.comparable(rec.prof)
    print("\n[%s] %d unique launches replayed (%d launches in the iteration) in %.1f s; replay (tag, kernel) set %s "
          "the iteration's (%d pairs)" % (label, len(rec.calls), sum(c.count for c in rec.calls.values()),
                                           time.time() - t0, "EQUALS" if prof == want else "DIFFERS FROM", len(want)))
    print(stats.table())
    assert not failures, "\n".join(failures[:20])
    assert prof == want, (sorted(want - prof)[:10], sorted(prof - want)[:10])


def _build(img, ch, B, **kw):
    from tests.common import make_args
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import model, scope as S
    args = make_args(img_size=img, ch=ch, batch_size=B, **kw)
    return model.BigGAN(args, store=S.VariableStore("cuda", seed=42)).build_model()


@pytest.mark.parametrize("label,img,ch,B,precision", [("c3@256", 128, 96, 256, "bf16"),
                                                      ("c2@64-fp32", 128, 64, 64, "fp32")])
def test_iteration_launches_match_float64(label, img, ch, B, precision):
    """BASELINE config 3 at batch 256 (bench.py's N = 1 line: da_policy full, ortho_cosine) and config 2 at batch 64
    in fp32 (bench.py's fp32_config2)."""
    from biggan_tensorflow_amd import functional as Fn
    try:
        gan = _build(img, ch, B, precision=precision)
        rec = record_iteration(gan, B, img)
        gan = None
        torch.cuda.empty_cache()
        replay_and_check(rec, label)
    finally:
        Fn.set_precision("fp32")
        gan = None
        torch.cuda.empty_cache()
