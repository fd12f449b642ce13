"""The regulariser's loss is bit-identical from launch to launch.  Its kernels (csrc/augment_loss.hip) end with one loss
term per block; added with float atomics, in arrival order, the loss of one weight took 6 to 11 different values over 300
launches (measured on one MI355X), and two training runs from one seed differed in the last bit of g_loss.  The terms now
go through per-block partials added in index order."""
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import functional as Fn

pytestmark = pytest.mark.gpu

CASES = [((3, 3, 96, 96), "ortho_cosine"),        # Gram form, 96 blocks
         ((3, 3, 192, 384), "ortho_cosine"),      # 384 blocks: more than one pass of the finalising block
         ((184, 16384), "ortho_cosine"),          # low-rank form, 64 blocks
         ((3, 3, 96, 192), "ortho"),              # identity form, 144 blocks
         ((3, 3, 8, 3), "ortho_cosine")]          # 3 blocks


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_regulariser_loss_is_the_same_on_every_launch(shape, kind):
    g = torch.Generator(device="cuda").manual_seed(3)
    w = torch.randn(*shape, device="cuda", generator=g) * 0.05
    with torch.no_grad():
        losses = torch.cat([Fn.OrthoCosineRegFn.apply(w, 1e-4, kind) for _ in range(100)]).cpu()
    assert torch.isfinite(losses).all() and float(losses[0]) > 0
    assert int(losses.view(torch.int32).unique().numel()) == 1
    # against float64 on the host: the order of the sum is fixed, its accuracy is that of an fp32 tree
    w64 = w.double().cpu().reshape(-1, shape[-1])
    a = w64.t() @ w64
    c = a.shape[0]
    if kind == "ortho":
        want = 1e-4 * 0.5 * float(((a - torch.eye(c, dtype=torch.float64)) ** 2).sum())
    else:
        ah = a / a.norm(dim=1, keepdim=True).clamp_min(1e-6)
        r = (ah.sum(dim=1, keepdim=True) - ah) / (c - 1) ** 0.5
        want = 1e-4 * 0.5 * float((r * r).sum())
    assert abs(float(losses[0]) - want) <= 1e-4 * want
