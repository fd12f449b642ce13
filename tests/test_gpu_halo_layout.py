"""LDS layout and step loop of the halo-tile kernel (csrc/igemm16.hip nn16h_kernel) against the tap kernel
(BG_NN16_HALO=0), EXACTLY.

The halo tile and the weight tiles are sized in 1 KB wave-instructions: the waves beyond a tile's last round skip that
LDS-DMA instruction, the weight slots follow the halo tile at 41 KB / 37 KB instead of 48 KB / 40 KB, and the step loop
walks (chunk, tap) cursors over two slots with compile-time offsets.  A skipped round that was needed, a tile at the
wrong offset, a stale or early-read weight or halo tile all show as wrong elements - and on small-integer operands every
product and every partial sum is exact in bf16 / fp32 (|sum| <= 2 * 9 * 384 < 2^24), so both kernels must store the same
bits whatever their accumulation order: torch.equal, no tolerance.

Shapes are the smallest that reach every branch: 2 images, 16^2 maps (one patch per image) and 32^2 (four);
Cin 32 / 64 (one chunk), 96 / 160 (a 32-channel tail), 192 (three chunks); Cout 8 (NF = 1: waves 4 - 7 issue no weight
DMA), 40 (NF = 2), 96 (NF = 3: waves 4 - 7 issue one instruction, waves 0 - 3 two), 104 (ragged last tile), 128 (NF = 4),
384 (three NF = 4 tiles).  The input gradients swap the roles (their columns are Cin: 32 -> NF 1, 64 -> 2,
96 / 192 -> 3, 160 -> five NF = 1 tiles; their reduction is Cout, and only 96, 128 and 384 take the halo form)."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CIN = (32, 64, 96, 160, 192)
COUT = (8, 40, 96, 104, 128, 384)
KINDS = ("conv_reflect", "conv_zero", "deconv3", "deconv4")
HALO, TAP = {}, {"BG_NN16_HALO": "0"}
SWITCHES = ("BG_NN16_HALO", "BG_NN16_HALO_K3S2", "BG_THIN_D2S")


@contextlib.contextmanager
def _env(**kv):
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(kv)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture
def bf16():
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    Fn.set_precision("bf16")
    yield Fn
    Fn.set_precision("fp32")


def _ints(g, lo, hi, *shape, keep=1.0):
    t = torch.randint(lo, hi + 1, shape, device="cuda", generator=g).float()
    if keep < 1.0:
        t = t * (torch.rand(*shape, device="cuda", generator=g) < keep)
    return t


def _operands(kind, N, H, Cin, Cout, seed, stride=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = 4 if kind == "deconv4" else 3
    Ho = H // stride if stride else (2 * H if kind == "deconv4" else H)
    x = _ints(g, -2, 2, N, H, H, Cin).bfloat16()
    w = _ints(g, -1, 1, *((k, k, Cin, Cout) if kind.startswith("conv") else (k, k, Cout, Cin)))
    dy = _ints(g, -1, 1, N, Ho, Ho, Cout, keep=0.25).bfloat16()
    return x, w, dy


def _launch(Fn, kind, x, w, dy, acc=None, box=None, stride=None):
    from biggan_tensorflow_amd import hip
    xc = x.clone().requires_grad_(True)
    H = x.shape[1]
    if kind.startswith("conv"):
        s = stride or 1
        mode = hip.PAD_REFLECT if kind == "conv_reflect" else hip.PAD_ZERO
        y = Fn.Conv2dFn.apply(xc, w, None, s, 1, H // s, H // s, mode, None, None if acc is None else acc.clone())
    else:
        s = 2 if kind == "deconv4" else 1
        y = Fn.Deconv2dFn.apply(xc, w, None, s, 1, None if acc is None else acc.clone(), box)
    y.backward(dy)
    return y.detach(), xc.grad.detach()


def _compare(Fn, kind, x, w, dy, halo=HALO, tap=TAP, **kw):
    with _env(**halo):
        a = _launch(Fn, kind, x, w, dy, **kw)
    if kw.get("box") is not None:
        kw = dict(kw, box=[None])                       # (the tap kernel has no fused statistics)
    with _env(**tap):
        b = _launch(Fn, kind, x, w, dy, **kw)
    for i, what in enumerate(("forward", "input gradient")):
        assert float(b[i].float().abs().max()) > 0, what
        bad = (a[i] != b[i]).nonzero()
        assert bad.numel() == 0, (what, int(bad.shape[0]), bad[:4].tolist())
    return a


@pytest.mark.parametrize("Cout", COUT)
@pytest.mark.parametrize("Cin", CIN)
@pytest.mark.parametrize("kind", KINDS)
def test_halo_form_is_exact_on_one_patch(bf16, kind, Cin, Cout):
    """16^2 maps: every (Cin, Cout) pair of the module docstring in the four window kinds - 3 x 3 stride-1 convolution with
    reflect and with zero padding, 3 x 3 stride-1 transposed convolution, 4 x 4 stride-2 transposed convolution (its four
    phases: the 2 x 2-window form, four steps between halo reloads)."""
    x, w, dy = _operands(kind, 2, 16, Cin, Cout, 1000 * KINDS.index(kind) + Cin + Cout)
    _compare(bf16, kind, x, w, dy)


@pytest.mark.parametrize("kind,Cin,Cout", [("conv_reflect", 96, 96), ("conv_zero", 192, 384), ("conv_reflect", 160, 104),
                                           ("deconv3", 192, 96), ("deconv3", 96, 384), ("deconv3", 64, 8),
                                           ("deconv4", 192, 96), ("deconv4", 160, 40), ("deconv4", 96, 128)])
def test_halo_form_is_exact_on_four_patches(bf16, kind, Cin, Cout):
    """32^2 maps: four patches per image, so that blocks of different patches, column tiles and phases share a CU."""
    x, w, dy = _operands(kind, 2, 32, Cin, Cout, 7 + Cin + Cout)
    _compare(bf16, kind, x, w, dy)


@pytest.mark.parametrize("kind", ("conv_reflect", "conv_zero"))
def test_halo_form_is_exact_on_the_stride_two_phases(bf16, kind):
    """Input gradient of a 3 x 3 stride-2 convolution 64 -> 64 through the halo form of its stride phases
    (BG_NN16_HALO_K3S2=1): windows of 1, 2, 2 and 4 taps over ONE chunk, i.e. 1, 2, 2 and 4 steps - a loop that ends in its
    first slot, and a block whose only weight tile is the prologue's."""
    x, w, dy = _operands(kind, 2, 32, 64, 64, 5, stride=2)
    _compare(bf16, kind, x, w, dy, halo={"BG_NN16_HALO_K3S2": "1"}, stride=2)


@pytest.mark.parametrize("Cout", (64, 96))
def test_depth_to_space_form_is_exact(bf16, Cout):
    """Input gradient of the discriminator's 8-channel image layer (3 x 3 stride 2): the depth-to-space form (THIN = 1,
    NF = 1, a 2 x 2 window) over one chunk and over a chunk with a 32-channel tail, against the generic stride phases of
    the tap kernel."""
    x, w, dy = _operands("conv_reflect", 2, 32, 8, Cout, 9 + Cout, stride=2)
    _compare(bf16, "conv_reflect", x, w, dy, tap={"BG_THIN_D2S": "0", "BG_NN16_HALO": "0"}, stride=2)


@pytest.mark.parametrize("kind,Cin,Cout", [("deconv4", 96, 96), ("conv_reflect", 192, 96)])
def test_halo_form_is_exact_with_accumulate(bf16, kind, Cin, Cout):
    """The residual sum fused into the epilogue (out += conv(x)): its staging tile overlays halo tile and weight slots."""
    x, w, dy = _operands(kind, 2, 16, Cin, Cout, 77)
    acc = _ints(torch.Generator(device="cuda").manual_seed(3), -3, 3, *dy.shape).bfloat16()
    _compare(bf16, kind, x, w, dy, acc=acc)


@pytest.mark.parametrize("k,Cin,Cout", [(4, 96, 96), (3, 160, 40)])
def test_fused_statistics_are_exact(bf16, k, Cin, Cout):
    """Batch-norm sums of the stored output, reduced in the epilogue over the same LDS: integers, so the float64 sums of the
    stored tensor are met exactly; the output itself equals the tap kernel's."""
    kind = "deconv4" if k == 4 else "deconv3"
    x, w, dy = _operands(kind, 2, 16, Cin, Cout, 123)
    box = [None]
    y, _ = _compare(bf16, kind, x, w, dy, box=box)
    assert box[0] is not None and box[0].numel() == 2 * Cout
    yd = y.double().reshape(-1, Cout)
    assert float((yd * yd).sum(0).max()) < 2 ** 24              # (every fp32 partial sum of the epilogue is exact)
    assert torch.equal(box[0].double(), torch.cat([yd.sum(0), (yd * yd).sum(0)]))
