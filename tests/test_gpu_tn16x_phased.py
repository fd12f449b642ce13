"""The phased form of the weight-gradient kernel (csrc/igemm16.hip, tn16x_phased_kernel: a 256 x 192 or 256 x 256 tile on
8 waves at one block per CU, a ring of 16-pixel K blocks, one phase and one raw barrier per block with the younger LDS-DMA in
flight across it) takes the K partition of the 256 x 128 form and feeds every 32 x 32 accumulator the same 16-pixel MFMA K blocks
in the same order, so the weight gradients are EQUAL bit for bit to tn16x_kernel<MODE, 32>'s - at both column tiles
(BG_TN16X_PHASED=1 with BG_TN16X_PHASED_BN = 192, 256) against BG_TN16X_PHASED=0.  One case per group is also checked
against float64 on the bf16 operands (relative L2 error < 6e-3, the bound of tests/test_gpu_nn16_pipe.py).

The wide forms need Mf = taps x gathered channels > 128, M >= 512 reduction pixels and a power-of-two pixel grid: maps of
16 x 16 (8 x 8 and 8 x 4 behind a stride-2 convolution), batches of 2 ... 27."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests.common import rel_err
from tests.test_gpu_nn16_phased import _kernels_of
from tests.test_gpu_nn16_pipe import TOL64

pytestmark = pytest.mark.gpu
BNS = ("192", "256")


class _Case:
    """(kind, N, H, Cin, Cout, k, s), W=: random bf16 x and dy, fp32 w; run() is the weight gradient of
    Conv2dFn (reflect padding 1) / Deconv2dFn (padding 1) in bf16 mode."""

    def __init__(self, kind, N, H, Cin, Cout, k, s, W=None):
        self.kind, self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.s = kind, N, H, W or H, Cin, Cout, k, s
        W = self.W
        g = torch.Generator().manual_seed(N * 7919 + H * 131 + Cin * 17 + Cout * 3 + k + s)
        self.x = torch.randn((N, H, W, Cin), generator=g).to(torch.bfloat16)
        if kind == "conv":
            self.Ho, self.Wo = H // s, W // s
            self.w = torch.randn((k, k, Cin, Cout), generator=g) * 0.05
            self.Ca, self.Cb, self.M = Cin, Cout, N * self.Ho * self.Wo
        else:
            self.Ho, self.Wo = H * s, W * s
            self.w = torch.randn((k, k, Cout, Cin), generator=g) * 0.05
            self.Ca, self.Cb, self.M = Cout, Cin, N * H * W
        self.Mf = k * k * self.Ca
        self.dy = torch.randn((N, self.Ho, self.Wo, Cout), generator=g).to(torch.bfloat16)
        self.xc, self.dyc, self.wc = self.x.cuda(), self.dy.cuda(), self.w.cuda()

    def run(self):
        from biggan_tensorflow_amd import functional as Fn, hip
        w = self.wc.clone().requires_grad_(True)
        if self.kind == "conv":
            y = Fn.Conv2dFn.apply(self.xc, w, None, self.s, 1, self.Ho, self.Wo, hip.PAD_REFLECT)
        else:
            y = Fn.Deconv2dFn.apply(self.xc, w, None, self.s, 1, None)
        y.backward(self.dyc)
        torch.cuda.synchronize()
        return w.grad.detach().clone()

    def reference(self):
        """float64 weight gradient from the bf16 operands."""
        x = self.x.double().permute(0, 3, 1, 2)
        w = self.w.double().requires_grad_(True)
        if self.kind == "conv":
            y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w.permute(3, 2, 0, 1).contiguous(), stride=self.s)
        else:
            y = F.conv_transpose2d(x, w.permute(3, 2, 0, 1).contiguous(), stride=self.s, padding=1)
        y.permute(0, 2, 3, 1).backward(self.dy.double())
        return w.grad.numpy()

    def workspace_split(self):
        """(splitk, rows per split, rows of the last split) of the weight gradient's plan: splitk is read off the workspace
        query (bytes / 4 / outputs), the rows follow as plan_tn16x rounds them (whole 64-pixel tiles)."""
        from biggan_tensorflow_amd import hip
        L = hip.lib()
        d = hip.conv_desc(self.N, self.H, self.W, self.Cin, self.Ho, self.Wo, self.Cout, self.k, self.s, 1,
                          hip.PAD_REFLECT if self.kind == "conv" else hip.PAD_ZERO, hip.COMPUTE_BF16, hip.BF16, hip.BF16, 1)
        query = L.bg_conv2d_wgrad_workspace_bytes if self.kind == "conv" else L.bg_deconv2d_wgrad_workspace_bytes
        nb = int(query(d))
        outputs = self.Mf * self.Cb
        if nb == 0:
            return 1, self.M, self.M
        assert nb % (4 * outputs) == 0, (nb, outputs)
        sk = nb // (4 * outputs)
        rps = (-(-self.M // sk) + 63) // 64 * 64
        assert -(-self.M // rps) == sk, "the plan's split is not the one the workspace holds"
        return sk, rps, self.M - (sk - 1) * rps


@functools.lru_cache(maxsize=None)
def _case(args, opts=()):
    return _Case(*args, **dict(opts))


def _run(c, phased, bn=None):
    os.environ["BG_TN16X_PHASED"] = phased
    if bn is not None:
        os.environ["BG_TN16X_PHASED_BN"] = bn
    try:
        return c.run()
    finally:
        os.environ.pop("BG_TN16X_PHASED", None)
        os.environ.pop("BG_TN16X_PHASED_BN", None)


def _forms_agree(args, check64, opts=(), repeats=1):
    """The weight gradient under BG_TN16X_PHASED = 0 and = 1 (both column tiles, `repeats` times each): equal; with check64
    also float64 within TOL64.  Returns the case."""
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    Fn.set_precision("bf16")
    try:
        c = _case(args, opts)
        base = _run(c, "0")
        for bn in BNS:
            for rep in range(repeats):
                got = _run(c, "1", bn)
                assert torch.equal(base, got), ("BG_TN16X_PHASED=1 BG_TN16X_PHASED_BN=%s run %d differs from the 256 x 128 form: "
                                                "max |d| %.3e" % (bn, rep, (base - got).abs().max().item()))
        if check64:
            err = rel_err(base.double().cpu().numpy(), c.reference())
            print("float64: rel err %.3e" % err)
            assert err < TOL64
        return c
    finally:
        Fn.set_precision("fp32")


def _names(c, phased, bn=None):
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    Fn.set_precision("bf16")
    try:
        if phased is None:
            return _kernels_of(c.run)[1]
        return _kernels_of(lambda: _run(c, phased, bn))[1]
    finally:
        Fn.set_precision("fp32")


def _ids(cases):
    return ["%s-n%d-h%d-%dto%d-k%ds%d" % c[0] for c in cases]


def _param(cases):
    return pytest.mark.parametrize("args,check64", cases, ids=_ids(cases))


# (kind, N, H, Cin, Cout, k, s) ; float64 check.  A convolution's column operand is dy (Cb = Cout).
COLUMN_TILES = [(("conv", 2, 16, 64, cout, 3, 1), cout == 264) for cout in (192, 384, 200, 264, 96)]


@_param(COLUMN_TILES)
def test_column_tiles(args, check64):
    """Cb = 192 and 384: whole 192-column tiles, three quarters of a 256-column tile resp. one and a half ; 200 = 192 + 8 and
    264: a full 192-column tile and a nearly empty one (264: a full 256-column tile and 8 columns) ; 96: one partly filled
    tile, which only the switch sends here.  512 pixels in 2 splits of 16 K blocks."""
    _forms_agree(args, check64)


ROW_TAILS = [(("conv", 2, 16, 72, 192, 3, 1), True), (("conv", 2, 16, 96, 192, 3, 1), False)]


@_param(ROW_TAILS)
def test_row_tails_and_taps_that_straddle_images(args, check64):
    """Ca = 72 and 96 under a 3 x 3 kernel: Mf = 648 and 864 rows - the last 256-row tile partial, 128-row A images that
    begin and end inside a tap."""
    _forms_agree(args, check64)


GATHERS = [(("conv", 2, 16, 64, 192, 3, 1), False), (("conv", 8, 16, 64, 192, 3, 2), True),
           (("deconv", 2, 16, 192, 64, 4, 2), True), (("deconv", 2, 16, 192, 64, 3, 1), False)]


@_param(GATHERS)
def test_gathers(args, check64):
    """Reflect-padded 3 x 3 convolutions at both strides (mirrored source pixels) ; 4 x 4 stride-2 and 3 x 3 transposed
    convolutions, whose gathered operand is dy and whose out-of-range sources read the zero page."""
    _forms_agree(args, check64)


# stride-2 convolutions on 16 x 16 (M = 64 N) and 16 x 8 (M = 32 N) maps; what the plan must make of them
K_WALK = [(("conv", 9, 16, 64, 192, 3, 2), (), "even", True),            # 576 = 3 x 192: equal splits of 6 tiles of 32
          (("conv", 10, 16, 64, 192, 3, 2), (), "short", False),         # 640 = 256 + 256 + 128
          (("conv", 27, 16, 64, 192, 3, 2), (("W", 8),), "odd", False),  # 864 = 3 x 256 + 96: 3 tiles of 32 in the last
          (("conv", 13, 16, 64, 192, 3, 2), (), "prologue", False)]      # 832 = 3 x 256 + 64: 4 K blocks, the prologue issues 6


@pytest.mark.parametrize("args,opts,what,check64", K_WALK, ids=[c[2] for c in K_WALK])
def test_k_walk(args, opts, what, check64):
    """Splits of equal length, a last split shorter than the others, an odd and an even number of 32-pixel tiles in a split,
    and a split of no more K blocks than the prologue issues (ring of 6: 6 blocks of 16 pixels).  In K blocks: 12 = two rings
    exactly, 16, 8, 6 = one ring, 4."""
    c = _forms_agree(args, check64, opts)
    sk, rps, last = c.workspace_split()
    tiles_last = -(-last // 32)
    print("M %d: %d splits of %d rows, the last %d (%d tiles)" % (c.M, sk, rps, last, tiles_last))
    assert sk > 1 and (rps // 32) % 2 == 0
    if what == "even":
        assert last == rps
    elif what == "short":
        assert last < rps and tiles_last % 2 == 0 and tiles_last * 2 > 6
    elif what == "odd":
        assert last < rps and tiles_last % 2 == 1
    else:
        assert 2 * tiles_last <= 6


def test_split_k_off():
    """Mf = 16 x 1024 rows by 640 columns: 64 x 5 tiles of 256 x 128 leave the plan no split (512 slots / 320 tiles), so the
    blocks write the weight gradient itself - 64 x 4 tiles at BN = 192, the last column tile 64 wide.  (The only way to a
    wide-form launch without a split: any M >= 512 is otherwise cut in at least two.)"""
    c = _forms_agree(("deconv", 2, 16, 640, 1024, 4, 2), False)
    assert c.workspace_split()[0] == 1


def test_recorded_names():
    """The forced form is what ran, at the column tile asked for; a Cb the rule refuses (200) keeps tn16x_kernel<0, 32>; a
    reduction too short for the wide forms (256 pixels) keeps tn16_kernel even when the form is forced."""
    c = _case(("conv", 2, 16, 64, 200, 3, 1))
    for bn in BNS:
        names = _names(c, "1", bn)
        assert "tn16x_phased_kernel<0, %s, 6>" % bn in names, names
        assert not any(n.startswith("tn16x_kernel") for n in names), names
    names = _names(c, None)
    assert "tn16x_kernel<0, 32>" in names and not any(n.startswith("tn16x_phased") for n in names), names
    names = _names(_case(("conv", 1, 16, 64, 192, 3, 1)), "1")
    assert "tn16_kernel<0>" in names and not any(n.startswith("tn16x") for n in names), names


def test_rule_takes_a_filled_round_of_192_column_tiles():
    """Unset switches.  Cb = 192 under Mf = 16 x 256 rows and 4096 pixels: 16 row tiles x 16 splits = one block on each of
    the 256 CUs - the rule takes BN = 192, and the result equals the 256 x 128 form's.  The same Cb on a grid of 6 blocks
    stays on tn16x_kernel<0, 32>."""
    args = ("deconv", 16, 16, 192, 256, 4, 2)
    c = _forms_agree(args, False)
    assert c.workspace_split()[:2] == (16, 256)
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    Fn.set_precision("bf16")
    try:
        base = _run(c, "0")
        got, names = _kernels_of(c.run)
    finally:
        Fn.set_precision("fp32")
    assert "tn16x_phased_kernel<0, 192, 6>" in names, names
    assert torch.equal(base, got)
    names = _names(_case(("conv", 2, 16, 64, 192, 3, 1)), None)
    assert "tn16x_kernel<0, 32>" in names and not any(n.startswith("tn16x_phased") for n in names), names


SCREEN = [("conv", 10, 16, 64, 192, 3, 2), ("deconv", 2, 16, 192, 64, 4, 2)]


@pytest.mark.parametrize("args", SCREEN, ids=_ids([(c, False) for c in SCREEN]))
def test_schedule_screen(args):
    """New barriers and counted waits: 25 runs per column tile in one process, each equal to the one output of the 256 x 128
    form (a screen for K blocks read before they landed or restaged before they were read)."""
    _forms_agree(args, False, repeats=25)
