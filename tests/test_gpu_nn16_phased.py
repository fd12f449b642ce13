"""The phased form of nn16_kernel (csrc/igemm16.hip; BG_NN16_PIPE = 3: a 256-row tile on 8 waves at one block per CU, two
64-channel stages filled half by half, four accumulator quadrants per K tile, one counted vmcnt per tile) feeds every
accumulator the same sequence of 32-channel MFMA K blocks as the two-stage form (BG_NN16_PIPE = 0) and takes the K splits
of the same plan, so the outputs are EQUAL bit for bit - forward, input gradient, split-K slabs and every epilogue variant,
at every column tile (BG_NN16X_BN = 128, 192, 256).  One case per group is also checked against float64 on the bf16 operands
(relative L2 error < 6e-3, the bound of tests/test_gpu_nn16_pipe.py).

All maps here have sides that are no multiple of 16, so none of the launches takes the halo-tile kernel."""
import os
import tempfile

import pytest
import torch

from tests.common import rel_err
from tests.test_gpu_nn16_pipe import _Case, _ids, STRADDLE, PHASES, EPILOGUE, TOL64

pytestmark = pytest.mark.gpu
BNS = ("128", "192", "256")
# The case lists are the pipe test's own, as the forms are compared on the same shapes; an edit there must not change what this
# file covers without showing here.
assert (len(STRADDLE), len(PHASES), len(EPILOGUE)) == (14, 3, 5), "the case lists of tests/test_gpu_nn16_pipe.py changed"
assert (("conv", 5, 10, 96, 72, 3, 1), {}) in [c for c, _ in STRADDLE], "the 500-row straddle case is gone"


def _kernels_of(fn):
    """Runs fn() with the launch recorder on: (result, kernel names the launchers recorded)."""
    from biggan_tensorflow_amd import hip
    L = hip.lib()
    fd, path = tempfile.mkstemp(suffix=".tsv")
    os.close(fd)
    L.bg_prof_reset()
    L.bg_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        L.bg_prof_dump(path.encode())
    finally:
        L.bg_prof_reset()
        L.bg_prof_enable(0)
    with open(path) as fh:
        names = [line.split("\t")[1] for line in fh.read().splitlines()[1:]]
    os.unlink(path)
    return out, names


def _run(c, pipe, bn=None):
    os.environ["BG_NN16_PIPE"] = pipe
    if bn is not None:
        os.environ["BG_NN16X_BN"] = bn
    try:
        return c.run()
    finally:
        os.environ.pop("BG_NN16_PIPE", None)
        os.environ.pop("BG_NN16X_BN", None)


def _forms_agree(case, check64, bns=BNS, repeats=1):
    """Runs `case` under BG_NN16_PIPE = 0 and = 3 (every column tile of `bns`, `repeats` times each): equal outputs; with
    check64 also float64 within TOL64.  Returns the case."""
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    Fn.set_precision("bf16")
    try:
        c = _Case(*case[0], **case[1])
        base = _run(c, "0")
        for bn in bns:
            for rep in range(repeats):
                outs = _run(c, "3", bn)
                for i, (a, b) in enumerate(zip(base, outs)):
                    assert torch.equal(a, b), ("BG_NN16_PIPE=3 BG_NN16X_BN=%s run %d: output %d differs from the two-stage form"
                                               % (bn, rep, i))
        if check64:
            for a, r in zip(base, c.reference()):
                err = rel_err(a.double().cpu().numpy(), r)
                print("float64: rel err %.3e" % err)
                assert err < TOL64
        return c
    finally:
        Fn.set_precision("fp32")


def _param(cases):
    return pytest.mark.parametrize("case,check64", cases, ids=_ids(cases))


# (kind, N, H, Cin, Cout, k, s), options ; float64 check
K_WALK = [((("conv", 2, 8, cin, 64, 1, 1), {}), cin == 320) for cin in (32, 64, 128, 192, 320, 448)]


@_param(K_WALK)
def test_k_walk_against_the_two_tile_loop(case, check64):
    """1 x 1 convolutions of 32 ... 448 channels: 1, 1, 2, 3, 5 and 7 K tiles - shorter than the prologue (two tiles), equal
    to it, odd and even remainders behind the two-tiles-per-trip loop."""
    _forms_agree(case, check64)


@_param(STRADDLE)
def test_stages_that_straddle_taps(case, check64):
    """Reflect-padded 3 x 3 convolutions whose 64-channel K tiles straddle taps (C = 96, 160, 72), both strides, 500 rows
    (two 256-row tiles, the last partial), every column tile."""
    _forms_agree(case, check64)


COLUMN_TAILS = [((("conv", 3, 6, 64, 264, 3, 1), {}), True), ((("conv", 3, 6, 64, 136, 3, 1), {}), False)]


@_param(COLUMN_TAILS)
def test_column_tails(case, check64):
    """264 and 136 output channels: one full and one nearly empty column tile at BN = 256 and at BN = 128; at BN = 192 a full
    and a partly filled tile (264) and one partly filled tile (136)."""
    _forms_agree(case, check64)


@_param(PHASES)
def test_stride_phases(case, check64):
    """Transposed 4 x 4 stride-2 convolution forward and input gradient, input gradient of a 3 x 3 stride-2 convolution."""
    _forms_agree(case, check64)


# splitk read off the workspace query of these descriptors (bytes / 4 / outputs), forward: Cin 512: 72 K tiles in 15 splits of
# 5, the last has 2 ; Cin 384: 54 tiles in 11 splits of 5, the last has 4 (shorter by an odd count) ; Cin 704: 99 tiles in 15
# splits of 7, the last has ONE.  No plan with an empty split was found: a scan of Cin = 64 ... 2048 in steps of 8 on 4 x 4 and
# 6 x 6 maps, 1 x 1 and 3 x 3 kernels, never leaves one (the kernel handles it: a block without K tiles stores zeros).
SPLIT_K = [((("conv", 2, 4, 512, 64, 3, 1), {}), True), ((("conv", 2, 4, 384, 64, 3, 1), {}), False),
           ((("conv", 2, 4, 704, 64, 3, 1), {}), False)]


@_param(SPLIT_K)
def test_split_k(case, check64):
    """A single tile with a deep K: the plan splits K unevenly; the slab reduce is part of the comparison."""
    from biggan_tensorflow_amd import hip
    c = _forms_agree(case, check64)
    nbytes = hip.lib().bg_conv2d_fwd_workspace_bytes(c.d)
    assert nbytes > c.y0.numel() * 4, "the plan of this shape no longer splits K"


def test_position_major_tile_inside_one_position():
    """Reflect-padded 3 x 3 convolution on a 4 x 4 map of 256 images: position-major rows, a 256-row tile covers exactly one
    position, so the form applies (forward, and the plain transposed gather of the input gradient)."""
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    case = (("conv", 256, 4, 64, 96, 3, 1), {})
    c = _forms_agree(case, True)
    Fn.set_precision("bf16")
    try:
        _, names = _kernels_of(lambda: _run(c, "3", "128"))
    finally:
        Fn.set_precision("fp32")
    assert any(n.startswith("nn16_kernel<4,") and n.endswith("true, false, 2, 4>") for n in names), names


def test_position_major_tile_across_positions_is_refused():
    """The same shape at 130 images: a 256-row tile would span positions, so BG_NN16_PIPE = 3 must leave the position-major
    launch (the input gradient) on the two-stage kernel - its recorded name is not the 8-wave instantiation - and the
    outputs stay equal."""
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    case = (("conv", 130, 4, 64, 96, 3, 1), {})
    c = _forms_agree(case, False)
    Fn.set_precision("bf16")
    try:
        _, names = _kernels_of(lambda: _run(c, "3"))
    finally:
        Fn.set_precision("fp32")
    # (the forward launch is image-major - every tap of a reflect-padded map has a source - and may take the form)
    pm = [n for n in names if n.startswith("nn16_kernel<") and ", true" in n]
    assert pm and not any(n.endswith(", 2, 4>") for n in pm), names


@_param(EPILOGUE)
def test_epilogue(case, check64):
    """Bias and the alpha scale; accumulation into a bf16 and into an fp32 output; the depth-to-space store; rows without an
    output pixel (BG_DGRAD_RING=0: the padded 7 x 7 gradient grid of a stride-2 convolution on a 6 x 6 map)."""
    args, opts = case
    opts = dict(opts)
    if opts.pop("padded_grid", False):
        os.environ["BG_DGRAD_RING"] = "0"
    try:
        _forms_agree((args, opts), check64)
    finally:
        os.environ.pop("BG_DGRAD_RING", None)


SCREEN = [(("conv", 2, 8, 448, 64, 1, 1), {}), (("conv", 5, 10, 96, 72, 3, 1), {}), (("conv", 2, 4, 512, 64, 3, 1), {})]


@pytest.mark.parametrize("case", SCREEN, ids=_ids([(c, False) for c in SCREEN]))
def test_schedule_screen(case):
    """A new barrier / counted-wait structure: 25 runs per column tile in one process, each equal to the one two-stage output
    (a screen for tiles read before they landed or restaged before they were read)."""
    _forms_agree(case, False, repeats=25)
