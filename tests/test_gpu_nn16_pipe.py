"""The pipeline forms of nn16_kernel (csrc/igemm16.hip; BG_NN16_PIPE = 0: two 64-channel stages, 1: 3-slot ring of 32-channel
stages at the 128-row tile, 2: the same ring under a 256-row tile on 8 waves) feed every accumulator the same sequence of
32-channel MFMA K blocks, so their outputs are EQUAL bit for bit - forward, input gradient, split-K slabs and every epilogue
variant.  One case per group is also checked against float64 on the bf16 operands (relative L2 error < 6e-3, the bound
of test_gpu_bf16.py::test_position_major_rows_match_the_image_major_walk: bf16 outputs, unit round-off 2^-9).

All maps here have sides that are no multiple of 16, so none of the launches takes the halo-tile kernel."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.common import rel_err

pytestmark = pytest.mark.gpu
TOL64 = 6e-3
PIPES = ("0", "1", "2")


def _bf16(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").to(torch.bfloat16)


class _Case:
    """One convolution (kind "conv": tf.pad + VALID conv, "deconv": transposed conv) through the C ABI of the bf16-resident
    path: forward (bias / alpha / accumulate / fp32 output / depth-to-space store on request) and, for bf16 outputs, the
    input gradient (optionally accumulated)."""

    def __init__(self, kind, N, H, Cin, Cout, k, s, bias=False, alpha=None, acc=False, y32=False, d2s=False):
        from biggan_tensorflow_amd import functional as Fn, hip
        self.kind, self.k, self.s, self.alpha, self.acc, self.y32, self.d2s = kind, k, s, alpha, acc, y32, d2s
        rng = np.random.default_rng(N + H + Cin + Cout + k + s)
        self.pad = 1 if k >= 3 else 0
        self.reflect = kind == "conv" and self.pad > 0
        if kind == "conv":
            Ho = (H + 2 * self.pad - k) // s + 1
            pm = hip.PAD_REFLECT
            wshape = (k, k, Cin, Cout)
        else:
            Ho = H * s
            pm = hip.PAD_ZERO
            wshape = (k, k, Cout, Cin)
        self.Ho = Ho
        self.x = _bf16(rng.standard_normal((N, H, H, Cin)))
        self.w0 = rng.standard_normal(wshape) * 0.1
        w = torch.tensor(self.w0, dtype=torch.float32, device="cuda")
        self.pp, self.pt = Fn.weight_packs(w)
        self.bias = torch.tensor(rng.standard_normal(Cout), dtype=torch.float32, device="cuda") if bias else None
        self.alpha_dev = torch.tensor([alpha], dtype=torch.float32, device="cuda") if alpha is not None else None
        ydt = torch.float32 if y32 else torch.bfloat16
        yshape = (N, 2 * Ho, 2 * Ho, Cout // 4) if d2s else (N, Ho, Ho, Cout)
        self.y0 = torch.tensor(rng.standard_normal(yshape), dtype=torch.float32, device="cuda").to(ydt)
        self.g = _bf16(rng.standard_normal((N, Ho, Ho, Cout)))
        self.dx0 = _bf16(rng.standard_normal((N, H, H, Cin)))
        self.d = hip.conv_desc(N, H, H, Cin, Ho, Ho, Cout, k, s, self.pad if kind == "conv" else 1, pm,
                               Fn.Precision.compute, hip.BF16, hip.F32 if y32 else hip.BF16, 1)

    def run(self):
        """[y, dx] (dx only for bf16 outputs without the depth-to-space store)."""
        from biggan_tensorflow_amd import hip
        from biggan_tensorflow_amd.hip import act, f32, stream, lib, check
        L, d, dev = lib(), self.d, self.x.device
        conv = self.kind == "conv"
        y = self.y0.clone()
        wf, wd = (self.pt, self.pp) if conv else (self.pp, self.pt)
        if self.d2s:
            assert L.bg_conv2d_fwd_d2s_supported(d, 2) == 1
            check(L.bg_conv2d_fwd_d2s(d, act(self.x), act(wf), f32(self.bias), f32(self.alpha_dev), act(y), 2, None, 0,
                                      stream()))
            return [y]
        ws, nb = hip.scratch(L.bg_conv2d_fwd_workspace_bytes if conv else L.bg_deconv2d_fwd_workspace_bytes, d, dev)
        fwd = L.bg_conv2d_fwd if conv else L.bg_deconv2d_fwd
        check(fwd(d, act(self.x), act(wf), f32(self.bias), f32(self.alpha_dev), act(y), int(self.acc), f32(ws), nb,
                  stream()))
        if self.y32:
            return [y]
        dx = self.dx0.clone()
        ws, nb = hip.scratch(L.bg_conv2d_dgrad_workspace_bytes if conv else L.bg_deconv2d_dgrad_workspace_bytes, d, dev)
        dgrad = L.bg_conv2d_dgrad if conv else L.bg_deconv2d_dgrad
        check(dgrad(d, act(self.g), act(wd), f32(self.alpha_dev), act(dx), int(self.acc), f32(ws), nb, stream()))
        return [y, dx]

    def reference(self):
        """float64 [y, dx] on the operands the kernels saw (x, dy and the packed weights are bf16)."""
        xt = self.x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
        wt = torch.tensor(self.w0, dtype=torch.float32).to(torch.bfloat16).double().permute(3, 2, 0, 1)
        if self.kind == "conv":
            xin = F.pad(xt, (1, 1, 1, 1), mode="reflect") if self.reflect else xt
            yr = F.conv2d(xin, wt, stride=self.s)
        else:
            yr = F.conv_transpose2d(xt, wt, stride=self.s, padding=(self.k - self.s) // 2)
        yr.backward(self.g.double().cpu().permute(0, 3, 1, 2))
        a = 1.0 if self.alpha is None else float(self.alpha_dev.item())
        y = a * yr.detach().permute(0, 2, 3, 1)
        dx = a * xt.grad.permute(0, 2, 3, 1)
        if self.bias is not None:
            y = y + self.bias.double().cpu()
        if self.d2s:
            n, h, w_, c4 = y.shape
            y = y.reshape(n, h, w_, 2, 2, c4 // 4).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w_, c4 // 4)
        if self.acc:
            y = y + self.y0.double().cpu()
            dx = dx + self.dx0.double().cpu()
        return [y.numpy(), dx.numpy()]


def _forms_agree(case, check64):
    """Runs `case` under BG_NN16_PIPE = 0, 1, 2: equal outputs; with check64 also float64 within TOL64."""
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn
    Fn.set_precision("bf16")
    try:
        c = _Case(*case[0], **case[1])
        outs = []
        for pipe in PIPES:
            os.environ["BG_NN16_PIPE"] = pipe
            outs.append(c.run())
        torch.cuda.synchronize()
        for pipe, o in zip(PIPES[1:], outs[1:]):
            for i, (a, b) in enumerate(zip(outs[0], o)):
                assert torch.equal(a, b), "BG_NN16_PIPE=%s: output %d differs from the two-stage form" % (pipe, i)
        if check64:
            for a, r in zip(outs[0], c.reference()):
                err = rel_err(a.double().cpu().numpy(), r)
                print("float64: rel err %.3e" % err)
                assert err < TOL64
    finally:
        os.environ.pop("BG_NN16_PIPE", None)
        Fn.set_precision("fp32")


def _ids(cases):
    return ["-".join(str(v) for v in c[0]) + "".join("-" + k for k in c[1]) for c, _ in cases]


def _param(cases):
    return pytest.mark.parametrize("case,check64", cases, ids=_ids(cases))


# (kind, N, H, Cin, Cout, k, s), options ; float64 check
K_WALK = [((("conv", 2, 8, cin, 64, 1, 1), {}), cin == 160) for cin in (32, 64, 96, 160)]


@_param(K_WALK)
def test_k_walk_against_ring_depth(case, check64):
    """1 x 1 convolutions of 32, 64, 96, 160 channels: 1, 2, 3, 5 stages of 32 channels (K is padded to 64-channel steps:
    2, 2, 4, 6 with the zero stages) - shorter than the ring, equal to it, wrap-around with a remainder."""
    _forms_agree(case, check64)


STRADDLE = [((("conv", 3, 6, cin, cout, 3, s), {}), (cin, cout, s) == (160, 72, 2))
            for cin in (96, 160) for s in (1, 2) for cout in (72, 40, 8)]
STRADDLE += [((("conv", 3, 6, 72, 40, 3, 1), {}), False),       # 9 chunks per tap: stages straddle taps as well
             ((("conv", 5, 10, 96, 72, 3, 1), {}), False)]      # 500 rows: four 128-row / two 256-row tiles, the last partial


@_param(STRADDLE)
def test_stages_that_straddle_taps(case, check64):
    """Reflect-padded 3 x 3 convolutions whose 64-channel K steps straddle taps (C = 96, 160, 72), both strides, rows that are
    no multiple of 128 or 256, output tiles of 96 (partly filled), 64 and 32 columns."""
    _forms_agree(case, check64)


PHASES = [((("deconv", 2, 4, 64, 32, 4, 2), {}), False), ((("deconv", 2, 8, 64, 32, 4, 2), {}), True),
          ((("conv", 2, 8, 64, 64, 3, 2), {}), False)]


@_param(PHASES)
def test_stride_phases(case, check64):
    """Transposed 4 x 4 stride-2 convolution, forward (four phases of 2 x 2 taps) and input gradient, on 4 x 4 and 8 x 8 maps;
    input gradient of a 3 x 3 stride-2 convolution (phases of 1 / 2 / 2 / 4 taps)."""
    _forms_agree(case, check64)


POSMAJOR = [((("conv", 130, 4, 64, 96, 3, 1), {}), True), ((("conv", 16, 4, 64, 96, 3, 1), {}), False)]


@_param(POSMAJOR)
def test_position_major_and_mirrored_tap_launches(case, check64):
    """Reflect-padded 3 x 3 convolution on a 4 x 4 map, forward and input gradient (plain transposed gather + mirrored-tap
    launches): position-major rows, 130 images (a tile covers parts of two positions) and 16 (eight positions)."""
    _forms_agree(case, check64)


def test_split_k():
    """Cin = 512 on a 4 x 4 map of 2 images: 72 K steps over a single tile, so the plan splits K unevenly; the slab reduce is
    part of the comparison."""
    _forms_agree((("conv", 2, 4, 512, 64, 3, 1), {}), True)


EPILOGUE = [((("conv", 3, 6, 96, 72, 3, 1), {"bias": True, "alpha": 0.37}), True),
            ((("conv", 3, 6, 96, 72, 3, 1), {"bias": True, "acc": True}), False),
            ((("conv", 3, 6, 96, 72, 3, 1), {"acc": True, "y32": True, "alpha": 1.5}), False),
            ((("conv", 2, 8, 32, 128, 3, 1), {"bias": True, "d2s": True}), False),
            ((("conv", 2, 6, 64, 64, 3, 2), {"padded_grid": True}), False)]


@_param(EPILOGUE)
def test_epilogue(case, check64):
    """Bias and the alpha scale; accumulation into a bf16 and into an fp32 output; the depth-to-space store; rows without an
    output pixel (BG_DGRAD_RING=0: the input gradient of a reflect-padded stride-2 convolution on a 6 x 6 map runs on the
    padded 7 x 7 grid, whose four phase grids are 4 x 4)."""
    args, opts = case
    opts = dict(opts)
    if opts.pop("padded_grid", False):
        os.environ["BG_DGRAD_RING"] = "0"
    try:
        _forms_agree((args, opts), check64)
    finally:
        os.environ.pop("BG_DGRAD_RING", None)
