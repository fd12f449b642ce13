"""Lists of ``launch_replay.Call`` objects for the geometries the conv / transposed-conv / rgbconv / attention entry points
ACCEPT (check_conv, bg_rgbconv_supported, bg_attention16_supported, bg_attention2_supported of include/biggan_hip.h) but
no model of the benchmark builds: small and non-square maps, every kernel size, both strides, both splits of an odd total
padding, both sides of every rung of the attention dispatch ladders.

Test helper, pure Python: nothing here touches the GPU or the library.  ``tests/test_gpu_geometry_sweep.py`` feeds the lists
to ``launch_replay.replay_all`` (float64 reference, derived per-element bound, NaN-prefilled outputs, guard bands, two
bit-identical runs); ``resolve`` is handed the loaded library to fill in what only it knows (workspace sizes, and whether
functional.Conv2dFn would send a thin fp32 layer to bg_rgbconv_*).

Every list is a fixed function of its arguments: flags and descriptors follow the call's index, never a random generator.
"""
import collections

from tests.launch_replay import BF16, F32, PAD_REFLECT, PAD_ZERO, Call

# ------------------------------------------------------------------------------------------
# the acceptance contract
# ------------------------------------------------------------------------------------------
# Every call of the sweep must return BG_OK unless its geometry matches a row here.  A row is
#   (rule, the sentence of include/biggan_hip.h that documents it, predicate(call) -> bool);
# a narrowed geometry must be rejected by the FORWARD entry too (error code + message), and at most MAX_REJECTED of one
# family's calls (convolution, transposed convolution, attention16, attention2: ``family``) may be narrowed.  Nothing
# model.py can build may match a row: functional.conv_route sends a layer with more than 4 x 4 taps to the fp32-tensor
# kernels before a descriptor of this kind is ever made.
def _resident_wide_kernel(call):
    """bf16-resident forward / input-gradient launch (the tap kernels of csrc/igemm16.hip walk at most 4 taps per axis)."""
    if call.name not in ("bg_conv2d_fwd", "bg_conv2d_dgrad", "bg_deconv2d_fwd", "bg_deconv2d_dgrad"):
        return False
    k, x_dtype, y_dtype = call.desc[7], call.desc[12], call.desc[13]
    return k > 4 and (x_dtype if call.name.endswith("fwd") else y_dtype) == BF16


NARROWED = [
    ("bf16-resident forward and input gradient: k <= 4",
     "The forward and the input gradient take kernels of at most 4 x 4 taps (k <= 4)",
     _resident_wide_kernel),
]
MAX_REJECTED = 0.20


def narrowed(call):
    """The NARROWED row that covers `call`, or None."""
    for row in NARROWED:
        if row[2](call):
            return row
    return None


def family(case_id):
    """conv | deconv | attention16 | attention2: the family of entry points a case of ``cases()`` belongs to."""
    return case_id.split("/")[0].split("_")[0]


# ------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------
CONV_K = (1, 2, 3, 4, 5, 7)
CONV_MAPS = ((2, 2), (3, 3), (3, 5), (4, 4), (5, 4), (6, 6), (8, 8))            # (5, 4): stride 1 only
FP32_GEMM = ((8, 8), (6, 5))          # (Cin, Cout) on the MFMA kernels: vectorised / scalar gathers
FP32_THIN = ((8, 3), (8, 1))          # <= 3 output channels: bg_rgbconv_* where bg_rgbconv_supported says so
BF16_RESIDENT = ((8, 16), (32, 32))
DECONV_K = (3, 4)
DECONV_MAPS = (2, 3, 4, 5)

Geom = collections.namedtuple("Geom", "H W Ho Wo k stride pad_lo pad_hi")


def conv_geometries(mode):
    """Every (map, k, stride, padding split) of the sweep that meets the header's preconditions: H, W multiples of the
    stride (the input gradient's), pad_lo < H, W, and for reflect padding pad_lo, pad_hi <= H - 1, W - 1 (tf.pad's rule:
    one reflection).  Ho = ceil(H / stride), the total padding is TF SAME's, pad_lo its low half; an odd total (odd k at
    stride 2) is also split the other way round."""
    out = []
    for k in CONV_K:
        for s in (1, 2):
            for H, W in CONV_MAPS:
                if (H, W) == (5, 4) and s != 1:
                    continue
                if H % s or W % s:
                    continue
                Ho, Wo = -(-H // s), -(-W // s)
                tot = max((Ho - 1) * s + k - H, 0)            # the same for W: both are multiples of the stride
                assert tot == max((Wo - 1) * s + k - W, 0)
                splits = [tot // 2]
                if tot % 2 and k % 2 and s == 2:
                    splits.append(tot - tot // 2)
                for lo in splits:
                    hi = tot - lo
                    lim = min(H, W) - 1
                    if lo > lim or (mode == PAD_REFLECT and hi > lim):
                        continue
                    out.append(Geom(H, W, Ho, Wo, k, s, lo, hi))
    return out


def _conv_desc(g, N, cin, cout, mode, resident):
    dt = BF16 if resident else F32
    return (N, g.H, g.W, cin, g.Ho, g.Wo, cout, g.k, g.stride, g.pad_lo, mode, 1 if resident else 0, dt, dt,
            1 if resident else 0)


def conv_calls(entry, precision, mode, group="gemm"):
    """bg_conv2d_<entry> over conv_geometries(mode).  precision "fp32": group "gemm" = FP32_GEMM, "thin" = FP32_THIN, N
    alternating 1 / 3; "bf16": BF16_RESIDENT, N = 3.  Each geometry gets every (Cin, Cout) of its group.  Forward: bias on
    the even calls; forward and input gradient: accumulate on the calls with index % 4 == 1."""
    pairs = BF16_RESIDENT if precision == "bf16" else (FP32_GEMM if group == "gemm" else FP32_THIN)
    calls = []
    for g in conv_geometries(mode):
        for cin, cout in pairs:
            i = len(calls)
            N = 3 if precision == "bf16" else (1, 3)[(i // 2) % 2]
            desc = _conv_desc(g, N, cin, cout, mode, precision == "bf16")
            if entry == "fwd":
                flags = dict(bias=i % 2 == 0, alpha=False, acc=int(i % 4 == 1), ws=0)
            elif entry == "dgrad":
                flags = dict(alpha=False, acc=int(i % 4 == 1), ws=0)
            else:
                flags = dict(ws=0)
            calls.append(Call("bg_conv2d_" + entry, desc, flags, (0, 0, 0)))
    return calls


def deconv_calls(precision):
    """bg_deconv2d_fwd / _dgrad / _wgrad: k in DECONV_K, stride 1 and 2, square maps DECONV_MAPS, Ho = stride * H, pad_lo =
    TF SAME's low crop of the transposed convolution."""
    pairs = BF16_RESIDENT if precision == "bf16" else FP32_GEMM
    calls = []
    for k in DECONV_K:
        for s in (1, 2):
            for H in DECONV_MAPS:
                lo = max(k - s, 0) // 2
                for cin, cout in pairs:
                    i = len(calls) // 3
                    N = 3 if precision == "bf16" else (1, 3)[(i // 2) % 2]
                    g = Geom(H, H, s * H, s * H, k, s, lo, 0)
                    desc = _conv_desc(g, N, cin, cout, PAD_ZERO, precision == "bf16")
                    calls.append(Call("bg_deconv2d_fwd", desc, dict(bias=i % 2 == 0, alpha=False, acc=int(i % 4 == 1), ws=0),
                                      (0, 0, 0)))
                    calls.append(Call("bg_deconv2d_dgrad", desc, dict(alpha=False, acc=int(i % 4 == 1), ws=0), (0, 0, 0)))
                    calls.append(Call("bg_deconv2d_wgrad", desc, dict(ws=0), (0, 0, 0)))
    return calls


def padded_grid_bytes(desc):
    """Bytes of the input gradient on the reflect-padded grid of a bg_conv2d_dgrad descriptor (extents rounded up to the
    stride): what the padded-grid + fold form needs as workspace at least, and the mirrored-source / ring forms do not.  The
    fold and the ring launches carry no profile record of their own, so this is how a test tells the forms apart."""
    N, H, W, cin, Ho, Wo, cout, k, s, lo, mode, compute, xdt = desc[:13]
    ext = lambda no: -(-((no - 1) * s + k) // s) * s          # noqa: E731
    return N * ext(Ho) * ext(Wo) * cin * (2 if xdt == BF16 else 4)


def double_mirror(desc):
    """A row or column of the reflect-padded map mirrors padded positions on both sides (H <= pad_lo + pad_hi + 1)."""
    N, H, W, cin, Ho, Wo, cout, k, s, lo, mode = desc[:11]
    if mode != PAD_REFLECT or lo == 0:
        return False
    for n, no in ((H, Ho), (W, Wo)):
        hi = (no - 1) * s + k - 1 - lo - (n - 1)
        if hi > 0 and max(1, n - 1 - hi) <= min(lo, n - 2):
            return True
    return False


def resolve(calls, L, desc_type):
    """Fill in what the library decides: a thin fp32 conv call becomes the bg_rgbconv_* call functional.Conv2dFn makes when
    bg_rgbconv_supported(desc) (one decision per layer, all three passes), and every call gets its workspace size."""
    out = []
    for c in calls:
        if not c.name.startswith(("bg_conv2d", "bg_deconv2d")):
            out.append(c)
            continue
        d = desc_type(*c.desc)
        name, flags = c.name, dict(c.flags)
        if name.startswith("bg_conv2d") and d.x_dtype == F32 and L.bg_rgbconv_supported(d):
            name = name.replace("conv2d", "rgbconv")
            flags.pop("alpha", None)
            flags.pop("ws", None)
            if name.endswith("wgrad"):
                flags["ws"] = int(L.bg_rgbconv_wgrad_workspace_bytes(d))
        else:
            flags["ws"] = int(getattr(L, name + "_workspace_bytes")(d))
        out.append(Call(name, c.desc, flags, c.align))
    return out


# ------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------
A16_D = (4, 16, 20, 32, 36, 64)                     # both sides of the DQT rungs 1 | 2 | 4 (d <= 16 | 32 | 64)
A16_DV = (4, 32, 36, 64, 68, 96, 100, 128, 132, 192, 196, 256)      # both sides of the DVT rungs 1 | 2 | 3 | 4 | 6 | 8
A2_D = (4, 16, 20, 32)
A2_DV = (4, 32, 36, 64, 68, 96, 100, 128)
ATTN_N = ((128, 128), (128, 256))                   # (N, Nk)


def a16_instance(d, dv):
    """(DQT, DVT) of the attn16_* instantiation A16_DISPATCH (csrc/attention16.hip) picks for (d, dv)."""
    dqt, dvt = (d + 15) // 16, (dv + 31) // 32
    if dqt <= 1 and dvt <= 4:
        return 1, (1 if dvt <= 1 else 2 if dvt <= 2 else 4)
    if dqt <= 2:
        return 2, (2 if dvt <= 2 else 3 if dvt <= 3 else 4 if dvt <= 4 else 8)
    return 4, (4 if dvt <= 4 else 6 if dvt <= 6 else 8)


def a2_instance(d, dv):
    """(DQ, DVT) of the attn_* instantiation ATTN_DISPATCH (csrc/attention.hip) picks for (d, dv)."""
    return (16 if d <= 16 else 32), min((dv + 31) // 32, 4)


def _a16_desc(N, Nk, d, dv):
    """B = 1; every tensor is a column slice of a buffer 4 columns wider, so every store has foreign columns next to it."""
    ldd, ldv = d + 4, dv + 4
    return (1, N, Nk, d, dv, 0,
            ldd, N * ldd, ldd, Nk * ldd, ldv, Nk * ldv, ldv, N * ldv,              # q, k, v, o
            ldv, N * ldv, ldd, N * ldd, ldd, Nk * ldd, ldv, Nk * ldv)              # dout, dq, dk, dv


def attention16_calls(kind, N, Nk):
    """kind "fwd": bg_attention16_fwd; "dkv": the dk / dv call of bg_attention16_bwd (which also writes delta); "dq": its
    dq-only call.  Full cross product A16_D x A16_DV."""
    calls = []
    for d in A16_D:
        for dv in A16_DV:
            desc = _a16_desc(N, Nk, d, dv)
            if kind == "fwd":
                calls.append(Call("bg_attention16_fwd", desc, {}, (0,) * 4))
            else:
                dq = kind == "dq"
                calls.append(Call("bg_attention16_bwd", desc, dict(dq=dq, dk=not dq, dv=not dq), (0,) * 8))
    return calls


def attention2_calls(kind, N, Nk):
    """bg_attention2_fwd / bg_attention2_bwd (contiguous fp32 tensors, B = 1) over A2_D x A2_DV."""
    calls = []
    for d in A2_D:
        for dv in A2_DV:
            if kind == "fwd":
                calls.append(Call("bg_attention2_fwd", (1, N, Nk, d, dv), {}, (0,) * 4))
            else:
                calls.append(Call("bg_attention2_bwd", (1, N, Nk, d, dv), {}, (0,) * 8))
    return calls


# ------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_geometry_sweep.py: id -> (environment, builder)
# ------------------------------------------------------------------------------------------
def cases():
    """Ordered id -> (env, calls): (family, precision, pad mode) with the families split so that no case has more than
    about 150 calls.  env = variables set around the replay (BG_DGRAD_RING selects the input gradient's reflect form on the
    bf16-resident path; only bg_conv2d_dgrad and its workspace query read it, so only those cases run under both)."""
    out = collections.OrderedDict()
    pads = (("reflect", PAD_REFLECT), ("zero", PAD_ZERO))
    for entry in ("fwd", "dgrad", "wgrad"):
        for pname, mode in pads:
            for group in ("gemm", "thin"):
                out["conv_%s_%s/fp32/%s" % (entry, group, pname)] = ({}, conv_calls(entry, "fp32", mode, group))
    for entry in ("fwd", "wgrad"):
        for pname, mode in pads:
            out["conv_%s/bf16/%s" % (entry, pname)] = ({}, conv_calls(entry, "bf16", mode))
    for ring in ("1", "0"):
        out["conv_dgrad_ring%s/bf16/reflect" % ring] = ({"BG_DGRAD_RING": ring}, conv_calls("dgrad", "bf16", PAD_REFLECT))
    out["conv_dgrad/bf16/zero"] = ({}, conv_calls("dgrad", "bf16", PAD_ZERO))       # (zero padding never reads it)
    for precision in ("fp32", "bf16"):
        out["deconv/%s/zero" % precision] = ({}, deconv_calls(precision))
    for kind in ("fwd", "dkv", "dq"):
        for N, Nk in ATTN_N:
            out["attention16_%s_Nk%d/bf16/-" % (kind, Nk)] = ({}, attention16_calls(kind, N, Nk))
    for kind in ("fwd", "bwd"):
        out["attention2_%s/fp32/-" % kind] = ({}, [c for N, Nk in ATTN_N for c in attention2_calls(kind, N, Nk)])
    return out
