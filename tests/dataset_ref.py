"""Shared by tests/test_dataset.py and tests/test_gpu_dataset.py: a numpy model of the two kernels of the device-resident
dataset (bg_dataset_store, bg_dataset_batch), the staging that data.DatasetCache does for a case of tests/input_ref.py's
table, and simulated wrong kernels that the case table has to tell apart from the right one.  The expected batches are
input_ref's own (``Case.want()``: the host path), computed once there and never changed."""
import numpy as np

from biggan_tensorflow_amd import data as D
from tests import input_ref as R

F = np.float32
CASES, RAGGED, GRID_STRIDE = R.CASES, R.RAGGED, R.GRID_STRIDE
FORCES = (None, D.KIND_U8, D.KIND_F32)                  # the rule, every image as uint8 source, every image finished
FILL = 0xFF                                             # arenas start as this byte: four of them are a NaN


def force_id(force):
    return {None: "rule", D.KIND_U8: "all_u8", D.KIND_F32: "all_f32"}[force]


def plan(case, force=None, budget=1 << 40, batch_size=0):
    return D.plan_entries(case.shapes, case.size, case.channels, budget, batch_size=batch_size, force_kind=force)


_finished = {}


def finished(case):
    """The images of a case resized and normalised, not flipped (the kind 1 form): [n, S, S, C] fp32, computed once."""
    if case.name not in _finished:
        a = R.host_path(case.images(), [0] * len(case.shapes), case.size, case.channels)
        a.setflags(write=False)
        _finished[case.name] = a
    return _finished[case.name]


def stages(case, p, wrong=None):
    """What the loader stages for the images of a case, as ``[(src uint8 [bytes], segs int64 [m,4]), ...]``: one packed
    uint8 buffer (data.pack_batch) for the kind 0 images and one fp32 stack for the kind 1 images, flips forced to 0.
    ``wrong == "store_flips"``: the staging applies the batch's flips."""
    S, C, out = case.size, case.channels, []
    imgs, fin = case.images(), finished(case)
    flipped = [bool(f) and wrong == "store_flips" for f in case.flips]
    which = [i for i in range(p.n) if p.kinds[i] == D.KIND_U8]
    if which:
        raw, _, geom = D.pack_batch([imgs[i][:, ::-1] if flipped[i] else imgs[i] for i in which], [False] * len(which), S, C)
        segs = [(off, p.offsets[i], -(-imgs[i].size // 16) * 16, 0) for off, i in zip(geom["offsets"], which)]
        out.append((raw.numpy().copy(), np.array(segs, np.int64).reshape(-1, 4)))
    which = [i for i in range(p.n) if p.kinds[i] == D.KIND_F32]
    if which:
        one = 4 * S * S * C
        src = np.stack([fin[i][:, ::-1] if flipped[i] else fin[i] for i in which]).astype(F)
        segs = [(k * one, p.offsets[i], one, 0) for k, i in enumerate(which)]
        out.append((np.ascontiguousarray(src).view(np.uint8).reshape(-1), np.array(segs, np.int64).reshape(-1, 4)))
    return out


def model_store(src, segs, arena, src_bytes=None, arena_bytes=None):
    """bg_dataset_store on numpy bytes: a refused segment copies nothing.  Returns the new arena."""
    arena = np.array(arena, np.uint8)
    sb = len(src) if src_bytes is None else src_bytes
    ab = len(arena) if arena_bytes is None else arena_bytes
    for s, d, n, _ in np.asarray(segs, np.int64).reshape(-1, 4):
        s, d, n = int(s), int(d), int(n)
        if min(s, d, n) < 0 or (s | d | n) & 3 or s + n > sb or d + n > ab:
            continue
        arena[d:d + n] = src[s:s + n]
    return arena


def model_arena(case, p, wrong=None):
    arena = np.full(p.arena_bytes, FILL, np.uint8)
    for src, segs in stages(case, p, wrong):
        arena = model_store(src, segs, arena)
    return arena


def sel_of(case):
    return np.array([(i, 1 if f else 0) for i, f in enumerate(case.flips)], np.int32).reshape(-1, 2)


def model_batch(arena, table, sel, size, channels, arena_bytes=None, wrong=None):
    """bg_dataset_batch on numpy arrays (``table`` of data.ENTRY_DTYPE).  kind 0 is input_ref.kernel_model, the
    restatement of bg_image_batch_u8 in single fp32 steps.  ``wrong`` names one of WRONG_KERNELS."""
    S, C = size, channels
    ab = len(arena) if arena_bytes is None else arena_bytes
    out = np.empty((len(sel), S, S, C), F)
    for n, (idx, flip) in enumerate(np.asarray(sel, np.int32).reshape(-1, 2)):
        if wrong == "sel_swapped":
            idx, flip = flip, idx
        ok = 0 <= idx < len(table)
        if ok:
            e = table[idx]
            h, w, kind, off = int(e["h"]), int(e["w"]), int(e["kind"]), int(e["offset"])
            ok = (kind in (0, 1) and h >= 1 and w >= 1 and (kind == 0 or (h == S and w == S)) and off >= 0 and off % 16 == 0
                  and off + h * w * C * (4 if kind == 1 else 1) <= ab)
        if not ok:
            out[n] = np.nan
            continue
        if kind == D.KIND_F32:
            f = arena[off:off + 4 * S * S * C].view(F).reshape(S, S, C)
            if wrong == "kind1_renormalised":
                f = ((f / F(127.5)).astype(F) - F(1)).astype(F)
            if flip:
                f = f.reshape(S, S * C)[:, ::-1].reshape(S, S, C) if wrong == "kind1_row_reversed" else f[:, ::-1]
            out[n] = f
        else:
            t = np.zeros(1, D.TABLE_DTYPE)
            t[0] = (off, h, w, 1 if flip else 0, e["scale_y"], e["scale_x"], 0)
            out[n] = R.kernel_model(arena, t, S, C, "source_flipped" if wrong == "kind0_source_mirrored" else None)[0]
    return out


# kind 1 reversing the whole float row instead of the pixel order; the store applying the flip; kind 1 normalised a
# second time; kind 0 mirroring the source instead of the output; the two columns of sel swapped
WRONG_KERNELS = ("kind1_row_reversed", "store_flips", "kind1_renormalised", "kind0_source_mirrored", "sel_swapped")


def modelled(case, force=None, wrong=None):
    """Plan, store and gather a case in the numpy model: [n, S, S, C] fp32."""
    p = plan(case, force)
    return model_batch(model_arena(case, p, wrong), p.table, sel_of(case), case.size, case.channels, wrong=wrong)


bits = R.bits
