"""Input pipeline of the reference (``utils.py:12-121``, ``BigGAN.py:768-787``) without TensorFlow:
file list + optional label file, PNG decoding, TF1 ``resize_images`` (legacy bilinear), random flip,
``x / 127.5 - 1``, shuffle-and-repeat batching with a prefetching worker thread that hands pinned host
batches to the GPU.  Host-side data preparation only: no arithmetic of the training step runs here.

On a GPU the loader by default only decodes: ``pack_batch`` lays the decoded uint8 pixels of a batch out in one
pinned buffer with a table of per-image geometry, and ``functional.image_batch_u8`` (csrc/input.hip) does the
resize, the flip and the normalisation on the device, bit-identical to ``ImageData.image_processing``, which stays
the reference implementation and the fallback (``BG_DEVICE_INPUT=0``, a CPU device, an array that is not uint8).

With ``BG_DEVICE_DATASET_GB`` set (opt-in) the loader keeps the dataset on the GPU: every file is decoded once, stored in
one arena in the smaller of two forms (its uint8 pixels, or the finished fp32 image), and every later batch is one
``functional.dataset_batch`` launch (csrc/dataset.hip) from the batch's indices and flips - the same batches, bit for bit.

Only what the reference's custom-dataset branch needs is provided: 8-bit non-interlaced PNG files (grey,
RGB, palette, with or without alpha), 8-bit Huffman sequential JPEG files (``decode_jpeg``; recognised by content, as
TensorFlow's decoder does) and ``.npy`` arrays ``[H, W, C]`` uint8; ``mnist`` / ``cifar10`` (Keras
downloads) raise ``NotImplementedError``.
"""
import csv
import os
import queue
import struct
import threading
import zlib
from glob import glob

import numpy as np
import torch


# ------------------------------------------------------------------------------------------
# PNG (ISO/IEC 15948): 8-bit, non-interlaced
# ------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _unfilter(raw, h, stride, bpp):
    try:                                                # C helper of libbiggan_hip.so (host code, no GPU involved)
        from . import hip
        out = np.empty((h, stride), np.uint8)
        if len(raw) < h * (stride + 1):
            raise ValueError("PNG: truncated image data")
        rc = hip.lib().bg_png_unfilter(bytes(raw), h, stride, bpp, out.ctypes.data_as(hip.c_void_p))
        if rc != 0:
            raise ValueError("PNG: " + hip.lib().bg_last_error().decode())
        return out
    except ImportError:                                 # library not built: pure-Python fallback (slow)
        return _unfilter_py(raw, h, stride, bpp)


def _unfilter_py(raw, h, stride, bpp):
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    pos = 0
    for r in range(h):
        ft = raw[pos]
        line = np.frombuffer(raw, np.uint8, stride, pos + 1).astype(np.int32)
        pos += 1 + stride
        if ft == 0:
            cur = line
        elif ft == 2:                                   # Up
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):                           # Sub / Average / Paeth: sequential along the row
            cur = np.zeros(stride, np.int32)
            for i in range(stride):
                left = cur[i - bpp] if i >= bpp else 0
                if ft == 1:
                    pred = left
                elif ft == 3:
                    pred = (left + prev[i]) >> 1
                else:
                    ul = prev[i - bpp] if i >= bpp else 0
                    pred = _paeth(int(left), int(prev[i]), int(ul))
                cur[i] = (line[i] + pred) & 255
        else:
            raise ValueError("PNG: bad filter type %d" % ft)
        out[r] = cur
        prev = cur
    return out


def decode_png(data, channels=3):
    """tf.image.decode_png(contents, channels): uint8 [H, W, channels] (channels 1, 3 or 4)."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, plte, trns = 8, [], None, None
    w = h = depth = ctype = interlace = None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if tag == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
        elif tag == b"PLTE":
            plte = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif tag == b"tRNS":
            trns = np.frombuffer(body, np.uint8)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    if depth != 8 or interlace != 0:
        raise NotImplementedError("PNG: only 8-bit non-interlaced files are supported (depth %s, interlace %s)"
                                  % (depth, interlace))
    nch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    px = _unfilter(zlib.decompress(b"".join(idat)), h, w * nch, nch).reshape(h, w, nch)
    if ctype == 3:
        rgb = plte[px[:, :, 0]]
        alpha = np.full((h, w, 1), 255, np.uint8)
        if trns is not None:
            lut = np.full(256, 255, np.uint8)
            lut[:len(trns)] = trns
            alpha = lut[px[:, :, 0]][:, :, None]
        px = np.concatenate([rgb, alpha], axis=2)
    elif ctype == 0:
        px = np.concatenate([px, px, px, np.full((h, w, 1), 255, np.uint8)], axis=2)
    elif ctype == 4:
        px = np.concatenate([px[:, :, :1]] * 3 + [px[:, :, 1:2]], axis=2)
    elif ctype == 2:
        px = np.concatenate([px, np.full((h, w, 1), 255, np.uint8)], axis=2)
    if channels == 4:
        return px
    if channels == 3:
        return px[:, :, :3]
    if channels == 1:                                   # TF converts RGB to grey with the Rec. 601 weights
        g = (0.299 * px[:, :, 0] + 0.587 * px[:, :, 1] + 0.114 * px[:, :, 2])
        return np.clip(np.rint(g), 0, 255).astype(np.uint8)[:, :, None]
    raise ValueError("decode_png: channels must be 1, 3 or 4")


# ------------------------------------------------------------------------------------------
# JPEG (ITU-T T.81): 8-bit Huffman sequential (SOF0 / SOF1), 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0
# ------------------------------------------------------------------------------------------
# Integer arithmetic throughout, the one of libjpeg's defaults (slow-integer inverse DCT, "fancy" chroma upsampling,
# 16-bit fixed-point colour transform).  ``decode_jpeg`` below is the specification: csrc/jpeg.hip (dequantisation,
# IDCT, upsampling, colour on the device) and csrc/jpeg_entropy.hip (the marker walk and the Huffman decode, host C)
# reproduce it exactly, and it is the fallback of both.
JPEG_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                        13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                        45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)
JPEG_SAMPLINGS = ((1, 1), (2, 1), (2, 2))               # luma h x v that the decoder takes; chroma is 1 x 1


def _jpeg_parse(data):
    """The marker walk up to the first scan: frame header, tables, restart interval, start of the entropy-coded data.
    ValueError for malformed data, NotImplementedError for what ``decode_jpeg`` documents as unsupported."""
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError("not a JPEG file")
    qt, huff, frame, restart, pos = {}, {}, None, 0, 2
    while True:
        if pos + 2 > n:
            raise ValueError("JPEG: truncated before the scan")
        if data[pos] != 0xFF:
            raise ValueError("JPEG: marker expected at byte %d" % pos)
        m = data[pos + 1]
        if m == 0xFF:                                   # fill byte
            pos += 1
            continue
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or m == 0x00:
            raise ValueError("JPEG: marker %02X before the scan" % m)
        if pos + 2 > n:
            raise ValueError("JPEG: truncated segment")
        ln = (data[pos] << 8) | data[pos + 1]
        if ln < 2 or pos + ln > n:
            raise ValueError("JPEG: truncated segment")
        seg, end = pos + 2, pos + ln
        if m == 0xDB:                                   # DQT
            while seg < end:
                pq, tq = data[seg] >> 4, data[seg] & 15
                if pq > 1 or tq > 3 or seg + 1 + 64 * (pq + 1) > end:
                    raise ValueError("JPEG: bad quantisation table")
                seg += 1
                t = np.zeros(64, np.int32)
                for k in range(64):
                    t[JPEG_ZIGZAG[k]] = ((data[seg] << 8) | data[seg + 1]) if pq else data[seg]
                    seg += 1 + pq
                qt[tq] = t
        elif m == 0xC4:                                 # DHT
            while seg < end:
                if seg + 17 > end:
                    raise ValueError("JPEG: bad Huffman table")
                tc, th = data[seg] >> 4, data[seg] & 15
                counts = [data[seg + 1 + i] for i in range(16)]
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or seg + 17 + total > end:
                    raise ValueError("JPEG: bad Huffman table")
                table, code, k = {}, 0, seg + 17
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        if code >= (1 << length):
                            raise ValueError("JPEG: bad Huffman table")
                        table[(length, code)] = data[k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[(tc, th)] = table
                seg = k
        elif m == 0xDD:                                 # DRI
            if ln != 4:
                raise ValueError("JPEG: bad restart interval")
            restart = (data[seg] << 8) | data[seg + 1]
        elif m in (0xC0, 0xC1):                         # SOF0 / SOF1
            if frame is not None or ln < 8:
                raise ValueError("JPEG: bad frame header")
            prec, h, w, nc = data[seg], (data[seg + 1] << 8) | data[seg + 2], (data[seg + 3] << 8) | data[seg + 4], data[seg + 5]
            if prec != 8:
                raise NotImplementedError("JPEG: %d-bit samples (8 only)" % prec)
            if ln != 8 + 3 * nc or h < 1 or w < 1:
                raise ValueError("JPEG: bad frame header")
            if nc not in (1, 3):
                raise NotImplementedError("JPEG: %d components (1 or 3)" % nc)
            comps = [(data[seg + 6 + 3 * i], data[seg + 7 + 3 * i] >> 4, data[seg + 7 + 3 * i] & 15, data[seg + 8 + 3 * i])
                     for i in range(nc)]
            if any(c[3] > 3 or c[1] < 1 or c[2] < 1 for c in comps):
                raise ValueError("JPEG: bad frame header")
            if nc == 1:
                hs, vs = 1, 1                           # one component: the MCU is one block whatever the header says
            else:
                hs, vs = comps[0][1], comps[0][2]
                if (hs, vs) not in JPEG_SAMPLINGS or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                    raise NotImplementedError("JPEG: sampling %s (luma 1x1, 2x1 or 2x2 with chroma 1x1)"
                                              % ", ".join("%dx%d" % (c[1], c[2]) for c in comps))
            frame = dict(w=w, h=h, ncomp=nc, hs=hs, vs=vs, ids=[c[0] for c in comps], tq=[c[3] for c in comps])
        elif 0xC2 <= m <= 0xCF and m != 0xC8:           # C4 was taken above; CC is DAC
            raise NotImplementedError("JPEG: %s (Huffman sequential files only)"
                                      % {0xC2: "progressive", 0xCC: "arithmetic coding"}.get(m, "frame type SOF%d" % (m - 0xC0)))
        elif m == 0xDA:                                 # SOS
            if frame is None:
                raise ValueError("JPEG: scan before the frame header")
            ns = data[seg] if ln >= 3 else 0
            if ns < 1 or ns > 4 or ln != 6 + 2 * ns:
                raise ValueError("JPEG: bad scan header")
            if ns != frame["ncomp"] or any(data[seg + 1 + 2 * i] != frame["ids"][i] for i in range(ns)):
                raise NotImplementedError("JPEG: a scan that does not interleave all components in frame order")
            tabs = [(data[seg + 2 + 2 * i] >> 4, data[seg + 2 + 2 * i] & 15) for i in range(ns)]
            if data[seg + 1 + 2 * ns] != 0 or data[seg + 2 + 2 * ns] != 63 or data[seg + 3 + 2 * ns] != 0:
                raise ValueError("JPEG: bad scan header")
            for i, (td, ta) in enumerate(tabs):
                if td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff or frame["tq"][i] not in qt:
                    raise ValueError("JPEG: the scan names a table that was not defined")
            w, h, hs, vs = frame["w"], frame["h"], frame["hs"], frame["vs"]
            mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
            grids = [(mx * hs, my * vs)] + [(mx, my)] * (frame["ncomp"] - 1)      # (blocks per row, block rows)
            blocks = sum(a * b for a, b in grids)
            if blocks > 4 * (n - end):                  # a block takes two bits at the least
                raise ValueError("JPEG: truncated scan")
            frame.update(mx=mx, my=my, grids=grids, blocks=blocks, restart=restart, scan=end,
                         dc=[huff[(0, t[0])] for t in tabs], ac=[huff[(1, t[1])] for t in tabs],
                         q=[qt[t] for t in frame["tq"]])
            return frame
        pos = end


def _jpeg_coefficients_py(data, f):
    """The entropy decode in Python: int16 [blocks, 64], de-zigzagged, not dequantised; component by component, block-row
    major."""
    n, pos = len(data), f["scan"]
    out = np.zeros((f["blocks"], 64), np.int16)
    acc = nbits = 0

    def bit():
        nonlocal pos, acc, nbits
        if nbits == 0:
            if pos >= n:
                raise ValueError("JPEG: truncated scan")
            acc = data[pos]
            pos += 1
            if acc == 0xFF:
                if pos >= n or data[pos] != 0:
                    raise ValueError("JPEG: truncated scan (marker in the entropy-coded data)")
                pos += 1
            nbits = 8
        nbits -= 1
        return (acc >> nbits) & 1

    def symbol(table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise ValueError("JPEG: bad Huffman code")

    def receive(s):
        v = 0
        for _ in range(s):
            v = (v << 1) | bit()
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

    hs, vs, mx, my, nc = f["hs"], f["vs"], f["mx"], f["my"], f["ncomp"]
    base, b0 = [], 0
    for bw, bh in f["grids"]:
        base.append(b0)
        b0 += bw * bh
    pred, rst = [0] * nc, 0
    for mcu in range(mx * my):
        if f["restart"] and mcu and mcu % f["restart"] == 0:
            nbits = 0                                   # the marker is byte aligned
            if pos + 2 > n or data[pos] != 0xFF or data[pos + 1] != 0xD0 + rst:
                raise ValueError("JPEG: restart marker %d expected" % rst)
            pos += 2
            rst = (rst + 1) & 7
            pred = [0] * nc
        mr, mc = divmod(mcu, mx)
        for c in range(nc):
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            for by in range(cv):
                for bx in range(ch):
                    blk = out[base[c] + (mr * cv + by) * f["grids"][c][0] + mc * ch + bx]
                    s = symbol(f["dc"][c])
                    if s > 11:
                        raise ValueError("JPEG: bad DC category")
                    if s:
                        pred[c] += receive(s)
                    if not -32768 <= pred[c] <= 32767:
                        raise ValueError("JPEG: DC value out of range")
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = symbol(f["ac"][c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63 or s > 10:
                            raise ValueError("JPEG: bad AC coefficient")
                        blk[JPEG_ZIGZAG[k]] = receive(s)
                        k += 1
    while pos < n and data[pos] == 0xFF and pos + 1 < n and data[pos + 1] == 0xFF:
        pos += 1
    if pos + 2 > n or data[pos] != 0xFF or data[pos + 1] != 0xD9:
        raise ValueError("JPEG: no end-of-image marker after the scan")
    return out


def jpeg_entropy_decode(data, use_lib=True):
    """JPEG bytes -> ``(info, coef)``: ``info`` the header (w, h, ncomp, hs, vs, grids = per component (blocks per row,
    block rows), q = per component the int32 [64] quantisation table in natural order, blocks) and ``coef`` int16
    [blocks, 64].  The C helper of libbiggan_hip.so does the work (host code, no GPU involved); without the library, or
    with ``use_lib=False``, the Python decoder does."""
    data = bytes(data)
    if use_lib:
        try:
            from . import hip
            L = hip.lib()
        except ImportError:                             # library not built: pure-Python fallback (slow)
            L = None
        if L is not None:
            def call(rc):
                if rc == 3:                             # BG_ERR_UNSUPPORTED
                    raise NotImplementedError(L.bg_last_error().decode())
                if rc != 0:
                    raise ValueError(L.bg_last_error().decode())
            hdr = hip.BgJpegInfo()
            call(L.bg_jpeg_info(data, len(data), hip.byref(hdr)))
            nc = hdr.ncomp
            info = dict(w=hdr.width, h=hdr.height, ncomp=nc, hs=hdr.hs, vs=hdr.vs, blocks=int(hdr.blocks),
                        grids=[(hdr.bw[c], hdr.bh[c]) for c in range(nc)],
                        q=[np.array(hdr.q[c][:], np.int32) for c in range(nc)])
            coef = np.empty((info["blocks"], 64), np.int16)
            call(L.bg_jpeg_coefficients(data, len(data), coef.ctypes.data_as(hip.c_void_p), coef.size))
            return info, coef
    f = _jpeg_parse(data)
    info = {k: f[k] for k in ("w", "h", "ncomp", "hs", "vs", "blocks", "grids", "q")}
    return info, _jpeg_coefficients_py(data, f)


def _fix(x):
    return np.int32(round(x * 8192))


def _idct_pass(v, shift):
    """libjpeg's slow-integer butterfly on eight int32 arrays; int32 arithmetic that wraps like the device's."""
    in0, in1, in2, in3, in4, in5, in6, in7 = v
    z1 = (in2 + in6) * _fix(0.541196100)
    t2 = z1 - in6 * _fix(1.847759065)
    t3 = z1 + in2 * _fix(0.765366865)
    t0 = (in0 + in4) * np.int32(8192)
    t1 = (in0 - in4) * np.int32(8192)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = in7, in5, in3, in1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * _fix(1.175875602)
    a = a * _fix(0.298631336)
    b = b * _fix(2.053119869)
    c = c * _fix(3.072711026)
    d = d * _fix(1.501321110)
    z1 = z1 * -_fix(0.899976223)
    z2 = z2 * -_fix(2.562915447)
    z3 = z3 * -_fix(1.961570560) + z5
    z4 = z4 * -_fix(0.390180644) + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    r = np.int32(1 << (shift - 1))
    return [(x + r) >> shift for x in (t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d)]


def jpeg_planes(info, coef):
    """Dequantisation and inverse DCT: per component the uint8 plane [block rows * 8, blocks per row * 8] (whole MCUs)."""
    planes, b0 = [], 0
    with np.errstate(over="ignore"):
        for (bw, bh), q in zip(info["grids"], info["q"]):
            blk = coef[b0:b0 + bw * bh].astype(np.int32).reshape(-1, 8, 8) * q.astype(np.int32).reshape(1, 8, 8)
            b0 += bw * bh
            ws = np.stack(_idct_pass([blk[:, k, :] for k in range(8)], 11), axis=1)        # pass 1: columns
            px = np.stack(_idct_pass([ws[:, :, k] for k in range(8)], 18), axis=2)         # pass 2: rows
            px = np.clip(px + 128, 0, 255).astype(np.uint8)
            planes.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return planes


def _jpeg_upsample(p, hs, vs):
    """libjpeg's "fancy" (triangle) upsampling of a cropped chroma plane by hs x vs; the neighbour of an edge sample is
    the sample itself, which is what its edge rules amount to."""
    p = p.astype(np.int32)
    if (hs, vs) == (1, 1):
        return p
    ch, cw = p.shape
    left, right = np.maximum(np.arange(cw) - 1, 0), np.minimum(np.arange(cw) + 1, cw - 1)
    out = np.empty((ch * vs, cw * 2), np.int32)
    if vs == 1:
        out[:, 0::2] = (3 * p + p[:, left] + 1) >> 2
        out[:, 1::2] = (3 * p + p[:, right] + 2) >> 2
        return out
    up, down = np.maximum(np.arange(ch) - 1, 0), np.minimum(np.arange(ch) + 1, ch - 1)
    r = np.empty((ch * 2, cw), np.int32)
    r[0::2] = 3 * p + p[up]
    r[1::2] = 3 * p + p[down]
    out[:, 0::2] = (3 * r + r[:, left] + 8) >> 4
    out[:, 1::2] = (3 * r + r[:, right] + 7) >> 4
    return out


def _jfix(x):
    return int(x * 65536 + 0.5)


def jpeg_pixels(info, planes, channels):
    """Crop, upsample, colour transform and ``channels``: uint8 [h, w, channels]."""
    w, h, hs, vs = info["w"], info["h"], info["hs"], info["vs"]
    y = planes[0][:h, :w]
    if channels == 1 or info["ncomp"] == 1:
        return np.repeat(y[:, :, None], channels, axis=2)
    cw, ch = -(-w // hs), -(-h // vs)
    cb = _jpeg_upsample(planes[1][:ch, :cw], hs, vs)[:h, :w] - 128
    cr = _jpeg_upsample(planes[2][:ch, :cw], hs, vs)[:h, :w] - 128
    y = y.astype(np.int32)
    r = y + ((_jfix(1.402) * cr + 32768) >> 16)
    b = y + ((_jfix(1.772) * cb + 32768) >> 16)
    g = y + ((-_jfix(0.34414) * cb + 32768 - _jfix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode_jpeg(data, channels=3, use_lib=True):
    """tf.image.decode_jpeg(contents, channels) with its defaults (slow-integer DCT, fancy upscaling): uint8
    [H, W, channels], channels 1 or 3.  A grey file at channels=3 replicates Y; a colour file at channels=1 is its Y
    plane (libjpeg's greyscale output).  8-bit Huffman sequential files with 1 or 3 components, luma sampling 1x1, 2x1
    or 2x2 with chroma 1x1, one interleaved scan, restart intervals; progressive, arithmetic-coded, 12-bit, four-component
    files and other samplings raise NotImplementedError, malformed data ValueError."""
    if channels not in (1, 3):
        raise ValueError("decode_jpeg: channels must be 1 or 3 (JPEG has no alpha)")
    info, coef = jpeg_entropy_decode(data, use_lib)
    return jpeg_pixels(info, jpeg_planes(info, coef), channels)


def decode_image(data, channels=3):
    """tf.image.decode_image: dispatch on the magic bytes (JPEG, PNG)."""
    if data[:2] == b"\xff\xd8":
        return decode_jpeg(data, channels)
    if data[:8] == b"\x89PNG\r\n\x1a\n":
        return decode_png(data, channels)
    raise ValueError("neither a PNG nor a JPEG file")


def resize_bilinear_legacy(img, size):
    """tf.image.resize_images(img, [size, size]) of TF 1.x: bilinear, align_corners=False, no half-pixel
    centres: source coordinate = destination index * (in / out)."""
    img = np.asarray(img, np.float32)
    H, W = img.shape[:2]

    def axis(n_in, n_out):
        src = np.arange(n_out, dtype=np.float32) * (n_in / float(n_out))
        lo = np.floor(src).astype(np.int64)
        hi = np.minimum(lo + 1, n_in - 1)
        return lo, hi, (src - lo).astype(np.float32)
    y0, y1, fy = axis(H, size)
    x0, x1, fx = axis(W, size)
    top = img[y0][:, x0] * (1 - fx)[None, :, None] + img[y0][:, x1] * fx[None, :, None]
    bot = img[y1][:, x0] * (1 - fx)[None, :, None] + img[y1][:, x1] * fx[None, :, None]
    return top * (1 - fy)[:, None, None] + bot * fy[:, None, None]


# ------------------------------------------------------------------------------------------
# utils.py:12-121
# ------------------------------------------------------------------------------------------
class ImageData:
    """utils.py:12-38."""

    def __init__(self, load_size, channels, custom_dataset, flip, seed=0):
        self.load_size = load_size
        self.channels = channels
        self.custom_dataset = custom_dataset
        self.flip = flip
        self.rng = np.random.default_rng(seed)
        self._lock = threading.Lock()                   # image_processing runs on the loader's decode threads

    def image_processing(self, filename):
        if not self.custom_dataset:
            x_decode = np.asarray(filename)             # in-memory dataset: the array itself
        elif str(filename).endswith(".npy"):
            x_decode = np.load(filename)
        else:
            with open(filename, "rb") as f:
                x_decode = decode_image(f.read(), channels=self.channels)
        img = resize_bilinear_legacy(x_decode, self.load_size)
        if self.flip:                                    # tf.image.random_flip_left_right
            with self._lock:
                flip = self.rng.random() < 0.5
            if flip:
                img = img[:, ::-1]
        return (img / 127.5 - 1).astype(np.float32)

    def image_processing_with_labels(self, filename, label):
        return self.image_processing(filename), np.asarray(label, np.float32)


def read_labels(path):
    """utils.py:41-51: tab-separated ``filename  tag tag ...``."""
    labels = {}
    with open(path, 'r') as csvFile:
        reader = csv.reader(csvFile, delimiter='\t', quotechar='"')
        for row in reader:
            filename = row.pop(0)
            labels[filename] = list(map(float, row))
    return labels


def read_weights(path):
    """A weight file has the label file's format; the first value of a row is that file's weight (utils.py:72-77)."""
    return {name: row[0] for name, row in read_labels(path).items()}


def load_data(dataset_name, label_file, weight_file=None, ignore_missing=False, n_labels=None, root="./dataset"):
    """utils.py:79-121 (custom datasets).  ``weight_file`` (utils.py:88-106): every file is listed ``int(w)`` times, a
    file the weight file does not name once.  The reference's probabilistic rounding of the fractional part is guarded
    by ``float(w) != w`` on a float and never runs: 2.7 gives two copies, 0.5 drops the file, and so it is here."""
    if dataset_name in ('mnist', 'cifar10'):
        raise NotImplementedError("dataset '%s' is a Keras download in the reference; no network here" % dataset_name)
    x = sorted(glob(os.path.join(root, dataset_name, '*.*')))
    if weight_file:
        weights = read_weights(weight_file)
        new_x = []
        for full in x:
            new_x.extend([full] * int(weights.get(os.path.basename(full), 1.0)))
        x = new_x
    if label_file:
        labels = read_labels(label_file)
        used_labels = []
        for full in x:
            fn = os.path.basename(full)
            if fn not in labels:
                if ignore_missing:
                    used_labels.append([0.0] * n_labels)
                else:
                    raise RuntimeError("No label found for file " + fn)
            else:
                used_labels.append(labels[fn])
    else:
        used_labels = None
    return x, used_labels


# ------------------------------------------------------------------------------------------
# device-side preprocessing: the host decodes and packs, bg_image_batch_u8 does the rest
# ------------------------------------------------------------------------------------------
RAW_ALIGN = 16                                          # every image of a packed batch starts on a 16-byte boundary
# BgImageEntry of include/biggan_hip.h: 32 bytes, shipped as int32 [n, 8]
TABLE_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("flip", "<i4"), ("scale_y", "<f4"),
                        ("scale_x", "<f4"), ("reserved", "<i4")])


# BgJpegEntry of include/biggan_hip.h: 480 bytes, shipped as int32 [n_jpeg, 120]
JPEG_COMP_DTYPE = np.dtype([("coef", "<i8"), ("bw", "<i4"), ("bh", "<i4")])
JPEG_TABLE_DTYPE = np.dtype([("slot", "<i8"), ("w", "<i4"), ("h", "<i4"), ("channels", "<i4"), ("ncomp", "<i4"),
                             ("hs", "<i4"), ("vs", "<i4"), ("block0", "<i4"), ("image", "<i4"), ("reserved", "<i4", (2,)),
                             ("comp", JPEG_COMP_DTYPE, (3,)), ("q", "<u2", (3, 64))])
assert TABLE_DTYPE.itemsize == 32 and JPEG_TABLE_DTYPE.itemsize == 480


class JpegImage:
    """An entropy-decoded JPEG file on its way to the device: the header (``jpeg_entropy_decode``) and the int16
    coefficients [blocks, 64].  ``shape`` / ``size`` are those of the pixels it decodes to; ``decode()`` finishes it on
    the host with the arithmetic bg_jpeg_batch_u8 would use."""

    def __init__(self, info, coef, channels):
        if channels not in (1, 3):
            raise ValueError("decode_jpeg: channels must be 1 or 3 (JPEG has no alpha)")
        self.info, self.coef, self.channels = info, coef, channels
        self.shape = (info["h"], info["w"], channels)
        self.size = info["h"] * info["w"] * channels
        self.upload_bytes = coef.nbytes + JPEG_TABLE_DTYPE.itemsize

    def decode(self):
        return jpeg_pixels(self.info, jpeg_planes(self.info, self.coef), self.channels)


def packable(img, channels):
    """True for what ``pack_batch`` takes: a uint8 array [h, w, channels] with h, w >= 1, or a ``JpegImage`` of as many
    channels."""
    if isinstance(img, JpegImage):
        return img.channels == channels
    return (isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == channels
            and img.shape[0] >= 1 and img.shape[1] >= 1)


def upload_bytes(img):
    """Bytes of a decoded image that cross the bus on the device path: its slot, or a JPEG's coefficients and entry."""
    return img.upload_bytes if isinstance(img, JpegImage) else -(-img.size // RAW_ALIGN) * RAW_ALIGN


def switch_bytes(images):
    """The uploaded bytes of a batch as ``device_path_pays`` is to count them: a JPEG's bytes weigh RAW_OVER_OUT_MAX /
    JPEG_OVER_OUT_MAX of a decoded image's, so that the one rule holds both thresholds in a mixed batch."""
    return sum(upload_bytes(a) * (RAW_OVER_OUT_MAX / JPEG_OVER_OUT_MAX if isinstance(a, JpegImage) else 1.0)
               for a in images)


def pack_batch(images, flips, size, channels=None, pin=False):
    """Decoded images (uint8 [h, w, C] arrays, sizes may differ) -> ``(raw, table, geom)`` for
    ``functional.image_batch_u8``: ``raw`` uint8 [raw_bytes] with image i at ``geom["offsets"][i]`` (a multiple of 16,
    padding zeroed), ``table`` int32 [n, 8] (``TABLE_DTYPE``: offset, h, w, flip, and the two scales
    ``float32(n_in / size)`` of ``resize_bilinear_legacy``), ``geom`` the validated geometry.  ``pin``: pinned host
    tensors (the target is a GPU).  ``channels`` defaults to the first image's.  Raises ValueError for anything else.

    A ``JpegImage`` gets a slot and a table entry like any other image, but its slot arrives empty (zeroed):
    ``geom["jpeg"]`` (None without JPEG images) holds what ``functional.jpeg_batch_u8`` fills it from: ``coef`` int16
    [64 * blocks], the images' coefficients back to back, ``table`` int32 [n_jpeg, 120] (``JPEG_TABLE_DTYPE``: slot, w, h,
    channels, ncomp, luma sampling, first block, index in ``table``, per component coefficient offset and block grid,
    quantisation tables), ``n``, ``blocks``, ``max_pixels`` and ``images`` (their indices in the batch)."""
    images = list(images)
    if not images:
        raise ValueError("pack_batch: no images")
    if len(flips) != len(images):
        raise ValueError("pack_batch: %d flips for %d images" % (len(flips), len(images)))
    if size < 1:
        raise ValueError("pack_batch: size %d" % size)
    if channels is None:
        channels = images[0].shape[2] if isinstance(images[0], (np.ndarray, JpegImage)) and len(images[0].shape) == 3 else 0
    if channels not in (1, 3, 4):
        raise ValueError("pack_batch: %s channels (1, 3 or 4)" % (channels,))
    table = np.zeros(len(images), TABLE_DTYPE)
    pos = 0
    for i, img in enumerate(images):
        if not packable(img, channels):
            raise ValueError("pack_batch: image %d is %s %s, expected uint8 [h, w, %d]"
                             % (i, getattr(img, "dtype", type(img).__name__), getattr(img, "shape", ""), channels))
        h, w = img.shape[:2]
        table[i] = (pos, h, w, 1 if flips[i] else 0, np.float32(h / float(size)), np.float32(w / float(size)), 0)
        pos += -(-(h * w * channels) // RAW_ALIGN) * RAW_ALIGN
    raw = torch.empty(pos, dtype=torch.uint8, pin_memory=bool(pin))
    view = raw.numpy()
    for e, img in zip(table, images):
        off, nb = int(e["offset"]), img.size
        if isinstance(img, JpegImage):
            view[off:off + -(-nb // RAW_ALIGN) * RAW_ALIGN] = 0
            continue
        view[off:off + nb] = img.reshape(-1)
        view[off + nb:off + -(-nb // RAW_ALIGN) * RAW_ALIGN] = 0
    jpeg = _pack_jpegs(images, table, channels, pin)
    tab = torch.from_numpy(table.view("<i4").reshape(len(images), 8))
    if pin:
        tab = tab.pin_memory()
    geom = dict(n=len(images), size=int(size), channels=int(channels), raw_bytes=int(pos),
                offsets=[int(o) for o in table["offset"]], shapes=[tuple(img.shape[:2]) for img in images], jpeg=jpeg)
    return raw, tab, geom


def _pack_jpegs(images, table, channels, pin):
    """The coefficient buffer and the per-JPEG table of ``pack_batch`` (None without a ``JpegImage``), validated here:
    the kernel checks every entry again, but a header that does not add up is an error of the host."""
    which = [i for i, img in enumerate(images) if isinstance(img, JpegImage)]
    if not which:
        return None
    jt = np.zeros(len(which), JPEG_TABLE_DTYPE)
    block0 = 0
    for e, i in zip(jt, which):
        img, info = images[i], images[i].info
        w, h, hs, vs, nc = info["w"], info["h"], info["hs"], info["vs"], info["ncomp"]
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        grids = [(mx * hs, my * vs)] + [(mx, my)] * (nc - 1)
        if (nc not in (1, 3) or (hs, vs) not in JPEG_SAMPLINGS or (nc == 1 and (hs, vs) != (1, 1))
                or [tuple(g) for g in info["grids"]] != grids or len(info["q"]) != nc
                or img.coef.dtype != np.int16 or img.coef.shape != (sum(a * b for a, b in grids), 64)):
            raise ValueError("pack_batch: image %d: the JPEG header and its coefficients do not agree" % i)
        e["slot"], e["w"], e["h"], e["channels"], e["ncomp"] = table[i]["offset"], w, h, channels, nc
        e["hs"], e["vs"], e["block0"], e["image"] = hs, vs, block0, i
        for c, (bw, bh) in enumerate(grids):
            e["comp"][c] = (64 * block0, bw, bh)
            e["q"][c] = info["q"][c]
            block0 += bw * bh
    if block0 >= 2 ** 31 - 64:
        raise ValueError("pack_batch: %d JPEG blocks in one batch" % block0)
    coef = torch.empty(64 * block0, dtype=torch.int16, pin_memory=bool(pin))
    cv = coef.numpy()
    for e, i in zip(jt, which):
        c0 = 64 * int(e["block0"])
        cv[c0:c0 + images[i].coef.size] = images[i].coef.reshape(-1)
    tab = torch.from_numpy(jt.view("<i4").reshape(len(which), 120))
    if pin:
        tab = tab.pin_memory()
    return dict(coef=coef, table=tab, n=len(which), blocks=int(block0), images=which,
                max_pixels=max(images[i].info["w"] * images[i].info["h"] for i in which))


def device_input_enabled(device, option=None):
    """The loader's ``device_preprocess`` switch: None = on for a GPU unless the environment says BG_DEVICE_INPUT=0."""
    if torch.device(device).type != "cuda":
        return False
    if option is None:
        return os.environ.get("BG_DEVICE_INPUT", "1") != "0"
    return bool(option)


RAW_OVER_OUT_MAX = 1.0      # the automatic switch packs a batch only while its uint8 bytes are at most its fp32 bytes
# ... and a batch of JPEG files while its coefficients and entries are at most 40 x its fp32 bytes: what the device path
# saves there is the host's IDCT, upsampling and colour, which cost per SOURCE pixel as the upload does.  Measured
# (JPEG input): 7 - 20 x the host path at uploaded / out = 0.39, 0.78, 4, 8, 16 and 32, with no trend towards
# a crossing; past the last measured point the host path is kept.
JPEG_OVER_OUT_MAX = 40.0


def device_path_pays(raw_bytes, n, size, channels):
    """The per-batch rule of the automatic switch: packing and uploading ``raw_bytes`` of decoded pixels is serial work
    of the worker thread, the host resize it replaces is spread over the decode pool and costs per OUTPUT pixel.
    Measured: at raw / out = 0.39 (160^2 -> 128^2) the device path is 1.5 - 2x the host path, at 4.0
    (512^2 -> 128^2) the host path is up to 2x the device path; interpolated in log-log the two cross at ~1.0, which
    is also where the upload stops being smaller than the fp32 batch."""
    return raw_bytes <= RAW_OVER_OUT_MAX * (n * size * size * channels * 4)


def decode_file(image_data, filename, entropy_only=False):
    """The decode step of ``ImageData.image_processing`` alone.  ``entropy_only``: a JPEG file that the device path can
    take (1 or 3 channels) comes back as a ``JpegImage``, entropy-decoded only."""
    if not image_data.custom_dataset:
        return np.asarray(filename)
    if str(filename).endswith(".npy"):
        return np.load(filename)
    with open(filename, "rb") as f:
        data = f.read()
    if entropy_only and data[:2] == b"\xff\xd8" and image_data.channels in (1, 3):
        return JpegImage(*jpeg_entropy_decode(data), channels=image_data.channels)
    return decode_image(data, channels=image_data.channels)


def finish_on_host(x_decode, size, flip):
    """What follows the decode in ``ImageData.image_processing``, with the flip already drawn."""
    img = resize_bilinear_legacy(x_decode, size)
    if flip:
        img = img[:, ::-1]
    return (img / 127.5 - 1).astype(np.float32)


def finish_decode(x):
    """The pixels of what ``decode_file`` returned."""
    return x.decode() if isinstance(x, JpegImage) else x


class PackedBatch:
    """One batch on its way to ``functional.image_batch_u8``: pinned ``raw`` and ``table`` plus the geometry."""

    def __init__(self, raw, table, geom):
        self.raw, self.table, self.geom = raw, table, geom

    def upload(self, device):
        """``(raw, table)`` on the device, the JPEG slots of raw filled: the decoded uint8 pixels of every image."""
        from . import functional as Fn
        g = self.geom
        with torch.cuda.device(device):                 # the kernel goes to the current stream of the current device
            raw = self.raw.to(device, non_blocking=True)
            table = self.table.to(device, non_blocking=True)
            j = g.get("jpeg")
            if j is not None:                           # fills the JPEG slots of raw from their coefficients
                Fn.jpeg_batch_u8(j["coef"].to(device, non_blocking=True), j["table"].to(device, non_blocking=True),
                                 j["n"], j["blocks"], j["max_pixels"], raw, table, g["n"])
            return raw, table

    def to_device(self, device):
        from . import functional as Fn
        g = self.geom
        with torch.cuda.device(device):
            raw, table = self.upload(device)
            return Fn.image_batch_u8(raw, table, g["n"], g["size"], g["channels"])


# ------------------------------------------------------------------------------------------
# device-resident dataset: decode every file once, keep it on the GPU, gather batches by index (csrc/dataset.hip)
# ------------------------------------------------------------------------------------------
# BgDatasetEntry of include/biggan_hip.h: 32 bytes, shipped as int32 [n_entries, 8]
ENTRY_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("kind", "<i4"), ("scale_y", "<f4"),
                        ("scale_x", "<f4"), ("reserved", "<i4")])
assert ENTRY_DTYPE.itemsize == 32
KIND_U8, KIND_F32 = 0, 1    # the cached form of an image: its decoded uint8 pixels [h,w,C] / the finished fp32 [S,S,C]
CACHE_DEPTH = 4             # scratch arenas for images past the budget: one per slot of the loader's queue


def dataset_cache_bytes(device, option=None):
    """The loader's ``cache_bytes`` switch resolved to the byte budget of the arena; 0 is off.  None reads
    BG_DEVICE_DATASET_GB (GiB, a float; unset, empty or 0: off); a device that is not a GPU is always off."""
    if torch.device(device).type != "cuda":
        return 0
    if option is None:
        text = os.environ.get("BG_DEVICE_DATASET_GB", "").strip()
        if not text:
            return 0
        gib = float(text)
        if not 0 <= gib < float("inf"):
            raise ValueError("BG_DEVICE_DATASET_GB=%s: a budget in GiB, 0 or more" % text)
        return int(gib * (1 << 30))
    if option < 0:
        raise ValueError("cache_bytes %r: 0 or more" % (option,))
    return int(option)


def _align(n):
    return -(-int(n) // RAW_ALIGN) * RAW_ALIGN


def _jpeg_frame(data):
    """The marker walk up to the frame header: ``(h, w, components)``, None for what ``decode_jpeg`` would refuse, or
    "more" when ``data`` (a prefix of the file) ends before the frame header."""
    n, pos = len(data), 2
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    while True:
        if pos + 2 > n:
            return "more"
        if data[pos] != 0xFF:
            return None
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD9, 0x00, 0xDA) or (0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8)):
            return None                                 # no frame header before the scan, or not Huffman sequential
        if pos + 2 > n:
            return "more"
        ln = (data[pos] << 8) | data[pos + 1]
        if ln < 2:
            return None
        if m in (0xC0, 0xC1):
            if pos + 8 > n:
                return "more"
            prec, h, w, nc = data[pos + 2], (data[pos + 3] << 8) | data[pos + 4], (data[pos + 5] << 8) | data[pos + 6], data[pos + 7]
            if prec != 8 or h < 1 or w < 1 or nc not in (1, 3):
                return None
            return h, w, nc
        pos += ln


HEADER_PREFIX = 4096                                    # bytes of a file that the planner reads first


def image_header(image_data, filename):
    """``(h, w, channels)`` of what ``decode_file`` would return, from the file's header alone: the IHDR chunk of a PNG
    file, the markers up to the frame header of a JPEG file, the header of an ``.npy`` file.  None for a file that the
    dataset cache cannot hold (an array that is not uint8 [h, w, channels], a channel count that ``packable`` refuses,
    a file that the decoders refuse)."""
    C = image_data.channels
    if not image_data.custom_dataset or C not in (1, 3, 4):
        return None
    if str(filename).endswith(".npy"):
        with open(filename, "rb") as f:
            try:
                major, _ = np.lib.format.read_magic(f)
                read = np.lib.format.read_array_header_1_0 if major == 1 else np.lib.format.read_array_header_2_0
                shape, _, dtype = read(f)
            except ValueError:
                return None
        if dtype != np.uint8 or len(shape) != 3 or shape[2] != C or shape[0] < 1 or shape[1] < 1:
            return None
        return int(shape[0]), int(shape[1]), C
    with open(filename, "rb") as f:
        data = f.read(HEADER_PREFIX)
        if data[:2] == b"\xff\xd8":
            frame = _jpeg_frame(data)
            if frame == "more":
                frame = _jpeg_frame(data + f.read())
            if frame is None or frame == "more" or C not in (1, 3):
                return None
            return frame[0], frame[1], C
    if data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) >= 33 and data[12:16] == b"IHDR":
        w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", data[16:29])
        if depth != 8 or interlace != 0 or ctype not in (0, 2, 3, 4, 6) or h < 1 or w < 1:
            return None
        return int(h), int(w), C
    return None


def entry_kind(h, w, size):
    """The cached form with fewer bytes, by the comparison ``device_path_pays`` makes (RAW_OVER_OUT_MAX = 1.0): the uint8
    source while its bytes are at most those of the finished fp32 image."""
    return KIND_U8 if h * w <= 4 * RAW_OVER_OUT_MAX * size * size else KIND_F32


class EntryPlan:
    """What ``plan_entries`` returns; see there."""


def plan_entries(shapes, size, channels, budget, batch_size=0, depth=CACHE_DEPTH, force_kind=None):
    """The arena layout for images of ``shapes`` [(h, w), ...] in cache order.  Pure host arithmetic:

    kinds        per image, ``entry_kind`` (or ``force_kind`` for all)
    nbytes       per image, the bytes of its cached form: h * w * C, or 4 * S * S * C
    n_cached     the longest prefix whose 16-byte aligned slots fit ``budget`` bytes; later images are never cached
    offsets      per image, the arena offset of its slot (a multiple of 16), -1 past the prefix
    cached_bytes the end of the prefix = the start of the scratch tail
    slot_bytes   the largest aligned slot of an image past the prefix (0 without one); the scratch tail is ``depth``
                 arenas of ``batch_size`` such slots, so that any batch finds room for all its uncached images
    arena_bytes  cached_bytes + depth * batch_size * slot_bytes (at least 16)
    table        ENTRY_DTYPE [n + depth * batch_size] (just [n] without a scratch tail): rows of cached images are final,
                 rows of uncached images stay zero (h = 0: refused by the kernel), scratch rows are written per batch"""
    S, C = int(size), int(channels)
    if S < 1 or C not in (1, 3, 4):
        raise ValueError("plan_entries: size %s, channels %s" % (size, channels))
    if force_kind not in (None, KIND_U8, KIND_F32):
        raise ValueError("plan_entries: force_kind %r" % (force_kind,))
    n = len(shapes)
    p = EntryPlan()
    p.size, p.channels, p.depth, p.batch_size, p.n = S, C, int(depth), int(batch_size), n
    p.shapes = [(int(h), int(w)) for h, w in shapes]
    if any(h < 1 or w < 1 for h, w in p.shapes):
        raise ValueError("plan_entries: an image without pixels")
    p.kinds = np.array([entry_kind(h, w, S) if force_kind is None else force_kind for h, w in p.shapes], np.int32)
    p.nbytes = np.array([h * w * C if k == KIND_U8 else 4 * S * S * C for (h, w), k in zip(p.shapes, p.kinds)], np.int64)
    ends = np.cumsum([_align(b) for b in p.nbytes]) if n else np.zeros(0, np.int64)
    p.n_cached = int(np.searchsorted(ends, int(budget), side="right"))
    p.cached_bytes = int(ends[p.n_cached - 1]) if p.n_cached else 0
    p.offsets = np.full(n, -1, np.int64)
    p.offsets[:p.n_cached] = np.concatenate([[0], ends[:p.n_cached]])[:p.n_cached]
    p.slot_bytes = max((_align(b) for b in p.nbytes[p.n_cached:]), default=0)
    rows = p.depth * p.batch_size if p.slot_bytes else 0
    if p.slot_bytes and p.batch_size < 1:
        raise ValueError("plan_entries: images past the budget need batch_size for the scratch tail")
    p.scratch_bytes = p.batch_size * p.slot_bytes       # of one of the depth scratch arenas
    p.arena_bytes = max(p.cached_bytes + p.depth * p.scratch_bytes, RAW_ALIGN)
    p.table = np.zeros(n + rows, ENTRY_DTYPE)
    for i in range(p.n_cached):
        p.table[i] = entry_row(p, i, p.offsets[i])
    return p


def entry_row(p, i, offset):
    """The BgDatasetEntry of image ``i`` of a plan at ``offset``."""
    h, w = p.shapes[i]
    if p.kinds[i] == KIND_F32:
        return (offset, p.size, p.size, KIND_F32, 0.0, 0.0, 0)
    return (offset, h, w, KIND_U8, np.float32(h / float(p.size)), np.float32(w / float(p.size)), 0)


def plan_dataset(files, image_data, budget, batch_size, pool=None, force_kind=None, depth=CACHE_DEPTH):
    """The plan of the dataset cache for a file list, or None when a file cannot be cached by its header (the cache is
    then off for the whole dataset).  Reads only the headers of the unique files (``image_header``, in ``pool``): a path
    that ``--weight_file`` lists several times is one entry, and entries are numbered in first-occurrence order.
    Returns ``plan_entries``' plan with ``files`` (the unique paths), ``entry_of`` (int64 [len(files)]: file list index
    -> entry).  Returns ``(plan, None)``, or ``(None, name)`` with the first file that did not fit."""
    first, entry_of = {}, np.empty(len(files), np.int64)
    for i, f in enumerate(files):
        entry_of[i] = first.setdefault(str(f) if image_data.custom_dataset else id(f), len(first))
    unique = [None] * len(first)
    for i, f in enumerate(files):
        if unique[entry_of[i]] is None:
            unique[entry_of[i]] = f
    heads = list((pool.map if pool is not None else map)(lambda f: image_header(image_data, f), unique))
    for f, hd in zip(unique, heads):
        if hd is None:
            return None, (str(f) if image_data.custom_dataset else "an in-memory array")
    p = plan_entries([hd[:2] for hd in heads], image_data.load_size, image_data.channels, budget, batch_size, depth,
                     force_kind)
    p.files, p.entry_of = unique, entry_of
    return p, None


class CachedBatch:
    """One batch of the dataset cache on its way to ``functional.dataset_batch``: the staged images that the arena does
    not hold yet (``stages``: per source buffer its kind, the pinned host data and the int64 [m,4] copy segments),
    the scratch rows of the entry table for images past the budget, and ``sel`` int32 [n,2] (entry row, flip)."""

    def __init__(self, cache, stages, rows, sel):
        self.cache, self.stages, self.rows, self.sel = cache, stages, rows, sel

    def to_device(self, device):
        from . import functional as Fn
        c, p = self.cache, self.cache.plan
        with torch.cuda.device(device):                 # everything goes to the current stream of the current device
            for kind, host, segs in self.stages:
                if kind == KIND_U8:
                    src = host.upload(device)[0]        # the decoded uint8 pixels, JPEG slots filled on the device
                elif isinstance(host, PackedBatch):
                    src = host.to_device(device)        # fp32 [m,S,S,C], flips 0: resized and normalised on the device
                else:
                    src = host.to(device, non_blocking=True)
                Fn.dataset_store(src, segs.to(device, non_blocking=True), c.arena)
            if self.rows is not None:
                row0, piece = self.rows
                c.table[row0:row0 + piece.shape[0]].copy_(piece, non_blocking=True)
            sel = self.sel.to(device, non_blocking=True)
            return Fn.dataset_batch(c.arena, c.table, sel, sel.shape[0], p.size, p.channels)


class DatasetCache:
    """The device-resident dataset of a ``BatchLoader``: one uint8 arena of exactly the planned size, the entry table
    (uploaded once) and the host bookkeeping.  ``schedule`` runs on the loader's worker thread, ``CachedBatch.to_device``
    on the consumer's.

    Ordering invariant: the worker marks an entry ``scheduled`` when it STAGES the image, long before the copy into the
    arena runs.  That is safe because items leave the loader's queue first in, first out, and ``__next__`` puts every
    launch of an item on one stream: the store of batch k precedes the gather of batch k + 1 (and the gather of batch k
    itself) in stream order, so a later batch that finds the flag set reads a slot that is filled by then.  The flag
    array belongs to the worker thread alone.  A consumer that changes streams between two ``next()`` calls has to order
    them itself, as for any tensor."""

    def __init__(self, plan, image_data, device, pool, device_preprocess, by_ratio):
        self.plan, self.image_data, self.device, self.pool = plan, image_data, torch.device(device), pool
        self.device_preprocess, self.by_ratio = device_preprocess, by_ratio
        self.arena = torch.empty(plan.arena_bytes, dtype=torch.uint8, device=self.device)
        self.table = torch.from_numpy(plan.table.view("<i4").reshape(-1, 8)).to(self.device)
        self.scheduled = np.zeros(plan.n, bool)
        self.turn = 0                                   # batches with images past the budget: picks the scratch arena

    def describe(self, listed):
        p = self.plan
        return ("# dataset cache: %d of %d files cached (%d listed), %d bytes (+ %d scratch), %d as uint8 source, %d as "
                "finished fp32" % (p.n_cached, p.n, listed, p.cached_bytes, p.arena_bytes - p.cached_bytes,
                                   int((p.kinds[:p.n_cached] == KIND_U8).sum()), int((p.kinds[:p.n_cached] == KIND_F32).sum())))

    def schedule(self, idx, flips):
        """The ``CachedBatch`` of file indices ``idx`` with ``flips`` drawn by the caller.  Decodes, with the loader's
        existing machinery and flips forced to 0, only the images that no earlier batch has staged (and those past the
        budget, every time)."""
        p, idata, S, C = self.plan, self.image_data, self.plan.size, self.plan.channels
        ents = [int(e) for e in p.entry_of[np.asarray(idx)]]
        missing = [e for e in dict.fromkeys(ents) if e >= p.n_cached or not self.scheduled[e]]
        arrs = list(self.pool.map(lambda e: decode_file(idata, p.files[e], entropy_only=True), missing))
        row_of, piece, scratch0 = {}, [], 0
        if any(e >= p.n_cached for e in missing):
            slot = self.turn % p.depth
            self.turn += 1
            scratch0 = p.cached_bytes + slot * p.scratch_bytes
            row0 = p.n + slot * p.batch_size
        groups = {KIND_U8: ([], []), KIND_F32: ([], [])}      # kind -> (decoded images, arena offsets)
        for e, a in zip(missing, arrs):
            if not packable(a, C) or tuple(a.shape[:2]) != p.shapes[e]:
                raise ValueError("dataset cache: %s decodes to %s %s, its header said uint8 %s"
                                 % (p.files[e], getattr(a, "dtype", type(a).__name__), tuple(getattr(a, "shape", ())),
                                    p.shapes[e] + (C,)))
            if e < p.n_cached:
                dst = int(p.offsets[e])
            else:
                dst = scratch0 + len(piece) * p.slot_bytes
                row_of[e] = row0 + len(piece)
                piece.append(entry_row(p, e, dst))
            groups[int(p.kinds[e])][0].append(a)
            groups[int(p.kinds[e])][1].append(dst)
        stages = []
        imgs, dsts = groups[KIND_U8]
        if imgs:
            raw, tab, geom = pack_batch(imgs, [False] * len(imgs), S, C, pin=True)
            segs = [(off, dst, _align(a.size), 0) for off, dst, a in zip(geom["offsets"], dsts, imgs)]
            stages.append((KIND_U8, PackedBatch(raw, tab, geom), torch.tensor(segs, dtype=torch.int64).pin_memory()))
        imgs, dsts = groups[KIND_F32]
        if imgs:
            one = 4 * S * S * C
            pays = self.device_preprocess and (not self.by_ratio or device_path_pays(switch_bytes(imgs), len(imgs), S, C))
            if pays:
                host = PackedBatch(*pack_batch(imgs, [False] * len(imgs), S, C, pin=True))
            else:
                host = torch.from_numpy(np.ascontiguousarray(np.stack(list(self.pool.map(      # (the resize's fancy
                    lambda a: finish_on_host(finish_decode(a), S, False), imgs))))).pin_memory()   # indexing sets strides)
            segs = [(i * one, dst, one, 0) for i, dst in enumerate(dsts)]
            stages.append((KIND_F32, host, torch.tensor(segs, dtype=torch.int64).pin_memory()))
        for e in missing:
            if e < p.n_cached:
                self.scheduled[e] = True
        sel = np.array([(row_of.get(e, e), 1 if f else 0) for e, f in zip(ents, flips)], np.int32).reshape(len(ents), 2)
        rows = None
        if piece:
            rows = (row0, torch.from_numpy(np.array(piece, ENTRY_DTYPE).view("<i4").reshape(len(piece), 8)).pin_memory())
        return CachedBatch(self, stages, rows, torch.from_numpy(sel).pin_memory())


class BatchLoader:
    """shuffle_and_repeat(dataset_num) + map_and_batch(batch_size, drop_remainder=True) +
    prefetch_to_device (BigGAN.py:776-781): an endless iterator of device batches.  One worker thread
    decodes ahead (queue depth 4); ``rank`` / ``world`` give each data-parallel rank a disjoint shard of
    every shuffled epoch.

    ``device_preprocess`` (None: on for a GPU unless BG_DEVICE_INPUT=0): the decode pool only decodes, the worker draws
    the batch's flips from ``image_data.rng`` - one draw per image in batch order, the stream the host path consumes
    with one worker, and the same at any worker count - and packs; ``__next__`` copies the bytes and launches
    ``bg_image_batch_u8`` on the current stream.  A batch with an array that is not uint8 [h, w, C] is finished on the
    host with the same flips, and so is, under None, a batch whose packed bytes exceed its fp32 bytes
    (``device_path_pays``: large sources); True packs every batch, False none.  Both paths give the same bits.

    A JPEG file is only entropy-decoded by the pool (``decode_file(entropy_only=True)``, the C helper): its coefficients
    travel with the batch and ``bg_jpeg_batch_u8`` fills its slot on the device before the resize; in a batch that is
    finished on the host it is decoded there from the same coefficients (``JpegImage.decode``).

    ``cache_bytes`` (None: BG_DEVICE_DATASET_GB in GiB; 0, or a device that is not a GPU: off, and nothing below
    happens): the byte budget of a device-resident dataset (``DatasetCache``, csrc/dataset.hip).  The constructor reads
    the files' headers and plans one arena; the worker then decodes and stages an image only the first time a batch names
    it, and ``__next__`` copies the staged images into the arena (``bg_dataset_store``) and builds the batch with one
    ``bg_dataset_batch`` launch from the indices and flips, which are drawn exactly as without the cache.  Same seeds,
    same batches, bit for bit.  Files past the budget are streamed through a scratch tail of the arena every time; a
    dataset with a file that cannot be cached by its header runs without the cache."""

    def __init__(self, files, labels, batch_size, image_data, device, seed=0, rank=0, world=1, depth=4, workers=8,
                 device_preprocess=None, cache_bytes=None):
        if len(files) < batch_size * world:
            raise ValueError("dataset has %d files, fewer than one global batch (%d)" % (len(files), batch_size * world))
        self.files, self.labels = list(files), labels
        self.batch_size, self.image_data, self.device = batch_size, image_data, torch.device(device)
        self._dev_index = 0
        if self.device.type == "cuda":
            self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.rank, self.world = rank, world
        self.device_preprocess = device_input_enabled(self.device, device_preprocess)
        self._by_ratio = device_preprocess is None      # the automatic switch decides per batch (device_path_pays)
        self.rng = np.random.default_rng(seed)          # same seed on every rank: identical permutations
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(max_workers=workers)     # zlib, the C unfilter and numpy release the GIL
        self.cache = None
        budget = dataset_cache_bytes(self.device, cache_bytes)
        if budget > 0:
            self._open_cache(budget)
        self.q = queue.Queue(maxsize=depth)
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._work, daemon=True)
        self.thread.start()

    def _work(self):
        try:
            if self.device.type == "cuda":
                # the current CUDA/HIP device is per THREAD and defaults to 0: without this, ranks 1..N-1 would create
                # a context (and pinned-allocator state) on GPU 0 from their loader threads
                torch.cuda.set_device(self._dev_index)
            while not self.stop.is_set():
                order = self.rng.permutation(len(self.files))
                per_step = self.batch_size * self.world
                for s in range(0, len(order) - per_step + 1, per_step):
                    idx = order[s + self.rank * self.batch_size: s + (self.rank + 1) * self.batch_size]
                    if self.cache is not None:
                        item = [self.cache.schedule(idx, self._draw_flips(len(idx)))]
                    elif self.device_preprocess:
                        item = [self._decode_and_pack(idx)]
                    else:
                        imgs = np.stack(list(self.pool.map(lambda i: self.image_data.image_processing(self.files[i]), idx)))
                        item = [torch.from_numpy(imgs)]
                    if self.labels is not None:
                        item.append(torch.tensor(np.asarray([self.labels[i] for i in idx], np.float32)))
                    if self.device.type == "cuda":
                        item = [t if isinstance(t, (PackedBatch, CachedBatch)) else t.pin_memory() for t in item]
                    while not self.stop.is_set():
                        try:
                            self.q.put(item, timeout=0.2)
                            break
                        except queue.Full:
                            continue
                    if self.stop.is_set():
                        return
        except Exception as e:                          # surface worker failures in the consumer
            self.q.put(e)

    def _open_cache(self, budget):
        import time
        t0 = time.perf_counter()
        plan, refused = plan_dataset(self.files, self.image_data, budget, self.batch_size, self.pool, depth=CACHE_DEPTH)
        if plan is None:
            print("# dataset cache: off, %s cannot be cached by its header" % refused)
            return
        self.cache = DatasetCache(plan, self.image_data, self.device, self.pool, self.device_preprocess, self._by_ratio)
        self.cache.plan_seconds = time.perf_counter() - t0
        print(self.cache.describe(len(self.files)))

    def _draw_flips(self, n):
        """One draw per image in batch order from ``image_data.rng``, under its lock."""
        idata = self.image_data
        if not idata.flip:
            return [False] * n
        with idata._lock:
            return [bool(idata.rng.random() < 0.5) for _ in range(n)]

    def _decode_and_pack(self, idx):
        idata = self.image_data
        arrs = list(self.pool.map(lambda i: decode_file(idata, self.files[i], entropy_only=True), idx))
        flips = self._draw_flips(len(arrs))
        pays = not self._by_ratio or device_path_pays(switch_bytes(arrs), len(arrs), idata.load_size, idata.channels)
        if pays and all(packable(a, idata.channels) for a in arrs):
            return PackedBatch(*pack_batch(arrs, flips, idata.load_size, idata.channels, pin=True))
        imgs = np.stack(list(self.pool.map(lambda af: finish_on_host(finish_decode(af[0]), idata.load_size, af[1]),
                                           zip(arrs, flips))))
        return torch.from_numpy(imgs)

    def __iter__(self):
        return self

    def __next__(self):
        item = self.q.get()
        if isinstance(item, Exception):
            raise item
        out = [t.to_device(self.device) if isinstance(t, (PackedBatch, CachedBatch)) else t.to(self.device, non_blocking=True)
               for t in item]
        return out[0] if self.labels is None else tuple(out)

    def close(self):
        self.stop.set()
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass
        self.thread.join(2)
        self.pool.shutdown(wait=False)
