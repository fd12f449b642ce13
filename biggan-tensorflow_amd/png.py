"""Device-side PNG encoding (csrc/png.hip; DESIGN.md "Device-side PNG encoding"): the host half.  ``plan`` lays out the
two device tables of a launch, ``encode_device`` runs the three launches on images that already lie in a uint8 arena on the
device (a sample grid, the strip arena of the sampling service) and ``assemble`` wraps the compressed bytes of one image
into a PNG file: zlib header, the segments, the Adler-32 combined from the per-segment halves, one IDAT chunk whose CRC
is taken on the host.  Opt-in: ``enabled()`` reads ``BG_DEVICE_PNG``; without it every file is written by
``utils.write_png`` as before.  Apart from ``encode_device`` nothing here touches the GPU or the library."""
import os
import struct
import zlib

import numpy as np

SEG_BYTES = 32768                          # production segment size (the DEFLATE window: nothing is lost to a decoder)
ALIGN = 16                                 # filtered streams and slots start on 16-byte boundaries
ADLER_BASE = 65521
IMAGE_ENTRY = np.dtype([("src_offset", "<i8"), ("h", "<i4"), ("row_bytes", "<i4"), ("dst_offset", "<i8")])   # BgPngImage
SEG_ENTRY = np.dtype([("src_offset", "<i8"), ("len", "<i4"), ("last", "<i4"), ("dst_offset", "<i8")])        # BgDeflateSeg
KIND_STORED, KIND_DYNAMIC = 0, 1


def enabled():
    """True under ``BG_DEVICE_PNG=1``."""
    return os.environ.get("BG_DEVICE_PNG", "") == "1"


def deflate_bound(length):
    """``bg_deflate_bound``: the bytes a segment's slot must hold (stored block 5 + len, empty stored block 5, slack)."""
    return int(length) + 16 if length > 0 else 16


def _align(n):
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


class Plan(object):
    """What one launch of the three kernels needs.  ``filter_table`` int32 [n,6] (BgPngImage) and ``seg_table`` int32
    [m,6] (BgDeflateSeg) in device layout; ``stream_bytes`` / ``slot_bytes`` / ``out_bytes``: the sizes of the filtered
    arena, the slot arena and the compacted output; per image ``stream_offsets`` / ``stream_lens`` (its filtered stream)
    and ``segments`` (the half-open range of its rows in ``seg_table``); ``slot_offsets`` per segment; ``bpp``, ``max_h``,
    ``seg_bytes``; ``images`` the (src_offset, h, w, c) it was made from."""


def plan(images, seg_bytes=SEG_BYTES):
    """``images``: [(src_offset, h, w, c)] inside one uint8 arena, c in 1/3/4 and common to all -> Plan.  The filtered
    stream of an image is h * (1 + w*c) bytes; it is cut into segments of ``seg_bytes`` (the last one shorter), each with
    a slot of ``deflate_bound(len)`` bytes; ``last`` marks the final segment of every stream."""
    seg_bytes = int(seg_bytes)
    if seg_bytes < 256 or seg_bytes > 32768 or seg_bytes & (seg_bytes - 1):
        raise ValueError("png.plan: seg_bytes %d is not a power of two from 256 to 32768" % seg_bytes)
    images = [tuple(int(v) for v in im) for im in images]
    if not images:
        raise ValueError("png.plan: no images")
    bpp = images[0][3]
    for off, h, w, c in images:
        if c not in (1, 3, 4) or c != bpp:
            raise ValueError("png.plan: %d channels (1, 3 or 4, the same for every image of a launch: %d)" % (c, bpp))
        if off < 0 or h < 1 or w < 1 or w * c > (1 << 24) or h > (1 << 20):
            raise ValueError("png.plan: image (offset %d, %d x %d x %d) is out of range" % (off, h, w, c))
    p = Plan()
    p.images, p.bpp, p.seg_bytes = images, bpp, seg_bytes
    p.max_h = max(h for _, h, _, _ in images)
    ft = np.zeros(len(images), IMAGE_ENTRY)
    segs, p.stream_offsets, p.stream_lens, p.segments = [], [], [], []
    stream_off = slot_off = 0
    for i, (off, h, w, c) in enumerate(images):
        n = h * (1 + w * c)
        ft[i] = (off, h, w * c, stream_off)
        p.stream_offsets.append(stream_off)
        p.stream_lens.append(n)
        first = len(segs)
        for pos in range(0, n, seg_bytes):
            ln = min(seg_bytes, n - pos)
            segs.append((stream_off + pos, ln, 1 if pos + ln == n else 0, slot_off))
            slot_off += _align(deflate_bound(ln))
        p.segments.append((first, len(segs)))
        stream_off += _align(n)
    st = np.zeros(len(segs), SEG_ENTRY)
    for j, s in enumerate(segs):
        st[j] = s
    p.filter_table = ft.view("<i4").reshape(len(images), 6)
    p.seg_table = st.view("<i4").reshape(len(segs), 6)
    p.slot_offsets = [s[3] for s in segs]
    p.seg_lens = [s[1] for s in segs]
    p.stream_bytes, p.slot_bytes = stream_off, slot_off
    p.out_bytes = sum(deflate_bound(s[1]) for s in segs)
    return p


def adler32_combine(adler1, adler2, len2):
    """The Adler-32 of A + B from adler32(A), adler32(B) and len(B) (zlib's adler32_combine)."""
    base = ADLER_BASE
    rem = int(len2) % base
    a1, b1 = adler1 & 0xffff, (adler1 >> 16) & 0xffff
    a2, b2 = adler2 & 0xffff, (adler2 >> 16) & 0xffff
    a = (a1 + a2 + base - 1) % base
    b = (rem * a1 + b1 + b2 + base - rem) % base
    return (b << 16) | a


def adler32_fold(parts):
    """[(adler_a, adler_b, len)] of consecutive segments, each taken on its own -> the Adler-32 of their concatenation."""
    adler = 1
    for a, b, n in parts:
        adler = adler32_combine(adler, ((int(b) & 0xffff) << 16) | (int(a) & 0xffff), n)
    return adler


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def assemble(w, h, c, compressed, adler):
    """The bytes of an 8-bit PNG file of a w x h image with c channels (1, 3 or 4) from the raw DEFLATE stream of its
    filtered rows (``compressed``: bytes, or a list of the segments' bytes) and their Adler-32: zlib header ``78 01``,
    the stream, the big-endian Adler, in one IDAT chunk between IHDR and IEND."""
    if c not in (1, 3, 4):
        raise ValueError("png.assemble: %d channels (1, 3 or 4)" % c)
    if not isinstance(compressed, (bytes, bytearray, memoryview)):
        compressed = b"".join(bytes(s) for s in compressed)
    idat = b"\x78\x01" + bytes(compressed) + struct.pack(">I", adler & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)) +
            _chunk(b"IDAT", idat) + _chunk(b"IEND", b""))


def idat_payload(data):
    """The concatenated IDAT bodies of a PNG file (what zlib.decompress takes)."""
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            out.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return b"".join(out)


def compress_device(src, p):
    """Run the deflate and compaction launches of Plan ``p`` on the filtered arena ``src`` (uint8 on the device) ->
    (out, records, seg_off, totals) on the device."""
    import torch
    from . import functional as Fn
    dev = src.device
    m, n = p.seg_table.shape[0], len(p.images)
    stab = torch.from_numpy(p.seg_table).to(dev)
    slots = torch.empty(p.slot_bytes, dtype=torch.uint8, device=dev)
    records = torch.empty(m, 4, dtype=torch.int32, device=dev)
    out = torch.empty(p.out_bytes, dtype=torch.uint8, device=dev)
    seg_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(n, 2, dtype=torch.int64, device=dev)
    Fn.deflate_segments(src, stab, p.seg_bytes, slots, records)
    Fn.deflate_compact(slots, stab, records, out, seg_off, totals)
    return out, records, seg_off, totals


def encode_device(arena, entries, seg_bytes=SEG_BYTES):
    """``arena``: uint8 [bytes] on the device; ``entries``: [(offset, h, w, c)] of images [h, w, c] that lie row-major in
    it -> the bytes of their PNG files, in order.  One filter launch, one deflate launch and one compaction for all of
    them; only the compressed bytes and the per-segment records cross to the host.  The same pixels give the same bytes
    however many images share the call."""
    import torch
    from . import functional as Fn
    p = plan(entries, seg_bytes)
    for off, h, w, c in p.images:
        if off + h * w * c > arena.numel():
            raise ValueError("png.encode_device: image (offset %d, %d x %d x %d) does not fit the arena of %d bytes"
                             % (off, h, w, c, arena.numel()))
    dev = arena.device
    filtered = torch.empty(p.stream_bytes, dtype=torch.uint8, device=dev)
    Fn.png_filter(arena, torch.from_numpy(p.filter_table).to(dev), p.max_h, p.bpp, filtered)
    out, records, seg_off, totals = compress_device(filtered, p)
    rec = records.cpu().numpy()                                                        # (synchronises)
    tot = totals.cpu().numpy()
    if (rec[:, 3] < 0).any():
        raise RuntimeError("png.encode_device: segment %d did not fit its arenas" % int(np.argmax(rec[:, 3] < 0)))
    total = int(tot[-1, 0] + tot[-1, 1])
    comp = out[:total].cpu().numpy().tobytes()
    files = []
    for i, (off, h, w, c) in enumerate(p.images):
        first, end = p.segments[i]
        adler = adler32_fold([(rec[j, 1], rec[j, 2], p.seg_lens[j]) for j in range(first, end)])
        files.append(assemble(w, h, c, comp[int(tot[i, 0]):int(tot[i, 0] + tot[i, 1])], adler))
    return files
