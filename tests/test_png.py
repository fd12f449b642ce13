"""Device-side PNG encoding, the host half (biggan_tensorflow_amd/png.py): the launch plan, the Adler-32 combination, the
file assembly around stand-in segments made by zlib, the filter reference against the project's own unfilter, the ABI
surface, and the default: without BG_DEVICE_PNG nothing changes.  No GPU."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data, hip, png, utils
from tests import png_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAN_CASES = [([(0, 1, 1, 1)], 256),
              ([(0, 2, 3, 3)], 256),
              ([(0, 5, 130, 1)], 256),                                   # 131-byte rows: segments cut rows
              ([(0, 7, 33, 4), (1024, 64, 64, 4), (20000, 1, 1, 4)], 256),
              ([(0, 64, 64, 3)], 4096),                                  # 12352 bytes: three whole segments and a rest
              ([(0, 128, 256, 1)], 32768),                               # 32896 bytes: one segment and 128 bytes
              ([(16 * i, 3 + i, 40 + 7 * i, 3) for i in range(10)], 512),
              ([(0, 256, 128, 1)], 32768)]                               # 33024 bytes


@pytest.mark.parametrize("images,seg_bytes", PLAN_CASES, ids=lambda v: str(v) if isinstance(v, int) else "n%d" % len(v))
def test_plan_invariants(images, seg_bytes):
    L = hip.lib()
    p = png.plan(images, seg_bytes)
    ft = p.filter_table.view(png.IMAGE_ENTRY).reshape(-1)
    st = p.seg_table.view(png.SEG_ENTRY).reshape(-1)
    assert p.filter_table.dtype == np.int32 and p.filter_table.shape == (len(images), 6)
    assert p.seg_table.dtype == np.int32 and p.seg_table.shape[1] == 6
    assert p.bpp == images[0][3] and p.max_h == max(im[1] for im in images)
    covered = np.zeros(p.stream_bytes, np.int32)
    slot_used = np.zeros(p.slot_bytes, np.int32)
    for i, (off, h, w, c) in enumerate(images):
        n = h * (1 + w * c)
        e = ft[i]
        assert (e["src_offset"], e["h"], e["row_bytes"]) == (off, h, w * c)
        assert e["dst_offset"] == p.stream_offsets[i] and e["dst_offset"] % 16 == 0 and p.stream_lens[i] == n
        first, end = p.segments[i]
        assert end > first
        mine = st[first:end]
        assert [int(s["last"]) for s in mine] == [0] * (end - first - 1) + [1]          # set exactly once per stream
        pos = e["dst_offset"]
        for s in mine:
            assert s["src_offset"] == pos and 1 <= s["len"] <= seg_bytes and s["src_offset"] % 16 == 0
            covered[pos:pos + s["len"]] += 1
            pos += s["len"]
        assert pos == e["dst_offset"] + n
        assert all(s["len"] == seg_bytes for s in mine[:-1])
        covered[e["dst_offset"] + n:png._align(e["dst_offset"] + n)] += 1              # alignment padding: nobody's
    assert (covered == 1).all()                                    # every stream byte is in exactly one segment
    for j, s in enumerate(st):
        need = L.bg_deflate_bound(int(s["len"]))
        assert png.deflate_bound(int(s["len"])) == need
        assert s["dst_offset"] == p.slot_offsets[j] and s["dst_offset"] % 16 == 0
        slot_used[s["dst_offset"]:s["dst_offset"] + need] += 1
        assert s["dst_offset"] + need <= p.slot_bytes
    assert slot_used.max() == 1                                    # the slots are disjoint
    assert p.out_bytes == sum(L.bg_deflate_bound(int(s["len"])) for s in st)
    assert sum(end - first for first, end in p.segments) == len(st)


def test_plan_rejects_what_the_kernels_cannot_run():
    for bad in (128, 300, 65536):
        with pytest.raises(ValueError):
            png.plan([(0, 4, 4, 3)], bad)
    with pytest.raises(ValueError):
        png.plan([(0, 4, 4, 3), (64, 4, 4, 4)], 256)               # bpp is common to a launch
    with pytest.raises(ValueError):
        png.plan([(0, 4, 4, 2)], 256)
    with pytest.raises(ValueError):
        png.plan([(-1, 4, 4, 3)], 256)
    with pytest.raises(ValueError):
        png.plan([], 256)


def test_adler32_combine_against_zlib():
    rng = np.random.RandomState(0)
    for trial in range(40):
        n = int(rng.randint(1, 5000))
        buf = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        cut = int(rng.randint(0, n + 1))
        a, b = buf[:cut], buf[cut:]
        assert png.adler32_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(buf), (n, cut)
    ff = b"\xff" * (3 * 32768)                                     # the largest sums a segment can reach
    parts = []
    for pos in range(0, len(ff), 32768):
        ad = zlib.adler32(ff[pos:pos + 32768])
        parts.append((ad & 0xffff, ad >> 16, 32768))
    assert png.adler32_fold(parts) == zlib.adler32(ff)
    cuts = sorted(rng.randint(0, len(ff), 7).tolist())
    pieces = [ff[a:b] for a, b in zip([0] + cuts, cuts + [len(ff)])]
    assert png.adler32_fold([(zlib.adler32(q) & 0xffff, zlib.adler32(q) >> 16, len(q)) for q in pieces]) == zlib.adler32(ff)
    assert png.adler32_fold([]) == 1 == zlib.adler32(b"")


def _pixels(h, w, c, seed):
    return PR.sinusoid_image(h, w, c, 0.01, seed)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("seg_bytes", [256, 32768])
def test_assemble_around_stand_in_segments_decodes_to_the_pixels(c, seg_bytes):
    a = _pixels(37, 45, c, seed=c)
    stream = PR.filter_rows(a).tobytes()
    segs, parts = PR.segments_with_zlib(stream, seg_bytes)
    assert len(segs) == -(-len(stream) // seg_bytes)
    for s in segs[:-1]:
        assert s.endswith(b"\x00\x00\xff\xff")                      # byte-aligned: the empty stored block
    blob = png.assemble(45, 37, c, segs, png.adler32_fold(parts))
    assert blob[:8] == b"\x89PNG\r\n\x1a\n" and blob.count(b"IDAT") == 1
    payload = png.idat_payload(blob)
    assert payload[:2] == b"\x78\x01" and struct.unpack(">I", payload[-4:])[0] == zlib.adler32(stream)
    assert zlib.decompress(payload) == stream                       # (zlib checks the Adler-32 itself)
    got = data.decode_png(blob, channels=4 if c == 4 else 3)
    want = a if c != 1 else np.repeat(a, 3, axis=2)
    assert np.array_equal(got, want)
    # each stand-in segment inflates on its own
    pos = 0
    for s, (_, _, n) in zip(segs, parts):
        assert zlib.decompressobj(-15).decompress(s) == stream[pos:pos + n]
        pos += n
    assert png.assemble(45, 37, c, b"".join(segs), png.adler32_fold(parts)) == blob


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 3), (5, 130, 1), (7, 33, 4), (64, 64, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_filter_rows_then_unfilter_is_the_identity(shape):
    h, w, c = shape
    a = _pixels(h, w, c, seed=h + w) if h > 2 else np.random.RandomState(1).randint(0, 256, shape).astype(np.uint8)
    f = PR.filter_rows(a)
    assert f.shape == (h, 1 + w * c) and f[:, 0].max() <= 4
    assert np.array_equal(data._unfilter(f.tobytes(), h, w * c, c).reshape(h, w, c), a)
    assert np.array_equal(data._unfilter_py(f.tobytes(), h, w * c, c).reshape(h, w, c), a)


def test_filter_rows_picks_every_type_and_breaks_ties_downwards():
    a = PR.five_filter_image()
    f = PR.filter_rows(a)
    assert set(f[:, 0].tolist()) == {0, 1, 2, 3, 4}
    assert np.array_equal(data._unfilter(f.tobytes(), a.shape[0], a.shape[1], 1).reshape(a.shape), a)
    flat = np.full((3, 8, 3), 9, np.uint8)
    assert PR.filter_rows(flat)[:, 0].tolist() == [1, 2, 2]          # Sub beats None on row 0; Up = Average = Paeth = 0 below
    assert PR.filter_rows(np.zeros((2, 4, 1), np.uint8))[:, 0].tolist() == [0, 0]


def test_header_binding_and_makefile_agree():
    header = open(os.path.join(ROOT, "include", "biggan_hip.h")).read()
    assert re.search(r"#define BG_ABI_VERSION 10\b", header) and hip.ABI_VERSION == 10
    for name in ("bg_png_filter", "bg_deflate_segments", "bg_deflate_compact"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in hip.SIGNATURES and hip.SIGNATURES[name][0] is ctypes.c_int
    assert re.search(r"\bsize_t bg_deflate_bound\(int len\)", header)
    assert hip.SIGNATURES["bg_deflate_bound"] == (ctypes.c_size_t, [ctypes.c_int])
    assert "typedef struct BgPngImage" in header and "typedef struct BgDeflateSeg" in header
    assert png.IMAGE_ENTRY.itemsize == 24 and png.SEG_ENTRY.itemsize == 24
    # the argument lists: one ctypes type per C parameter
    for name in ("bg_png_filter", "bg_deflate_segments", "bg_deflate_compact"):
        params = re.search(r"\bint %s\(([^)]*)\)" % name, header).group(1).split(",")
        assert len(params) == len(hip.SIGNATURES[name][1]), name
        for text, ctype in zip(params, hip.SIGNATURES[name][1]):
            want = ctypes.c_void_p if "*" in text else ctypes.c_int64 if "int64_t" in text else ctypes.c_int
            assert ctype is want, (name, text)
    assert "png.hip" in open(os.path.join(ROOT, "biggan-tensorflow_amd", "csrc", "Makefile")).read()
    L = hip.lib()
    assert L.bg_abi_version() == 10 and L.bg_png_filter and L.bg_deflate_segments and L.bg_deflate_compact


def test_deflate_bound_is_monotone_and_holds_a_stored_block():
    L = hip.lib()
    prev = 0
    for n in list(range(1, 600)) + [4095, 4096, 32767, 32768]:
        b = L.bg_deflate_bound(n)
        assert b >= n + 5 + 5                                       # a stored block and the empty stored block behind it
        assert b >= prev and b == png.deflate_bound(n)
        prev = b


def test_entry_points_check_their_arguments_before_any_launch():
    L = hip.lib()
    fake = ctypes.c_void_p(4096)                                    # never dereferenced: every call fails validation
    assert L.bg_png_filter(None, 64, fake, 1, 1, 3, fake, 64, None) == 1 and b"NULL" in L.bg_last_error()
    assert L.bg_png_filter(fake, 64, fake, 1, 1, 2, fake, 64, None) == 1 and b"bpp" in L.bg_last_error()
    assert L.bg_png_filter(fake, 64, fake, 0, 1, 3, fake, 64, None) == 1
    assert L.bg_png_filter(fake, 0, fake, 1, 1, 3, fake, 64, None) == 1
    for seg in (0, 128, 255, 300, 65536):
        assert L.bg_deflate_segments(fake, 64, fake, 1, seg, fake, 64, fake, None) == 1
        assert b"seg_bytes" in L.bg_last_error()
    assert L.bg_deflate_segments(fake, 64, fake, 1, 256, fake, 64, None, None) == 1
    assert L.bg_deflate_compact(fake, 64, fake, fake, 1, fake, 64, fake, None, 1, None) == 1
    assert L.bg_deflate_compact(fake, 64, fake, fake, 1, fake, 64, fake, fake, 2, None) == 1      # more streams than segments


def test_the_default_does_not_move(tmp_path, monkeypatch):
    """Without BG_DEVICE_PNG every file is what utils.write_png has always written: filter type 0 on every row, one
    zlib level-6 stream."""
    monkeypatch.delenv("BG_DEVICE_PNG", raising=False)
    assert not png.enabled()
    a = _pixels(20, 31, 3, seed=4)
    blob = open(utils.write_png(a, str(tmp_path / "a.png")), "rb").read()
    raw = np.concatenate([np.zeros((20, 1), np.uint8), a.reshape(20, 93)], axis=1).tobytes()
    assert png.idat_payload(blob) == zlib.compress(raw, 6)
    assert blob == (b"\x89PNG\r\n\x1a\n" + png._chunk(b"IHDR", struct.pack(">IIBBBBB", 31, 20, 8, 2, 0, 0, 0)) +
                    png._chunk(b"IDAT", zlib.compress(raw, 6)) + png._chunk(b"IEND", b""))
    for value, want in (("1", True), ("0", False), ("", False), ("true", False)):
        monkeypatch.setenv("BG_DEVICE_PNG", value)
        assert png.enabled() is want
    monkeypatch.setenv("BG_DEVICE_PNG", "1")                        # write_png itself never looks at the variable
    assert open(utils.write_png(a, str(tmp_path / "b.png")), "rb").read() == blob
