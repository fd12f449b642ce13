"""Device-side PNG encoding on the device (csrc/png.hip): bg_png_filter against tests/png_ref.filter_rows byte for byte,
bg_deflate_segments as a byte compressor read back by zlib (every segment also on its own, inside guard bands),
png.encode_device (batch independence, determinism), file sizes against the host path, and the two users under
BG_DEVICE_PNG=1: BigGAN.save_samples and one round of the sampling service."""
import heapq
import os
import zlib

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import data, functional as Fn, png, utils
from tests import png_ref as PR

pytestmark = pytest.mark.gpu

BAND, FILL = 64, 0xA5


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- filter kernel
def _filter_images():
    rng = np.random.RandomState(3)
    return {"1x1x1": rng.randint(0, 256, (1, 1, 1)).astype(np.uint8),
            "2x3x3": rng.randint(0, 256, (2, 3, 3)).astype(np.uint8),
            "5x130x1": PR.sinusoid_image(5, 130, 1, 0.02, 5),        # 130-byte rows, odd pitch with the type byte
            "7x33x4": PR.sinusoid_image(7, 33, 4, 0.01, 7),
            "64x64x3": PR.sinusoid_image(64, 64, 3, 0.0, 64),
            "five": PR.five_filter_image()}


def _run_filter(images, seg_bytes=256, spoil=None):
    """Filter ``images`` (same c) in one launch from one arena -> (plan, filtered arena bytes inside guard bands)."""
    offs, pos = [], 0
    for a in images:
        offs.append(pos)
        pos += (a.size + 15) // 16 * 16
    arena = np.zeros(pos, np.uint8)
    for a, off in zip(images, offs):
        arena[off:off + a.size] = a.reshape(-1)
    p = png.plan([(off,) + a.shape for a, off in zip(images, offs)], seg_bytes)
    table = p.filter_table.copy()
    if spoil is not None:
        spoil(table.view(png.IMAGE_ENTRY).reshape(-1), pos, p.stream_bytes)
    buf = torch.full((BAND + p.stream_bytes + BAND,), FILL, dtype=torch.uint8, device="cuda")
    Fn.png_filter(_cuda(arena), _cuda(table), p.max_h, p.bpp, buf[BAND:BAND + p.stream_bytes])
    got = buf.cpu().numpy()
    assert (got[:BAND] == FILL).all() and (got[BAND + p.stream_bytes:] == FILL).all()
    return p, got[BAND:BAND + p.stream_bytes]


@pytest.mark.parametrize("name", ["1x1x1", "2x3x3", "5x130x1", "7x33x4", "64x64x3", "five"])
def test_filter_kernel_equals_the_reference(name):
    a = _filter_images()[name]
    want = PR.filter_rows(a)
    p, got = _run_filter([a])
    assert np.array_equal(got[:want.size].reshape(want.shape), want)
    assert (got[want.size:] == FILL).all()                           # the alignment padding is nobody's
    if name == "five":
        assert set(want[:, 0].tolist()) == {0, 1, 2, 3, 4}
    if name == "64x64x3":
        assert want[:, 0].max() > 0                                  # a smooth image does not stay unfiltered


def test_filter_entries_that_do_not_fit_write_nothing():
    """Four images in one launch; three entries are spoiled, each in one way: a source extent past its arena, a
    destination extent past its arena, an h above max_h.  Their streams stay untouched, the fourth is right."""
    imgs = [PR.sinusoid_image(6, 9, 3, 0.02, s) for s in range(4)]

    def spoil(t, src_bytes, dst_bytes):
        t[0]["src_offset"] = src_bytes - imgs[0].size + 1
        t[1]["dst_offset"] = dst_bytes - 6 * 28 + 1
        t[3]["h"] = 7
    p, got = _run_filter(imgs, spoil=spoil)
    want = np.full(p.stream_bytes, FILL, np.uint8)
    f = PR.filter_rows(imgs[2])
    want[p.stream_offsets[2]:p.stream_offsets[2] + f.size] = f.reshape(-1)
    assert np.array_equal(got, want)
    p, got = _run_filter(imgs)                                       # unspoiled: all four
    for i in range(4):
        f = PR.filter_rows(imgs[i])
        assert np.array_equal(got[p.stream_offsets[i]:p.stream_offsets[i] + f.size], f.reshape(-1)), i


# ---------------------------------------------------------------- deflate kernel on raw buffers
def _deflate(buf, seg_bytes=256):
    """Compress uint8 ``buf`` as one stream in segments of ``seg_bytes`` -> (segment bytes, records int32 [m,4]).  Every
    slot lies between guard bands that must survive, as must the unused rest of the slot."""
    buf = np.ascontiguousarray(buf, np.uint8)
    n = buf.size
    lens = [min(seg_bytes, n - pos) for pos in range(0, n, seg_bytes)]
    st = np.zeros(len(lens), png.SEG_ENTRY)
    pos, slot = 0, BAND
    for j, ln in enumerate(lens):
        st[j] = (pos, ln, 1 if j == len(lens) - 1 else 0, slot)
        pos += ln
        slot += (Fn.deflate_bound(ln) + 15) // 16 * 16 + BAND
    dst = torch.full((slot,), FILL, dtype=torch.uint8, device="cuda")
    records = torch.full((len(lens), 4), -7, dtype=torch.int32, device="cuda")
    table = _cuda(st.view("<i4").reshape(len(lens), 6))
    Fn.deflate_segments(_cuda(buf), table, seg_bytes, dst, records)
    rec, out = records.cpu().numpy(), dst.cpu().numpy()
    used = np.zeros(slot, bool)
    segs = []
    for j, ln in enumerate(lens):
        off, nb = int(st[j]["dst_offset"]), int(rec[j, 0])
        assert rec[j, 3] in (0, 1) and 0 < nb <= Fn.deflate_bound(ln), (j, rec[j])
        used[off:off + nb] = True
        segs.append(out[off:off + nb].tobytes())
    assert (out[~used] == FILL).all()                                # guard bands and slot tails are intact
    # compaction: the same bytes end to end, the totals of the one stream
    flat = torch.full((sum(Fn.deflate_bound(ln) for ln in lens) + BAND,), FILL, dtype=torch.uint8, device="cuda")
    seg_off = torch.zeros(len(lens) + 1, dtype=torch.int64, device="cuda")
    totals = torch.zeros(1, 2, dtype=torch.int64, device="cuda")
    Fn.deflate_compact(dst, table, records, flat[:-BAND], seg_off, totals)
    total = sum(len(s) for s in segs)
    assert seg_off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(s) for s in segs])]).tolist()
    assert totals.cpu().tolist() == [[0, total]]
    flat = flat.cpu().numpy()
    assert flat[:total].tobytes() == b"".join(segs) and (flat[total:] == FILL).all()
    return segs, rec


def _check_stream(buf, segs, rec, seg_bytes=256):
    buf = np.ascontiguousarray(buf, np.uint8).tobytes()
    d = zlib.decompressobj(-15)
    assert d.decompress(b"".join(segs)) + d.flush() == buf and d.eof and d.unused_data == b""
    pos = 0
    for j, s in enumerate(segs):                                     # every segment inflates on its own
        piece = buf[pos:pos + seg_bytes]
        one = zlib.decompressobj(-15)
        assert one.decompress(s) == piece, j
        assert one.eof == (j == len(segs) - 1)
        if j < len(segs) - 1:
            assert s.endswith(b"\x00\x00\xff\xff")
        ad = zlib.adler32(piece)
        assert (int(rec[j, 1]), int(rec[j, 2])) == (ad & 0xffff, ad >> 16), j
        pos += len(piece)
    assert png.adler32_fold([(rec[j, 1], rec[j, 2], min(seg_bytes, len(buf) - j * seg_bytes))
                             for j in range(len(segs))]) == zlib.adler32(buf)


def _text(n, seed=0):
    """Compressible bytes with runs: a skewed alphabet, every symbol repeated 1-6 times."""
    rng = np.random.RandomState(seed)
    sym = (rng.exponential(6.0, n).astype(np.int64) % 64 + 32).astype(np.uint8)
    return np.repeat(sym, rng.randint(1, 7, n))[:n]


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 3 * 256 + 1])
def test_deflate_lengths_around_the_segment_size(n):
    buf = _text(n, seed=n)
    segs, rec = _deflate(buf)
    assert len(segs) == -(-n // 256)
    _check_stream(buf, segs, rec)
    if n >= 255:
        assert rec[0, 3] == png.KIND_DYNAMIC and rec[0, 0] < 200      # the text does compress


@pytest.mark.parametrize("value", [0, 255], ids=["zeros", "ff"])
def test_deflate_one_value_at_full_size(value):
    """32768 equal bytes: one literal, then 127 matches of 258 (the length cap) and one of 1 -> a literal; the block is
    matches and the end-of-block symbol but for two literals.  0xFF gives the largest Adler sums."""
    buf = np.full(32768, value, np.uint8)
    segs, rec = _deflate(buf, 32768)
    _check_stream(buf, segs, rec, 32768)
    assert rec[0, 3] == png.KIND_DYNAMIC and rec[0, 0] < 64


def test_deflate_only_matches_and_end_of_block():
    """Three runs of 259 equal bytes: each is its first byte as a literal and one match of 258, so the block is three
    literals, three matches and the end-of-block symbol (the first byte of a run can only be a literal)."""
    buf = np.repeat(np.array([7, 9, 7], np.uint8), 259)
    segs, rec = _deflate(buf, 1024)
    _check_stream(buf, segs, rec, 1024)
    assert rec[0, 3] == png.KIND_DYNAMIC


def test_deflate_one_distinct_byte_then_another():
    for n in (40, 256):
        buf = np.full(n, 0x41, np.uint8)
        buf[-1] = 0x42
        segs, rec = _deflate(buf)
        _check_stream(buf, segs, rec)
    buf = np.full(200, 0x41, np.uint8)                                # and one distinct literal alone
    segs, rec = _deflate(buf)
    _check_stream(buf, segs, rec)
    assert rec[0, 3] == png.KIND_DYNAMIC


def test_deflate_without_any_match_sends_a_distance_code_of_length_zero():
    buf = (np.arange(3000) % 251).astype(np.uint8)                    # no two equal neighbours anywhere
    segs, rec = _deflate(buf)
    _check_stream(buf, segs, rec)
    few = (np.arange(3000) % 7 * 31).astype(np.uint8)                 # 7 symbols, no run: compresses without a match
    segs, rec = _deflate(few)
    _check_stream(few, segs, rec)
    assert (rec[:, 3] == png.KIND_DYNAMIC).all() and rec[0, 0] < 256 * 3 // 8 + 40


def test_deflate_noise_takes_the_stored_block():
    buf = np.random.RandomState(11).randint(0, 256, 5 * 256 + 17).astype(np.uint8)
    segs, rec = _deflate(buf)
    _check_stream(buf, segs, rec)
    assert (rec[:, 3] == png.KIND_STORED).all()
    assert [int(v) for v in rec[:, 0]] == [256 + 10] * 5 + [17 + 5]
    big = np.random.RandomState(12).randint(0, 256, 32768).astype(np.uint8)
    segs, rec = _deflate(big, 32768)
    _check_stream(big, segs, rec, 32768)
    assert rec[0, 3] == png.KIND_STORED and rec[0, 0] == 32768 + 5 <= Fn.deflate_bound(32768)


def _huffman_depth(counts, merged_first):
    """The longest code of an unlimited Huffman code for these counts; among equal weights a merged node is taken before
    (``merged_first``) or after the leaves - every such tree is optimal, their depths differ."""
    heap = [(c, i, 0) for i, c in enumerate(counts)]
    heapq.heapify(heap)
    tick = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], -tick if merged_first else tick, max(a[2], b[2]) + 1))
        tick += 1
    return heap[0][2]


def _fibonacci(n):
    fib = [1, 1]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    return fib


@pytest.mark.parametrize("shift", [0, 1], ids=["F(k)", "F(k+1)"])
def test_deflate_fibonacci_counts_force_the_length_limit(shift):
    """Symbol k appears F(k) times, k = 1..20 (17710 bytes), shuffled, in one 32768 segment.  With the end-of-block symbol
    the counts are 1, 1, 1, 2, 3, 5, ...: an unlimited Huffman code for them is 20 bits deep when the tie among the three
    ones is resolved towards the merged node (checked here), but an equally optimal tree that takes leaves first is only
    11 deep, so this case alone need not reach a limiter.  F(k+1) times (1, 2, 3, 5, ...; 28655 bytes) has no such tie:
    after every merge the running node is lighter than the second next leaf, every optimal tree is the 20-deep chain
    (checked here for both tie rules), and any 15-bit limiter has to act."""
    fib = _fibonacci(21)[shift:shift + 20]
    assert _huffman_depth(fib + [1], merged_first=True) > 15
    if shift:
        assert _huffman_depth(fib + [1], merged_first=False) == _huffman_depth(fib + [1], merged_first=True) == 20
    buf = np.repeat(np.arange(1, 21, dtype=np.uint8) * 11, fib)
    np.random.RandomState(5).shuffle(buf)
    assert buf.size == (28655 if shift else 17710)
    segs, rec = _deflate(buf, 32768)
    _check_stream(buf, segs, rec, 32768)
    assert rec[0, 3] == png.KIND_DYNAMIC
    assert rec[0, 0] < 0.6 * buf.size                                 # the entropy of the counts is 2.6 bits a symbol


def test_deflate_a_run_across_a_segment_boundary():
    pat = (np.arange(700) % 251).astype(np.uint8)
    buf = np.concatenate([pat[:200], np.full(300, 7, np.uint8), pat[:100]])      # the run covers bytes 200..499
    segs, rec = _deflate(buf)
    assert len(segs) == 3
    _check_stream(buf, segs, rec)


def test_deflate_entries_that_do_not_fit_write_nothing():
    buf = _text(600, seed=2)
    st = np.zeros(4, png.SEG_ENTRY)
    size = 4 * 512
    st[0] = (0, 256, 0, 0)
    st[1] = (600 - 255, 256, 0, 512)                                  # source extent past the arena
    st[2] = (256, 256, 0, size - 256 - 15)                            # slot past the arena by one byte
    st[3] = (0, 257, 1, 1024)                                         # longer than seg_bytes
    dst = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
    records = torch.zeros(4, 4, dtype=torch.int32, device="cuda")
    Fn.deflate_segments(_cuda(buf), _cuda(st.view("<i4").reshape(4, 6)), 256, dst, records)
    rec, out = records.cpu().numpy(), dst.cpu().numpy()
    assert rec[:, 3].tolist() == [1, -1, -1, -1] and rec[1:, 0].tolist() == [0, 0, 0]
    assert (out[rec[0, 0]:] == FILL).all()
    assert zlib.decompressobj(-15).decompress(out[:rec[0, 0]].tobytes()) == buf[:256].tobytes()


# ---------------------------------------------------------------- the whole encoder
def _arena_of(images):
    offs, pos = [], 0
    for a in images:
        offs.append(pos)
        pos += (a.size + 15) // 16 * 16
    arena = np.zeros(pos, np.uint8)
    for a, off in zip(images, offs):
        arena[off:off + a.size] = a.reshape(-1)
    return _cuda(arena), [(off,) + a.shape for a, off in zip(images, offs)]


def _check_file(blob, a, seg_bytes):
    """The two gates of every case: the IDAT payload inflates to the reference filtered stream, the file decodes to the
    pixels; and the payload is within the bound."""
    h, w, c = a.shape
    want = PR.filter_rows(a).tobytes()
    payload = png.idat_payload(blob)
    assert zlib.decompress(payload) == want
    got = data.decode_png(blob, channels=4 if c == 4 else 3)
    assert np.array_equal(got, a if c != 1 else np.repeat(a, 3, axis=2))
    bound = sum(Fn.deflate_bound(min(seg_bytes, len(want) - pos)) for pos in range(0, len(want), seg_bytes))
    assert len(payload) <= 2 + bound + 4
    assert blob.count(b"IDAT") == 1


def test_encoder_does_not_depend_on_what_shares_the_launch():
    images = [PR.sinusoid_image(3 + 5 * i, 11 + 9 * i, 3, 0.01 * (i % 3), i) for i in range(10)]
    arena, entries = _arena_of(images)
    together = png.encode_device(arena, entries, seg_bytes=512)
    assert len(together) == 10
    for a, blob in zip(images, together):
        _check_file(blob, a, 512)
    alone = [png.encode_device(arena, [e], seg_bytes=512)[0] for e in entries]
    assert alone == together
    assert png.encode_device(arena, entries, seg_bytes=512) == together          # a second call: equal bytes
    assert len({len(b) for b in together}) > 5


@pytest.mark.parametrize("name", ["1x1x1", "2x3x3", "5x130x1", "7x33x4", "64x64x3", "five"])
def test_encoder_on_the_filter_cases(name):
    a = _filter_images()[name]
    arena, entries = _arena_of([a])
    for seg_bytes in (256, 32768):
        _check_file(png.encode_device(arena, entries, seg_bytes=seg_bytes)[0], a, seg_bytes)


def test_encoder_refuses_what_it_cannot_read():
    a = PR.sinusoid_image(8, 8, 3, 0.0, 1)
    arena, entries = _arena_of([a])
    wide = torch.zeros(2 * arena.numel(), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        png.encode_device(wide[::2], entries)                        # a non-contiguous arena
    with pytest.raises(RuntimeError):
        png.encode_device(arena.cpu(), entries)                      # not on the device
    with pytest.raises(RuntimeError):
        png.encode_device(arena.to(torch.int32), entries)
    with pytest.raises(ValueError):
        png.encode_device(arena, [(8,) + a.shape])                   # past the arena's end
    with pytest.raises(ValueError):
        png.encode_device(arena, entries, seg_bytes=1000)


SIZE_CASES = {"sin-0": (256, 256, 3, 0.0), "sin-0.01": (256, 256, 3, 0.01), "sin-0.03": (256, 256, 3, 0.03),
              "rgba": (128, 128, 4, 0.0)}


@pytest.mark.parametrize("name", sorted(SIZE_CASES))
def test_files_are_not_larger_than_the_host_path(name, tmp_path):
    """Against utils.write_png (filter 0, zlib level 6) of the same pixels: adaptive filters, distance-1 runs and one
    dynamic code per 32 KiB segment must not lose to it on image-like content."""
    h, w, c, sigma = SIZE_CASES[name]
    a = PR.sinusoid_image(h, w, c, sigma, seed=h + c)
    arena, entries = _arena_of([a])
    blob = png.encode_device(arena, entries)[0]
    _check_file(blob, a, png.SEG_BYTES)
    host = os.path.getsize(utils.write_png(a, str(tmp_path / "host.png")))
    print("%s: device %d bytes, host %d bytes" % (name, len(blob), host))
    assert len(blob) <= host


# ---------------------------------------------------------------- model level
def test_save_samples_under_the_variable_writes_the_same_pixels(tmp_path, monkeypatch):
    from tests.test_gpu_sampling import _assert_untouched, _sampling_model, _snapshot
    monkeypatch.delenv("BG_DEVICE_PNG", raising=False)
    gan = _sampling_model(tmp_path)
    snap = _snapshot(gan)
    host = {os.path.basename(p): open(p, "rb").read() for p in gan.save_samples(0, 1)}
    monkeypatch.setenv("BG_DEVICE_PNG", "1")
    dev = {os.path.basename(p): open(p, "rb").read() for p in gan.save_samples(0, 1)}
    _assert_untouched(gan, snap)
    assert sorted(dev) == sorted(host) and len(dev) == 4
    for name in sorted(host):
        want = data.decode_png(host[name])
        assert np.array_equal(data.decode_png(dev[name]), want), name
        assert zlib.decompress(png.idat_payload(dev[name])) == PR.filter_rows(want).tobytes(), name
        assert dev[name] != host[name] and want.std() > 0
    assert {os.path.basename(p): open(p, "rb").read() for p in gan.save_samples(0, 1)} == dev
    monkeypatch.delenv("BG_DEVICE_PNG")
    assert {os.path.basename(p): open(p, "rb").read() for p in gan.save_samples(0, 1)} == host
    _assert_untouched(gan, snap)


def test_service_round_under_the_variable(tmp_path, monkeypatch):
    """Three request files, one of them a single latent, answered with the variable unset and set: equal strips, identical
    .out files, and per request the order .out, NAME.tmp.png -> NAME.png, removal of the request."""
    from tests.test_gpu_service import _latents, _model, _quit, _snapshot, _assert_untouched, _write_request
    monkeypatch.delenv("BG_DEVICE_PNG", raising=False)
    gan = _model(tmp_path, n_labels=3)
    lat = {"a": _latents(gan, 1, 1), "b": _latents(gan, 5, 2), "c": _latents(gan, 2, 3)}
    gan.save(gan.checkpoint_dir, gan.counter)
    snap = _snapshot(gan)
    rdir = gan.args.request_dir

    def one_round(log=None):
        for k, (z, cls) in lat.items():
            _write_request(gan, k, z, cls, ["use_discriminator=1"])
        _quit(gan)
        if log is not None:
            real_rename, real_remove, real_vectors = os.rename, os.remove, utils.write_vectors
            monkeypatch.setattr(os, "rename", lambda a, b: (log.append(("rename", os.path.basename(a),
                                                                        os.path.basename(b))), real_rename(a, b))[1])
            monkeypatch.setattr(os, "remove", lambda a: (log.append(("remove", os.path.basename(a))), real_remove(a))[1])
            monkeypatch.setattr(utils, "write_vectors", lambda p, rows: (log.append(("out", os.path.basename(p))),
                                                                         real_vectors(p, rows))[1])
        assert gan.service() == 3
        files = {f: open(os.path.join(rdir, f), "rb").read() for f in sorted(os.listdir(rdir))}
        for f in files:
            os.remove(os.path.join(rdir, f))
        return files
    host = one_round()
    monkeypatch.setenv("BG_DEVICE_PNG", "1")
    log = []
    dev = one_round(log)
    monkeypatch.undo()
    _assert_untouched(gan, snap)
    assert sorted(dev) == sorted(host) and sum(f.endswith(".png") for f in dev) == 3
    assert not any(f.endswith((".txt", ".tmp.png", ".err")) for f in dev)
    for f in sorted(host):
        if f.endswith(".out"):
            assert dev[f] == host[f], f
        else:
            want = data.decode_png(host[f])
            assert want.shape == (64, 64 * lat[f[0]][0].shape[0], 3) and want.std() > 0
            assert np.array_equal(data.decode_png(dev[f]), want), f
            assert zlib.decompress(png.idat_payload(dev[f])) == PR.filter_rows(want).tobytes(), f
            assert dev[f] != host[f]
    for k in lat:
        outs = [i for i, e in enumerate(log) if e[0] == "out" and e[1].startswith(k + "_")]
        ren = log.index(("rename", k + ".tmp.png", k + ".png"))
        rem = log.index(("remove", k + ".txt"))
        assert outs and max(outs) < ren < rem, (k, log)
