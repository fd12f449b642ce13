"""Reference for the training-log tests, independent of biggan_tensorflow_amd.trainlog (it imports nothing from it):

* the histogram rule of TF 1.x ``core/lib/histogram/histogram.cc`` restated in NumPy: the table loop,
  ``searchsorted(side='right')`` (= upper_bound), ``math.fsum`` statistics, the run-collapsed encoding;
* a bitwise CRC-32C (Castagnoli) and the TFRecord mask;
* a generic protobuf wire-format parser, a TFRecord reader that verifies both CRCs of every record, and decoders for
  ``Event`` / ``Summary`` / ``HistogramProto`` by field number.
"""
import math
import struct
import sys

import numpy as np

DBL_MAX = sys.float_info.max


def limits():
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    neg = [-x for x in pos]
    neg.reverse()
    return np.array([-DBL_MAX] + neg + [0.0] + pos + [DBL_MAX], dtype=np.float64)


LIMITS = limits()


def histogram(x):
    """dict(counts [1551] int64, min, max, num, sum, sum_squares, nonfinite, abs_sum) of the finite elements of x."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    fin = np.isfinite(x)
    d = x[fin].astype(np.float64)
    b = np.searchsorted(LIMITS, d, side="right")
    counts = np.zeros(len(LIMITS), dtype=np.int64)
    np.add.at(counts, b, 1)
    vals = d.tolist()
    return dict(counts=counts,
                min=min(vals) if vals else DBL_MAX, max=max(vals) if vals else -DBL_MAX, num=float(len(vals)),
                sum=math.fsum(vals), sum_squares=math.fsum(v * v for v in vals),
                nonfinite=int(x.size - d.size), abs_sum=math.fsum(abs(v) for v in vals))


def collapse(counts, lim=None):
    """EncodeToProto(preserve_zero_buckets=false), the loop as written: [(end, count)]."""
    lim = LIMITS if lim is None else lim
    n = len(counts)
    out = []
    i = 0
    while i < n:
        end, count = float(lim[i]), float(counts[i])
        i += 1
        if count <= 0:
            while i < n and counts[i] <= 0:
                end, count = float(lim[i]), float(counts[i])
                i += 1
        out.append((end, count))
    return out


def sum_bounds(h):
    """The issue's tolerances: |sum - fsum| <= 2 n 2^-53 sum|x|, |sum_squares - fsum| <= 2 n 2^-53 sum x^2."""
    n = max(h["num"], 1.0)
    return 2.0 * n * 2.0 ** -53 * h["abs_sum"], 2.0 * n * 2.0 ** -53 * h["sum_squares"]


# ------------------------------------------------------------------------------------------ CRC-32C
def crc32c(data, crc=0):
    c = crc ^ 0xFFFFFFFF
    for byte in bytes(data):
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
    return c ^ 0xFFFFFFFF


def masked(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------ TFRecord
def read_records(path):
    """The data of every record of the file; raises AssertionError when a length CRC or a data CRC does not verify or the
    file ends inside a record."""
    raw = open(path, "rb").read()
    out, pos = [], 0
    while pos < len(raw):
        assert pos + 12 <= len(raw), "truncated header"
        head = raw[pos:pos + 8]
        (n,) = struct.unpack("<Q", head)
        (hc,) = struct.unpack("<I", raw[pos + 8:pos + 12])
        assert hc == masked(head), "length crc"
        assert pos + 12 + n + 4 <= len(raw), "truncated record"
        data = raw[pos + 12:pos + 12 + n]
        (dc,) = struct.unpack("<I", raw[pos + 12 + n:pos + 16 + n])
        assert dc == masked(data), "data crc"
        out.append(data)
        pos += 16 + n
    return out


# ------------------------------------------------------------------------------------------ protobuf
def parse(buf):
    """[(field, wire_type, value)]: varint -> int, 64-bit -> 8 bytes, length-delimited -> bytes, 32-bit -> 4 bytes."""
    out, pos = [], 0

    def varint():
        nonlocal pos
        v, shift = 0, 0
        while True:
            b = buf[pos]
            pos += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                return v

    while pos < len(buf):
        key = varint()
        field, wire = key >> 3, key & 7
        if wire == 0:
            out.append((field, wire, varint()))
        elif wire == 1:
            out.append((field, wire, buf[pos:pos + 8]))
            pos += 8
        elif wire == 2:
            n = varint()
            out.append((field, wire, buf[pos:pos + n]))
            pos += n
        elif wire == 5:
            out.append((field, wire, buf[pos:pos + 4]))
            pos += 4
        else:
            raise AssertionError("wire type %d" % wire)
        assert pos <= len(buf)
    return out


def _dbl(b):
    return struct.unpack("<d", b)[0]


def decode_histogram(buf):
    h = dict(min=0.0, max=0.0, num=0.0, sum=0.0, sum_squares=0.0, bucket_limit=[], bucket=[])
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
    for field, wire, v in parse(buf):
        if field in names:
            assert wire == 1
            h[names[field]] = _dbl(v)
        elif field in (6, 7):
            assert wire == 2 and len(v) % 8 == 0
            h["bucket_limit" if field == 6 else "bucket"] += list(struct.unpack("<%dd" % (len(v) // 8), v))
        else:
            raise AssertionError("HistogramProto field %d" % field)
    return h


def decode_event(buf):
    """dict(wall_time, step, file_version or None, values = [(tag, 'scalar', float32) | (tag, 'histo', dict)])."""
    ev = dict(wall_time=0.0, step=0, file_version=None, values=None)
    for field, wire, v in parse(buf):
        if field == 1:
            assert wire == 1
            ev["wall_time"] = _dbl(v)
        elif field == 2:
            assert wire == 0
            ev["step"] = v - (1 << 64) if v >> 63 else v
        elif field == 3:
            assert wire == 2
            ev["file_version"] = v.decode()
        elif field == 5:
            assert wire == 2
            ev["values"] = []
            for f2, w2, val in parse(v):
                assert f2 == 1 and w2 == 2, "Summary.value"
                tag, item = None, None
                for f3, w3, x in parse(val):
                    if f3 == 1:
                        tag = x.decode()
                    elif f3 == 2:
                        assert w3 == 5
                        item = ("scalar", np.frombuffer(x, dtype="<f4")[0])
                    elif f3 == 5:
                        assert w3 == 2
                        item = ("histo", decode_histogram(x))
                    else:
                        raise AssertionError("Summary.Value field %d" % f3)
                ev["values"].append((tag,) + item)
        else:
            raise AssertionError("Event field %d" % field)
    return ev


def read_events(path):
    return [decode_event(r) for r in read_records(path)]
