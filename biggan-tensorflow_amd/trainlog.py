"""Training logs of the reference (BigGAN.py:1011-1019, 1100-1104; utils.py:291-294, 322-333): a TensorBoard event file
under ``<log_dir>/<model_dir>/`` with one scalar per loss every iteration and a histogram of every variable every
``--histogram_freq`` iterations.

TensorFlow and TensorBoard are not dependencies: the file format (TFRecord framing with masked CRC-32C, the ``Event`` /
``Summary`` / ``HistogramProto`` messages) and the histogram rule (TF 1.x ``core/lib/histogram/histogram.cc``: 1551 bucket
limits, ``upper_bound``, run-collapsed encoding) are restated here; DESIGN.md ("Training logs") lists them and says what is
unpinned.

``EventWriter``          the file: version record, ``add_scalars``, ``add_histograms``, ``flush``, ``close``
``VariableHistograms``   histograms of every entry of ``store.vars``; on a CUDA store one ``bg_var_hist`` launch over the
                         flat arenas (csrc/varhist.hip) and a copy of the counts, on a CPU store (or with
                         ``BG_DEVICE_HIST=0``) the same rule in NumPy on host copies of the variables
"""
import ctypes
import os
import socket
import struct
import sys
import time

import numpy as np
import torch

DBL_MAX = sys.float_info.max
N_LIMITS = 1551
ZERO_BUCKET = 775            # limits[775] == 0.0; +-0.0 and positive denormals fall into bucket 776


# ------------------------------------------------------------------------------------------
# bucket limits (histogram.cc InitDefaultBucketsInner)
# ------------------------------------------------------------------------------------------
def _build_limits():
    pos = []
    v = 1e-12
    while v < 1e20:                 # repeated double multiplication, not pow(): the table is defined by this loop
        pos.append(v)
        v *= 1.1
    return np.array([-DBL_MAX] + [-x for x in reversed(pos)] + [0.0] + pos + [DBL_MAX], dtype=np.float64)


_LIMITS = None


def bucket_limits():
    """The 1551 bucket limits as float64 (read-only; built once)."""
    global _LIMITS
    if _LIMITS is None:
        lim = _build_limits()
        assert lim.shape == (N_LIMITS,)
        lim.setflags(write=False)
        _LIMITS = lim
    return _LIMITS


def collapse(counts, limits=None):
    """Histogram::EncodeToProto(preserve_zero_buckets=false): every non-empty bucket as (limit, count); every run of
    empty buckets as ONE entry that carries the run's last limit and count 0.  ``counts`` [n_limits] or
    [n, n_limits]; returns (limits, counts) as float64 arrays, or a list of such pairs for a 2-D input."""
    limits = bucket_limits() if limits is None else np.asarray(limits, np.float64)
    c = np.asarray(counts)
    single = c.ndim == 1
    c2 = c.reshape(1, -1) if single else c
    nz = c2 > 0
    nxt = np.ones_like(nz)                      # "the next bucket is non-empty, or there is none"
    nxt[:, :-1] = nz[:, 1:]
    keep = nz | nxt
    rows, cols = np.nonzero(keep)               # row-major: per row, ascending buckets
    lim = limits[cols]
    cnt = np.where(nz[rows, cols], c2[rows, cols], 0).astype(np.float64)
    ends = np.cumsum(keep.sum(axis=1))
    out, a = [], 0
    for b in ends:
        out.append((lim[a:b], cnt[a:b]))
        a = b
    return out[0] if single else out


# ------------------------------------------------------------------------------------------
# CRC-32C and the TFRecord frame (lib/io/record_writer.cc)
# ------------------------------------------------------------------------------------------
_CRC_TABLE = None


def crc32c_py(data, crc=0):
    """Table-driven CRC-32C (Castagnoli) in Python: the fallback of ``crc32c`` and its cross-check."""
    global _CRC_TABLE
    if _CRC_TABLE is None:
        t = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
            t.append(c)
        _CRC_TABLE = t
    t = _CRC_TABLE
    c = crc ^ 0xFFFFFFFF
    for b in bytes(data):
        c = (c >> 8) ^ t[(c ^ b) & 255]
    return c ^ 0xFFFFFFFF


_crc_native = None


def crc32c(data, crc=0):
    """CRC-32C of ``data``: ``bg_crc32c`` when the library loads, the Python loop otherwise (identical results)."""
    global _crc_native
    if _crc_native is None:
        try:
            from . import hip
            _crc_native = hip.lib().bg_crc32c
        except (ImportError, OSError, AttributeError):
            _crc_native = False
    data = bytes(data)
    if _crc_native:
        return int(_crc_native(data, len(data), crc)) & 0xFFFFFFFF
    return crc32c_py(data, crc)


def masked_crc(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


def tfrecord(data):
    """uint64 length | uint32 masked crc of those 8 bytes | data | uint32 masked crc of data (little-endian)."""
    head = struct.pack("<Q", len(data))
    return head + struct.pack("<I", masked_crc(head)) + data + struct.pack("<I", masked_crc(data))


# ------------------------------------------------------------------------------------------
# protobuf wire format (event.proto, summary.proto), hand-written
# ------------------------------------------------------------------------------------------
def _varint(n):
    n &= 0xFFFFFFFFFFFFFFFF          # int64 fields: two's complement, ten bytes when negative
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field, wire):
    return _varint((field << 3) | wire)


def _f_double(field, v):
    return _key(field, 1) + struct.pack("<d", v)


def _f_float(field, v):
    return _key(field, 5) + struct.pack("<f", v)


def _f_varint(field, v):
    return _key(field, 0) + _varint(int(v))


def _f_bytes(field, b):
    return _key(field, 2) + _varint(len(b)) + b


def _f_double_opt(field, v):
    """proto3 scalar outside a oneof: a zero is not written."""
    v = float(v)
    return b"" if struct.pack("<d", v) == b"\0" * 8 else _f_double(field, v)


def encode_histogram(hist):
    """HistogramProto: min 1, max 2, num 3, sum 4, sum_squares 5, bucket_limit 6, bucket 7 (packed doubles)."""
    mn, mx, num, s, sq, limits, counts = hist
    limits = np.ascontiguousarray(limits, dtype="<f8")
    counts = np.ascontiguousarray(counts, dtype="<f8")
    return (_f_double_opt(1, mn) + _f_double_opt(2, mx) + _f_double_opt(3, num) + _f_double_opt(4, s) +
            _f_double_opt(5, sq) + _f_bytes(6, limits.tobytes()) + _f_bytes(7, counts.tobytes()))


def encode_event(wall_time, step=0, file_version=None, values=None):
    """Event: wall_time 1 (double), step 2 (int64), file_version 3 | summary 5.  ``values``: encoded Summary.Value's."""
    out = _f_double(1, float(wall_time))
    if step:
        out += _f_varint(2, step)
    if file_version is not None:
        out += _f_bytes(3, file_version.encode())
    if values is not None:
        out += _f_bytes(5, b"".join(_f_bytes(1, v) for v in values))           # Summary: value 1 (repeated)
    return out


def scalar_value(tag, v):
    return _f_bytes(1, tag.encode()) + _f_float(2, float(v))                   # Summary.Value: tag 1, simple_value 2


def histogram_value(tag, hist):
    return _f_bytes(1, tag.encode()) + _f_bytes(5, encode_histogram(hist))     # Summary.Value: tag 1, histo 5


class EventWriter:
    """``tf.summary.FileWriter`` without the graph: ``<dir>/events.out.tfevents.<int(time)>.<hostname>``, a new file per
    writer, first record ``Event(wall_time, file_version="brain.Event:2")``."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        base = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(time.time()), socket.gethostname()))
        path, k = base, 0
        while os.path.exists(path):              # a second run within the same second still gets a file of its own
            k += 1
            path = "%s.%d" % (base, k)
        self.path = path
        self._f = open(path, "xb")
        self._write(encode_event(time.time(), file_version="brain.Event:2"))
        self.flush()

    def _write(self, event):
        self._f.write(tfrecord(event))

    def add_scalars(self, step, scalars):
        """One Event whose Summary carries one simple_value per entry of ``scalars`` (tag -> float)."""
        self._write(encode_event(time.time(), step, values=[scalar_value(k, v) for k, v in scalars.items()]))

    def add_histograms(self, step, hists):
        """One Event whose Summary carries one histogram per (tag, (min, max, num, sum, sum_squares, limits, counts))."""
        self._write(encode_event(time.time(), step, values=[histogram_value(k, h) for k, h in hists]))

    def flush(self):
        if self._f is not None:
            self._f.flush()

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None


# ------------------------------------------------------------------------------------------
# variable histograms
# ------------------------------------------------------------------------------------------
def histogram_tag(name):
    """tf.summary.histogram(var.name + '/hist'): ``name:0/hist``, and TF 1.x replaces the illegal ':' by '_'."""
    return name + "_0/hist"


def host_histogram(x, limits=None):
    """The rule on the host: (counts [n_limits] int64, stats [6] float64 = min, max, num, sum, sum_squares, nonfinite)
    of one array; non-finite elements are counted in stats[5] only."""
    limits = bucket_limits() if limits is None else limits
    x = np.asarray(x, dtype=np.float32).ravel()
    fin = np.isfinite(x)
    d = x[fin].astype(np.float64)
    counts = np.bincount(np.searchsorted(limits, d, side="right"), minlength=len(limits))
    if d.size:
        stats = [d.min(), d.max(), float(d.size), d.sum(), (d * d).sum(), float(x.size - d.size)]
    else:
        stats = [DBL_MAX, -DBL_MAX, 0.0, 0.0, 0.0, float(x.size)]
    return counts, np.array(stats, dtype=np.float64)


class VariableHistograms:
    """Histograms of every entry of ``store.vars`` (trainables as arena views, plus u, pop_mean / pop_var, the moving
    statistics, the renorm variables, alphahelper_w); Adam slots and EMA shadows are not variables of the store, as they
    are left out by the reference (utils.py:327).

    Device path: the item table is compiled into a plan and uploaded here, once; ``compute()`` is one ``bg_var_hist``
    call on the current stream, one copy of counts and statistics into pinned memory, and the collapse on the host."""

    def __init__(self, store, device=None, device_path=None):
        self.store = store
        self.names = list(store.vars.keys())
        self.tags = [histogram_tag(n) for n in self.names]
        self.limits = bucket_limits()
        self.device = torch.device(device if device is not None else store.device)
        if device_path is None:
            device_path = self.device.type == "cuda" and os.environ.get("BG_DEVICE_HIST", "1") != "0"
        self.device_path = bool(device_path)
        self.nonfinite = {}                     # name -> count, of the last compute()
        self._ptrs = None
        if self.device_path:
            self._upload()

    # ---- device path ----------------------------------------------------------------------
    def _tensors(self):
        out = []
        for n in self.names:
            t = self.store.vars[n]
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise RuntimeError("variable %s is not a contiguous fp32 CUDA tensor" % n)
            out.append(t)
        return out

    def _upload(self):
        from . import hip
        L = hip.lib()
        tensors = self._tensors()
        n = len(tensors)
        items = (hip.BgHistItem * n)()
        for it, t in zip(items, tensors):
            it.x, it.n = t.data_ptr(), t.numel()
        nc = hip.c_int(0)
        hip.check(L.bg_var_hist_plan_chunks(items, n, ctypes.byref(nc)))
        n_chunks = nc.value
        plan = np.zeros(int(L.bg_var_hist_plan_bytes(n, n_chunks)) // 8, dtype=np.int64)
        hip.check(L.bg_var_hist_plan(items, n, plan.ctypes.data_as(hip.c_void_p), plan.nbytes))
        dev = self.device
        self._n, self._n_chunks = n, n_chunks
        self._plan = torch.from_numpy(plan).to(dev)
        self._limits_dev = torch.from_numpy(np.array(self.limits)).to(dev)
        self._counts = torch.empty(n, N_LIMITS, dtype=torch.int32, device=dev)          # (uint32 bits)
        self._stats = torch.empty(n, 6, dtype=torch.float64, device=dev)
        self._ws_bytes = int(L.bg_var_hist_workspace_bytes(n, n_chunks))
        self._ws = torch.empty(max(self._ws_bytes // 8, 1), dtype=torch.float64, device=dev)
        self._counts_h = torch.empty(n, N_LIMITS, dtype=torch.int32).pin_memory()
        self._stats_h = torch.empty(n, 6, dtype=torch.float64).pin_memory()
        self._ptrs = [t.data_ptr() for t in tensors]

    def launch(self):
        """Enqueue the histogram kernels on the current stream (nothing is copied, nothing waits)."""
        from . import hip
        if [self.store.vars[n].data_ptr() for n in self.names] != self._ptrs:
            self._upload()                      # (a variable was re-bound since: compile the plan again)
        hip.check(hip.lib().bg_var_hist(hip.ptr(self._plan), self._n, self._n_chunks, hip.ptr(self._limits_dev), N_LIMITS,
                                        hip.ptr(self._counts), hip.ptr(self._stats), hip.ptr(self._ws), self._ws_bytes,
                                        hip.stream()))

    def fetch(self):
        """Counts [n, 1551] (uint32) and statistics [n, 6] of the last launch, copied to pinned memory and waited for."""
        self._counts_h.copy_(self._counts, non_blocking=True)
        self._stats_h.copy_(self._stats, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self._counts_h.numpy().view(np.uint32), self._stats_h.numpy()

    # ---- host path ------------------------------------------------------------------------
    def host_counts(self):
        n = len(self.names)
        counts = np.zeros((n, N_LIMITS), dtype=np.int64)
        stats = np.zeros((n, 6), dtype=np.float64)
        for i, name in enumerate(self.names):
            counts[i], stats[i] = host_histogram(self.store.vars[name].detach().cpu().numpy(), self.limits)
        return counts, stats

    # ---- both -----------------------------------------------------------------------------
    def finish(self, counts, stats, warn=True):
        """[(tag, (min, max, num, sum, sum_squares, limits, counts))] in the collapsed encoding.  A variable with
        non-finite elements gets no histogram (TF's histogram op would abort the run): one warning names it."""
        self.nonfinite = {}
        out = []
        for i, (lim, cnt) in enumerate(collapse(counts, self.limits)):
            bad = int(stats[i, 5])
            if bad:
                self.nonfinite[self.names[i]] = bad
                if warn:
                    print("warning: %s has %d non-finite element%s: no histogram for it in this event"
                          % (self.names[i], bad, "" if bad == 1 else "s"), flush=True)
                continue
            s = stats[i]
            out.append((self.tags[i], (float(s[0]), float(s[1]), float(s[2]), float(s[3]), float(s[4]), lim, cnt)))
        return out

    def compute(self, warn=True):
        if self.device_path:
            self.launch()
            counts, stats = self.fetch()
        else:
            counts, stats = self.host_counts()
        return self.finish(counts, stats, warn)
