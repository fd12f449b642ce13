"""Time one histogram event of the training log (trainlog.VariableHistograms + EventWriter) and split it.

    python tools/log_bench.py [--img_size 128 --ch 96 --batch 32 --precision bf16] [--reps 5] [--timeout 300]

Defaults are BASELINE config 3 (128^2, ch 96, bf16).  Prints one JSON line, ms per event (mean of --reps after one untimed
pass), for the device path and, in the same process, for the host path it replaces (BG_DEVICE_HIST=0):

    device.kernel_ms     bg_var_hist: zero-fill, the histogram kernel and the finalise kernel, between two device events
    device.copy_ms       counts [n,1551] uint32 and statistics [n,6] into pinned memory, and the wait for them
    device.write_ms      collapse of the empty runs, protobuf encoding, CRCs and the file write
    device.event_ms      the whole event as the training loop runs it (compute() + add_histograms())
    host.counts_ms       every variable copied to the host and bucketed there with NumPy (searchsorted + bincount)
    host.write_ms, host.event_ms   as above
    scalar_event_ms      one add_scalars() event of four losses

The measurement runs in a child process under its own time limit (--timeout seconds); host work uses at most 16 threads.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _measure(a):
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import main as M, model, scope as S, trainlog as T
    out_dir = tempfile.mkdtemp(prefix="log_bench_")
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--log_dir", out_dir]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    writer = T.EventWriter(os.path.join(out_dir, gan.model_dir))
    dev = T.VariableHistograms(gan.store, device_path=True)
    host = T.VariableHistograms(gan.store, device_path=False)
    elements = sum(t.numel() for t in gan.store.vars.values())

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.reps, r

    def kernel_ms():
        dev.launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            dev.launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    k_ms = kernel_ms()
    copy_ms, (counts, stats) = timed(dev.fetch)
    write_ms, _ = timed(lambda: writer.add_histograms(0, dev.finish(counts, stats)))
    event_ms, _ = timed(lambda: writer.add_histograms(0, dev.compute()))
    h_counts_ms, (h_counts, h_stats) = timed(host.host_counts)
    h_write_ms, _ = timed(lambda: writer.add_histograms(0, host.finish(h_counts, h_stats)))
    h_event_ms, _ = timed(lambda: writer.add_histograms(0, host.compute()))
    losses = {"d_loss": 1.0, "g_loss": 2.0, "d_cls_loss": 3.0, "g_cls_loss": 4.0}
    scalar_ms, _ = timed(lambda: writer.add_scalars(1, losses))
    writer.close()
    res = {"img_size": a.img_size, "ch": a.ch, "precision": a.precision, "reps": a.reps,
           "variables": len(dev.names), "elements": int(elements), "chunks": int(dev._n_chunks),
           "device": {"kernel_ms": round(k_ms, 4), "kernel_GBps": round(elements * 4 / k_ms / 1e6, 1),
                      "copy_ms": round(copy_ms, 3), "write_ms": round(write_ms, 3), "event_ms": round(event_ms, 3)},
           "host": {"counts_ms": round(h_counts_ms, 3), "write_ms": round(h_write_ms, 3), "event_ms": round(h_event_ms, 3)},
           "scalar_event_ms": round(scalar_ms, 4),
           "counts_equal": bool(np.array_equal(counts.astype(np.int64), h_counts)),
           "min_max_num_equal": bool(np.array_equal(stats[:, :3], h_stats[:, :3])),
           "event_file_bytes": os.path.getsize(writer.path)}
    os.remove(writer.path)
    os.removedirs(os.path.dirname(writer.path))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="time limit of the GPU step, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return _measure(a)
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k) or 16)))
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    try:
        rc = subprocess.run(cmd, env=env, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("log_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("log_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
