"""The input pipeline on the GPU box: BatchLoader's host path (decode, resize, flip, normalise on the CPU, fp32 batches
over the bus) against its device path (decode only, uint8 over the bus, bg_image_batch_u8) in the same process.

    python tools/input_bench.py loader [--src 160] [--size 128] [--files 512] [--batches 64,256] [--workers 1,4,8,16]
    python tools/input_bench.py kernel [--src 160] [--size 128] [--batch 256] [--reps 200]
    python tools/input_bench.py train  [--src 160] [--files 1024] [--batch 256] [--iters 20] [--workers 8]
                                       [--img_size 128 --ch 96 --precision bf16]

Every mode synthesises its dataset (RGB PNG files of --src x --src pixels: a smooth pattern plus noise, so that inflate
has real work) in a temporary folder and reads nothing else.  One JSON line per measurement:

    loader   images/s of ``next(loader)`` per path, worker count and batch size, each after two untimed batches and over
             at least 12 batches (the queue holds 4), ending in a device synchronise; ``raw_over_out`` is the ratio of
             packed uint8 bytes to fp32 output bytes of the device path
    kernel   bg_image_batch_u8 alone for C = 3 and C = 4: microseconds per launch between two device events around
             --reps launches, and GB/s over the bytes it reads (pixels + table) and writes
    train    ms per training iteration (defaults: BASELINE config 3 at 256 images) fed by the host path, by the device
             path and by synthetic batches

The measurement runs in a child process under its own time limit (--timeout seconds); worker counts are capped at 16.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _dataset(root, name, files, src, channels=3, seed=0):
    import numpy as np
    from biggan_tensorflow_amd import utils
    folder = os.path.join(root, "dataset", name)
    os.makedirs(folder)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:src, 0:src].astype(np.float32) / src
    for i in range(files):
        ph = rng.uniform(0, 6.28, 3)
        base = np.stack([np.sin(6 * xx + ph[0]) + np.cos(4 * yy + ph[1]), np.sin(5 * yy + ph[2]) * np.cos(3 * xx),
                         xx - yy], axis=2) * 60 + 128
        img = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        if channels == 4:
            img = np.concatenate([img, np.full((src, src, 1), 255, np.uint8)], axis=2)
        utils.write_png(img, os.path.join(folder, "%05d.png" % i))
    return os.path.join(root, "dataset")


def _ints(s):
    return [int(v) for v in s.split(",") if v]


def _loader(a, tmp):
    import torch
    from biggan_tensorflow_amd import data as D
    root = _dataset(tmp, "bench", a.files, a.src)
    files, _ = D.load_data("bench", "", root=root)
    ratio = (-(-(a.src * a.src * 3) // 16) * 16) / float(a.size * a.size * 3 * 4)
    for batch in _ints(a.batches):
        for workers in _ints(a.workers):
            workers = min(workers, 16)
            for path in ("host", "device", "host", "device"):             # alternating: each path twice
                ld = D.BatchLoader(files, None, batch, D.ImageData(a.size, 3, True, True, seed=1), "cuda", seed=2,
                                   workers=workers, device_preprocess=(path == "device"))
                try:
                    for _ in range(2):
                        x = next(ld)
                    torch.cuda.synchronize()
                    count = max(12, -(-a.min_images // batch))
                    t0 = time.perf_counter()
                    for _ in range(count):
                        x = next(ld)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    ld.close()
                assert tuple(x.shape) == (batch, a.size, a.size, 3)
                print(json.dumps({"mode": "loader", "path": path, "src": a.src, "size": a.size, "batch": batch,
                                  "workers": workers, "batches": count, "images_per_s": round(batch * count / dt, 1),
                                  "raw_over_out": round(ratio, 3)}), flush=True)


def _kernel(a, tmp):
    import numpy as np
    import torch
    from biggan_tensorflow_amd import data as D, functional as Fn
    rng = np.random.default_rng(0)
    for c in (3, 4):
        imgs = [rng.integers(0, 256, (a.src, a.src, c), dtype=np.uint8) for _ in range(a.batch)]
        raw, table, geom = D.pack_batch(imgs, [i % 2 for i in range(a.batch)], a.size, c, pin=True)
        raw_d, table_d = raw.cuda(), table.cuda()
        out = torch.empty(a.batch, a.size, a.size, c, device="cuda")
        for _ in range(20):
            Fn.image_batch_u8(raw_d, table_d, a.batch, a.size, c, out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            Fn.image_batch_u8(raw_d, table_d, a.batch, a.size, c, out=out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.reps
        moved = a.batch * a.src * a.src * c + table.numel() * 4 + out.numel() * 4
        h2d0 = time.perf_counter()
        for _ in range(10):
            raw.to("cuda", non_blocking=True)
        torch.cuda.synchronize()
        h2d_us = (time.perf_counter() - h2d0) * 1e5
        print(json.dumps({"mode": "kernel", "channels": c, "batch": a.batch, "src": a.src, "size": a.size, "reps": a.reps,
                          "us_per_launch": round(us, 2), "bytes_read_and_written": moved,
                          "gb_per_s": round(moved / us / 1e3, 1), "raw_bytes": raw.numel(),
                          "h2d_copy_of_raw_us": round(h2d_us, 1)}), flush=True)


def _train(a, tmp):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from biggan_tensorflow_amd import data as D, main as M, model, scope as S
    root = _dataset(tmp, "bench", a.files, a.src)
    files, _ = D.load_data("bench", "", root=root)
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    gan.settle_host()
    workers = min(a.workers, 16)
    for feed in ("synthetic", "host", "device", "synthetic", "host", "device"):
        ld = None
        if feed != "synthetic":
            ld = D.BatchLoader(files, None, a.batch, D.ImageData(a.img_size, 3, True, True, seed=1), "cuda", seed=2,
                               workers=workers, device_preprocess=(feed == "device"))
        nxt = (lambda: next(ld)) if ld is not None else (lambda: gan.synthetic_batch())
        try:
            for _ in range(3):
                gan.train_step(nxt())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                gan.train_step(nxt())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            if ld is not None:
                ld.close()
        print(json.dumps({"mode": "train", "feed": feed, "img_size": a.img_size, "ch": a.ch, "batch": a.batch,
                          "precision": a.precision, "src": a.src, "workers": workers, "iters": a.iters,
                          "ms_per_iter": round(dt / a.iters * 1e3, 2),
                          "images_per_s": round(a.batch * a.iters / dt, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("loader", "kernel", "train"))
    ap.add_argument("--src", type=int, default=160, help="side of the source images")
    ap.add_argument("--size", type=int, default=128, help="side of the batch (loader, kernel)")
    ap.add_argument("--files", type=int, default=0, help="files of the synthetic dataset (default 512; train 1024)")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--workers", default="", help="decode threads: a list for loader (default 1,4,8,16), one for train (8)")
    ap.add_argument("--min_images", type=int, default=1024, help="loader: time at least this many images per line")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--timeout", type=int, default=540, help="time limit of the GPU step, seconds")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.files = a.files or (1024 if a.mode == "train" else 512)
    if a.mode == "train":
        a.workers = int(a.workers or 8)
    else:
        a.workers = a.workers or "1,4,8,16"
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("input_bench: no GPU (there is nothing to measure without one)")
        import biggan_tensorflow_amd  # noqa: F401
        return {"loader": _loader, "kernel": _kernel, "train": _train}[a.mode](a, a.child)
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k) or 16)))
    tmp = tempfile.mkdtemp(prefix="input_bench_")
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child", tmp]
    try:
        rc = subprocess.run(cmd, env=env, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("input_bench: the GPU step ran past its %d s limit" % a.timeout)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if rc != 0:
        raise SystemExit("input_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
