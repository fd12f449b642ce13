"""JPEG input on the GPU box: BatchLoader's host path (entropy decode in C, then IDCT, upsampling and colour in numpy,
resize, flip, normalise on the CPU, fp32 batches over the bus) against its device path (entropy decode only, int16
coefficients over the bus, bg_jpeg_batch_u8 + bg_image_batch_u8) in the same process.

    python tools/jpeg_bench.py loader [--srcs 160,512] [--size 128] [--files 128] [--batch 64] [--workers 8]
    python tools/jpeg_bench.py kernel [--srcs 160,512] [--size 128] [--batch 64] [--reps 50]

Both modes synthesise their datasets with Pillow (RGB JPEG files at quality 90, 4:2:0 and 4:4:4: a smooth pattern plus
noise) in a temporary folder and read nothing else; without Pillow there is nothing to measure and the tool says so.  One
JSON line per measurement:

    loader   images/s of ``next(loader)`` per source size, sampling and path (``BG_DEVICE_INPUT=0`` is the host path), each
             after two untimed batches, ending in a device synchronise; ``upload_over_out`` is the ratio of the bytes the
             device path uploads (coefficients and tables) to the fp32 bytes of the batch, what ``device_path_pays`` sees
    kernel   bg_jpeg_batch_u8 alone: microseconds per call between two device events around --reps calls, the split
             between its kernels from the profiler's kernel records where it has them, and GB/s over the bytes each stage
             reads and writes (IDCT: coefficients in, planes out; colour: planes in, pixels out)

The measurement runs in a child process under its own time limit (--timeout seconds); worker counts are capped at 16.
"""
import argparse
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SUBSAMPLING = {"420": 2, "444": 0}


def _jpeg_bytes(src, sampling, count, seed=0):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:src, 0:src].astype(np.float32) / src
    out = []
    for _ in range(count):
        ph = rng.uniform(0, 6.28, 3)
        base = np.stack([np.sin(6 * xx + ph[0]) + np.cos(4 * yy + ph[1]), np.sin(5 * yy + ph[2]) * np.cos(3 * xx),
                         xx - yy], axis=2) * 60 + 128
        img = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=90, subsampling=SUBSAMPLING[sampling])
        out.append(buf.getvalue())
    return out


def _dataset(root, name, files, src, sampling):
    folder = os.path.join(root, "dataset", name)
    os.makedirs(folder)
    for i, data in enumerate(_jpeg_bytes(src, sampling, files)):
        with open(os.path.join(folder, "%05d.jpg" % i), "wb") as f:
            f.write(data)
    return os.path.join(root, "dataset")


def _ints(s):
    return [int(v) for v in s.split(",") if v]


def _loader(a, tmp):
    import torch
    from biggan_tensorflow_amd import data as D
    workers = min(a.workers, 16)
    for src in _ints(a.srcs):
        for sampling in ("420", "444"):
            name = "bench_%d_%s" % (src, sampling)
            root = _dataset(tmp, name, a.files, src, sampling)
            files, _ = D.load_data(name, "", root=root)
            one = D.decode_file(D.ImageData(a.size, 3, True, True), files[0], entropy_only=True)
            ratio = D.upload_bytes(one) / float(a.size * a.size * 3 * 4)
            for path in ("host", "device", "host", "device"):             # alternating: each path twice
                os.environ["BG_DEVICE_INPUT"] = "0" if path == "host" else "1"
                ld = D.BatchLoader(files, None, a.batch, D.ImageData(a.size, 3, True, True, seed=1), "cuda", seed=2,
                                   workers=workers, device_preprocess=(path == "device"))
                try:
                    for _ in range(2):
                        x = next(ld)
                    torch.cuda.synchronize()
                    count = max(4, -(-a.min_images // a.batch))
                    t0 = time.perf_counter()
                    for _ in range(count):
                        x = next(ld)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    ld.close()
                assert tuple(x.shape) == (a.batch, a.size, a.size, 3)
                print(json.dumps({"mode": "loader", "path": path, "src": src, "sampling": sampling, "size": a.size,
                                  "batch": a.batch, "workers": workers, "batches": count,
                                  "images_per_s": round(a.batch * count / dt, 1), "upload_over_out": round(ratio, 3),
                                  "device_path_pays": bool(D.device_path_pays(D.upload_bytes(one), 1, a.size, 3))}),
                      flush=True)


def _kernel_split(run):
    """Microseconds per call of each kernel of ``run()`` from the profiler's kernel records; {} where it has none."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                run()
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            for tag in ("jpeg_validate", "jpeg_idct", "jpeg_colour"):
                if tag in ev.key:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    split[tag] = round(total / 10.0, 2)
        return split
    except Exception as e:                               # a profiler without device records: the total stands alone
        print("jpeg_bench: no per-kernel split (%s)" % e, file=sys.stderr)
        return {}


def _kernel(a, tmp):
    import torch
    from biggan_tensorflow_amd import data as D, functional as Fn
    for src in _ints(a.srcs):
        for sampling in ("420", "444"):
            files = _jpeg_bytes(src, sampling, min(a.batch, 16))
            imgs = [D.JpegImage(*D.jpeg_entropy_decode(files[i % len(files)]), channels=3) for i in range(a.batch)]
            raw, table, geom = D.pack_batch(imgs, [i % 2 for i in range(a.batch)], a.size, 3, pin=True)
            j = geom["jpeg"]
            raw_d, table_d, coef_d, jt_d = raw.cuda(), table.cuda(), j["coef"].cuda(), j["table"].cuda()
            ws = torch.empty(Fn.jpeg_batch_workspace_bytes(j["n"], j["blocks"]), dtype=torch.uint8, device="cuda")

            def run():
                Fn.jpeg_batch_u8(coef_d, jt_d, j["n"], j["blocks"], j["max_pixels"], raw_d, table_d, a.batch, ws=ws)
            for _ in range(10):
                run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.reps
            idct_bytes = j["coef"].numel() * 2 + j["blocks"] * 64
            colour_bytes = j["blocks"] * 64 + a.batch * src * src * 3
            split = _kernel_split(run)
            line = {"mode": "kernel", "src": src, "sampling": sampling, "batch": a.batch, "reps": a.reps,
                    "blocks": j["blocks"], "us_per_call": round(us, 2), "idct_bytes": idct_bytes,
                    "colour_bytes": colour_bytes, "gb_per_s_call": round((idct_bytes + colour_bytes) / us / 1e3, 1),
                    "coef_bytes": j["coef"].numel() * 2, "raw_bytes": raw.numel(), "us_per_kernel": split}
            if split.get("jpeg_idct"):
                line["gb_per_s_idct"] = round(idct_bytes / split["jpeg_idct"] / 1e3, 1)
            if split.get("jpeg_colour"):
                line["gb_per_s_colour"] = round(colour_bytes / split["jpeg_colour"] / 1e3, 1)
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("loader", "kernel"))
    ap.add_argument("--srcs", default="160,512", help="sides of the source images")
    ap.add_argument("--size", type=int, default=128, help="side of the batch")
    ap.add_argument("--files", type=int, default=128, help="files of each synthetic dataset")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", type=int, default=8, help="decode threads")
    ap.add_argument("--min_images", type=int, default=256, help="loader: time at least this many images per line")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=540, help="time limit of the GPU step, seconds")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        import PIL  # noqa: F401
    except ImportError:
        print("jpeg_bench: Pillow is not installed, so there is no JPEG folder to measure on; nothing was run")
        return
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("jpeg_bench: no GPU (there is nothing to measure without one)")
        import biggan_tensorflow_amd  # noqa: F401
        return {"loader": _loader, "kernel": _kernel}[a.mode](a, a.child)
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k) or 16)))
    tmp = tempfile.mkdtemp(prefix="jpeg_bench_")
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child", tmp]
    try:
        rc = subprocess.run(cmd, env=env, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("jpeg_bench: the GPU step ran past its %d s limit" % a.timeout)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if rc != 0:
        raise SystemExit("jpeg_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
