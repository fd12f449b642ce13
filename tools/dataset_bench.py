"""The device-resident dataset on the GPU box: BatchLoader with the cache (BG_DEVICE_DATASET_GB / cache_bytes) against
the streaming loader in the same process.

    python tools/dataset_bench.py loader [--files 512] [--size 128] [--batch 256] [--workers 8] [--epochs 6]
    python tools/dataset_bench.py kernel [--src 160] [--size 128] [--batch 256] [--reps 200]
    python tools/dataset_bench.py train  [--src 512] [--files 1024] [--batch 256] [--iters 20] [--workers 8]
                                         [--img_size 128 --ch 96 --precision bf16]

Every mode synthesises its datasets (RGB files: a smooth pattern plus noise, so that inflate and the Huffman decode have
real work) in a temporary folder and reads nothing else.  One JSON line per measurement:

    loader   per folder (160^2 PNG, 512^2 PNG, 256^2 JPEG, each to --size): images/s of ``next(loader)`` for the streaming
             loader and for the cached loader in its steady state (timed from the second epoch on, over --epochs epochs and at
             least --cached_batches batches, so that the batches waiting in the queue do not flatter it),
             run alternately and each twice; for the cached loader also the one-time planning seconds, the images/s of
             its first epoch (decode + store + gather) and what the arena holds
    kernel   bg_dataset_batch alone at C = 3 and C = 4, all kind 0 (--src^2 uint8 sources) and all kind 1: microseconds
             per launch between two device events around --reps launches, and GB/s over the bytes it reads (cached
             images, entries, sel) and writes, computed from the shapes
    train    ms per training iteration (defaults: BASELINE config 3 at 256 images) from a --src^2 PNG folder fed by
             synthetic batches, by the streaming loader and by the cached loader

The measurement runs in a child process under its own time limit (--timeout seconds); at most 16 decode threads.  There
is nothing to measure without a GPU, and the tool says so instead of falling back.
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


def _image(rng, src):
    import numpy as np
    yy, xx = np.mgrid[0:src, 0:src].astype(np.float32) / src
    ph = rng.uniform(0, 6.28, 3)
    base = np.stack([np.sin(6 * xx + ph[0]) + np.cos(4 * yy + ph[1]), np.sin(5 * yy + ph[2]) * np.cos(3 * xx),
                     xx - yy], axis=2) * 60 + 128
    return np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)


def _png_dataset(root, name, files, src, seed=0):
    import numpy as np
    from biggan_tensorflow_amd import utils
    folder = os.path.join(root, "dataset", name)
    os.makedirs(folder)
    rng = np.random.default_rng(seed)
    for i in range(files):
        utils.write_png(_image(rng, src), os.path.join(folder, "%05d.png" % i))
    return os.path.join(root, "dataset")


def _jpeg_dataset(root, name, files, src, seed=0):
    """Baseline 4:2:0 files written by Pillow; None without Pillow."""
    import numpy as np
    try:
        from PIL import Image
    except ImportError:
        return None
    folder = os.path.join(root, "dataset", name)
    os.makedirs(folder)
    rng = np.random.default_rng(seed)
    for i in range(files):
        Image.fromarray(_image(rng, src)).save(os.path.join(folder, "%05d.jpg" % i), quality=90, subsampling=2)
    return os.path.join(root, "dataset")


def _time_loader(ld, batch, count, skip):
    import torch
    for _ in range(skip):
        next(ld)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        x = next(ld)
    torch.cuda.synchronize()
    return batch * count / (time.perf_counter() - t0), x


def _loader(a, tmp):
    from biggan_tensorflow_amd import data as D
    workers = min(a.workers, 16)
    folders = [("png160", lambda: _png_dataset(tmp, "png160", a.files, 160)),
               ("png512", lambda: _png_dataset(tmp, "png512", a.files, 512)),
               ("jpeg256", lambda: _jpeg_dataset(tmp, "jpeg256", a.files, 256))]
    for name, make in folders:
        root = make()
        if root is None:
            print(json.dumps({"mode": "loader", "folder": name, "not_measured": "no JPEG writer on this machine"}), flush=True)
            continue
        files, _ = D.load_data(name, "", root=root)
        per_epoch = len(files) // a.batch
        for feed in ("streaming", "cached", "streaming", "cached"):       # alternating: each feed twice
            t0 = time.perf_counter()
            ld = D.BatchLoader(files, None, a.batch, D.ImageData(a.size, 3, True, True, seed=1), "cuda", seed=2,
                               workers=workers, cache_bytes=(a.budget_gb * (1 << 30) if feed == "cached" else 0))
            line = {"mode": "loader", "folder": name, "feed": feed, "files": len(files), "size": a.size, "batch": a.batch,
                    "workers": workers}
            try:
                if feed == "cached":
                    p = ld.cache.plan
                    line.update(planning_s=round(ld.cache.plan_seconds, 4), constructor_s=round(time.perf_counter() - t0, 4),
                                cached_files=p.n_cached, arena_bytes=p.arena_bytes,
                                kind0=int((p.kinds == 0).sum()), kind1=int((p.kinds == 1).sum()))
                    first, _ = _time_loader(ld, a.batch, per_epoch, 0)                # epoch 1: decode, store, gather
                    line["first_epoch_images_per_s"] = round(first, 1)
                    # no file drops out of an epoch here (--files is a multiple of --batch), so from the second epoch on
                    # the worker stages nothing: the steady state
                    count = max(a.epochs * per_epoch, a.cached_batches)
                    rate, x = _time_loader(ld, a.batch, count, 0)
                else:
                    count = a.epochs * per_epoch
                    rate, x = _time_loader(ld, a.batch, count, 2)
            finally:
                ld.close()
            assert tuple(x.shape) == (a.batch, a.size, a.size, 3)
            line.update(batches=count, images_per_s=round(rate, 1))
            print(json.dumps(line), flush=True)
        shutil.rmtree(os.path.join(root, name), ignore_errors=True)


def _kernel(a, tmp):
    import numpy as np
    import torch
    from biggan_tensorflow_amd import data as D, functional as Fn
    rng = np.random.default_rng(0)
    for c in (3, 4):
        for kind in (D.KIND_U8, D.KIND_F32):
            p = D.plan_entries([(a.src, a.src)] * a.batch, a.size, c, 1 << 40, force_kind=kind)
            arena = torch.from_numpy(rng.integers(0, 256, p.arena_bytes, dtype=np.uint8)).cuda()
            if kind == D.KIND_F32:                      # finite floats in [-1, 1]
                arena = (torch.rand(p.arena_bytes // 4, device="cuda") * 2 - 1).view(torch.uint8)
            table = torch.from_numpy(p.table.view("<i4").reshape(-1, 8)).cuda()
            order = rng.permutation(a.batch)
            sel = torch.from_numpy(np.stack([order, np.arange(a.batch) % 2], axis=1).astype(np.int32)).cuda()
            out = torch.empty(a.batch, a.size, a.size, c, device="cuda")
            for _ in range(20):
                Fn.dataset_batch(arena, table, sel, a.batch, a.size, c, out=out)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                Fn.dataset_batch(arena, table, sel, a.batch, a.size, c, out=out)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.reps
            moved = int(p.nbytes.sum()) + table.numel() * 4 + sel.numel() * 4 + out.numel() * 4
            print(json.dumps({"mode": "kernel", "channels": c, "kind": int(kind), "batch": a.batch, "src": a.src,
                              "size": a.size, "reps": a.reps, "us_per_launch": round(us, 2), "bytes_read_and_written": moved,
                              "gb_per_s": round(moved / us / 1e3, 1), "arena_bytes": p.arena_bytes}), flush=True)


def _train(a, tmp):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from biggan_tensorflow_amd import data as D, main as M, model, scope as S
    root = _png_dataset(tmp, "bench", a.files, a.src)
    files, _ = D.load_data("bench", "", root=root)
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    gan.settle_host()
    workers = min(a.workers, 16)
    per_epoch = len(files) // a.batch
    for feed in ("synthetic", "streaming", "cached", "synthetic", "streaming", "cached"):
        ld = None
        if feed != "synthetic":
            ld = D.BatchLoader(files, None, a.batch, D.ImageData(a.img_size, 3, True, True, seed=1), "cuda", seed=2,
                               workers=workers, cache_bytes=(a.budget_gb * (1 << 30) if feed == "cached" else 0))
        nxt = (lambda: next(ld)) if ld is not None else (lambda: gan.synthetic_batch())
        try:
            # the cached loader is timed in its steady state: the first epoch (and what the worker staged ahead) is over
            for _ in range(per_epoch + 6 if feed == "cached" else 3):
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
                          "precision": a.precision, "src": a.src, "files": len(files), "workers": workers, "iters": a.iters,
                          "ms_per_iter": round(dt / a.iters * 1e3, 2),
                          "images_per_s": round(a.batch * a.iters / dt, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("loader", "kernel", "train"))
    ap.add_argument("--src", type=int, default=0, help="side of the source images (kernel: 160, train: 512)")
    ap.add_argument("--size", type=int, default=128, help="side of the batch (loader, kernel)")
    ap.add_argument("--files", type=int, default=0, help="files per synthetic dataset (default 512; train 1024)")
    ap.add_argument("--workers", type=int, default=8, help="decode threads")
    ap.add_argument("--epochs", type=int, default=6, help="loader: epochs timed per line")
    ap.add_argument("--cached_batches", type=int, default=200,
                    help="loader: time the cached loader over at least this many batches (the queue's prefetched ones would "
                         "flatter a short window)")
    ap.add_argument("--budget_gb", type=float, default=8.0, help="the cache's budget")
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
    a.src = a.src or (512 if a.mode == "train" else 160)
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("dataset_bench: no GPU (there is nothing to measure without one)")
        import biggan_tensorflow_amd  # noqa: F401
        return {"loader": _loader, "kernel": _kernel, "train": _train}[a.mode](a, a.child)
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k) or 16)))
    env.pop("BG_DEVICE_DATASET_GB", None)               # the feeds set the budget themselves
    tmp = tempfile.mkdtemp(prefix="dataset_bench_")
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child", tmp]
    try:
        rc = subprocess.run(cmd, env=env, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("dataset_bench: the GPU step ran past its %d s limit" % a.timeout)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if rc != 0:
        raise SystemExit("dataset_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
