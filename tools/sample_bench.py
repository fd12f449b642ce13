"""Time one in-training sampling event (BigGAN.save_samples: the default 64-image EMA grid) and split it three ways.

    python tools/sample_bench.py [--img_size 128 --ch 96 --batch 32 --precision bf16] [--sample_num 64] [--reps 5]
                                 [--timeout 300]

Defaults are the generator of BASELINE config 3 (128^2, ch 96, bf16) at its per-GPU batch of 32.  Prints one JSON line,
ms per event (mean of --reps after one untimed pass):

    generator_ms      the generator sweep alone: ceil(64 / batch) no-grad passes on the moving averages, float images out
    grid_device_ms    grid assembly on the device path: zero-fill + bg_image_tiles_u8 per batch + the D2H copy of the bytes
    grid_host_ms      the same grid on the host path, in the same process: .float().cpu().numpy() of the images +
                      utils.grid_u8 (a float64 grid on the host); the two grids are compared byte for byte
    png_ms            utils.write_png of the grid (zlib level 6)
    save_samples_ms   the whole event as the training loop runs it

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
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, main as M, model, sampling as Sp, scope as S, utils
    out_dir = tempfile.mkdtemp(prefix="sample_bench_")
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--sample_num", str(a.sample_num), "--precision", a.precision, "--sample_dir", out_dir]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    gan.train_step(gan.synthetic_batch())
    dim, _, batches = Sp.grid_plan(a.sample_num, a.batch)
    B, side = a.batch, gan.img_size
    z = gan.static_sample_set()[0][:batches * B]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.reps, r

    gen_ms, imgs = timed(lambda: gan.generate(z))

    def device_path():
        grid = torch.zeros(dim * side, dim * side, gan.c_dim, dtype=torch.uint8, device="cuda")
        for b in range(0, imgs.shape[0], B):
            Fn.image_tiles_u8(imgs[b:b + B], grid, dim, dim, tile0=b)
        return grid.cpu().numpy()

    def host_path():
        return utils.grid_u8(utils.inverse_transform(imgs.float().cpu().numpy()[:dim * dim]), [dim, dim])

    dev_ms, g_dev = timed(device_path)
    host_ms, g_host = timed(host_path)
    png = os.path.join(out_dir, "grid.png")
    png_ms, _ = timed(lambda: utils.write_png(g_dev, png))
    event_ms, paths = timed(lambda: gan.save_samples(0, 1))
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "sample_num": a.sample_num,
           "grid": [int(g_dev.shape[0]), int(g_dev.shape[1]), int(g_dev.shape[2])], "image_dtype": str(imgs.dtype),
           "reps": a.reps, "generator_ms": round(gen_ms, 3), "grid_device_ms": round(dev_ms, 3),
           "grid_host_ms": round(host_ms, 3), "png_ms": round(png_ms, 3), "save_samples_ms": round(event_ms, 3),
           "grids_equal": bool((g_dev == g_host).all()), "float_bytes": int(imgs.numel() * 4), "grid_bytes": int(g_dev.size)}
    for p in paths + [png]:
        os.remove(p)
    os.rmdir(out_dir)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--sample_num", type=int, default=64)
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
        raise SystemExit("sample_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("sample_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
