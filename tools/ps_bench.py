"""Time one frequency-check event (BigGAN.power_spectrum: the radial power spectrum of generated images, metrics.py) stage
by stage.

    python tools/ps_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16] [--images 1024] [--reps 3]
                             [--timeout 600]

Defaults are BASELINE config 3 (128^2, ch 96, bf16, batch 256) with the default 1024 images.  Prints one JSON line, ms per
event (mean of --reps after one untimed pass):

    generator_ms    the generator sweep alone: images / batch no-grad passes on the moving averages (host clock)
    power_ms        bg_ps_power of every batch of the event (device events around the launches)
    profile_ms      bg_ps_profile of every batch, with the 2-D sum (device events)
    tail_ms         the host tail: the read of the [images, NB] profiles, their fp64 mean and the scores (host clock)
    event_ms        the whole event as the training loop runs it (BigGAN.power_spectrum after its first call)
    metric_share    (event_ms - generator_ms) / event_ms
    power_gbps      bytes bg_ps_power must move at least (images in, power out, the row transforms out and in again)
                    over power_ms; power_hbm_fraction is that over the 8.0 TB/s HBM3E peak of the MI355X
    rfft2_ms        for information, where torch.fft.rfft2 works: |rfft2(luminance)|^2 / S^4 in torch on one batch, beside
                    power_batch_ms, bg_ps_power on the same batch; rfft2_max_rel compares the two results

The measurement runs in a child process under its own time limit (--timeout seconds); host work uses at most 16 threads.
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBPS = 8000.0


def _measure(a):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, main as M, model, scope as S
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--ps_freq", "1", "--ps_images", str(a.images)]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    gan.train_step(gan.synthetic_batch())

    def timed(fn, reps=a.reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps, r

    def device_timed(fn, reps=10 * a.reps):
        fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / reps

    plan = gan.monitor_plan("ps")
    side, W, nb = plan.side, plan.side // 2 + 1, plan.n_bins
    z, cls_z = gan.monitor_fake_inputs(plan)

    def sweep():
        batches = []
        gan.generate(z, cls_z, ema=True, _consume=batches.append)
        return batches
    gen_ms, batches = timed(sweep)
    left, kept = plan.n_images, []
    for g in batches:                                      # what PowerSpectrum.add keeps: no padding
        g = g[:min(int(g.shape[0]), left)]
        left -= int(g.shape[0])
        if g.shape[0]:
            kept.append(g)
    ws = Fn.ps_workspace(max(int(g.shape[0]) for g in kept), side, "cuda")
    powers = [torch.empty(int(g.shape[0]), side, W, device="cuda") for g in kept]
    power_ms = device_timed(lambda: [Fn.ps_power(g, p, ws) for g, p in zip(kept, powers)])
    profiles = torch.zeros(plan.n_images, nb, dtype=torch.float64, device="cuda")
    sum2d = torch.zeros(side, W, dtype=torch.float64, device="cuda")

    def profile():
        lo = 0
        for p in powers:
            Fn.ps_profile(p, profiles[lo:lo + p.shape[0]], sum2d)
            lo += p.shape[0]
    profile_ms = device_timed(profile)
    first = gan.power_spectrum()                                       # draws, the real set
    runner = gan._monitors["ps"]

    def tail():
        rows = profiles.cpu().numpy()
        total = rows[0] * 0.0
        for row in rows:
            total += row
        return runner.scores(runner.real, {"profile": total / len(rows)})
    tail_ms, _ = timed(tail)
    moved = sum(g.numel() * g.element_size() + 4 * p.numel() + 2 * 8 * p.numel() for g, p in zip(kept, powers))
    x, power0 = kept[0], powers[0]
    del batches, kept, powers
    torch.cuda.empty_cache()
    event_ms, result = timed(gan.power_spectrum)
    # for information: the same batch through torch.fft.rfft2
    power_batch_ms = device_timed(lambda: Fn.ps_power(x, power0, ws))
    rfft2_ms = rfft2_rel = None
    try:
        lum = torch.tensor([0.299, 0.587, 0.114], device="cuda")

        def by_rfft2():
            xf = x.float()
            y = xf[..., 0] if xf.shape[-1] == 1 else (xf[..., :3] * lum).sum(dim=-1)
            f = torch.fft.rfft2(y)
            return (f.real * f.real + f.imag * f.imag) / float(side) ** 4
        rfft2_ms = device_timed(by_rfft2)
        want = by_rfft2()
        rfft2_rel = float(((power0 - want).abs().max() / want.abs().max()).item())
    except Exception as e:                                             # no FFT library on this machine: information only
        print("ps_bench: torch.fft.rfft2 is not usable here (%s: %s)" % (type(e).__name__, e), file=sys.stderr)
    gbps = moved / (power_ms * 1e-3) / 1e9
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "images": plan.n_images,
           "bins": nb, "reps": a.reps, "generator_ms": round(gen_ms, 2), "power_ms": round(power_ms, 3),
           "profile_ms": round(profile_ms, 3), "tail_ms": round(tail_ms, 3), "event_ms": round(event_ms, 2),
           "metric_share": round((event_ms - gen_ms) / event_ms, 4), "power_bytes_moved": moved,
           "power_gbps": round(gbps, 1), "power_hbm_fraction": round(gbps / HBM_PEAK_GBPS, 4),
           "power_batch_ms": round(power_batch_ms, 4), "rfft2_ms": None if rfft2_ms is None else round(rfft2_ms, 4),
           "rfft2_max_rel": rfft2_rel, "peak_bytes": plan.peak_bytes,
           "scores": {k: round(v, 6) for k, v in first.items()}, "scores_again": {k: round(v, 6) for k, v in result.items()}}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="time limit of the GPU step, seconds")
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
        raise SystemExit("ps_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("ps_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
