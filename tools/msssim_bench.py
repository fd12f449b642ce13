"""Time one diversity-score event (BigGAN.msssim: the mean MS-SSIM of generated pairs, metrics.py) stage by stage.

    python tools/msssim_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16] [--pairs 1024] [--reps 3]
                                 [--timeout 600]

Defaults are BASELINE config 3 (128^2, ch 96, bf16, batch 256) with the default 1024 pairs.  Prints one JSON line, ms per
event (mean of --reps after one untimed pass):

    generator_ms    the generator sweep alone: 2 x pairs / batch no-grad passes on the moving averages (host clock)
    level_ms        bg_msssim_level per pyramid level, all batches of the event (device events around the launches)
    finish_ms       bg_msssim_finish of every batch and the host's read of the [pairs] scores (host clock)
    event_ms        the whole event as the training loop runs it (BigGAN.msssim after its first call)
    metric_share    (event_ms - generator_ms) / event_ms: what the metric adds to the sweep that the event cannot avoid
    level0_gbps     bytes of the level-0 images, each counted once, over the level-0 time; level0_hbm_fraction is that over
                    the 8.0 TB/s HBM3E peak of the MI355X (its measured copy rate is 6.29 TB/s)

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
            "--precision", a.precision, "--msssim_freq", "1", "--msssim_pairs", str(a.pairs)]
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

    plan = gan.monitor_plan("msssim")
    H, C, levels = plan.img_size, plan.c_dim, len(plan.sides)
    z, cls_z = gan.monitor_fake_inputs(plan)

    def sweep():
        batches = []
        gan.generate(z, cls_z, ema=True, _consume=batches.append)
        return batches
    gen_ms, batches = timed(sweep)
    left, kept = 2 * plan.n_pairs, []
    for g in batches:                                      # what Msssim.add keeps of an even batch: no padding
        g = g[:min(int(g.shape[0]), left) // 2 * 2]
        left -= int(g.shape[0])
        if g.shape[0]:
            kept.append(g)
    assert left == 0, "an odd --batch splits pairs across batches: use an even one here"
    ws = [Fn.msssim_workspace(g.shape[0] // 2, H, C, "cuda") for g in kept]
    inputs = [[(g, None) for g in kept]]
    level_ms = []
    for i, side in enumerate(plan.sides):
        pools = [None] * len(kept)
        if i + 1 < levels:
            pools = [torch.empty(2, g.shape[0] // 2, side // 2, side // 2, C, device="cuda") for g in kept]

        def run(i=i, pools=pools):
            for (x, y), w, pool in zip(inputs[i], ws, pools):
                Fn.msssim_level(x, y, H, i, w, pool)
        level_ms.append(device_timed(run))
        inputs.append([(p[0], p[1]) for p in pools if p is not None])
    scores = torch.zeros(plan.n_pairs, dtype=torch.float64, device="cuda")

    def finish():
        lo = 0
        for g, w in zip(kept, ws):
            Fn.msssim_finish(w, g.shape[0] // 2, H, C, scores, lo)
            lo += g.shape[0] // 2
        return scores.cpu().numpy()
    finish_ms, per_pair = timed(finish)
    level0_bytes = sum(g.numel() * g.element_size() for g in kept)
    del batches, kept, inputs, ws
    torch.cuda.empty_cache()
    first = gan.msssim()                                               # draws, the real baseline
    event_ms, result = timed(gan.msssim)
    assert abs(float(per_pair.mean()) - result["msssim"]) < 1e-12
    gbps = level0_bytes / (level_ms[0] * 1e-3) / 1e9
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "pairs": plan.n_pairs,
           "levels": plan.sides, "reps": a.reps, "generator_ms": round(gen_ms, 2),
           "level_ms": [round(v, 3) for v in level_ms], "finish_ms": round(finish_ms, 3), "event_ms": round(event_ms, 2),
           "metric_share": round((event_ms - gen_ms) / event_ms, 4), "level0_bytes": level0_bytes,
           "level0_gbps": round(gbps, 1), "level0_hbm_fraction": round(gbps / HBM_PEAK_GBPS, 4),
           "peak_bytes": plan.peak_bytes, "scores": {k: round(v, 6) for k, v in first.items()}}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--pairs", type=int, default=1024)
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
        raise SystemExit("msssim_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("msssim_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
