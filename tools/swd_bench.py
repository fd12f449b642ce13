"""Time one quality-score event (BigGAN.swd: the sliced Wasserstein distance of metrics.py) stage by stage.

    python tools/swd_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16] [--images 2048] [--reps 2]
                              [--timeout 600]

Defaults are BASELINE config 3 (128^2, ch 96, bf16, batch 256) with the default 2048 images per set.  Prints one JSON
line, ms per event (mean of --reps after one untimed pass), every stage summed over the pyramid levels:

    generator_ms    the generator sweep alone: images / batch no-grad passes on the moving averages
    pyramid_ms      bg_swd_pyr_down + bg_swd_pyr_lap of every batch and level
    gather_ms       bg_swd_descriptors of every batch and level, and bg_swd_stats_finish
    project_ms      bg_swd_project, both sets in one launch per level
    sort_ms         bg_swd_sort_segments: 2 x 512 segments of 128 x images floats per level
    l1_ms           bg_swd_l1
    torch_sort_ms   the same segments through torch.sort (values and int64 indices), for the record
    real_set_ms     the one-time real set: synthetic images, pyramid, gather
    event_ms        the whole event as the training loop runs it (BigGAN.swd with the real set in place)

The measurement runs in a child process under its own time limit (--timeout seconds); host work uses at most 16 threads.
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _measure(a):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, main as M, metrics, model, scope as S
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--swd_freq", "1", "--swd_images", str(a.images)]
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

    plan = gan.monitor_plan("swd")
    levels = len(plan.sides)
    m = metrics.Swd(plan, "cuda")

    def real_set():
        m.begin("real")
        for batch in gan.monitor_real_batches(plan):
            m.add(batch)
        return m.finish()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.real = real_set()
    torch.cuda.synchronize()
    real_ms = (time.perf_counter() - t0) * 1e3                       # one-time: timed cold, as a run pays it
    z, cls_z = gan.monitor_fake_inputs(plan)

    def sweep():
        batches = []
        gan.generate(z, cls_z, ema=True, _consume=batches.append)
        return batches
    gen_ms, batches = timed(sweep)

    def pyramid():
        out = []
        for g in batches:
            per = []
            for i in range(levels):
                if i + 1 < levels:
                    g1 = Fn.swd_pyr_down(g)
                    per.append(Fn.swd_pyr_lap(g, g1))
                    g = g1
                else:
                    per.append(g)
            out.append(per)
        return out
    pyr_ms, pyr = timed(pyramid)

    def gather():
        desc = [torch.empty(plan.n_rows, plan.K, dtype=torch.float32, device="cuda") for _ in range(levels)]
        part = [Fn.swd_partials(plan.n_images, plan.c_dim, "cuda") for _ in range(levels)]
        lo = 0
        for per in pyr:
            b = min(per[0].shape[0], plan.n_images - lo)
            for i in range(levels):
                Fn.swd_descriptors(per[i][:b], m.pos["fake"][i][lo:lo + b], desc[i], lo * 128, part[i])
            lo += b
        return desc, [Fn.swd_stats(w) for w in part]
    gather_ms, fake = timed(gather)
    del pyr, batches

    proj = torch.empty(2 * plan.S, plan.n_rows, dtype=torch.float32, device="cuda")

    def project():
        for i in range(levels):
            Fn.swd_project(m.real[0][i], m.real[1][i], m.dirs[i], proj, fake[0][i], fake[1][i])
    project_ms, _ = timed(project)
    unsorted = proj.clone()

    # both sorts once, on the unsorted projections of the last level, times the number of levels (a repeat would sort
    # sorted data); torch.sort second, so that the allocator's first touch of its buffers is the only thing it pays extra
    Fn.swd_sort_segments(torch.rand(2, plan.n_rows, device="cuda"), plan.n_rows)       # (code objects loaded)
    torch.sort(torch.rand(2, plan.n_rows, device="cuda"), dim=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Fn.swd_sort_segments(proj, plan.n_rows)
    torch.cuda.synchronize()
    sort_ms = (time.perf_counter() - t0) * 1e3 * levels
    ours = proj.clone()
    t0 = time.perf_counter()
    theirs = torch.sort(unsorted, dim=1)[0]
    torch.cuda.synchronize()
    torch_sort_ms = (time.perf_counter() - t0) * 1e3 * levels
    same = bool(torch.equal(ours, theirs))
    del theirs, ours, unsorted

    def l1():
        for i in range(levels):
            Fn.swd_l1(proj[:plan.S], proj[plan.S:], plan.repeats)
    l1_ms, _ = timed(l1)
    del proj, fake, m
    torch.cuda.empty_cache()
    gan.swd()                                                          # builds the model's own metric (real set)
    event_ms, scores = timed(gan.swd)
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "images": plan.n_images,
           "levels": plan.sides, "rows": plan.n_rows, "reps": a.reps, "generator_ms": round(gen_ms, 2),
           "pyramid_ms": round(pyr_ms, 2), "gather_ms": round(gather_ms, 2), "project_ms": round(project_ms, 2),
           "sort_ms": round(sort_ms, 2), "l1_ms": round(l1_ms, 2), "torch_sort_ms": round(torch_sort_ms, 2),
           "sorts_equal": same, "real_set_ms": round(real_ms, 2), "event_ms": round(event_ms, 2),
           "generator_share": round(gen_ms / event_ms, 3), "real_bytes": plan.real_bytes,
           "projection_bytes": plan.projection_bytes, "scores": {k: round(v, 4) for k, v in scores.items()}}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
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
        raise SystemExit("swd_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("swd_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
