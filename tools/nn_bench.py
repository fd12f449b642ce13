"""Time one nearest-training-image event (BigGAN.save_neighbours, neighbours.py) stage by stage, and the two search
kernels against the torch expressions one would write without them.

    python tools/nn_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16] [--images 32768] [--size 64]
                             [--reps 5] [--timeout 600]

Defaults are BASELINE config 3 (128^2, ch 96, bf16, batch 256) against a synthetic set of 32768 images at side 64
(D = 12288, 805 MB).  Prints one JSON line; times are ms, the mean of --reps after one untimed pass, with the fastest and
slowest repeat where two implementations are compared:

    set_build_ms    the one-time resident set: synthetic images, bg_nn_pack (timed cold, as a run pays it)
    generator_ms    the generator sweep of the static samples on the moving averages
    pack_ms         bg_nn_pack of the queries, plain and mirrored
    distances_ms    bg_nn_distances, plain and mirrored
    topk_ms         bg_nn_topk, plain and mirrored
    fetch_ms        the neighbours' full-size images for the grid (first event: nothing kept yet)
    grid_png_ms     grid assembly, PNG and table
    event_ms        the whole event as the training loop runs it, with the set in place
    compare         per Q in --queries: bg_nn_distances against the chunked ((q[:, None].float() - s[None].float()) ** 2).sum(-1),
                    bg_nn_topk against torch.topk(largest=False), each as [mean, fastest, slowest], and the distance kernel's
                    effective GB/s (set bytes x query tiles of 8 / time)

The measurement runs in a child process under its own time limit (--timeout seconds); host work uses at most 16 threads.
"""
import argparse
import contextlib
import io
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
    from biggan_tensorflow_amd import functional as Fn, main as M, model, neighbours as NB, scope as S
    out_dir = tempfile.mkdtemp(prefix="nn_bench_")
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--nn_freq", "1", "--nn_images", str(a.images), "--nn_size", str(a.size),
            "--sample_dir", out_dir]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    gan.train_step(gan.synthetic_batch())

    def times(fn, reps=a.reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, r

    def mean(ts):
        return round(sum(ts) / len(ts), 3)

    def spread(ts):
        return [mean(ts), round(min(ts), 3), round(max(ts), 3)]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = gan._nn_set()
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    plan = s.plan
    zs, cs = gan.static_sample_set()
    n = min(gan.sample_num, gan.batch_size)
    gen_ts, images = times(lambda: gan.generate(zs[:n], None if cs is None else cs[:n], ema=True))
    pack_ts, packed = times(lambda: [Fn.nn_pack(images, plan.f, m) for m in (False, True)])
    dist_ts, dists = times(lambda: [Fn.nn_distances(q, s.arena) for q in packed])
    topk_ts, _ = times(lambda: [Fn.nn_topk(d, gan.nn_k) for d in dists])
    result = s.search(images, gan.nn_k, True)
    samples = images.float().cpu().numpy()

    def fetch_all():
        s.images.clear()
        for q in NB.grid_queries(result):
            for i in result["index"][q]:
                gan._nn_fetch(int(i))
    fetch_ts, _ = times(fetch_all)
    png_ts, _ = times(lambda: NB.write_event(result, samples, gan._nn_fetch, out_dir, NB.event_names("bench", 0, 0)))

    def event():
        with contextlib.redirect_stdout(io.StringIO()):              # (its "NN: ..." line)
            gan.save_neighbours(0, 1)
    event_ts, _ = times(event)

    compare = {}
    g = torch.Generator(device="cuda").manual_seed(1)
    for Q in a.queries:
        q = (torch.rand(Q, plan.D, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
        chunk = max(1, (1 << 28) // (Q * plan.D))                    # at most 1 GiB of fp32 differences at a time

        def by_torch():
            return torch.cat([((q[:, None].float() - s.arena[lo:lo + chunk][None].float()) ** 2).sum(-1)
                              for lo in range(0, plan.N, chunk)], dim=1)
        hip_d, d = times(lambda: Fn.nn_distances(q, s.arena))
        torch_d, d_t = times(by_torch)
        hip_k, (v, i) = times(lambda: Fn.nn_topk(d, gan.nn_k))
        torch_k, (v_t, i_t) = times(lambda: torch.topk(d, gan.nn_k, dim=1, largest=False))
        tiles = (Q + 7) // 8
        compare[str(Q)] = {"distances_ms": spread(hip_d), "torch_distances_ms": spread(torch_d),
                           "topk_ms": spread(hip_k), "torch_topk_ms": spread(torch_k),
                           "distances_gbps": round(plan.bytes * tiles / (mean(hip_d) * 1e-3) / 1e9, 1),
                           "max_rel_diff_to_torch": float(((d - d_t).abs() / d_t).max()),
                           "topk_values_equal": bool(torch.equal(v, v_t))}
        del d, d_t
    event = mean(event_ts)
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "N": plan.N, "D": plan.D,
           "set_bytes": plan.bytes, "queries": n, "k": gan.nn_k, "reps": a.reps, "set_build_ms": round(build_ms, 2),
           "generator_ms": mean(gen_ts), "pack_ms": mean(pack_ts), "distances_ms": mean(dist_ts), "topk_ms": mean(topk_ts),
           "fetch_ms": mean(fetch_ts), "grid_png_ms": mean(png_ts), "event_ms": event,
           "shares": {k: round(mean(v) / event, 3) for k, v in (("generator", gen_ts), ("pack", pack_ts),
                                                                 ("distances", dist_ts), ("topk", topk_ts),
                                                                 ("grid_png", png_ts))},
           "compare": compare}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--images", type=int, default=32768)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--queries", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--reps", type=int, default=5)
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
        raise SystemExit("nn_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("nn_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
