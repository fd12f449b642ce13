"""Time one precision / recall / density / coverage event (BigGAN.prdc, metrics.Prdc, csrc/prdc.hip) stage by stage, beside
the same scores computed through the matrix-writing kernels of the memorisation check.

    python tools/prdc_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16] [--images 4096] [--k 3] [--size 64]
                               [--slab 1024] [--reps 3] [--timeout 900]

Defaults are BASELINE config 3 (128^2, ch 96, bf16, batch 256) with the default 4096 images at side 64 (D = 12288).
Prints one JSON line, ms per event (mean of --reps after one untimed pass):

    generator_ms    the generator sweep alone: images / batch no-grad passes on the moving averages (host clock)
    pack_ms         bg_nn_pack of every batch of the event into the resident set (device events)
    radii_ms        bg_prdc_radii of the generated set
    cover_real_ms   bg_prdc_cover(q = real with its radii, set = fake): count only (precision, density)
    cover_fake_ms   bg_prdc_cover(q = fake with its radii, set = real): count and nearest distance (recall, coverage)
    reduce_ms       bg_prdc_reduce
    fused_ms        the four launches in a row
    event_ms        the whole event as the training loop runs it (BigGAN.prdc after its first call)
    metric_share    (event_ms - generator_ms) / event_ms
    pairs_per_s     element pairs (row pairs x D) of the three distance passes over their time

    materialised    the same integers without csrc/prdc.hip, in query slabs of --slab rows: radii_ms is bg_nn_distances of
                    the generated set against itself into a [slab, M] matrix, the diagonal set to +inf, bg_nn_topk and its
                    k-th column; pairs_ms is bg_nn_distances of the real slab against the generated set and torch
                    comparisons on the matrix, which serve both directions at once (count per column, count and minimum
                    per row); total_ms their sum with the torch reduction.  ``equal``: the four integers are the fused ones
                    (the two kernels call one function)

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
    from biggan_tensorflow_amd import functional as Fn, main as M, model, scope as S
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--pr_freq", "1", "--pr_images", str(a.images), "--pr_k", str(a.k),
            "--pr_size", str(a.size)]
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

    def device_timed(fn, reps=a.reps):
        r = fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            r = fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / reps, r

    first, runner, sets = gan.prdc(details=True)                       # draws, the real set and its radii
    plan, real, fake = runner.plan, runner.real, sets["pr"]
    k, N, Mf, D = plan.k, plan.N, plan.M, plan.D
    z, cls_z = runner.fake_inputs

    def sweep():
        batches = []
        gan.generate(z, cls_z, ema=True, _consume=batches.append)
        return batches
    gen_ms, batches = timed(sweep)
    desc = torch.empty(Mf, D, dtype=torch.bfloat16, device="cuda")

    def pack():
        lo = 0
        for g in batches:
            b = min(int(g.shape[0]), Mf - lo)
            if b > 0:
                Fn.nn_pack(g[:b], plan.f, False, out=desc[lo:lo + b])
            lo += b
    pack_ms, _ = device_timed(pack)
    assert torch.equal(desc, fake["desc"])
    del batches
    radius_f = torch.empty(Mf, device="cuda")
    count_f = torch.empty(Mf, dtype=torch.int32, device="cuda")
    count_r = torch.empty(N, dtype=torch.int32, device="cuda")
    dmin_r = torch.empty(N, device="cuda")
    out4 = torch.empty(4, dtype=torch.int64, device="cuda")
    radii_ms, _ = device_timed(lambda: Fn.prdc_radii(desc, k, out=radius_f))
    cover_real_ms, _ = device_timed(lambda: Fn.prdc_cover(real["desc"], real["radius"], desc, count=count_f, dmin=None))
    cover_fake_ms, _ = device_timed(lambda: Fn.prdc_cover(desc, radius_f, real["desc"], count=count_r, dmin=dmin_r))
    reduce_ms, _ = device_timed(lambda: Fn.prdc_reduce(count_f, count_r, dmin_r, real["radius"], out=out4))

    def fused():
        Fn.prdc_radii(desc, k, out=radius_f)
        Fn.prdc_cover(real["desc"], real["radius"], desc, count=count_f, dmin=None)
        Fn.prdc_cover(desc, radius_f, real["desc"], count=count_r, dmin=dmin_r)
        return Fn.prdc_reduce(count_f, count_r, dmin_r, real["radius"], out=out4)
    fused_ms, _ = device_timed(fused)
    fused4 = out4.cpu().tolist()

    # ---- the same integers through bg_nn_distances / bg_nn_topk and torch, a slab of queries at a time
    slab = min(a.slab, N, Mf)
    matrix = torch.empty(slab, Mf, device="cuda")
    m_radius_f = torch.empty(Mf, device="cuda")
    inf = torch.tensor(float("inf"), device="cuda")

    def mat_radii():
        for lo in range(0, Mf, slab):
            q = desc[lo:lo + slab]
            d = Fn.nn_distances(q, desc, out=matrix[:q.shape[0]])
            d.diagonal(offset=lo).copy_(inf.expand(q.shape[0]))        # the row itself, by index
            m_radius_f[lo:lo + q.shape[0]] = Fn.nn_topk(d, k)[0][:, k - 1]
        return m_radius_f
    mat_radii_ms, _ = device_timed(mat_radii)
    m_count_f = torch.zeros(Mf, dtype=torch.int64, device="cuda")
    m_count_r = torch.zeros(N, dtype=torch.int64, device="cuda")
    m_dmin_r = torch.empty(N, device="cuda")

    def mat_pairs():
        m_count_f.zero_()
        for lo in range(0, N, slab):
            q = real["desc"][lo:lo + slab]
            n = q.shape[0]
            d = Fn.nn_distances(q, desc, out=matrix[:n])               # [i, j] = d(r_i, f_j) = d(f_j, r_i), the same bits
            m_count_f.add_((d <= real["radius"][lo:lo + n, None]).sum(dim=0))
            m_count_r[lo:lo + n] = (d <= m_radius_f[None, :]).sum(dim=1)
            m_dmin_r[lo:lo + n] = d.min(dim=1).values
    mat_pairs_ms, _ = device_timed(mat_pairs)

    def mat_reduce():
        return torch.stack([(m_count_f > 0).sum(), m_count_f.sum(), (m_count_r > 0).sum(),
                            (m_dmin_r <= real["radius"]).sum()])
    mat_reduce_ms, mat4 = device_timed(mat_reduce)
    mat4 = mat4.cpu().tolist()
    del matrix
    torch.cuda.empty_cache()
    event_ms, again = timed(gan.prdc)
    passes_ms = radii_ms + cover_real_ms + cover_fake_ms
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "N": N, "M": Mf, "D": D, "k": k,
           "reps": a.reps, "generator_ms": round(gen_ms, 2), "pack_ms": round(pack_ms, 3), "radii_ms": round(radii_ms, 3),
           "cover_real_ms": round(cover_real_ms, 3), "cover_fake_ms": round(cover_fake_ms, 3),
           "reduce_ms": round(reduce_ms, 4), "fused_ms": round(fused_ms, 3), "event_ms": round(event_ms, 2),
           "metric_share": round((event_ms - gen_ms) / event_ms, 4),
           "pairs_per_s": round((Mf * Mf + 2.0 * N * Mf) * D / (passes_ms * 1e-3), 0),
           "materialised": {"slab": slab, "radii_ms": round(mat_radii_ms, 3), "pairs_ms": round(mat_pairs_ms, 3),
                            "reduce_ms": round(mat_reduce_ms, 4),
                            "total_ms": round(mat_radii_ms + mat_pairs_ms + mat_reduce_ms, 3),
                            "matrix_bytes": slab * Mf * 4, "equal": mat4 == fused4,
                            "radii_equal": bool(torch.equal(m_radius_f, radius_f))},
           "out4": fused4, "peak_bytes": plan.peak_bytes,
           "scores": {k_: round(v, 6) for k_, v in first.items()}, "scores_again": {k_: round(v, 6) for k_, v in again.items()}}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--slab", type=int, default=1024, help="query rows per materialised [slab, M] matrix")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="time limit of the GPU step, seconds")
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
        raise SystemExit("prdc_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("prdc_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
