"""Time the singular-value monitor (spectrum.SingularValues, csrc/spectrum.hip) on the weights of a configuration.

    python tools/sv_bench.py [--img_size 128 --ch 96] [--k 3 --iters 8 --tol 1e-2] [--reps 5] [--timeout 600]

Defaults are the fp32 weights of BASELINE config 3 (128^2, ch 96), freshly initialised: flat spectra, the slowest kind to
converge.  Prints one JSON line:

    weights, weight_bytes   monitored /kernel variables and their fp32 bytes
    build_ms                the monitor's construction: the basis draws (QR on the host) and the device table
    cold_ms, cold_rounds    the first event, from the random basis (host clock, readbacks included)
    warm_ms, warm_rounds    the following event, from the basis the first one left (mean of --reps)
    call_ms                 one bg_sv_batch of --iters iterations over all weights (device events)
    iter_ms                 (call of 2 x iters - call of 0 iterations) / (2 x iters): one iteration's three launches
    launches_per_call       3 x iters + 5 per table of at most 256 weights
    achieved_gbps           the algorithmic bytes (2 x iters + 2) x weight_bytes over call_ms; hbm_fraction: over 8.0 TB/s
    svdvals_ms              torch.linalg.svdvals of the same weights on the GPU, one after the other, or "not measured"

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
    from biggan_tensorflow_amd import main as M, model, scope as S, spectrum
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", "4",
            "--precision", "fp32"]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mon = spectrum.SingularValues(gan.store, gan.device, a.k, a.iters, a.tol)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    plan = mon.plan

    def device_timed(fn, reps):
        fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / reps

    t0 = time.perf_counter()
    cold = mon.event()
    cold_ms = (time.perf_counter() - t0) * 1e3
    warm_ms, warm = 0.0, None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        warm = mon.event()
        warm_ms += (time.perf_counter() - t0) * 1e3 / a.reps
    call_ms = device_timed(lambda: mon.launch(a.iters), a.reps)
    zero_ms = device_timed(lambda: mon.launch(0), a.reps)
    long_ms = device_timed(lambda: mon.launch(2 * a.iters), a.reps)
    gbps = (2 * a.iters + 2) * plan.weight_bytes / (call_ms * 1e-3) / 1e9
    try:
        mats = [v.detach().reshape(r, c) for v, r, c in zip(mon._weights, plan.rows, plan.cols)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()                # (once, no warm-up: a full decomposition per weight takes seconds)
        for m in mats:
            torch.linalg.svdvals(m)
        torch.cuda.synchronize()
        svd_ms = round((time.perf_counter() - t0) * 1e3, 1)
    except Exception as e:                     # (no GPU SVD in this build of torch)
        svd_ms = "not measured (%s)" % type(e).__name__
    res = {"img_size": a.img_size, "ch": a.ch, "k": a.k, "iters": a.iters, "tol": a.tol, "reps": a.reps,
           "weights": plan.n, "weight_bytes": plan.weight_bytes, "workspace_bytes": plan.ws_bytes,
           "basis_bytes": 4 * plan.q_floats, "build_ms": round(build_ms, 1),
           "cold_ms": round(cold_ms, 2), "cold_rounds": cold["rounds"], "cold_resid_max": float("%.3g" % cold["resid_max"]),
           "warm_ms": round(warm_ms, 2), "warm_rounds": warm["rounds"], "warm_resid_max": float("%.3g" % warm["resid_max"]),
           "call_ms": round(call_ms, 3), "ritz_only_ms": round(zero_ms, 3),
           "iter_ms": round((long_ms - zero_ms) / (2 * a.iters), 4),
           "launches_per_call": (3 * a.iters + 5) * len(mon.tables), "achieved_gbps": round(gbps, 1),
           "hbm_fraction": round(gbps / HBM_PEAK_GBPS, 4), "svdvals_ms": svd_ms}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-2)
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
        raise SystemExit("sv_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("sv_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
