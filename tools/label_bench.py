"""Time training iterations of the class-conditional model (--n_labels 1000) with each label loss and each way of drawing
the generator's labels, which bench.py (no labels) does not take, and the two label-loss launches on their own.

    python tools/label_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16 --n_labels 1000]
                                [--steps 10 --warmup 3] [--only logistic,mixed,table,launches] [--tree PATH]
                                [--timeout 300]

Defaults are BASELINE config 3 on one GPU (128^2, ch 96, batch 256, bf16, --da_policy full, ortho_cosine regulariser)
and bench.py's timing protocol (seed 42 store, settle_host, synchronised warm-up steps, one synchronisation around the
timed steps).  Settings:

    logistic   --cls_loss_type logistic (bg_sigmoid_ce, one launch), synthetic one-hot draws: what ran before
    mixed      --cls_loss_type 900-logistic,100-euclidean (sizes scaled to --n_labels): the two launches of labels.hip
    table      logistic, the generator's labels drawn from a device label table of 4096 multi-hot rows (randint +
               bg_gather_rows) instead of synthetic one-hots (randint + index_put)
    launches   bg_label_loss_sums + bg_label_loss_finish alone on [batch, n_labels], next to bg_sigmoid_ce and
               bg_gather_rows: microseconds per call over 200 back-to-back calls

Synthetic images; eager iterations (D step then G step).  ``--tree``: import the package from another checkout of this
repository (e.g. the parent commit, for the logistic setting).  The GPU work of each setting runs in a child process
under its own time limit (``--timeout`` seconds); the first setting that fails or runs over ends the run.  Prints one
JSON line.
"""
import argparse
import json
import os
import sys
import time


def _model(a, cls_loss_type):
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import main as M, model, scope as S
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--da_policy", "full", "--g_regularization", "ortho_cosine", "--n_labels", str(a.n_labels),
            "--precision", a.precision, "--cls_loss_type", cls_loss_type]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    return gan.build_model()


def _time_iterations(a, cls_loss_type, table):
    import gc
    import torch
    gan = _model(a, cls_loss_type)
    if table:
        g = torch.Generator().manual_seed(7)
        rows = (torch.rand(4096, a.n_labels, generator=g) < 0.01).float()
        gan.labels = rows.tolist()
        gan.label_table = rows.cuda()
    real = gan.synthetic_batch(a.batch)
    labels = gan.synthetic_labels(a.batch)
    gan.settle_host()
    for _ in range(a.warmup):
        gan.train_step(real, labels)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        gan.train_step(real, labels)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    del gan, real, labels
    gc.collect()
    torch.cuda.empty_cache()
    return round(ms, 3)


def _time_launches(a, spec, reps=200):
    import torch
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import hip, utils
    L, P = hip.lib(), hip.ptr
    B, n = a.batch, a.n_labels
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, n, generator=g) * 3).cuda()
    t = (torch.rand(B, n, generator=g) < 0.3).float().cuda()
    w = torch.ones(n, device="cuda")
    sl = utils.parse_cls_loss_type(spec, n)
    slices = torch.tensor([[utils.CLS_LOSS_KINDS[k], s] for k, s in sl], dtype=torch.int32, device="cuda")
    cols = torch.tensor([i for i, (_, s) in enumerate(sl) for _ in range(s)], dtype=torch.int32, device="cuda")
    sums = torch.zeros(len(sl), dtype=torch.float64, device="cuda")
    loss = torch.empty(1, device="cuda")
    dl = torch.empty_like(x)
    table = (torch.rand(4096, n, generator=g) < 0.01).float().cuda()
    idx = torch.randint(0, 4096, (B,), generator=g).cuda()
    out = torch.empty(B, n, device="cuda")

    def pair():
        hip.check(L.bg_label_loss_sums(P(x), P(t), P(w), P(slices), P(cols), P(sums), B, n, len(sl), hip.stream()))
        hip.check(L.bg_label_loss_finish(P(x), P(t), P(w), P(slices), P(cols), P(sums), float(B), 5.0, P(loss), P(dl),
                                         B, n, len(sl), hip.stream()))

    def single():
        hip.check(L.bg_sigmoid_ce(P(x), P(t), P(w), 5.0 / (B * n), P(loss), P(dl), B, n, hip.stream()))

    def gather():
        hip.check(L.bg_gather_rows(P(table), P(idx), P(out), 4096, n, B, hip.stream()))
    res = {}
    for name, fn in (("label_loss_two_launches_us", pair), ("sigmoid_ce_one_launch_us", single),
                     ("gather_rows_us", gather)):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        res[name] = round((time.perf_counter() - t0) * 1e6 / reps, 2)
    return res


def _one(a, setting, mixed):
    if setting == "logistic":
        return {"ms_per_iteration_logistic": _time_iterations(a, "logistic", False)}
    if setting == "mixed":
        return {"ms_per_iteration_mixed": _time_iterations(a, mixed, False)}
    if setting == "table":
        return {"ms_per_iteration_logistic_table_draws": _time_iterations(a, "logistic", True)}
    return _time_launches(a, mixed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--n_labels", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="logistic,mixed,table,launches", help="comma-separated settings")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import the package from")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds allowed to each setting's child process")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    euc = max(a.n_labels // 10, 1)
    mixed = "%d-logistic,%d-euclidean" % (a.n_labels - euc, euc) if a.n_labels > 1 else "euclidean"
    if a.child:                                  # one setting, in a process of its own
        sys.path.insert(0, os.path.abspath(a.tree))
        print(json.dumps(_one(a, a.child, mixed)), flush=True)
        return
    import subprocess
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "n_labels": a.n_labels,
           "steps": a.steps, "mixed_spec": mixed}
    for setting in a.only.split(","):
        if setting not in ("logistic", "mixed", "table", "launches"):
            raise SystemExit("unknown setting %r (logistic, mixed, table, launches)" % setting)
        # the GPU work of each setting runs in a child process under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", setting] + \
            [x for k in ("img_size", "ch", "batch", "precision", "n_labels", "steps", "warmup", "tree")
             for x in ("--" + k, str(getattr(a, k)))]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit("setting %r ran past %.0f s: stopping" % (setting, a.timeout))
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-2000:])
            raise SystemExit("setting %r failed with exit status %d: stopping" % (setting, out.returncode))
        res.update(json.loads(out.stdout.strip().splitlines()[-1]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
