"""Time training iterations at --c_dim 3, 4 and 1 (RGB, RGBA with the alpha mask and the alpha helper, grayscale),
which bench.py does not take.

    python tools/rgba_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16] [--steps 10 --warmup 3]
                               [--c_dims 3,4,1] [--g_only]

Defaults are BASELINE config 3 on one GPU (128^2, ch 96, batch 256, bf16, --da_policy full).  Synthetic images; eager
iterations (D step then G step, or the G step alone with --g_only, e.g. under a kernel trace).  Prints one JSON line
with ms per iteration at each channel count.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(a, c_dim):
    import torch
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import main as M, model, scope as S
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--c_dim", str(c_dim)]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), store=S.VariableStore("cuda", seed=1)).build_model()
    B = a.batch
    real = gan.synthetic_batch(B)

    def step():
        if a.g_only:
            gan.g_step(B)
        else:
            gan.train_step(real)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    del gan
    torch.cuda.empty_cache()
    return round(ms, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c_dims", default="3,4,1")
    ap.add_argument("--g_only", action="store_true")
    a = ap.parse_args()
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "g_only": a.g_only,
           "steps": a.steps}
    for c in (int(s) for s in a.c_dims.split(",")):
        res["ms_per_iteration_c%d" % c] = _time(a, c)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
