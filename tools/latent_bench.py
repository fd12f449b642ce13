"""Time training iterations with the generator's latent-stage flags, which bench.py does not take.

    python tools/latent_bench.py --n_labels 1000 --cls_embedding true [--shared_z 32] [--g_z_dense_concat true]
                                 [--img_size 128 --ch 96 --batch 256 --precision bf16] [--steps 10 --warmup 3]
                                 [--g_only]

Defaults are BASELINE config 3 on one GPU (128^2, ch 96, batch 256, bf16, --da_policy full).  Synthetic images and
one-hot labels; eager iterations (D step then G step, or the G step alone with --g_only, e.g. under a kernel trace).
Prints one JSON line with ms per iteration.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--n_labels", type=int, default=0)
    ap.add_argument("--cls_embedding", default="false")
    ap.add_argument("--shared_z", type=int, default=0)
    ap.add_argument("--g_z_dense_concat", default="false")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--g_only", action="store_true")
    a = ap.parse_args()

    import torch
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import main as M, model, scope as S
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--n_labels", str(a.n_labels), "--cls_embedding", a.cls_embedding,
            "--shared_z", str(a.shared_z), "--g_z_dense_concat", a.g_z_dense_concat]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), store=S.VariableStore("cuda", seed=1)).build_model()
    B = a.batch
    real = gan.synthetic_batch(B)
    labels = gan.synthetic_labels(B) if gan.acgan else None

    def step():
        if a.g_only:
            gan.g_step(B, cls_z=labels)
        else:
            gan.train_step(real, labels)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    print(json.dumps({"img_size": a.img_size, "ch": a.ch, "batch": B, "precision": a.precision,
                      "n_labels": a.n_labels, "cls_embedding": a.cls_embedding, "shared_z": a.shared_z,
                      "g_z_dense_concat": a.g_z_dense_concat, "g_only": a.g_only, "steps": a.steps,
                      "ms_per_iteration": round(ms, 3),
                      "group_cbn": os.environ.get("BG_GROUP_CBN", "1")}))


if __name__ == "__main__":
    main()
