"""Time training iterations with the discriminator's reconstruction heads (--d_reconstruction, --d_reconstruction_halfres,
--d_reconstruction_texture) next to the model without them, which is all bench.py takes.

    python tools/recon_bench.py [--img_size 128 --ch 96 --batch 256 --precision bf16] [--steps 10 --warmup 3]
                                [--only off,texture,halfres,coarse,both] [--fuse both|1|0] [--d_only]

Defaults are BASELINE config 3 on one GPU (128^2, ch 96, batch 256, bf16, --da_policy full, ortho_cosine regulariser)
and bench.py's timing protocol (seed 42 store, settle_host, synchronised warm-up steps, one synchronisation around the
timed steps), so the "off" figure is bench.py's own.  Settings: off (no flag), texture, halfres, coarse (the full-size
coarse head), both (halfres + texture).  Every setting with a head is timed with the batch norm and the GLU of each
upscale stage in one kernel (BG_FUSE_BNGLU=1, the default) and as bn then glu (BG_FUSE_BNGLU=0).  Synthetic images; eager
iterations (D step then G step, or the D step alone with --d_only, e.g. under a kernel trace).  Prints one JSON line with
ms per iteration of each run.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = {
    "off": [],
    "texture": ["--d_reconstruction_texture", "true"],
    "halfres": ["--d_reconstruction_halfres", "true"],
    "coarse": ["--d_reconstruction", "true"],
    "both": ["--d_reconstruction_halfres", "true", "--d_reconstruction_texture", "true"],
}


def _time(a, setting, fuse):
    import gc
    import torch
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import main as M, model, scope as S
    os.environ["BG_FUSE_BNGLU"] = "1" if fuse else "0"
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--da_policy", "full", "--g_regularization", "ortho_cosine", "--n_labels", "0", "--precision", a.precision]
    argv += SETTINGS[setting]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    B = a.batch
    real = gan.synthetic_batch(B)

    def step():
        if a.d_only:
            gan.d_step(real)
        else:
            gan.train_step(real)
    gan.settle_host()
    for _ in range(a.warmup):
        step()
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    del gan, real
    gc.collect()
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
    ap.add_argument("--only", default="off,texture,halfres,coarse,both", help="comma-separated settings")
    ap.add_argument("--fuse", choices=("both", "1", "0"), default="both", help="BG_FUSE_BNGLU of the runs with a head")
    ap.add_argument("--d_only", action="store_true")
    a = ap.parse_args()
    res = {"img_size": a.img_size, "ch": a.ch, "batch": a.batch, "precision": a.precision, "d_only": a.d_only,
           "steps": a.steps}
    for setting in a.only.split(","):
        if setting not in SETTINGS:
            raise SystemExit("unknown setting %r (one of %s)" % (setting, ", ".join(SETTINGS)))
        if setting == "off":
            res["ms_per_iteration_off"] = _time(a, setting, True)
        else:
            for fuse in ((1, 0) if a.fuse == "both" else (int(a.fuse),)):
                res["ms_per_iteration_%s_fuse%d" % (setting, fuse)] = _time(a, setting, bool(fuse))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
