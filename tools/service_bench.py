"""Time poll rounds of the sampling service (BigGAN.service) in-process and split them by stage.

    python tools/service_bench.py [--img_size 128 --ch 96 --batch 32] [--precisions bf16,fp32] [--reps 3] [--timeout 900]

Defaults are the generator of BASELINE config 3 (128^2, ch 96) at its per-GPU batch of 32, in bf16 and in fp32.  Every
request asks for the discriminator's outputs too.  Three rounds per precision, all in one call:

    singles     4 * batch files of one latent each, pending together: they share 4 generator batches
    full        4 files of batch latents each: the same 4 batches, 4 wide strips
    one_by_one  the files of ``singles`` fed one file per round: a full batch per image, the reference's cost model

Prints one JSON line per precision and round, ms per round (mean of --reps after one untimed pass of every shape; a host
clock around synchronised work):

    round_ms          the whole round as the service runs it: listing, reading, planning, the device work, responses
                      written by the thread pool, request files removed
    images_per_s      images answered / round_ms
    file_io_ms        listing + reading + planning, and the .out files + removals (serial, measured on their own)
    generator_ms      the generator passes of the round alone (float images out)
    discriminator_ms  generator + discriminator passes minus generator_ms
    place_copy_ms     zero-fill of the arena + one bg_image_place_u8 per batch + the D2H copy of the strips
    png_ms            utils.write_png of every strip, serial (the round encodes them on up to 8 threads)

The measurement runs in a child process under its own time limit (--timeout seconds); host work uses at most 16 threads.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _measure_precision(a, precision):
    import numpy as np
    import torch
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, main as M, model, scope as S, service as Sv, utils
    req_dir = tempfile.mkdtemp(prefix="service_bench_")
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", precision, "--request_dir", req_dir]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    gan.train_step(gan.synthetic_batch())
    B, side = a.batch, gan.img_size
    rng = np.random.RandomState(1)
    z = rng.standard_normal((4 * B, gan.z_dim)).astype(np.float32)

    def put(name, rows):
        path = os.path.join(req_dir, name + ".txt")
        with open(path, "w") as f:
            f.write("!use_discriminator=1\n")
            for row in rows:
                f.write("\t".join(str(np.float32(v)) for v in row) + "\n")
        return path

    def clear():
        for f in os.listdir(req_dir):
            os.remove(os.path.join(req_dir, f))

    def plan():
        return Sv.plan_round(Sv.read_requests(Sv.list_requests(req_dir)), B, gan.z_dim, 0, side, gan.c_dim)

    def mean_ms(fn, prepare=None):
        """ms per call of fn: one untimed pass, then --reps timed ones; ``prepare`` runs before each, off the clock."""
        total = 0.0
        for rep in range(a.reps + 1):
            if prepare:
                prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                total += time.perf_counter() - t0
        return total * 1e3 / a.reps

    layouts = {"singles": [("s%03d" % i, z[i:i + 1]) for i in range(4 * B)],
               "full": [("f%d" % i, z[i * B:(i + 1) * B]) for i in range(4)]}
    results = []
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        def serve_pending():
            return gan._serve_round(plan(), req_dir, pool)

        def stages(files):
            """The stages of the round that answers ``files`` together, each on its own."""
            clear()
            for name, rows in files:
                put(name, rows)
            io_read = mean_ms(plan)
            rnd = plan()
            group = rnd.groups[0]
            gen = mean_ms(lambda: gan.generate(group.z))
            gen_d = mean_ms(lambda: gan.generate(group.z, with_discriminator=True))
            imgs, outs = gan.generate(group.z, with_discriminator=True)
            pad = -imgs.shape[0] % B
            imgs = torch.cat([imgs, imgs[:1].expand(pad, -1, -1, -1)]) if pad else imgs
            table = torch.from_numpy(group.table).cuda()
            host = {}

            def place_copy():
                arena = torch.zeros(group.arena_bytes, dtype=torch.uint8, device="cuda")
                for b in range(0, imgs.shape[0], B):
                    Fn.image_place_u8(imgs[b:b + B], table[b:b + B], arena)
                buf = torch.empty(group.arena_bytes, dtype=torch.uint8, pin_memory=True)
                buf.copy_(arena, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                host["arena"] = buf.numpy()
            place = mean_ms(place_copy)
            arena = host["arena"]
            o = {k: v.cpu().numpy() for k, v in outs.items()}
            tmp = os.path.join(req_dir, "bench.tmp.png")

            def encode():
                for req in group.files:
                    utils.write_png(arena[req.offset:req.offset + side * req.pitch].reshape(side, req.n * side, gan.c_dim),
                                    tmp)
            png = mean_ms(encode)
            os.remove(tmp)

            def outs_and_removals():
                for req in group.files:
                    for k in sorted(o):
                        utils.write_vectors(os.path.join(req_dir, req.name + "_" + k + ".out"),
                                            o[k][req.first:req.first + req.n])
                    os.remove(req.path)

            def refill():
                for name, rows in files:
                    put(name, rows)
            io_write = mean_ms(outs_and_removals, refill)
            clear()
            return {"file_io_ms": io_read + io_write, "generator_ms": gen, "discriminator_ms": gen_d - gen,
                    "place_copy_ms": place, "png_ms": png}

        for kind in ("singles", "full"):
            files = layouts[kind]
            split = stages(files)
            round_ms = mean_ms(serve_pending, lambda: [put(n, r) for n, r in files])
            clear()
            results.append((kind, len(files), 4 * B, round_ms, split))
        # the reference's cost model: every file a round (and a padded batch) of its own
        files = layouts["singles"]
        split = stages(files[:1])

        def one_by_one():
            for n, r in files:
                put(n, r)
                serve_pending()
        round_ms = mean_ms(one_by_one)
        clear()
        results.append(("one_by_one", len(files), 4 * B, round_ms, {k: v * len(files) for k, v in split.items()}))
    shutil.rmtree(req_dir)
    for kind, n_files, n_img, round_ms, split in results:
        res = {"round": kind, "precision": precision, "img_size": a.img_size, "ch": a.ch, "batch": B, "files": n_files,
               "images": n_img, "reps": a.reps, "round_ms": round(round_ms, 3),
               "images_per_s": round(n_img / (round_ms * 1e-3), 1)}
        res.update({k: round(v, 3) for k, v in split.items()})
        print(json.dumps(res), flush=True)
    del gan
    torch.cuda.empty_cache()


def _measure(a):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for precision in a.precisions.split(","):
        _measure_precision(a, precision)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precisions", default="bf16,fp32")
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
        raise SystemExit("service_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("service_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
