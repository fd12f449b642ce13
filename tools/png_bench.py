"""Time the device-side PNG encoder (csrc/png.hip, png.py) against the host path (utils.write_png) on the two things the
project writes: a sample grid and the strips of a sampling-service round.

    python tools/png_bench.py [--img_size 128 --ch 96 --batch 32] [--precision bf16] [--reps 5] [--timeout 900]

Defaults are the generator of BASELINE config 3 (128^2, ch 96, batch 32, bf16): the default 8 x 8 grid is 1024 x 1024 x 3
and a round of 4 * batch one-latent request files is 128 strips.  Prints one JSON line per workload, all measured in one
call (mean of --reps after one untimed pass; device stages by events on the stream, the rest by a host clock around
synchronised work):

    filter_ms / deflate_ms / compact_ms   the three launches on the bytes where they lie
    d2h_ms            records and totals, then the compressed bytes, to the host
    assemble_ms       Adler combination, CRC and framing on the host (png.assemble)
    device_png_ms     png.encode_device as the users call it: tables up, the launches, copies, assembly
    host_png_ms       D2H of the raw bytes + utils.write_png of the same pixels, serial: the path without the variable
    whole_unset_ms / whole_set_ms   BigGAN.save_samples (all grids of one event) / one service round, BG_DEVICE_PNG
                      unset and set
    device_bytes / host_bytes   sizes of the files

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


def _measure(a):
    import numpy as np
    import torch
    import biggan_tensorflow_amd  # noqa: F401
    from biggan_tensorflow_amd import functional as Fn, main as M, model, png, sampling as Sp, scope as S, service as Sv, \
        utils
    torch.set_num_threads(min(16, torch.get_num_threads()))
    work = tempfile.mkdtemp(prefix="png_bench_")
    req_dir = os.path.join(work, "request")
    os.makedirs(req_dir)
    argv = ["--gan_type", "hinge", "--img_size", str(a.img_size), "--ch", str(a.ch), "--batch_size", str(a.batch),
            "--precision", a.precision, "--request_dir", req_dir, "--sample_dir", os.path.join(work, "samples")]
    gan = model.BigGAN(M.parse_args(argv, make_dirs=False), device="cuda", store=S.VariableStore("cuda", seed=42))
    gan.build_model()
    gan.train_step(gan.synthetic_batch())
    B, side, C = a.batch, gan.img_size, gan.c_dim

    def mean_ms(fn, prepare=None):
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

    def event_ms(fn):
        total = 0.0
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                total += e0.elapsed_time(e1)
        return total / a.reps

    def stages(arena, entries):
        """The encoder's stages on images that lie in ``arena``, and the host path on the same pixels."""
        p = png.plan(entries)
        ftab, stab = torch.from_numpy(p.filter_table).cuda(), torch.from_numpy(p.seg_table).cuda()
        m, n = p.seg_table.shape[0], len(entries)
        filtered = torch.empty(p.stream_bytes, dtype=torch.uint8, device="cuda")
        slots = torch.empty(p.slot_bytes, dtype=torch.uint8, device="cuda")
        records = torch.empty(m, 4, dtype=torch.int32, device="cuda")
        out = torch.empty(p.out_bytes, dtype=torch.uint8, device="cuda")
        seg_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        totals = torch.empty(n, 2, dtype=torch.int64, device="cuda")
        res = {"images": n, "segments": m, "raw_bytes": int(sum(h * w * c for _, h, w, c in entries))}
        res["filter_ms"] = event_ms(lambda: Fn.png_filter(arena, ftab, p.max_h, p.bpp, filtered))
        res["deflate_ms"] = event_ms(lambda: Fn.deflate_segments(filtered, stab, p.seg_bytes, slots, records))
        res["compact_ms"] = event_ms(lambda: Fn.deflate_compact(slots, stab, records, out, seg_off, totals))
        got = {}

        def d2h():
            got["rec"], got["tot"] = records.cpu().numpy(), totals.cpu().numpy()
            got["comp"] = out[:int(got["tot"][-1].sum())].cpu().numpy().tobytes()
        res["d2h_ms"] = mean_ms(d2h)
        rec, tot, comp = got["rec"], got["tot"], got["comp"]
        res["kinds_stored"] = int((rec[:, 3] == 0).sum())

        def assemble():
            got["files"] = [png.assemble(w, h, c, comp[int(tot[i, 0]):int(tot[i].sum())], png.adler32_fold(
                [(rec[j, 1], rec[j, 2], p.seg_lens[j]) for j in range(*p.segments[i])]))
                for i, (_, h, w, c) in enumerate(entries)]
        res["assemble_ms"] = mean_ms(assemble)
        res["device_png_ms"] = mean_ms(lambda: png.encode_device(arena, entries))
        assert png.encode_device(arena, entries) == got["files"]
        tmp = os.path.join(work, "host.tmp.png")
        sizes = []

        def host():
            del sizes[:]
            raw = arena.cpu().numpy()
            for off, h, w, c in entries:
                utils.write_png(raw[off:off + h * w * c].reshape(h, w, c), tmp)
                sizes.append(os.path.getsize(tmp))
        res["host_png_ms"] = mean_ms(host)
        res["device_bytes"], res["host_bytes"] = sum(len(f) for f in got["files"]), sum(sizes)
        return res

    def with_variable(value, fn, prepare=None):
        old = os.environ.pop("BG_DEVICE_PNG", None)
        if value:
            os.environ["BG_DEVICE_PNG"] = "1"
        try:
            return mean_ms(fn, prepare)
        finally:
            os.environ.pop("BG_DEVICE_PNG", None)
            if old is not None:
                os.environ["BG_DEVICE_PNG"] = old

    common = {"precision": a.precision, "img_size": side, "ch": a.ch, "batch": B, "reps": a.reps}
    # ---- the default sample grid
    dim, _, batches = Sp.grid_plan(gan.sample_num, B)
    zs, cs = gan.static_sample_set()
    grid = torch.zeros(dim * side, dim * side, C, dtype=torch.uint8, device="cuda")
    gan.generate(zs[:batches * B], None if cs is None else cs[:batches * B], grid=grid, gh=dim, gw=dim)
    res = dict(common, workload="grid", shape=list(grid.shape))
    res.update(stages(grid.reshape(-1), [(0,) + tuple(grid.shape)]))
    res["whole_unset_ms"] = with_variable(False, lambda: gan.save_samples(0, 1))
    res["whole_set_ms"] = with_variable(True, lambda: gan.save_samples(0, 1))
    res["files_per_event"] = len(gan.save_samples(0, 1))
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}), flush=True)

    # ---- a service round of 4 * batch one-latent files
    rng = np.random.RandomState(1)
    z = rng.standard_normal((4 * B, gan.z_dim)).astype(np.float32)

    def refill():
        for i in range(4 * B):
            with open(os.path.join(req_dir, "s%03d.txt" % i), "w") as f:
                f.write("\t".join(str(np.float32(v)) for v in z[i]) + "\n")

    def clear():
        for f in os.listdir(req_dir):
            os.remove(os.path.join(req_dir, f))

    def plan():
        return Sv.plan_round(Sv.read_requests(Sv.list_requests(req_dir)), B, gan.z_dim, 0, side, C)
    refill()
    group = plan().groups[0]
    arena = torch.zeros(group.arena_bytes, dtype=torch.uint8, device="cuda")
    gan.generate(torch.from_numpy(group.z).cuda(), None, _place=(torch.from_numpy(group.table).cuda(), arena))
    res = dict(common, workload="service_round", strips=len(group.files))
    res.update(stages(arena, [(r.offset, side, r.n * side, C) for r in group.files]))
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        res["whole_unset_ms"] = with_variable(False, lambda: gan._serve_round(plan(), req_dir, pool), refill)
        clear()
        res["whole_set_ms"] = with_variable(True, lambda: gan._serve_round(plan(), req_dir, pool), refill)
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}), flush=True)
    shutil.rmtree(work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_size", type=int, default=128)
    ap.add_argument("--ch", type=int, default=96)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
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
        raise SystemExit("png_bench: the GPU step ran past its %d s limit" % a.timeout)
    if rc != 0:
        raise SystemExit("png_bench: the GPU step ended with status %d" % rc)


if __name__ == "__main__":
    main()
