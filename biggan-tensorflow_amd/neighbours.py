"""Is the generator copying the training set?  The nearest training images of generated samples by brute force in pixel
space: every sample against the whole training set, which lives on the device as bf16 search descriptors (the image
box-averaged down to ``--nn_size``).  DESIGN.md ("Nearest training images") gives the plan and the kernel;
csrc/nearest.hip holds the kernels; tests/nn_ref.py restates them in float64.

``NnPlan`` is host arithmetic only: the side of the descriptors, how many files fit, the bytes.  ``NearestSet`` runs a
plan on the device: ``add`` packs batches of training images into the arena once, ``search`` packs queries (plain and,
for a run trained with --random_flip, mirrored), measures them against every row and merges the two lists.  The rest
is the host side of an event: which rows the grid shows, the table, the file names.  Nothing here draws from the
training run's generators, the sampler's or the loader's."""
import os

import numpy as np
import torch

from . import functional as Fn

MIN_SIDE = 8
MAX_K = 8
GRID_ROWS = 8
DEFAULT_GB = 8.0               # the cap on the resident set (BG_NN_GB): a stated default, not a measurement
SYNTHETIC_IMAGES = 2048        # the set of a run without a dataset folder


def budget_bytes(option=None):
    """The cap on the resident set in bytes: ``option`` GiB, else the environment variable BG_NN_GB, else 8 GiB."""
    gb = float(os.environ.get("BG_NN_GB", DEFAULT_GB)) if option is None else float(option)
    if not gb > 0:
        raise ValueError("nn: BG_NN_GB=%s (GiB, > 0)" % gb)
    return int(gb * (1 << 30))


def search_side(img_size, nn_size):
    """min(img_size, --nn_size); both must be powers of two and the result >= 8."""
    img_size, nn_size = int(img_size), int(nn_size)
    if nn_size < MIN_SIDE or nn_size & (nn_size - 1):
        raise ValueError("nn: --nn_size %d: a power of two >= %d" % (nn_size, MIN_SIDE))
    if img_size < MIN_SIDE or img_size & (img_size - 1):
        raise ValueError("nn: --img_size %d: the box filter needs a power of two >= %d" % (img_size, MIN_SIDE))
    return min(img_size, nn_size)


class NnPlan:
    """What one run of the search needs, from the flags alone.

    side, f     descriptors are side x side x c_dim, each value the mean of an f x f box, f = img_size / side
    D           side * side * c_dim values per image (a multiple of 64)
    listed      files the listing (cut to --nn_images) offers; N of them fit ``budget`` bytes at D * 2 bytes each
    N, bytes    rows and size of the resident set;  truncated: N < listed"""

    def __init__(self, img_size, c_dim, batch_size, nn_size=64, nn_images=0, static_sample_seed=0, n_files=None,
                 budget=None):
        if c_dim not in (1, 3, 4):
            raise ValueError("nn: c_dim %d (1, 3 or 4)" % c_dim)
        if int(nn_images) < 0:
            raise ValueError("nn: --nn_images %d" % nn_images)
        self.side = search_side(img_size, nn_size)
        self.img_size, self.c_dim, self.batch_size = int(img_size), int(c_dim), int(batch_size)
        self.f = self.img_size // self.side
        self.D = self.side * self.side * self.c_dim
        self.from_files = n_files is not None
        listed = int(n_files) if self.from_files else (int(nn_images) or SYNTHETIC_IMAGES)
        if self.from_files and int(nn_images) > 0:
            listed = min(listed, int(nn_images))
        if listed < 1:
            raise ValueError("nn: no training images to search")
        self.listed = listed
        self.budget = budget_bytes() if budget is None else int(budget)
        self.N = min(listed, self.budget // (self.D * 2))
        if self.N < 1:
            raise ValueError("nn: BG_NN_GB leaves %d bytes, one descriptor takes %d" % (self.budget, self.D * 2))
        self.truncated = self.N < listed
        self.bytes = self.N * self.D * 2
        self.seed = (int(static_sample_seed) + 7919 * 11) % (1 << 32)

    def describe(self):
        s = "%d images as %dx%dx%d bf16 (box %d), %.1f MB" % (self.N, self.side, self.side, self.c_dim, self.f,
                                                              self.bytes / 1e6)
        if self.truncated:
            s += "; the first %d of %d listed (BG_NN_GB)" % (self.N, self.listed)
        return s


def check_k(k):
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError("nn: --nn_k %d (1..%d)" % (k, MAX_K))
    return k


def merge_lists(plain, mirrored, k):
    """One query's two result lists -> its first k of their union.  ``plain`` / ``mirrored``: sequences of (squared
    distance, set index), index < 0 for a padding entry; ``mirrored`` may be None.  One entry per set index, the smaller
    distance kept and the plain one on equality; sorted by (distance, index).  Returns [(distance, index, mirrored)]."""
    best = {}
    for flag, entries in ((False, plain), (True, mirrored or ())):
        for d, i in entries:
            d, i = float(d), int(i)
            if i < 0:
                continue
            if i not in best or d < best[i][0]:
                best[i] = (d, i, flag)
    return sorted(best.values(), key=lambda e: (e[0], e[1]))[:int(k)]


def synthetic_batch(plan, batch, device):
    """Batch ``batch`` of the set of a run without a dataset: uniform noise in [-1, 1) from a generator seeded by the plan
    and the batch number, so that one image can be drawn again for the grid."""
    lo = batch * plan.batch_size
    gen = torch.Generator(device=device)
    gen.manual_seed((plan.seed + batch) % (1 << 32))
    return torch.rand(min(plan.batch_size, plan.N - lo), plan.img_size, plan.img_size, plan.c_dim, device=device,
                      generator=gen) * 2.0 - 1.0


class NearestSet:
    """A plan on the device: the arena bf16 [N, D] of the training set's descriptors and the search over it."""

    def __init__(self, plan, device, files=None):
        self.plan, self.device = plan, torch.device(device)
        self.arena = torch.empty(plan.N, plan.D, dtype=torch.bfloat16, device=self.device)
        self.files = list(files[:plan.N]) if files is not None else ["synthetic:%d" % i for i in range(plan.N)]
        self.filled = 0
        self.images = {}                       # set index -> its full-size image fp32 [S,S,C] (numpy), as the grids need them

    def add(self, img):
        """Training images [b, S, S, C] (fp32 or bf16) into the next rows; those past N are dropped."""
        p = self.plan
        b = min(int(img.shape[0]), p.N - self.filled)
        if b <= 0:
            return
        if tuple(img.shape[1:]) != (p.img_size, p.img_size, p.c_dim):
            raise ValueError("nn: images of %s, the plan is for %s" % (tuple(img.shape[1:]), (p.img_size, p.img_size, p.c_dim)))
        Fn.nn_pack(img[:b], p.f, False, out=self.arena[self.filled:self.filled + b])
        self.filled += b

    def finish(self):
        if self.filled != self.plan.N:
            raise RuntimeError("nn: %d of %d images arrived" % (self.filled, self.plan.N))
        return self

    def search_packed(self, q, k):
        """(squared distances fp32 [Q,k], indices int32 [Q,k]) of packed queries bf16 [Q, D], on the host."""
        v, i = Fn.nn_topk(Fn.nn_distances(q, self.arena), k)
        return v.cpu().numpy(), i.cpu().numpy()

    def search(self, images, k, mirror):
        """The k nearest rows of every image [Q,S,S,C]; ``mirror``: its mirror image is searched as well.  Returns the
        dict of ``BigGAN.nearest``: dist [Q,k] (RMS per element, sqrt(d / D)), index, mirrored, files; a place past the set
        holds (inf, -1, False, "")."""
        p, k = self.plan, check_k(k)
        Q = int(images.shape[0])
        plain = self.search_packed(Fn.nn_pack(images, p.f, False), k)
        flipped = self.search_packed(Fn.nn_pack(images, p.f, True), k) if mirror else None
        dist = np.full((Q, k), np.inf, dtype=np.float64)
        index = np.full((Q, k), -1, dtype=np.int64)
        mirrored = np.zeros((Q, k), dtype=bool)
        files = [[""] * k for _ in range(Q)]
        for qi in range(Q):
            merged = merge_lists(zip(plain[0][qi], plain[1][qi]),
                                 None if flipped is None else zip(flipped[0][qi], flipped[1][qi]), k)
            for r, (d, i, m) in enumerate(merged):
                dist[qi, r], index[qi, r], mirrored[qi, r] = np.sqrt(d / p.D), i, m
                files[qi][r] = self.files[i]
        return {"dist": dist, "index": index, "mirrored": mirrored, "files": files}


# ---- the host side of an event --------------------------------------------------------------------------
def event_names(model_name, epoch, idx, prefix="nn"):
    """File names of one event: the grid and the table."""
    stem = '{}_{}_{:02d}_{:05d}'.format(model_name, prefix, int(epoch), int(idx))
    return {"png": stem + ".png", "txt": stem + ".txt"}


def grid_queries(result, rows=GRID_ROWS):
    """The queries the grid shows: those with the smallest rank-1 distance, ascending (ties: the lower query number)."""
    first = np.asarray(result["dist"])[:, 0]
    return sorted(range(len(first)), key=lambda q: (first[q], q))[:int(rows)]


def grid_images(result, queries, samples, fetch):
    """fp32 [rows * (k + 1), S, S, C]: per shown query its sample, then its neighbours, a mirrored hit shown mirrored.
    ``samples``: the queries' images [Q,S,S,C] (numpy); ``fetch(index)``: the training image of a set index.  A place past
    the set stays black (-1)."""
    k = np.asarray(result["index"]).shape[1]
    out = np.full((len(queries) * (k + 1),) + tuple(samples.shape[1:]), -1.0, dtype=np.float32)
    for r, q in enumerate(queries):
        out[r * (k + 1)] = samples[q]
        for j in range(k):
            i = int(result["index"][q][j])
            if i >= 0:
                img = fetch(i)
                out[r * (k + 1) + 1 + j] = img[:, ::-1] if result["mirrored"][q][j] else img
    return out


def tsv_lines(result):
    """One line per (query, rank): query number, rank (from 1), RMS distance, 0/1 mirrored, file name."""
    lines = []
    for q, row in enumerate(np.asarray(result["index"])):
        for r, i in enumerate(row):
            if i >= 0:
                lines.append("%d\t%d\t%.6f\t%d\t%s" % (q, r + 1, result["dist"][q][r], int(result["mirrored"][q][r]),
                                                     result["files"][q][r]))
    return lines


def scalars(result, prefix="nn"):
    first = np.asarray(result["dist"])[:, 0]
    return {prefix + "_dist_min": float(first.min()), prefix + "_dist_mean": float(first.mean())}


def write_event(result, samples, fetch, folder, names):
    """The grid (written like the sample grids: utils.save_images) and the table of one event; returns their paths."""
    from .utils import save_images
    queries = grid_queries(result)
    k = np.asarray(result["index"]).shape[1]
    png = save_images(grid_images(result, queries, samples, fetch), [len(queries), k + 1], os.path.join(folder, names["png"]))
    txt = os.path.join(folder, names["txt"])
    with open(txt, "w") as f:
        f.write("".join(line + "\n" for line in tsv_lines(result)))
    return [png, txt]
