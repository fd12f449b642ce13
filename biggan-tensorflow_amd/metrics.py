"""In-training quality score: the sliced Wasserstein distance (SWD) between Laplacian-pyramid patches of real and generated
images (Karras et al. 2018, "Progressive Growing of GANs", section 5 and table 1).  One number per pyramid level - fine
texture at full resolution, layout at 16 px - as ``swd_<side>`` (x 1e3) and their mean ``swd_avg``.  DESIGN.md gives
the definition; csrc/swd.hip holds the kernels; tests/swd_ref.py restates the metric in float64.

``SwdPlan`` is host arithmetic only: levels, the power-of-two image count, buffer sizes, seeds and the draws.  ``Swd``
runs a plan on the device.  The metric has random generators of its own, derived from --static_sample_seed: nothing is
drawn from the training run's generators, the sampler's, or the loader's, and every draw is made once per run, so
consecutive events differ by the weights alone."""
import numpy as np
import torch

from . import functional as Fn, sampling as Sp

PATCHES = 128          # per image and level
TAPS = 49              # 7 x 7
REPEATS = 4
N_DIRS = 128           # directions per repeat
MIN_SIDE = 16


def level_sides(img_size):
    """[img_size, img_size / 2, ..., 16]: 64 px gives 3 levels, 128 px 4, 256 px 5, 512 px 6."""
    img_size = int(img_size)
    if img_size < 2 * MIN_SIDE or img_size & (img_size - 1):
        raise ValueError("swd: --img_size %d: the pyramid needs a power of two >= %d" % (img_size, 2 * MIN_SIDE))
    sides = [img_size]
    while sides[-1] > MIN_SIDE:
        sides.append(sides[-1] // 2)
    return sides


def floor_pow2(n):
    n = int(n)
    if n < 1:
        raise ValueError("swd: no images to measure (%d)" % n)
    return 1 << (n.bit_length() - 1)


class SwdPlan:
    """What one run of the metric needs, from the flags alone.

    n_images    --swd_images rounded down to a power of two (the sort takes power-of-two segments), and to the largest
                power of two <= the number of dataset files when there is a dataset
    n_rows      N = 128 * n_images descriptors per level and set;  K = 49 * c_dim values each;  S = 4 * 128 directions
    seeds       one per draw, derived from --static_sample_seed"""

    def __init__(self, img_size, c_dim, batch_size, swd_images, static_sample_seed, n_files=None, repeats=REPEATS,
                 n_dirs=N_DIRS):
        if c_dim not in (1, 3, 4):
            raise ValueError("swd: c_dim %d (1, 3 or 4)" % c_dim)
        self.sides = level_sides(img_size)
        self.img_size, self.c_dim, self.batch_size = int(img_size), int(c_dim), int(batch_size)
        self.n_images = floor_pow2(swd_images if n_files is None else min(int(swd_images), int(n_files)))
        self.from_files = n_files is not None
        self.repeats, self.n_dirs = int(repeats), int(n_dirs)
        self.n_rows = PATCHES * self.n_images
        self.K = TAPS * self.c_dim
        self.S = self.repeats * self.n_dirs
        base = int(static_sample_seed)
        self.seeds = {name: (base + 7919 * (i + 1)) % (1 << 32)
                      for i, name in enumerate(("directions", "pos_real", "pos_fake", "latents", "labels", "real"))}

    # ---- sizes in bytes -------------------------------------------------------------------------
    @property
    def desc_bytes(self):
        """One level of one set: fp32 [N, K]."""
        return self.n_rows * self.K * 4

    @property
    def real_bytes(self):
        """What stays resident between events: the real set's descriptors of every level."""
        return len(self.sides) * self.desc_bytes

    @property
    def projection_bytes(self):
        """The sort buffer of one level: both sets, S segments of N floats each."""
        return 2 * self.S * self.n_rows * 4

    @property
    def peak_bytes(self):
        """Real and fake descriptors of every level plus one level's projections."""
        return 2 * self.real_bytes + self.projection_bytes

    # ---- draws -------------------------------------------------------------------------------------
    def draw_directions(self):
        """Per level fp32 [K, S]: per repeat a normal [K, n_dirs] draw, every column scaled to unit length."""
        rng = np.random.RandomState(self.seeds["directions"])
        out = []
        for _ in self.sides:
            d = rng.randn(self.repeats, self.K, self.n_dirs)
            d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
            out.append(np.ascontiguousarray(d.transpose(1, 0, 2).reshape(self.K, self.S).astype(np.float32)))
        return out

    def draw_positions(self, which):
        """Per level int32 [n_images, 128, 2] = (y, x): patch centres uniform in [3, side - 3), independent per level."""
        rng = np.random.RandomState(self.seeds["pos_" + which])
        return [rng.randint(3, side - 3, size=(self.n_images, PATCHES, 2)).astype(np.int32) for side in self.sides]

    def draw_latents(self, z_dim, trunc):
        """fp32 [n_images, 1, 1, z_dim] (sampling.draw_z) from a torch generator of the metric's own."""
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seeds["latents"])
        return Sp.draw_z(self.n_images, z_dim, g, trunc)

    def draw_labels(self, label_table):
        """fp32 [n_images, n_labels]: rows of the label table, drawn with replacement."""
        return Sp.draw_n_tags(label_table, self.n_images, np.random.RandomState(self.seeds["labels"]))


class Swd:
    """A plan on the device.  ``begin`` / ``add`` / ``finish`` fill one set's descriptors a batch of images at a time
    (pyramid, gather, discard); ``scores`` projects, sorts and compares the two sets, one level at a time."""

    def __init__(self, plan, device):
        self.plan, self.device = plan, torch.device(device)
        self.dirs = [torch.from_numpy(d).to(self.device) for d in plan.draw_directions()]
        self.pos = {w: [torch.from_numpy(p).to(self.device) for p in plan.draw_positions(w)] for w in ("real", "fake")}
        self.real = None                       # (descriptors per level, statistics per level) of the real set, kept
        self.fake_inputs = None                # (latents, class vectors or None) of the fake set, drawn once by the model

    def begin(self, which):
        p = self.plan
        self._which, self._filled = which, 0
        self._desc = [torch.empty(p.n_rows, p.K, dtype=torch.float32, device=self.device) for _ in p.sides]
        self._part = [Fn.swd_partials(p.n_images, p.c_dim, self.device) for _ in p.sides]

    def add(self, img):
        """Images [b, S, S, C] (fp32 or bf16); those past n_images (the padding of a last generator batch) are dropped."""
        p = self.plan
        b = min(int(img.shape[0]), p.n_images - self._filled)
        if b <= 0:
            return
        g = img[:b]
        if tuple(g.shape[1:]) != (p.img_size, p.img_size, p.c_dim):
            raise ValueError("swd: images of %s, the plan is for %s" % (tuple(g.shape[1:]), (p.img_size, p.img_size, p.c_dim)))
        lo = self._filled
        for i in range(len(p.sides)):
            if i + 1 < len(p.sides):
                g1 = Fn.swd_pyr_down(g)
                level = Fn.swd_pyr_lap(g, g1)
            else:
                level, g1 = g, None                # the last level is the 16 px Gaussian itself
            Fn.swd_descriptors(level, self.pos[self._which][i][lo:lo + b], self._desc[i], lo * PATCHES, self._part[i])
            g = g1
        self._filled += b

    def finish(self):
        if self._filled != self.plan.n_images:
            raise RuntimeError("swd: %d of %d images arrived" % (self._filled, self.plan.n_images))
        out = (self._desc, [Fn.swd_stats(w) for w in self._part])
        self._desc = self._part = None
        return out

    def scores(self, fake, prefix="swd"):
        """{prefix_<side>: 1e3 * distance, prefix_avg: their mean} of the kept real set against ``fake`` (what ``finish``
        returned).  One projection launch and one sort per level cover both sets; the host reads all levels at once."""
        p = self.plan
        sums = torch.empty(len(p.sides), p.repeats, dtype=torch.float64, device=self.device)
        for i in range(len(p.sides)):
            proj = torch.empty(2 * p.S, p.n_rows, dtype=torch.float32, device=self.device)
            Fn.swd_project(self.real[0][i], self.real[1][i], self.dirs[i], proj, fake[0][i], fake[1][i])
            Fn.swd_sort_segments(proj, p.n_rows)
            Fn.swd_l1(proj[:p.S], proj[p.S:], p.repeats, out=sums[i])
            del proj
        per_level = (sums.cpu().numpy() / float(p.n_rows * p.n_dirs)).mean(axis=1) * 1e3
        out = {"%s_%d" % (prefix, side): float(v) for side, v in zip(p.sides, per_level)}
        out[prefix + "_avg"] = float(np.mean(per_level))
        return out


def format_scores(scores):
    return ", ".join("%s: %.4f" % kv for kv in scores.items())
