"""In-training quality score: the sliced Wasserstein distance (SWD) between Laplacian-pyramid patches of real and generated
images (Karras et al. 2018, "Progressive Growing of GANs", section 5 and table 1).  One number per pyramid level - fine
texture at full resolution, layout at 16 px - as ``swd_<side>`` (x 1e3) and their mean ``swd_avg``.  DESIGN.md gives
the definition; csrc/swd.hip holds the kernels; tests/swd_ref.py restates the metric in float64.

``SwdPlan`` is host arithmetic only: levels, the power-of-two image count, buffer sizes, seeds and the draws.  ``Swd``
runs a plan on the device.  The metric has random generators of its own, derived from --static_sample_seed: nothing is
drawn from the training run's generators, the sampler's, or the loader's, and every draw is made once per run, so
consecutive events differ by the weights alone.

In-training diversity score: the mean multi-scale structural similarity (MS-SSIM; Wang, Simoncelli and Bovik 2003) of
pairs of generated images that share a class vector (Odena et al. 2017), as ``msssim`` (lower is more diverse, 1.0 is
collapse).  ``MsssimPlan`` / ``Msssim`` follow the same split and the same rules for draws; csrc/msssim.hip holds the
kernels; tests/msssim_ref.py restates the metric in float64.

In-training frequency check: the azimuthally averaged power spectrum of real and generated images (Durall et al. 2020,
"Watch your Up-Convolution"), as ``ps_dist`` / ``ps_hf`` / ``ps_peak`` / ``ps_peak_at``: grid artefacts of an up-sampling
route are spikes at the axis and corner Nyquist frequencies, blur is a deficit of the high bins.  ``PowerSpectrumPlan`` /
``PowerSpectrum`` follow the same split and the same rules for draws; csrc/powerspec.hip holds the kernels;
tests/ps_ref.py restates the metric in float64.

In-training fidelity / coverage split: improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage
(Naeem et al. 2020) of the generated set against the real set in the box-filtered pixel descriptors of the memorisation
check, as ``pr_precision`` / ``pr_recall`` / ``pr_density`` / ``pr_coverage``: samples off the data manifold lower the
first and third, dropped modes the second and fourth.  ``PrdcPlan`` / ``Prdc`` follow the same split and the same rules
for draws; csrc/prdc.hip holds the kernels; tests/prdc_ref.py restates the metric in float64."""
import math

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


class MonitorPlan:
    """What the plans of the monitors share.  A plan class states ``name`` (its tag in messages), ``seed_stride`` and
    ``draws`` (the names of its seeds, in order), and its constructor sets ``n_fake`` (images generated per event) and
    ``n_stream`` (real images read at the first event)."""
    name, seed_stride, draws = None, None, ()
    images_per_label = 1                   # generated images that share one drawn row of the label table

    def __init__(self, img_size, c_dim, batch_size, static_sample_seed, n_files):
        if c_dim not in (1, 3, 4):
            raise ValueError("%s: c_dim %d (1, 3 or 4)" % (self.name, c_dim))
        self.img_size, self.c_dim, self.batch_size = int(img_size), int(c_dim), int(batch_size)
        self.from_files = n_files is not None
        base = int(static_sample_seed)
        self.seeds = {name: (base + self.seed_stride * (i + 1)) % (1 << 32) for i, name in enumerate(self.draws)}

    def real_order(self):
        """Indices into the dataset's listing of the real images, in stream order; None: the first ``n_stream`` files."""
        return None

    def draw_latents(self, z_dim, trunc):
        """fp32 [n_fake, 1, 1, z_dim] (sampling.draw_z) from a torch generator of the metric's own."""
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seeds["latents"])
        return Sp.draw_z(self.n_fake, z_dim, g, trunc)

    def draw_labels(self, label_table):
        """fp32 [n_fake, n_labels]: rows of the label table, drawn with replacement, each for ``images_per_label``
        consecutive images."""
        rows = Sp.draw_n_tags(label_table, self.n_fake // self.images_per_label, np.random.RandomState(self.seeds["labels"]))
        return np.repeat(rows, self.images_per_label, axis=0)


class Monitor:
    """What the runners share: a plan on the device with the kept real set and the fake set's inputs, the bookkeeping of
    ``add`` and ``finish``, and the event driver.  A runner has ``begin`` / ``add`` / ``finish`` of its own, states
    ``prefix`` (of its scores' names) and may override ``begin_set`` / ``name_scores`` / ``real_scores``.  ``ops``: the
    launch wrappers (functional.py)."""
    prefix = None

    def __init__(self, plan, device, ops=None):
        self.plan, self.device = plan, torch.device(device)
        self.ops = Fn if ops is None else ops
        self.real = None                       # what ``finish`` returned for the real set, computed at the first event
        self.fake_inputs = None                # (latents, class vectors or None) of the fake set, drawn once by the model

    # ---- bookkeeping of one set ----------------------------------------------------------------------
    def _expect(self, n):
        self._n, self._filled = int(n), 0

    def _take(self, img):
        """The rows of ``img`` that the set still misses (None when it is full); the caller adds them to ``_filled``."""
        p = self.plan
        b = min(int(img.shape[0]), self._n - self._filled)
        if b <= 0:
            return None
        g = img[:b]
        if tuple(g.shape[1:]) != (p.img_size, p.img_size, p.c_dim):
            raise ValueError("%s: images of %s, the plan is for %s" % (p.name, tuple(g.shape[1:]), (p.img_size, p.img_size, p.c_dim)))
        return g

    def _check_full(self):
        if self._filled != self._n:
            raise RuntimeError("%s: %d of %d images arrived" % (self.plan.name, self._filled, self._n))

    # ---- one event --------------------------------------------------------------------------------------
    def begin_set(self, real):
        self.begin(self.plan.n_stream if real else None)

    def name_scores(self, fake, ema):
        """The scores of one finished fake set under the names they are logged by: ps_dist / ps_dist_noema."""
        return {k + ("" if ema else "_noema"): v for k, v in self.scores(self.real, fake).items()}

    def real_scores(self):
        """What the real set alone adds to the first event's scores."""
        return {}

    def event(self, real_batches, generate, ema, noema, details=False):
        """One event: (scores, {tag: what ``finish`` returned} when ``details``, else {}).  The first one measures the
        real set, from the batches that ``real_batches()`` yields, and keeps it.  Then the moving averages' fake set and
        / or the live weights', as ``ema`` / ``noema`` say: ``generate(ema, consume)`` passes every generated batch to
        ``consume``.  A finished fake set is dropped once its scores are named unless ``details`` asks for it."""
        first = self.real is None
        if first:
            self.begin_set(True)
            for batch in real_batches():
                self.add(batch)
            self.real = self.finish()
        out, sets = {}, {}
        for from_ema, wanted in ((True, ema), (False, noema)):
            if wanted:
                self.begin_set(False)
                generate(from_ema, self.add)
                fake = self.finish()
                out.update(self.name_scores(fake, from_ema))
                if details:
                    sets[self.prefix + ("" if from_ema else "_noema")] = fake
                del fake                       # (the next set is generated without this one resident)
        if first:
            out.update(self.real_scores())
        return out, sets


class SwdPlan(MonitorPlan):
    """What one run of the metric needs, from the flags alone.

    n_images    --swd_images rounded down to a power of two (the sort takes power-of-two segments), and to the largest
                power of two <= the number of dataset files when there is a dataset
    n_rows      N = 128 * n_images descriptors per level and set;  K = 49 * c_dim values each;  S = 4 * 128 directions
    seeds       one per draw, derived from --static_sample_seed"""
    name, seed_stride = "swd", 7919
    draws = ("directions", "pos_real", "pos_fake", "latents", "labels", "real")

    def __init__(self, img_size, c_dim, batch_size, swd_images, static_sample_seed, n_files=None, repeats=REPEATS,
                 n_dirs=N_DIRS):
        super().__init__(img_size, c_dim, batch_size, static_sample_seed, n_files)
        self.sides = level_sides(img_size)
        self.n_fake = self.n_stream = self.n_images = \
            floor_pow2(swd_images if n_files is None else min(int(swd_images), int(n_files)))
        self.repeats, self.n_dirs = int(repeats), int(n_dirs)
        self.n_rows = PATCHES * self.n_images
        self.K = TAPS * self.c_dim
        self.S = self.repeats * self.n_dirs

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


class Swd(Monitor):
    """A plan on the device.  ``begin`` / ``add`` / ``finish`` fill one set's descriptors a batch of images at a time
    (pyramid, gather, discard); ``scores`` projects, sorts and compares the two sets, one level at a time."""

    prefix = "swd"

    def __init__(self, plan, device):
        super().__init__(plan, device)         # real: (descriptors per level, statistics per level) of the real set
        self.dirs = [torch.from_numpy(d).to(self.device) for d in plan.draw_directions()]
        self.pos = {w: [torch.from_numpy(p).to(self.device) for p in plan.draw_positions(w)] for w in ("real", "fake")}

    def begin(self, which):
        p = self.plan
        self._which = which
        self._expect(p.n_images)
        self._desc = [torch.empty(p.n_rows, p.K, dtype=torch.float32, device=self.device) for _ in p.sides]
        self._part = [Fn.swd_partials(p.n_images, p.c_dim, self.device) for _ in p.sides]

    def add(self, img):
        """Images [b, S, S, C] (fp32 or bf16); those past n_images (the padding of a last generator batch) are dropped."""
        p, g = self.plan, self._take(img)
        if g is None:
            return
        lo, b = self._filled, int(g.shape[0])
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
        self._check_full()
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

    def begin_set(self, real):
        self.begin("real" if real else "fake")

    def name_scores(self, fake, ema):
        return self.scores(fake, "swd" if ema else "swd_noema")            # swd_64 / swd_noema_64


# ---- in-training diversity score: mean MS-SSIM of generated pairs (csrc/msssim.hip; DESIGN.md gives the definition) ----
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli and Bovik 2003
MS_TAPS, MS_SIGMA, MS_MIN_SIDE = 11, 1.5, 16


def msssim_sides(img_size):
    """[img_size, img_size / 2, ...]: L = min(5, log2(img_size) - 3) levels, the coarsest of at least 16 px: 32 px gives 2
    levels, 64 px 3, 128 px 4, 256 px and more 5."""
    img_size = int(img_size)
    if img_size < MS_MIN_SIDE or img_size & (img_size - 1):
        raise ValueError("msssim: --img_size %d: the pyramid needs a power of two >= %d" % (img_size, MS_MIN_SIDE))
    levels = min(len(MS_WEIGHTS), img_size.bit_length() - 1 - 3)
    return [img_size >> i for i in range(levels)]


def msssim_weights(levels):
    """The first ``levels`` of the published five weights over their sum.  (With fewer than five levels the score is this
    project's convention and not comparable with published five-level numbers.)"""
    w = np.asarray(MS_WEIGHTS[:int(levels)], dtype=np.float64)
    return w / w.sum()


class MsssimPlan(MonitorPlan):
    """What one run of the diversity score needs, from the flags alone.

    n_pairs       P = --msssim_pairs generated pairs; the two images of a pair have independent latents and, with
                  --n_labels, one class vector (a row of the label table): the intra-class diversity of AC-GAN
    n_real_pairs  pairs of the real baseline: P random pairs of the first 2 P dataset files (fewer when the dataset has
                  fewer than 2 P files), or P pairs of uniform noise without a dataset
    seeds         one per draw, derived from --static_sample_seed; none is shared with SwdPlan or NnPlan"""
    name, seed_stride, draws = "msssim", 15485863, ("latents", "labels", "real", "real_pairs")
    images_per_label = 2                   # rows 2 p and 2 p + 1 are pair p: independent latents, one class vector

    def __init__(self, img_size, c_dim, batch_size, msssim_pairs, static_sample_seed, n_files=None):
        super().__init__(img_size, c_dim, batch_size, static_sample_seed, n_files)
        self.sides = msssim_sides(img_size)
        self.weights = msssim_weights(len(self.sides))
        self.n_pairs = int(msssim_pairs)
        if self.n_pairs < 1:
            raise ValueError("msssim: no pairs to measure (%d)" % self.n_pairs)
        self.n_real_pairs = self.n_pairs if n_files is None else min(self.n_pairs, int(n_files) // 2)
        if self.n_real_pairs < 1:
            raise ValueError("msssim: the real baseline needs two dataset files, there are %d" % int(n_files))
        self.n_fake, self.n_stream = 2 * self.n_pairs, 2 * self.n_real_pairs

    # ---- sizes in bytes -------------------------------------------------------------------------
    @property
    def batch_pairs(self):
        """The most pairs one ``add`` launches: a generator batch and the image carried over from the one before."""
        return (self.batch_size + 1) // 2

    @property
    def tiles_per_pair(self):
        return sum((s // 16) ** 2 for s in self.sides)

    @property
    def workspace_bytes(self):
        """The fp64 partial sums of one generator batch: (cs, ssim) per pair, 16 x 16 tile, channel and level."""
        return self.batch_pairs * self.tiles_per_pair * self.c_dim * 2 * 8

    @property
    def pyramid_bytes(self):
        """The pooled fp32 images of one generator batch, both sets, every level below the first."""
        return sum(2 * self.batch_pairs * s * s * self.c_dim * 4 for s in self.sides[1:])

    @property
    def score_bytes(self):
        return self.n_pairs * 8

    @property
    def peak_bytes(self):
        """All that exists during an event besides the generator's own batch: nothing of size P x S^2."""
        return self.workspace_bytes + self.pyramid_bytes + self.score_bytes

    # ---- draws -------------------------------------------------------------------------------------
    def draw_real_pairs(self):
        """int64 [n_real_pairs, 2]: a random perfect matching of the first 2 n_real_pairs dataset files."""
        perm = np.random.RandomState(self.seeds["real_pairs"]).permutation(2 * self.n_real_pairs)
        return perm.reshape(self.n_real_pairs, 2).astype(np.int64)

    def real_order(self):
        return self.draw_real_pairs().reshape(-1)


class Msssim(Monitor):
    """A plan on the device.  ``begin`` / ``add`` / ``finish``: images arrive a generator batch at a time, rows 2 p and
    2 p + 1 of the stream being pair p.  A batch may hold an odd number of images, so the last image of one batch can be
    the first of a pair that the next batch completes: it is carried.  Per batch one workspace and one pooled pyramid
    exist; what stays is the fp64 score of every pair.  ``ops``: the launch wrappers (functional.py)."""
    prefix = "msssim"

    def begin(self, n_pairs=None):
        n_pairs = self.plan.n_pairs if n_pairs is None else int(n_pairs)
        self._expect(2 * n_pairs)
        self._scores = torch.zeros(n_pairs, dtype=torch.float64, device=self.device)
        self._pairs, self._carry = 0, None

    def _launch(self, x):
        """x [2 p, S, S, C]: p pairs as consecutive rows -> their scores at rows ``self._pairs`` on."""
        p, ops = self.plan, self.ops
        n = int(x.shape[0]) // 2
        ws = ops.msssim_workspace(n, p.img_size, p.c_dim, self.device)
        a, b = x, None
        for i, side in enumerate(p.sides):
            pool = None
            if i + 1 < len(p.sides):
                pool = torch.empty(2, n, side // 2, side // 2, p.c_dim, dtype=torch.float32, device=self.device)
            ops.msssim_level(a, b, p.img_size, i, ws, pool)
            if pool is not None:
                a, b = pool[0], pool[1]
        ops.msssim_finish(ws, n, p.img_size, p.c_dim, self._scores, self._pairs)
        self._pairs += n

    def add(self, img):
        """Images [b, S, S, C] (fp32 or bf16); those past 2 n_pairs (the padding of a last generator batch) are dropped."""
        g = self._take(img)
        if g is None:
            return
        self._filled += int(g.shape[0])
        if self._carry is not None:                        # the pair that straddles two batches
            self._launch(torch.cat([self._carry.to(g.dtype), g[:1]]))
            self._carry, g = None, g[1:]
        even = (int(g.shape[0]) // 2) * 2
        if even:
            self._launch(g[:even])
        if int(g.shape[0]) > even:
            self._carry = g[even:].clone()

    def finish(self):
        """The mean of the pairs' scores, the doubles added on the host in index order."""
        self._check_full()                                 # (every image in: no pair is left half carried)
        per_pair = self._scores.cpu().numpy()
        self.per_pair, self._scores = per_pair, None
        total = 0.0
        for v in per_pair:
            total += float(v)
        return total / (self._n // 2)

    def begin_set(self, real):
        self.begin(self.plan.n_real_pairs if real else None)

    def name_scores(self, fake, ema):
        return {"msssim" if ema else "msssim_noema": fake}

    def real_scores(self):
        return {"msssim_real": self.real}


# ---- in-training frequency check: radial power spectrum of real and generated images (csrc/powerspec.hip) ----
PS_SIDES = (16, 32, 64, 128, 256, 512)
PS_FLOOR = 1e-30                      # log10 is taken of max(mean profile, PS_FLOOR)
PS_DECADES = 8.0                      # range of ps.png below the real set's largest non-DC value


def ps_bins(S):
    """NB(S) = (isqrt(2 S^2) + 1) // 2 + 1: the bins run to the corner (S/2, S/2): 12 / 24 / 46 / 92 / 182 / 363."""
    return (math.isqrt(2 * int(S) * int(S)) + 1) // 2 + 1


def ps_bin_table(S):
    """int64 [S, S/2 + 1]: the bin r = (isqrt(4 (ky^2 + kx^2)) + 1) // 2 of every coefficient of the half plane, rows in
    DFT order (ky = 0 .. S/2 - 1, -S/2 .. -1), in integers."""
    S = int(S)
    ky = np.arange(S, dtype=np.int64)
    ky = np.where(ky < S // 2, ky, ky - S)
    m4 = 4 * (ky[:, None] ** 2 + np.arange(S // 2 + 1, dtype=np.int64)[None, :] ** 2)
    root = np.array([math.isqrt(int(v)) for v in m4.reshape(-1)], dtype=np.int64).reshape(m4.shape)
    return (root + 1) // 2


def ps_counts(S):
    """int64 [NB]: coefficients of the FULL plane per bin: columns 0 < kx < S/2 of the half plane count twice."""
    S = int(S)
    w = np.full(S // 2 + 1, 2, dtype=np.int64)
    w[0] = w[-1] = 1
    return np.bincount(ps_bin_table(S).reshape(-1), weights=np.tile(w, S), minlength=ps_bins(S)).astype(np.int64)


class PowerSpectrumPlan(MonitorPlan):
    """What one run of the frequency check needs, from the flags alone.

    side, n_bins  S = --img_size, a power of two from 16 to 512; NB(S) radial bins, ``counts`` coefficients each
    n_images      --ps_images generated images per event; ``n_real`` real ones, once: the first n_images files of the
                  listing (all of them when the dataset has fewer), or n_images images of uniform noise without a dataset
    seeds         one per draw, derived from --static_sample_seed; none is shared with the other monitors"""
    name, seed_stride, draws = "ps", 32452843, ("latents", "labels", "real")

    def __init__(self, img_size, c_dim, batch_size, ps_images, static_sample_seed, n_files=None):
        super().__init__(img_size, c_dim, batch_size, static_sample_seed, n_files)
        if self.img_size not in PS_SIDES:
            raise ValueError("ps: --img_size %d: the transform takes a power of two from 16 to 512" % self.img_size)
        self.side = self.img_size
        self.n_fake = self.n_images = int(ps_images)
        if self.n_images < 1:
            raise ValueError("ps: no images to measure (%d)" % self.n_images)
        self.n_stream = self.n_real = self.n_images if n_files is None else min(self.n_images, int(n_files))
        if self.n_real < 1:
            raise ValueError("ps: the dataset has no files")
        self.n_bins = ps_bins(self.side)
        self.counts = ps_counts(self.side)
        self.first_hf = self.side // 4                                 # ps_hf / ps_peak read the bins r >= S/4

    # ---- sizes in bytes -------------------------------------------------------------------------
    @property
    def plane(self):
        return self.side * (self.side // 2 + 1)

    @property
    def workspace_bytes(self):
        """Twiddle table and row transforms of one generator batch (what bg_ps_workspace_bytes returns)."""
        return 4096 + self.batch_size * self.plane * 8

    @property
    def power_bytes(self):
        return self.batch_size * self.plane * 4

    @property
    def kept_bytes(self):
        """What a set leaves behind: fp64 profiles of every image and one fp64 2-D sum."""
        return self.n_images * self.n_bins * 8 + self.plane * 8

    @property
    def peak_bytes(self):
        return self.workspace_bytes + self.power_bytes + self.kept_bytes


class PowerSpectrum(Monitor):
    """A plan on the device.  ``begin`` / ``add`` / ``finish``: images arrive a batch at a time; per batch one power buffer
    and one workspace exist, what stays is the fp64 profile of every image and the fp64 2-D sum.  ``finish`` returns
    {"profile": the fp64 mean profile [NB], "sum2d": the summed power [S, S/2 + 1], "n": images}.  ``ops``: the launch
    wrappers (functional.py)."""
    prefix = "ps"

    def begin(self, n_images=None):
        p = self.plan
        self._expect(p.n_images if n_images is None else n_images)
        self._profiles = torch.zeros(self._n, p.n_bins, dtype=torch.float64, device=self.device)
        self._sum2d = torch.zeros(p.side, p.side // 2 + 1, dtype=torch.float64, device=self.device)

    def add(self, img):
        """Images [b, S, S, C] (fp32 or bf16); those past n_images (the padding of a last generator batch) are dropped."""
        g = self._take(img)
        if g is None:
            return
        b = int(g.shape[0])
        power = self.ops.ps_power(g)
        self.ops.ps_profile(power, self._profiles[self._filled:self._filled + b], self._sum2d)
        self._filled += b

    def finish(self):
        self._check_full()
        rows = self._profiles.cpu().numpy()
        total = np.zeros(self.plan.n_bins, dtype=np.float64)
        for row in rows:                                   # the fp64 mean over images, added in image order
            total += row
        out = {"profile": total / self._n, "sum2d": self._sum2d.cpu().numpy(), "n": self._n}
        self._profiles = self._sum2d = None
        return out

    # ---- host tail ---------------------------------------------------------------------------------
    @staticmethod
    def log_profile(profile):
        return np.log10(np.maximum(np.asarray(profile, dtype=np.float64), PS_FLOOR))

    def scores(self, real, fake, prefix="ps"):
        """D = L_fake - L_real over the bins: ``_dist`` sqrt(mean D^2) over r >= 1 (decades), ``_hf`` mean D over
        r >= S/4 (above 0: excess fine structure, below 0: blur), ``_peak`` max D over r >= S/4 and ``_peak_at`` its
        r / S (cycles per pixel).  DC (bin 0) is not read."""
        S, lo = self.plan.side, self.plan.first_hf
        D = self.log_profile(fake["profile"]) - self.log_profile(real["profile"])
        at = lo + int(np.argmax(D[lo:]))
        return {prefix + "_dist": float(np.sqrt(np.mean(D[1:] ** 2))), prefix + "_hf": float(np.mean(D[lo:])),
                prefix + "_peak": float(D[at]), prefix + "_peak_at": at / float(S)}

    def table(self, real, fakes):
        """Rows of ps.txt, one per radius: r, r / S, n_r, L_real, L_<name> of every fake set in ``fakes`` (a dict, in
        order), then D of each.  Returns (header, rows)."""
        S = self.plan.side
        Lr = self.log_profile(real["profile"])
        Lf = {k: self.log_profile(v["profile"]) for k, v in fakes.items()}
        header = ["r", "r/S", "n_r", "L_real"] + ["L_" + k for k in Lf] + ["D_" + k for k in Lf]
        rows = []
        for r in range(self.plan.n_bins):
            rows.append([r, r / float(S), int(self.plan.counts[r]), Lr[r]] + [L[r] for L in Lf.values()] +
                        [L[r] - Lr[r] for L in Lf.values()])
        return header, rows

    @staticmethod
    def full_plane(sum2d):
        """fp64 [S, S/2 + 1] -> [S, S] with DC at (S/2, S/2): column kx < 0 of row ky is column -kx of row -ky."""
        h = np.asarray(sum2d, dtype=np.float64)
        S = h.shape[0]
        full = np.empty((S, S), dtype=np.float64)
        full[:, :S // 2 + 1] = h
        neg = (-np.arange(S)) % S
        for kx in range(S // 2 + 1, S):
            full[:, kx] = h[neg, S - kx]
        return np.fft.fftshift(full)

    def image(self, real, fake):
        """uint8 [S, 2 S]: the mean 2-D spectra of the real and the fake set side by side, log10, the 8 decades below
        the real set's largest non-DC value scaled to 0..255."""
        S = self.plan.side
        planes = [self.full_plane(x["sum2d"]) / float(x["n"]) for x in (real, fake)]
        ref = planes[0].copy()
        ref[S // 2, S // 2] = 0.0
        top = math.log10(max(float(ref.max()), PS_FLOOR))
        out = []
        for pl in planes:
            L = np.log10(np.maximum(pl, PS_FLOOR))
            out.append(np.clip((L - (top - PS_DECADES)) / PS_DECADES, 0.0, 1.0))
        return np.round(np.concatenate(out, axis=1) * 255.0).astype(np.uint8)


    def save(self, folder, real, sets):
        """``ps.txt`` and ``ps.png`` in ``folder``; ``sets``: {"ps": the fake set, "ps_noema": the live weights' set}, one
        or both.  The image shows the moving averages' set when there is one.  Returns the two paths."""
        import os
        from .utils import write_png
        names = {"ps": "fake", "ps_noema": "fake_noema"}
        header, rows = self.table(real, {names[k]: v for k, v in sets.items()})
        txt, png = os.path.join(folder, "ps.txt"), os.path.join(folder, "ps.png")
        with open(txt, "w") as f:
            f.write("# " + "\t".join(header) + "\n")
            for row in rows:
                f.write("\t".join(["%d" % row[0], "%.6f" % row[1], "%d" % row[2]] + ["%.6f" % v for v in row[3:]]) + "\n")
        write_png(self.image(real, sets["ps"] if "ps" in sets else sets["ps_noema"]), png)
        return [txt, png]


# ---- in-training precision / recall / density / coverage (csrc/prdc.hip) ----
PR_MAX_K = 8


def check_pr_k(k):
    k = int(k)
    if k < 1 or k > PR_MAX_K:
        raise ValueError("prdc: --pr_k %d (1..%d)" % (k, PR_MAX_K))
    return k


class PrdcPlan(MonitorPlan):
    """What one run of the precision / recall / density / coverage check needs, from the flags alone.

    side, f, D    descriptors are side x side x c_dim (neighbours.search_side(img_size, --pr_size)), each value the mean of
                  an f x f box; D = side * side * c_dim values per image, a multiple of 64
    k             the neighbour whose distance is a row's radius (--pr_k, 1..8)
    N, M          real and generated images per event: --pr_images both, N capped by the number of dataset files; the real
                  ones are the first N files of the listing, or N images of uniform noise without a dataset
    seeds         one per draw, derived from --static_sample_seed; none is shared with the other monitors"""
    name, seed_stride, draws = "prdc", 49979687, ("latents", "labels", "real")

    def __init__(self, img_size, c_dim, batch_size, pr_images=4096, pr_k=3, pr_size=64, static_sample_seed=0, n_files=None):
        from .neighbours import search_side
        super().__init__(img_size, c_dim, batch_size, static_sample_seed, n_files)
        self.k = check_pr_k(pr_k)
        self.side = search_side(img_size, pr_size)
        self.f = self.img_size // self.side
        self.D = self.side * self.side * self.c_dim
        self.n_fake = self.M = self.n_images = int(pr_images)
        if self.M <= self.k:
            raise ValueError("prdc: --pr_images %d: more than --pr_k %d images are needed" % (self.M, self.k))
        self.n_stream = self.N = self.n_real = self.M if n_files is None else min(self.M, int(n_files))
        if self.N <= self.k:
            raise ValueError("prdc: the dataset has %d files, more than --pr_k %d are needed" % (self.N, self.k))

    # ---- sizes in bytes -------------------------------------------------------------------------
    @property
    def set_bytes(self):
        """One resident descriptor set of the larger of the two sizes."""
        return max(self.N, self.M) * self.D * 2

    @property
    def vector_bytes(self):
        """Per set its radii; per event a count per row of either set and the real rows' nearest distance; the four
        integers."""
        return 4 * (self.N + self.M) + 4 * (self.N + self.M) + 4 * self.N + 32

    @property
    def peak_bytes(self):
        return self.N * self.D * 2 + self.M * self.D * 2 + self.vector_bytes


class Prdc(Monitor):
    """A plan on the device.  ``begin`` / ``add`` / ``finish``: images arrive a batch at a time and are packed
    (bg_nn_pack) into the resident bf16 buffer [n, D]; ``finish`` measures the set's radii and returns
    {"desc": bf16 [n, D], "radius": fp32 [n], "n": n}, both on the device.  ``scores`` takes two such sets.  ``ops``: the
    launch wrappers (functional.py)."""
    prefix = "pr"

    def begin(self, n_images=None):
        p = self.plan
        self._expect(p.M if n_images is None else n_images)
        self._desc = torch.empty(self._n, p.D, dtype=torch.bfloat16, device=self.device)

    def add(self, img):
        """Images [b, S, S, C] (fp32 or bf16); those past n (the padding of a last generator batch) are dropped."""
        g = self._take(img)
        if g is None:
            return
        b = int(g.shape[0])
        self.ops.nn_pack(g, self.plan.f, False, out=self._desc[self._filled:self._filled + b])
        self._filled += b

    def finish(self):
        self._check_full()
        out = {"desc": self._desc, "radius": self.ops.prdc_radii(self._desc, self.plan.k), "n": self._n}
        self._desc = None
        return out

    def counts(self, real, fake):
        """The event's three passes over two finished sets: (count_f int32 [M], count_r int32 [N], dmin_r fp32 [N], out4
        int64 [4]), all on the device."""
        count_f, _ = self.ops.prdc_cover(real["desc"], real["radius"], fake["desc"], dmin=None)
        count_r, dmin_r = self.ops.prdc_cover(fake["desc"], fake["radius"], real["desc"])
        return count_f, count_r, dmin_r, self.ops.prdc_reduce(count_f, count_r, dmin_r, real["radius"])

    @staticmethod
    def ratios(out4, k, N, M, prefix="pr"):
        """The four scores in Python floats from the four integers."""
        a = [int(v) for v in out4]
        return {prefix + "_precision": a[0] / float(M), prefix + "_recall": a[2] / float(N),
                prefix + "_density": a[1] / float(k * M), prefix + "_coverage": a[3] / float(N)}

    def scores(self, real, fake, prefix="pr"):
        """``_precision``: the share of fakes inside some real row's k-NN ball; ``_density``: the balls a fake lies in,
        over k; ``_recall``: the share of reals inside some fake's ball; ``_coverage``: the share of reals whose nearest
        fake is inside the real's own ball.  One 32-byte copy to the host."""
        out4 = self.counts(real, fake)[3].cpu().tolist()
        return self.ratios(out4, self.plan.k, real["n"], fake["n"], prefix)


# kind -> (plan class, runner class, the model's flags that the plan's constructor takes after batch_size)
MONITORS = {"swd": (SwdPlan, Swd, ("swd_images",)),
            "msssim": (MsssimPlan, Msssim, ("msssim_pairs",)),
            "ps": (PowerSpectrumPlan, PowerSpectrum, ("ps_images",)),
            "prdc": (PrdcPlan, Prdc, ("pr_images", "pr_k", "pr_size"))}


def format_scores(scores):
    return ", ".join("%s: %.4f" % kv for kv in scores.items())
