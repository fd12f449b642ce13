"""Float64 numpy restatement of the sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018,
"Progressive Growing of GANs", section 5), written from the definition in DESIGN.md, and the error bounds that the GPU
tests hold the kernels of csrc/swd.hip to.  NHWC throughout.

Two stated deviations from the paper's script: the images are the [-1, 1] floats (no 8-bit rounding; the metric is
invariant to x -> a x + b with a > 0), and a channel without deviation gets all-zero descriptors instead of a division by
zero."""
import numpy as np

F5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
W25 = np.outer(F5, F5) / 256.0                  # f (x) f / 256
PATCHES, SIDE, TAPS = 128, 7, 49
U32 = 2.0 ** -24                                 # unit round-off of fp32


# ---------------------------------------------------------------------------------------------------- pyramid
def blur(x, gain=1.0):
    """conv(x, gain * f (x) f / 256) with the mirror boundary that does not repeat the edge (numpy.pad mode 'reflect')."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    p = np.pad(x, ((0, 0), (2, 2), (2, 2), (0, 0)), mode="reflect")
    out = np.zeros_like(x)
    for dy in range(5):
        for dx in range(5):
            out += (gain * W25[dy, dx]) * p[:, dy:dy + H, dx:dx + W, :]
    return out


def down(x):
    return blur(x)[:, ::2, ::2, :]


def up(x):
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    u = np.zeros((B, 2 * H, 2 * W, C))
    u[:, ::2, ::2, :] = x
    return blur(u, 4.0)


def level_sides(img_size):
    """[img_size, img_size / 2, ..., 16]: 64 px gives 3 levels, 128 px 4, 256 px 5, 512 px 6."""
    sides = [int(img_size)]
    while sides[-1] > 16:
        sides.append(sides[-1] // 2)
    return sides


def gaussian_pyramid(x):
    g = [np.asarray(x, np.float64)]
    while g[-1].shape[1] > 16:
        g.append(down(g[-1]))
    return g


def laplacian_pyramid(x):
    g = gaussian_pyramid(x)
    return [g[i] - up(g[i + 1]) for i in range(len(g) - 1)] + [g[-1]]


# per-element bounds of the fp32 kernels: (taps + 2) * 2^-24 * sum |w_i x_i|, the sum in float64
def down_bound(x, taps=25):
    return (taps + 2) * U32 * down(np.abs(np.asarray(x, np.float64)))


def lap_bound(g, g1, taps=25):
    return (taps + 2) * U32 * (np.abs(np.asarray(g, np.float64)) + up(np.abs(np.asarray(g1, np.float64))))


def laplacian_pyramid_bounds(x):
    """Bounds of the levels of an fp32 pyramid built level on level from the exact input x: a level inherits the error of
    the levels it was computed from (both operators are linear with non-negative weights, so a bound goes through them
    as a value does) and adds its own rounding."""
    g = gaussian_pyramid(x)
    eg = [np.zeros_like(g[0])]
    for i in range(1, len(g)):
        eg.append(down(eg[i - 1]) + down_bound(np.abs(g[i - 1]) + eg[i - 1]))
    out = []
    for i in range(len(g) - 1):
        out.append(eg[i] + up(eg[i + 1]) + lap_bound(np.abs(g[i]) + eg[i], np.abs(g[i + 1]) + eg[i + 1]))
    return out + [eg[-1]]


# ---------------------------------------------------------------------------------------------------- descriptors
def draw_positions(rng, n_images, side):
    """int32 [n_images, 128, 2] = (y, x), uniform in [3, side - 3)."""
    return rng.randint(3, side - 3, size=(n_images, PATCHES, 2)).astype(np.int32)


def descriptors(level, pos):
    """[B * 128, 49 C]: row b * 128 + k is the 7 x 7 patch around pos[b, k] in [c, dy, dx] order; a centre outside
    [3, H - 4] gives a zero row."""
    level = np.asarray(level)
    B, H, W, C = level.shape
    out = np.zeros((B * PATCHES, TAPS * C), level.dtype)
    for b in range(B):
        for k in range(PATCHES):
            y, x = int(pos[b, k, 0]), int(pos[b, k, 1])
            if 3 <= y <= H - 4 and 3 <= x <= W - 4:
                out[b * PATCHES + k] = level[b, y - 3:y + 4, x - 3:x + 4, :].transpose(2, 0, 1).reshape(-1)
    return out


def channel_stats(desc):
    """(mean [C], biased deviation [C]) over all descriptors of the set."""
    d = np.asarray(desc, np.float64).reshape(desc.shape[0], -1, TAPS)
    return d.mean(axis=(0, 2)), d.std(axis=(0, 2))


def normalise(desc):
    d = np.asarray(desc, np.float64).reshape(desc.shape[0], -1, TAPS)
    mean, std = channel_stats(desc)
    rstd = np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)
    return ((d - mean[None, :, None]) * rstd[None, :, None]).reshape(desc.shape[0], -1)


# ---------------------------------------------------------------------------------------------------- distance
def draw_directions(rng, K, repeats=4, n_dirs=128):
    """fp32 [K, repeats * n_dirs]: per repeat a normal [K, n_dirs] draw, every column scaled to unit length."""
    cols = []
    for _ in range(repeats):
        d = rng.randn(K, n_dirs)
        cols.append(d / np.sqrt((d * d).sum(axis=0, keepdims=True)))
    return np.concatenate(cols, axis=1).astype(np.float32)


def sorted_projections(desc, dirs):
    return np.sort(normalise(desc) @ np.asarray(dirs, np.float64), axis=0)


def distance(desc_a, desc_b, dirs, repeats=4):
    """mean |sorted A - sorted B| over all N x n_dirs entries of a repeat, averaged over the repeats."""
    pa, pb = sorted_projections(desc_a, dirs), sorted_projections(desc_b, dirs)
    n_dirs = dirs.shape[1] // repeats
    return float(np.mean([np.abs(pa[:, r * n_dirs:(r + 1) * n_dirs] - pb[:, r * n_dirs:(r + 1) * n_dirs]).mean()
                          for r in range(repeats)]))


def scores(real, fake, pos_real, pos_fake, dirs, repeats=4, prefix="swd"):
    """{'<prefix>_<side>': 1e3 * distance per level, '<prefix>_avg': their mean}.  pos_* and dirs: one entry per level."""
    lr, lf = laplacian_pyramid(real), laplacian_pyramid(fake)
    out = {}
    for i, (a, b) in enumerate(zip(lr, lf)):
        out["%s_%d" % (prefix, a.shape[1])] = 1e3 * distance(descriptors(a, pos_real[i]), descriptors(b, pos_fake[i]),
                                                            dirs[i], repeats)
    out[prefix + "_avg"] = float(np.mean(list(out.values())))
    return out


# ---------------------------------------------------------------------------------------------------- error bounds
def projection_bound(desc, dirs, level_err=None):
    """Worst-case error, over all (n, s), of the fp32 projections of one set against float64 ones.

    The dot product: K fp32 fma and one rounding of every normalised value, (K + 4) * 2^-24 * sum_k |a_nk| |d_ks| (the 4
    covers the rounding of a_nk, of the statistics, and slack).  ``level_err`` ([N, K], the per-element bound of the fp32
    pyramid level gathered like the descriptors): with x' = x + e the mean moves by at most mean(e) =: em and the
    deviation by at most rms(e) =: es per channel, so a' - a = (e - dm) / s' + (x - m)(1 / s' - 1 / s) is at most
    (e_nk + em_c + |a_nk| es_c) / (s_c - es_c), which goes through |d| like a value."""
    a = np.abs(normalise(desc))
    d = np.abs(np.asarray(dirs, np.float64))
    K = a.shape[1]
    bound = (K + 4) * U32 * (a @ d)
    if level_err is not None:
        _, std = channel_stats(desc)
        e = np.asarray(level_err, np.float64).reshape(a.shape[0], -1, TAPS)
        em = e.mean(axis=(0, 2))
        es = np.sqrt((e * e).mean(axis=(0, 2)))
        live = std > es
        scale = np.where(live, 1.0 / np.where(live, std - es, 1.0), 0.0)
        da = (e + em[None, :, None] + a.reshape(e.shape) * es[None, :, None]) * scale[None, :, None]
        bound = bound + da.reshape(a.shape) @ d
    return float(bound.max())


def distance_gate(desc_a, desc_b, dirs, err_a=None, err_b=None):
    """The distance is 1-Lipschitz in the sup-norm of either set's projections (sorting is a contraction in it, and the
    mean of absolute differences of two vectors moves by at most the sup-norm of the perturbation), so the gate is the
    sum of the two sets' worst-case projection errors."""
    return projection_bound(desc_a, dirs, err_a) + projection_bound(desc_b, dirs, err_b)


def end_to_end_inputs(seed=0, B=4, side=32, C=3):
    """fp32 real = one pass of the 5-tap blur over uniform noise, fake = two passes."""
    rng = np.random.RandomState(seed)
    noise = rng.uniform(-1.0, 1.0, size=(2, B, side, side, C))
    real = blur(noise[0]).astype(np.float32)
    fake = blur(blur(noise[1])).astype(np.float32)
    return real, fake, rng


def end_to_end_case(seed=0, B=4, side=32, C=3, repeats=2, n_dirs=16):
    """The end-to-end case of the GPU test: inputs, draws, and per level the float64 descriptors, distance and gate."""
    real, fake, rng = end_to_end_inputs(seed, B, side, C)
    sides = level_sides(side)
    pos_real = [draw_positions(rng, B, s) for s in sides]
    pos_fake = [draw_positions(rng, B, s) for s in sides]
    dirs = [draw_directions(rng, TAPS * C, repeats, n_dirs) for _ in sides]
    lr, lf = laplacian_pyramid(real), laplacian_pyramid(fake)
    er, ef = laplacian_pyramid_bounds(real), laplacian_pyramid_bounds(fake)
    levels = []
    for i in range(len(sides)):
        da, db = descriptors(lr[i], pos_real[i]), descriptors(lf[i], pos_fake[i])
        gate = distance_gate(da, db, dirs[i], descriptors(er[i], pos_real[i]), descriptors(ef[i], pos_fake[i]))
        levels.append(dict(da=da, db=db, dirs=dirs[i], dist=distance(da, db, dirs[i], repeats), gate=gate))
    return dict(real=real, fake=fake, sides=sides, pos_real=pos_real, pos_fake=pos_fake, dirs=dirs, repeats=repeats,
                n_dirs=n_dirs, levels=levels)
