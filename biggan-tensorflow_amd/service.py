"""Host-side planning of the sampling service (BigGAN.py:1298-1369): which request files of a poll round are answered
together, which generator batch and slot every latent rides in, and where every image lands.  Pure functions on numpy:
nothing here touches the GPU or the model (the counterpart of ``sampling.py``; ``BigGAN.service`` runs the plan).

The reference serves files one after another and pads each to a whole ``batch_size``; a front end that asks for one image
at a time pays a full batch per image.  Here the pending files of a round share generator batches: a *group* is a
maximal run of files with the same (ema, use_discriminator), its latents are laid end to end, and only its last batch is
padded.  Consecutive images of a batch then belong to different response strips, so every image gets a destination of
its own (``functional.image_place_u8``): the strips ``[S, n_f*S, C]`` of a group (``save_images(samples, [1, n])``) lie
in one uint8 arena, each on a 16-byte boundary, and cross to the host in one copy."""
import os

import numpy as np

STRIP_ALIGN = 16
D_OUTPUT_KEYS = ("real", "cls")            # what discriminator() returns without the reconstruction heads
PLACE_ENTRY = np.dtype([("offset", "<i8"), ("pitch", "<i4"), ("skip", "<i4")])       # BgPlaceEntry


class RequestError(ValueError):
    """A request file that cannot be served; the message goes into ``NAME.err``."""


class Request(object):
    """One request file of a round.  ``z`` fp32 [n, z_dim], ``cls`` fp32 [n, n_labels] or None; ``offset`` / ``pitch``:
    where its strip lies in the group's arena; ``first``: the position of its first latent in the group."""

    def __init__(self, path, cmds, z, cls):
        self.path = path
        self.name = os.path.splitext(os.path.basename(path))[0]
        self.cmds = cmds
        self.z, self.cls = z, cls
        self.n = int(z.shape[0])
        self.ema = cmds["ema"] == '1' if "ema" in cmds else True                       # BigGAN.py:1328-1329
        self.use_discriminator = cmds.get("use_discriminator") == '1'                  # BigGAN.py:1331-1334
        self.d_outputs = None
        if self.use_discriminator and cmds.get("discriminator_outputs"):
            self.d_outputs = cmds["discriminator_outputs"].split(',')
        self.load_checkpoint = cmds.get("load_checkpoint")
        self.offset = self.pitch = self.first = 0

    def wants(self, key):
        return self.d_outputs is None or key in self.d_outputs


class Group(object):
    """Files answered by the same generator batches.  ``load_checkpoint``: the checkpoint to load before the group runs
    (or None).  ``batches``: per batch ``batch_size`` slots, each ``(file index, latent index)`` or None for a padding
    slot.  ``z`` / ``cls``: the group's latents end to end (unpadded: ``BigGAN.generate`` pads with the first one, which
    is what the padding slots stand for).  ``table``: int32 [batches * batch_size, 4], the placement entries of every
    slot in batch order.  ``arena_bytes``: the size of the strip arena."""

    def __init__(self, ema, use_discriminator, load_checkpoint=None):
        self.ema, self.use_discriminator, self.load_checkpoint = ema, use_discriminator, load_checkpoint
        self.files = []
        self.batches = []
        self.z = self.cls = self.table = None
        self.total = self.arena_bytes = 0


class Round(object):
    """``groups`` in serving order; ``errors``: (path, message) of the malformed files; ``quit``: the path of the quit
    file or None.  Files behind a quit file appear nowhere: they stay on disk."""

    def __init__(self):
        self.groups, self.errors, self.quit = [], [], None


def parse_request(path, cmds, vectors, z_dim, n_labels):
    """(cmds, vectors) of ``utils.read_vectors`` -> Request; RequestError for a bad number, a wrong length or an unknown
    ``discriminator_outputs`` key.  A vector has z_dim numbers, plus n_labels after them under --n_labels
    (BigGAN.py:1341-1345)."""
    width = int(z_dim) + int(n_labels)
    for i, v in enumerate(vectors):
        if len(v) != width:
            raise RequestError("vector %d has %d numbers, the model takes %d (z_dim %d + n_labels %d)"
                               % (i, len(v), width, z_dim, n_labels))
    a = np.asarray(vectors, dtype=np.float64).reshape(len(vectors), width)
    with np.errstate(over="ignore"):
        a = a.astype(np.float32)
    bad = ~np.isfinite(a)
    if bad.any():
        raise RequestError("vector %d holds a number that is not a finite float32" % int(np.argwhere(bad)[0][0]))
    req = Request(path, cmds, np.ascontiguousarray(a[:, :z_dim]),
                  np.ascontiguousarray(a[:, z_dim:]) if n_labels else None)
    for key in req.d_outputs or ():
        if key not in D_OUTPUT_KEYS:
            raise RequestError("discriminator_outputs: unknown key '%s' (known: %s)" % (key, ", ".join(D_OUTPUT_KEYS)))
    return req


def place_table(entries):
    """[(offset, pitch, skip), ...] -> int32 [n, 4], the device layout of BgPlaceEntry (little-endian int64 offset)."""
    t = np.zeros(len(entries), dtype=PLACE_ENTRY)
    for i, (offset, pitch, skip) in enumerate(entries):
        t[i] = (offset, pitch, skip)
    return t.view("<i4").reshape(len(entries), 4)


def _close(group, batch_size, img_size, c_dim):
    """Lay out a group: strips, slots, padding, placement table."""
    B, S, C = int(batch_size), int(img_size), int(c_dim)
    slots, off = [], 0
    for fi, req in enumerate(group.files):
        req.first, req.offset, req.pitch = len(slots), off, req.n * S * C
        off += (S * req.pitch + STRIP_ALIGN - 1) // STRIP_ALIGN * STRIP_ALIGN
        slots += [(fi, j) for j in range(req.n)]
    group.total, group.arena_bytes = len(slots), off
    slots += [None] * (-len(slots) % B)                                                # only the last batch is padded
    group.batches = [slots[b:b + B] for b in range(0, len(slots), B)]
    served = [r for r in group.files if r.n]
    if served:
        group.z = np.concatenate([r.z for r in served])
        group.cls = None if served[0].cls is None else np.concatenate([r.cls for r in served])
    group.table = place_table([(0, S * C, 1) if s is None else
                               (group.files[s[0]].offset + s[1] * S * C, group.files[s[0]].pitch, 0) for s in slots])
    return group


def plan_round(files, batch_size, z_dim, n_labels, img_size, c_dim):
    """``files``: [(path, cmds, vectors)] of a poll round in sorted name order; ``vectors`` may be the exception that
    reading the file raised (a bad number).  Returns a Round.

    A group is a maximal run of files with the same (ema, use_discriminator); a file carrying ``load_checkpoint`` or
    ``quit`` closes the group before it (the checkpoint is loaded before the new group runs).  ``quit`` ends the round:
    earlier files are answered, later ones are left alone (BigGAN.py:1324-1326 returns at once).  Malformed files join
    no group."""
    rnd, cur = Round(), None

    def close():
        if cur is not None:
            rnd.groups.append(_close(cur, batch_size, img_size, c_dim))
    for path, cmds, vectors in files:
        if isinstance(vectors, Exception):
            rnd.errors.append((path, str(vectors)))
            continue
        if "quit" in cmds:
            rnd.quit = path
            break
        try:
            req = parse_request(path, cmds, vectors, z_dim, n_labels)
        except RequestError as e:
            rnd.errors.append((path, str(e)))
            continue
        if cur is None or req.load_checkpoint is not None or (cur.ema, cur.use_discriminator) != (req.ema,
                                                                                                   req.use_discriminator):
            close()
            cur = Group(req.ema, req.use_discriminator, req.load_checkpoint)
        cur.files.append(req)
    close()
    return rnd


def list_requests(request_dir):
    """The ``*.txt`` files of the request folder in sorted name order (BigGAN.py:1314-1315; the reference's own order is
    os.listdir's)."""
    return [os.path.join(request_dir, f) for f in sorted(os.listdir(request_dir))
            if f.lower().endswith('.txt') and os.path.isfile(os.path.join(request_dir, f))]


def read_requests(paths):
    """[(path, cmds, vectors or the ValueError of a bad number)] for ``plan_round``.  A file that vanished between the
    listing and the read is dropped."""
    from .utils import read_vectors
    out = []
    for p in paths:
        try:
            cmds, vectors = read_vectors(p)
        except FileNotFoundError:
            continue
        except (ValueError, UnicodeDecodeError) as e:                                  # (csv.Error is no ValueError)
            cmds, vectors = {}, RequestError("bad number: %s" % e)
        except Exception as e:
            cmds, vectors = {}, RequestError("unreadable: %s" % e)
        out.append((p, cmds, vectors))
    return out


def write_response(req, request_dir, arena, outs, img_size, c_dim):
    """Answer one request from its group's results (``arena`` uint8 [arena_bytes], or under BG_DEVICE_PNG=1 the files'
    PNG bytes by request path, and ``outs`` {key: fp32 [total, ...]} on the host): the ``.out`` files, then ``NAME.tmp.png`` renamed to ``NAME.png``, then the request file goes - a
    client that waits for the PNG finds everything.  A file without vectors is only removed (BigGAN.py:1350, 1366)."""
    from .utils import write_png, write_vectors
    if req.n:
        stem = os.path.join(request_dir, req.name)
        if req.use_discriminator:
            for key in sorted(outs):
                if req.wants(key):
                    write_vectors(stem + "_" + key + ".out", outs[key][req.first:req.first + req.n])
        S = int(img_size)
        if isinstance(arena, dict):                                                    # encoded on the device (png.py)
            with open(stem + ".tmp.png", "wb") as f:
                f.write(arena[req.path])
        else:
            strip = arena[req.offset:req.offset + S * req.pitch].reshape(S, req.n * S, int(c_dim))
            write_png(strip, stem + ".tmp.png")
        os.rename(stem + ".tmp.png", stem + ".png")
    os.remove(req.path)
    return req.name


def write_error(path, message):
    """A malformed request: ``NAME.err`` holds the message, the request goes."""
    err = os.path.splitext(path)[0] + ".err"
    with open(err + ".tmp", "w") as f:
        f.write(message + "\n")
    os.rename(err + ".tmp", err)
    os.remove(path)
    return err
