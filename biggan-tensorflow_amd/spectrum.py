"""Singular-value monitor (extension flags --sv_freq / --sv_k / --sv_iters / --sv_tol; csrc/spectrum.hip).

The diagnostic of Brock et al. 2019 for a collapse that is on its way: the top singular values sigma_0, sigma_1, ... of every
weight matrix of G and D over training.  Spectral norm keeps a one-step estimate of sigma_0 only, and a full decomposition
per weight is far too slow inside a training loop; ``bg_sv_batch`` runs a block power iteration with 8 basis vectors over
all weights at once and reports, with every value, a residual that bounds its distance from a true singular value:
some sigma^2 of the weight lies within ``resid[i] * sv[0]^2`` of ``sv[i]^2``.

``SvPlan`` is the host part (which variables, their reshape, the layout of basis and workspace); ``SingularValues`` owns
the device buffers.  The basis is drawn from a generator of the monitor's own, is no variable of the store and is not
checkpointed: after a resume the first event starts cold.  Nothing that the training run reads is touched.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import hip
from .hip import check, lib, stream

SEED = 0x53564D4F          # the monitor's own generator
MAX_ROUNDS = 8
TABLE_MAX = 256            # items per bg_sv_batch call
NETWORKS = ("generator", "discriminator")


def monitored(store):
    """name -> variable: every trainable variable of generator/ and discriminator/ whose name ends in /kernel (the live
    weights, not the moving averages)."""
    return OrderedDict((n, v) for n, v in store.vars.items()
                       if store.trainable.get(n) and n.endswith("/kernel") and n.split("/")[0] in NETWORKS)


class SvPlan:
    """Host side: the monitored weights with rows = numel / cols, cols = the last axis (the reshape of spectral norm),
    b_eff = min(8, rows, cols), and the offsets of every weight's basis (floats) and scratch (bytes, 16-byte aligned)."""

    def __init__(self, store, k=3, iters=8, tol=1e-2):
        if not 1 <= int(k) <= 4:
            raise ValueError("--sv_k %s: 1..4 singular values per weight" % k)
        if not 1 <= int(iters) <= 256:
            raise ValueError("--sv_iters %s: 1..256 iterations per round" % iters)
        if not float(tol) > 0.0:
            raise ValueError("--sv_tol %s: a positive residual" % tol)
        self.k, self.iters, self.tol = int(k), int(iters), float(tol)
        self.names, self.rows, self.cols, self.beff = [], [], [], []
        self.q_offsets, self.ws_offsets = [], []
        q_off = ws_off = 0
        L = lib()
        for name, v in monitored(store).items():
            cols = int(v.shape[-1])
            rows = int(v.numel()) // cols
            self.names.append(name)
            self.rows.append(rows)
            self.cols.append(cols)
            self.beff.append(min(hip.SV_BLOCK, rows, cols))
            self.q_offsets.append(q_off)
            q_off += cols * hip.SV_BLOCK
            self.ws_offsets.append(ws_off)
            ws_off += (int(L.bg_sv_workspace_bytes(rows, cols)) + 15) // 16 * 16
        self.q_floats, self.ws_bytes = q_off, ws_off
        self.n = len(self.names)
        self.weight_bytes = 4 * sum(r * c for r, c in zip(self.rows, self.cols))


def draw_basis(cols, beff, gen):
    """[cols, 8] fp32 with ``beff`` orthonormal columns (QR of a Gaussian draw from ``gen`` in float64) and zeros beyond."""
    q = torch.zeros(cols, hip.SV_BLOCK, dtype=torch.float64)
    q[:, :beff], _ = torch.linalg.qr(torch.randn(cols, beff, dtype=torch.float64, generator=gen))
    return q.to(torch.float32)


def refill_basis(q, beff, gen):
    """Replace the zero columns with index < beff of the basis ``q`` [cols, 8] (host, fp32) by draws from ``gen`` made
    orthonormal to the other columns (two projections in float64).  Returns the new basis, or None if none was zero."""
    q64 = q.to(torch.float64)
    zero = [i for i in range(beff) if not bool(q64[:, i].any())]
    if not zero:
        return None
    for i in zero:
        keep = [j for j in range(beff) if j != i and bool(q64[:, j].any())]
        v = torch.randn(q64.shape[0], dtype=torch.float64, generator=gen)
        for _ in range(2):
            if keep:
                v = v - q64[:, keep] @ (q64[:, keep].T @ v)
        q64[:, i] = v / v.norm()
    return q64.to(torch.float32)


class SingularValues:
    """The monitor of one model: the device table of its weights (built once, the arenas are stable), the flat basis buffer,
    the outputs and the workspace."""

    def __init__(self, store, device, k=3, iters=8, tol=1e-2, seed=SEED):
        self.plan = p = SvPlan(store, k, iters, tol)
        self.device = torch.device(device)
        self.gen = torch.Generator()
        self.gen.manual_seed(int(seed))
        weights = list(monitored(store).values())
        for w in weights:
            if not (w.is_cuda and w.is_contiguous() and w.dtype == torch.float32):
                raise RuntimeError("SingularValues needs contiguous CUDA fp32 weights (there is no CPU fallback)")
        host_q = torch.cat([draw_basis(c, b, self.gen).reshape(-1) for c, b in zip(p.cols, p.beff)]) if p.n else \
            torch.zeros(0)
        self.q = host_q.to(self.device)
        self.out = torch.zeros(max(p.n, 1), 2, hip.SV_BLOCK, dtype=torch.float32, device=self.device)   # [item][sv | resid][8]
        self.ws = hip.workspace(p.ws_bytes, self.device)
        items = (hip.BgSvItem * max(p.n, 1))()
        for i, w in enumerate(weights):
            it = items[i]
            it.w = w.data_ptr()
            it.q = self.q.data_ptr() + 4 * p.q_offsets[i]
            it.sv = self.out.data_ptr() + 4 * 2 * hip.SV_BLOCK * i
            it.resid = it.sv + 4 * hip.SV_BLOCK
            it.ws_offset, it.rows, it.cols = p.ws_offsets[i], p.rows[i], p.cols[i]
        self.tables = []
        for lo in range(0, p.n, TABLE_MAX):
            sub = (hip.BgSvItem * min(TABLE_MAX, p.n - lo))(*[items[i] for i in range(lo, min(lo + TABLE_MAX, p.n))])
            self.tables.append((torch.frombuffer(bytearray(bytes(sub)), dtype=torch.uint8).to(self.device), len(sub)))
        self._weights = weights              # (keeps the views alive)
        self._deficient = []                 # items whose last event left a zero among the first b_eff values
        self.calls = 0

    def basis(self, i):
        """The basis of weight i as a view [cols, 8] of the flat buffer."""
        p = self.plan
        return self.q.narrow(0, p.q_offsets[i], p.cols[i] * hip.SV_BLOCK).view(p.cols[i], hip.SV_BLOCK)

    def _refill(self):
        for i in self._deficient:
            new = refill_basis(self.basis(i).cpu(), self.plan.beff[i], self.gen)
            if new is not None:
                self.basis(i).copy_(new.to(self.device))
        self._deficient = []

    def launch(self, iters):
        """One ``bg_sv_batch`` per table of at most 256 weights on the current stream."""
        for table, n in self.tables:
            check(lib().bg_sv_batch(hip.ptr(table), n, int(iters), hip.ptr(self.ws), self.plan.ws_bytes, stream()))
            self.calls += 1

    def event(self):
        """Rounds of --sv_iters iterations until the largest residual among the reported k values of all weights is at
        most --sv_tol, at most 8 rounds, one readback per round.  Returns {"weights": [{name, rows, cols, sv [k],
        resid [k]}], "rounds": rounds used, "resid_max": the largest reported residual}."""
        p = self.plan
        if p.n == 0:
            return dict(weights=[], rounds=0, resid_max=0.0)
        self._refill()
        rounds, worst, out = 0, float("inf"), None
        while rounds < MAX_ROUNDS and not worst <= p.tol:
            self.launch(p.iters)
            out = self.out.cpu().numpy().astype(np.float64)
            rounds += 1
            worst = max(float(out[i, 1, :min(p.k, p.beff[i])].max()) for i in range(p.n))
        self._deficient = [i for i in range(p.n) if (out[i, 0, :p.beff[i]] == 0.0).any()]
        weights = [dict(name=p.names[i], rows=p.rows[i], cols=p.cols[i], sv=out[i, 0, :p.k].copy(),
                        resid=out[i, 1, :p.k].copy()) for i in range(p.n)]
        return dict(weights=weights, rounds=rounds, resid_max=worst)


def scalars(result, k, sigma_of=None):
    """The event's scalars in the order they are written: sv/<variable name>/s0 .. s{k-1}, sv_g_max, sv_d_max (the largest
    sigma_0 per network), sv_resid_max and, with ``sigma_of`` (name -> the sigma that spectral norm last wrote, or None),
    sv_sn_ratio_min / sv_sn_ratio_max of the monitor's sigma_0 over it.  Also returns the names of the two maxima."""
    out = OrderedDict()
    top = {}
    for w in result["weights"]:
        for i in range(k):
            out["sv/%s/s%d" % (w["name"], i)] = float(w["sv"][i])
        net = w["name"].split("/")[0]
        if net not in top or w["sv"][0] > top[net][0]:
            top[net] = (float(w["sv"][0]), w["name"])
    for net, tag in (("generator", "sv_g_max"), ("discriminator", "sv_d_max")):
        if net in top:
            out[tag] = top[net][0]
    out["sv_resid_max"] = float(result["resid_max"])
    if sigma_of is not None:
        ratios = []
        for w in result["weights"]:
            s = sigma_of(w["name"])
            if s is not None and s > 0.0:
                ratios.append(float(w["sv"][0]) / s)
        if ratios:
            out["sv_sn_ratio_min"], out["sv_sn_ratio_max"] = min(ratios), max(ratios)
    return out, top


def format_line(result, top):
    g, d = top.get("generator", (0.0, "-")), top.get("discriminator", (0.0, "-"))
    return "SV: G max s0 %.6g (%s), D max s0 %.6g (%s), resid %.3g, rounds %d" % (
        g[0], g[1], d[0], d[1], result["resid_max"], result["rounds"])
