"""The singular-value kernels (csrc/spectrum.hip) and the monitor on the device against tests/sv_ref.py: the float64 run
of the same algorithm from the same start, LAPACK through the theorem, the cap on the residual, the residual of every
returned pair evaluated in float64, and the orthonormality of the basis.  Every bound is derived in sv_ref.py from the
fp32 rounding points; nothing is fitted to the device.  W and guard bands after q, sv and resid must come back untouched.
The outputs are not bit-reproducible (fp64 atomics in the second pass), so no test compares bits of two launches."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import hip, model, scope as S, spectrum
from tests import sv_ref as R, trainlog_ref as TR, weight_ref as WR
from tests.common import make_args
from tests.test_sv import rejections

pytestmark = pytest.mark.gpu

BAND, FILL = 1024, 12345.0
NAMES = [c[0] for c in R.CASES]


class Table:
    """A device table of weights with their bases; q, sv and resid of every item end in a guard band of FILL."""

    def __init__(self, mats, ws_start=0):
        """``mats``: [(w fp32 numpy or CUDA tensor [rows, cols], q0 fp32 numpy [cols, 8])]; ``ws_start``: byte offset of
        the first item's scratch (so that a table of one item can have ws_offset > 0)."""
        L = hip.lib()
        self.n = len(mats)
        self.w, self.w0, self.q, self.sv, self.resid = [], [], [], [], []
        items = (hip.BgSvItem * self.n)()
        off = ws_start
        for i, (w, q0) in enumerate(mats):
            w = w if torch.is_tensor(w) else torch.from_numpy(np.array(w, dtype=np.float32)).cuda()
            rows, cols = w.shape
            self.w.append(w)
            self.w0.append(w.clone() if w.numel() < (1 << 24) else None)
            for store, n, init in ((self.q, cols * 8, q0), (self.sv, 8, None), (self.resid, 8, None)):
                buf = torch.full((n + BAND,), FILL, dtype=torch.float32, device="cuda")
                if init is not None:
                    buf[:n] = torch.from_numpy(np.array(init, dtype=np.float32)).reshape(-1).cuda()
                store.append(buf)
            it = items[i]
            it.w, it.q, it.sv, it.resid = w.data_ptr(), self.q[i].data_ptr(), self.sv[i].data_ptr(), self.resid[i].data_ptr()
            it.ws_offset, it.rows, it.cols = off, rows, cols
            off += (int(L.bg_sv_workspace_bytes(rows, cols)) + 15) // 16 * 16
        self.items = items
        self.ws_bytes = off
        self.ws = torch.full(((off + BAND * 4) // 4,), FILL, dtype=torch.float32, device="cuda")
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()

    def run(self, iters):
        hip.check(hip.lib().bg_sv_batch(hip.ptr(self.table), self.n, iters, hip.ptr(self.ws), self.ws_bytes, hip.stream()))
        torch.cuda.synchronize()
        return self.outputs()

    def outputs(self):
        outs = []
        for i in range(self.n):
            rows, cols = self.w[i].shape
            assert self.w0[i] is None or torch.equal(self.w[i], self.w0[i])
            for buf, n in ((self.q[i], cols * 8), (self.sv[i], 8), (self.resid[i], 8)):
                assert bool((buf[n:] == FILL).all()), "a guard band was written"
            outs.append(dict(sv=self.sv[i][:8].double().cpu().numpy(), resid=self.resid[i][:8].double().cpu().numpy(),
                             q=self.q[i][:cols * 8].view(cols, 8).double().cpu().numpy()))
        assert bool((self.ws[(self.ws_bytes + 3) // 4:] == FILL).all()), "the workspace was written past ws_bytes"
        return outs


def _report(name, k, out):
    bd = k["bounds"]
    kk = min(R.K, 8, k["rows"], k["cols"])
    l0 = bd["s0"] ** 2
    gap = np.abs(out["sv"] ** 2 - k["ref"]["sv"] ** 2)[:kk] / l0
    print("%s: sv %s\n  gap/bound %s\n  resid %s cap %s\n  defect %.3g / %.3g"
          % (name, out["sv"][:kk], gap / bd["gap"][:kk], out["resid"][:kk], bd["cap"][:kk], R.defect_of(out["q"])[0],
             bd["defect"]))


# ---------------------------------------------------------------- the shape cases, a fixed number of iterations
@pytest.mark.parametrize("name", NAMES)
def test_fixed_iterations_against_the_float64_run_and_lapack(name):
    k = R.case(name)
    out = Table([(k["w"], k["q0"])]).run(k["iters"])[0]                   # (a table of one item)
    _report(name, k, out)
    assert R.gate(k, out) == []
    if name == "rank1_8x8":
        assert (out["sv"][1:] <= 1e-6 * out["sv"][0]).all()               # the rounding level of sigma_0


def test_the_ritz_step_alone_on_the_true_singular_vectors():
    """iters = 0 with Q set to the top-8 right singular vectors: sv is the truth within the bounds with no float64
    residual to add, and the residual stays below the cap."""
    for name in ("37x5", "64x256", "65x257", "1030x24", "equal_40x12"):
        k = R.case(name)
        b = min(8, k["rows"], k["cols"])
        bd = R.bounds(k["w"], k["truth"])
        out = Table([(k["w"], R.true_basis(k["w"]))]).run(0)[0]
        err = np.abs(out["sv"][:b] ** 2 - k["truth"][:b] ** 2) / bd["s0"] ** 2
        print(name, "err / bound", err / bd["gap"][:b], "resid / cap", out["resid"][:b] / bd["cap"][:b])
        assert (err <= bd["gap"][:b]).all() and (out["resid"][:b] <= bd["cap"][:b]).all()
        assert R.defect_of(out["q"])[0] <= bd["defect"] and not out["q"][:, b:].any()
        own = R.pair_resid(R.apply_gram(k["w"]), out["q"], out["sv"])
        assert (np.abs(out["resid"] - own)[:b] <= bd["resid_err"]).all()


def test_two_calls_warm_start_like_one_call_of_twice_the_iterations():
    for name in ("64x256", "65x257", "1030x24"):
        k = R.case(name)
        t = k["iters"]
        ref = R.run(k["w"], k["q0"], 2 * t, np.float64)
        k2 = dict(k, ref=ref, bounds=R.bounds(k["w"], k["truth"], ref["resid"]))
        once = Table([(k["w"], k["q0"])]).run(2 * t)[0]
        twice = Table([(k["w"], k["q0"])])
        twice.run(t)
        warm = twice.run(t)[0]
        assert R.gate(k2, once) == [] and R.gate(k2, warm) == []
        kk = min(R.K, 8, k["rows"], k["cols"])
        diff = np.abs(once["sv"] ** 2 - warm["sv"] ** 2)[:kk] / k2["bounds"]["s0"] ** 2
        print(name, "once against warm / bound", diff / k2["bounds"]["gap"][:kk])
        assert (diff <= k2["bounds"]["gap"][:kk]).all()


def test_one_table_of_all_cases_against_single_calls():
    ks = [R.case(n) for n in NAMES]
    together = Table([(k["w"], k["q0"]) for k in ks])
    assert [it.ws_offset for it in together.items][1] > 0
    # iterations differ per case (3 or 6): the table runs the 3-iteration cases, then the 6-iteration case on its own
    # with ws_offset > 0 in a table of one item
    outs = together.run(3)
    for k, out in zip(ks, outs):
        if k["iters"] != 3:
            continue
        single = Table([(k["w"], k["q0"])]).run(3)[0]
        kk = min(R.K, 8, k["rows"], k["cols"])
        diff = np.abs(out["sv"] ** 2 - single["sv"] ** 2)[:kk] / k["bounds"]["s0"] ** 2
        assert R.gate(k, out) == [] and (diff <= k["bounds"]["gap"][:kk]).all(), k["name"]
    k = R.case("65x257")
    assert R.gate(k, Table([(k["w"], k["q0"])], ws_start=4096).run(6)[0]) == []


def test_every_grid_stride_loop_takes_a_second_trip():
    """65600 x 2052 (538 MB): more than 2048 units in both streaming passes, so the unit loops of sv_project_kernel
    (2050 units: 256 KB each, capped at one per 32 rows) and of sv_backproject_kernel (257 x 9 = 2313 units of 256 rows x
    256 columns) stride a second time; the column loops of sv_project_body (2052 > 256), sv_orth_kernel, sv_ritz_kernel and
    sv_resid_kernel (2052 > 512), and their row loops, do as well.  W is an 8 x 2052 matrix of spectrum 2^-i stacked 8200
    times, so that W^T W = 8200 A^T A and the truth is sqrt(8200) times the LAPACK values of A: no float64 run of the
    large matrix is needed, and the rank is 8, so the block holds the whole range after one iteration."""
    m, cols = 8200, 2052
    a = R.make_matrix(8, cols, R.pow2(8), 77)
    sigma = np.sqrt(float(m)) * R.truth(a)
    w = torch.from_numpy(a).cuda().repeat(m, 1).contiguous()
    assert tuple(w.shape) == (65600, 2052)
    a64 = a.astype(np.float64)
    # the bounds of sv_ref.py need ||W||_F and sigma_0 only: both follow from A
    bd = R.bounds(a, R.truth(a))
    out = Table([(w, R.make_basis(cols, 78))]).run(3)[0]
    del w
    l0 = sigma[0] ** 2
    err = np.abs(out["sv"] ** 2 - sigma ** 2) / l0
    print("sv", out["sv"], "\n err / bound", err / bd["gap"], "\n resid", out["resid"], "cap", bd["cap"])
    assert np.isfinite(out["sv"]).all() and np.isfinite(out["resid"]).all()
    assert (err <= bd["gap"]).all() and (out["resid"] <= bd["cap"]).all()
    own = R.pair_resid(lambda x: m * (a64.T @ (a64 @ x)), out["q"], out["sv"])
    assert (np.abs(out["resid"] - own) <= bd["resid_err"]).all()
    assert R.defect_of(out["q"])[0] <= bd["defect"]


def test_bad_arguments_are_rejected_on_the_device_with_nothing_launched():
    k = R.case("37x5")
    t = Table([(k["w"], k["q0"]), (k["w"], k["q0"])])
    q_before = [q.clone() for q in t.q]
    L = hip.lib()
    got = rejections(L, ctypes.c_void_p(t.table.data_ptr()), ctypes.c_void_p(t.ws.data_ptr()), t.ws_bytes)
    torch.cuda.synchronize()
    for word, (rc, msg) in got.items():
        assert rc == WR.ERR_ARG and word in msg, (word, rc, msg)
    for i in range(2):
        assert torch.equal(t.q[i], q_before[i]) and bool((t.sv[i] == FILL).all()) and bool((t.resid[i] == FILL).all())
    assert bool((t.ws == FILL).all())
    # an item whose scratch does not lie inside ws_bytes is left alone; the other one is computed
    hip.check(L.bg_sv_batch(hip.ptr(t.table), 2, 3, hip.ptr(t.ws), t.items[1].ws_offset + 64, hip.stream()))
    torch.cuda.synchronize()
    assert bool((t.sv[1] == FILL).all()) and torch.equal(t.q[1], q_before[1])
    out = dict(sv=t.sv[0][:8].double().cpu().numpy(), resid=t.resid[0][:8].double().cpu().numpy(),
               q=t.q[0][:40].view(5, 8).double().cpu().numpy())
    assert R.gate(k, out) == []


def test_against_two_hundred_steps_of_spectral_norm():
    """One fixed 96 x 24 weight of spectrum 2^-i: the sigma of bg_spectral_norm_fwd after 200 calls (its power iteration
    gains a factor 4 per call, so it sits at its fp32 fixed point) and the monitor's sv[0] agree within the sum of the two
    bounds.  Spectral norm's: v_ = W u in fp32 over cols terms, u_ = v^ W in fp32 over rows terms (any order: (rows + cols) u
    against ||W||_F), the normalisations and sigma = ss rs_u of weight_ref.py (sn_sigma_m(cols) + 2 SN_V_M roundings of
    sigma_0 <= ||W||_F)."""
    rows, cols = 96, 24
    w_np = R.make_matrix(rows, cols, R.pow2(cols), 55)
    sigma_true = R.truth(w_np)
    L = hip.lib()
    w = torch.from_numpy(w_np).cuda()
    u = torch.from_numpy(np.random.RandomState(56).standard_normal(cols).astype(np.float32)).cuda()
    v, sig, wn = torch.zeros(rows, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(rows, cols, device="cuda")
    nb = int(L.bg_spectral_norm_workspace_bytes(rows, cols))
    ws = hip.workspace(nb, "cuda")
    for _ in range(200):
        hip.check(L.bg_spectral_norm_fwd(hip.ptr(w), hip.ptr(u), hip.ptr(u), hip.ptr(v), hip.ptr(sig), hip.ptr(wn), rows, cols,
                                         hip.ptr(ws), nb, hip.stream()))
    out = Table([(w_np, R.make_basis(cols, 57))]).run(3)[0]
    fro = float(np.sqrt((w_np.astype(np.float64) ** 2).sum()))
    sn_bound = (rows + cols + WR.sn_sigma_m(cols) + 2 * WR.SN_V_M) * R.U32 * fro
    bd = R.bounds(w_np, sigma_true, R.run(w_np, R.make_basis(cols, 57), 3, np.float64)["resid"])
    sv_bound = bd["gap"][0] * bd["s0"]               # |sv^2 - s^2| <= gap s^2 and sv + s >= s
    got = abs(float(sig.item()) - out["sv"][0])
    print("spectral norm %.9g monitor %.9g truth %.9g: apart %.3g, bounds %.3g + %.3g"
          % (sig.item(), out["sv"][0], sigma_true[0], got, sn_bound, sv_bound))
    assert got <= sn_bound + sv_bound


# ---------------------------------------------------------------- the plumbing model
def _model(tmp_path, tag, **kw):
    d = tmp_path / tag
    flags = dict(img_size=64, ch=8, batch_size=4, log_dir=str(d / "logs"), checkpoint_dir=str(d / "ckpt"),
                 sample_dir=str(d / "samples"), result_dir=str(d / "results"))
    flags.update(kw)
    return model.BigGAN(make_args(**flags), store=S.VariableStore("cuda", seed=5)).build_model()


def test_event_agrees_with_svdvals_of_every_weight_and_leaves_the_run_alone(tmp_path):
    gan = _model(tmp_path, "event", sv_k=4)
    gan.train_step(gan.synthetic_batch())
    gan.sync_sharded_state()
    torch.cuda.synchronize()
    before = {k: v.detach().clone() for k, v in gan.state_tensors().items()}
    rng = (gan.gen.get_state().clone(), torch.get_rng_state().clone(), np.random.get_state()[1].copy())
    values, line, result = gan.singular_values()
    values2, _, result2 = gan.singular_values()                 # the second event starts warm
    after = gan.state_tensors()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(gan.gen.get_state(), rng[0]) and torch.equal(torch.get_rng_state(), rng[1])
    assert np.array_equal(np.random.get_state()[1], rng[2])
    names = [n for n in gan.store.vars if n.endswith("/kernel") and gan.store.trainable[n]]
    assert [w["name"] for w in result["weights"]] == names
    assert result["resid_max"] <= gan.sv_tol and values["sv_resid_max"] == result["resid_max"]
    assert 1 <= result2["rounds"] <= result["rounds"] <= 8
    worst = 0.0
    for res in (result, result2):
        for w in res["weights"]:
            var = gan.store.vars[w["name"]].detach().reshape(w["rows"], w["cols"]).cpu().numpy()
            sigma = R.truth(var)
            bd = R.bounds(var, sigma)
            kk = min(4, w["rows"], w["cols"])
            miss = R.theorem_miss(w["sv"], w["resid"], sigma, bd["floor"] + bd["local"])[:kk]
            worst = max(worst, float((miss / max(bd["s0"] ** 2, 1e-300)).max()))
            assert (miss <= 0).all(), (w["name"], w["sv"], sigma[:4], w["resid"])
            assert (w["sv"][kk:] == 0).all() and (w["resid"] <= gan.sv_tol).all()
    print(line, "\nworst theorem margin (negative is inside): %.3g of sigma_0^2" % worst)
    assert line.startswith("SV: G max s0 ") and ", rounds %d" % result["rounds"] in line
    g = max((w for w in result["weights"] if w["name"].startswith("generator/")), key=lambda w: w["sv"][0])
    assert values["sv_g_max"] == g["sv"][0] and "(%s)" % g["name"] in line
    # spectral norm's sigma is v^ W u^ <= sigma_0 of the weights it saw, one optimiser step ago; its one-step iteration
    # from a fresh u can sit well below sigma_0 of a flat spectrum
    assert gan.sn and 0.9 <= values["sv_sn_ratio_min"] <= values["sv_sn_ratio_max"] < 4.0


def _train(tmp_path, tag, sv_freq):
    gan = _model(tmp_path, tag, sv_freq=sv_freq)
    seen = []
    step = gan.train_step

    def recording_step(*a, **k):
        out = step(*a, **k)
        seen.append({name: np.float32(v.item()) for name, v in out.items()})
        return out

    gan.train_step = recording_step
    gan.log_events = True
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        gan.train(iterations=2, resume=False)
    return gan, seen, [l for l in out.getvalue().splitlines() if l.startswith("SV: ")]


@pytest.fixture(scope="module")
def run_pair(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("sv_pair")
    watched, seen, lines = _train(tmp_path, "watched", 1)
    plain, seen2, lines2 = _train(tmp_path, "plain", 0)
    return dict(watched=watched, plain=plain, seen=seen, seen2=seen2, lines=lines, lines2=lines2, tmp_path=tmp_path)


def test_training_with_the_monitor_is_bit_identical(run_pair):
    a, b = run_pair["watched"].state_tensors(), run_pair["plain"].state_tensors()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(run_pair["watched"].gen.get_state(), run_pair["plain"].gen.get_state())
    assert len(run_pair["seen"]) == 2 and run_pair["seen"] == run_pair["seen2"]
    assert run_pair["plain"]._sv is None and run_pair["watched"]._sv is not None
    assert len(run_pair["lines"]) == 2 and run_pair["lines2"] == []


def test_training_logs_the_values(run_pair):
    gan = run_pair["watched"]
    d = os.path.join(str(run_pair["tmp_path"] / "watched" / "logs"), gan.model_dir)
    ev = TR.read_events(os.path.join(d, os.listdir(d)[0]))
    events = [e for e in ev[1:] if e["values"][0][0].startswith("sv/")]
    steps = [e["step"] for e in ev[1:] if "d_loss" in [t for t, _, _ in e["values"]]]
    assert [e["step"] for e in events] == steps and len(events) == 2
    names = gan._sv.plan.names
    for e in events:
        tags = [t for t, _, _ in e["values"]]
        assert tags[:3 * len(names)] == ["sv/%s/s%d" % (n, i) for n in names for i in range(3)]
        assert tags[3 * len(names):] == ["sv_g_max", "sv_d_max", "sv_resid_max", "sv_sn_ratio_min", "sv_sn_ratio_max"]
        vals = {t: v for t, _, v in e["values"]}
        assert all(kind == "scalar" and np.isfinite(v) and v >= 0 for _, kind, v in e["values"])
        assert vals["sv_resid_max"] <= gan.sv_tol
        assert vals["sv_g_max"] == max(v for t, v in vals.items() if t.startswith("sv/generator/") and t.endswith("/s0"))


def test_phase_test_writes_one_row_per_weight(tmp_path):
    gan = _model(tmp_path, "phase", sv_freq=1, test_num=1)
    with contextlib.redirect_stdout(io.StringIO()):
        gan.test()
    path = os.path.join(str(tmp_path / "phase" / "results"), gan.model_dir, "sv.txt")
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert [r[0] for r in rows] == gan._sv.plan.names and all(len(r) == 3 + 3 + 3 for r in rows)
    for r, rr, cc in zip(rows, gan._sv.plan.rows, gan._sv.plan.cols):
        assert (int(r[1]), int(r[2])) == (rr, cc)
        sv = [float(x) for x in r[3:6]]
        assert sv == sorted(sv, reverse=True) and all(0 <= float(x) <= gan.sv_tol for x in r[6:9])
