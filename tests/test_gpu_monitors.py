"""The four quality monitors (SWD, MS-SSIM, power spectrum, PRDC) in one run of the tiny model that test_gpu_swd.py and
its siblings build: what they share - the event driver of metrics.Monitor, the real-set reader and the fake-input helper
of model.py - must leave them independent of each other and repeatable.  The scores themselves are checked against
float64 in each monitor's own file.

The config is the siblings': 64 px, ch 8 (32 px is built only behind an attribute that no flag sets).

Counts: 4 SWD images, 3 MS-SSIM pairs, 5 spectrum images, 8 PRDC images with k = 3.  No batch size has both a padded last
generator batch for all of 4, 5, 6 and 8 images and an MS-SSIM pair that straddles two batches (a straddle needs an odd
batch size below 6, and 1, 3 and 5 each divide one of the counts), so there are two cases: 3 (4, 5 and 8 are padded; the
pair of images 2 and 3 straddles the two batches of the six) and 7 (the nearest to the tiny config's 4 that divides none of
5, 6 and 8: every last batch is padded).  The models take no training step: the moving averages equal the live weights,
which the monitors' own files tell apart."""
import pytest

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import model, scope as S
from tests.common import make_args

pytestmark = pytest.mark.gpu

ORDER = ("swd", "msssim", "ps", "prdc")                    # the training loop's order (the searches in between left out)
EMA_KEYS = {"swd": ["swd_64", "swd_32", "swd_16", "swd_avg"],
            "msssim": ["msssim"],
            "ps": ["ps_dist", "ps_hf", "ps_peak", "ps_peak_at"],
            "prdc": ["pr_precision", "pr_recall", "pr_density", "pr_coverage"]}
NOEMA_KEYS = {"swd": ["swd_noema_64", "swd_noema_32", "swd_noema_16", "swd_noema_avg"],
              "msssim": ["msssim_noema"],
              "ps": [k + "_noema" for k in EMA_KEYS["ps"]],
              "prdc": [k + "_noema" for k in EMA_KEYS["prdc"]]}
FIRST_ONLY = {"swd": [], "msssim": ["msssim_real"], "ps": [], "prdc": []}


def _model(tmp_path, tag, batch_size):
    d = tmp_path / tag
    flags = dict(img_size=64, ch=8, batch_size=batch_size, sample_ema="both", swd_images=4, msssim_pairs=3, ps_images=5,
                 pr_images=8, pr_k=3, log_dir=str(d / "logs"), checkpoint_dir=str(d / "ckpt"),
                 sample_dir=str(d / "samples"), result_dir=str(d / "results"))
    return model.BigGAN(make_args(**flags), store=S.VariableStore("cuda", seed=5)).build_model()


def _event(gan, kind):
    return {"swd": gan.swd, "msssim": gan.msssim, "ps": gan.power_spectrum, "prdc": gan.prdc}[kind]()


@pytest.mark.parametrize("batch_size", [3, 7])
def test_the_four_monitors_in_one_run_are_repeatable_and_independent(tmp_path, batch_size):
    gan = _model(tmp_path, "all", batch_size)
    assert gan.generate_ema_samples and gan.generate_noema_samples
    first = {kind: _event(gan, kind) for kind in ORDER}
    second = {kind: _event(gan, kind) for kind in ORDER}
    plans = {kind: gan._monitors[kind].plan for kind in ORDER}
    assert [plans[kind].n_fake for kind in ORDER] == [4, 6, 5, 8] and [plans[kind].n_stream for kind in ORDER] == [4, 6, 5, 8]
    for kind in ORDER:
        print(kind, first[kind])
        # the moving averages' scores, then the live weights', then what only the first event reports
        assert list(first[kind]) == EMA_KEYS[kind] + NOEMA_KEYS[kind] + FIRST_ONLY[kind]
        assert list(second[kind]) == EMA_KEYS[kind] + NOEMA_KEYS[kind]
        # two events on unchanged weights
        assert second[kind] == {k: first[kind][k] for k in second[kind]}
    # every monitor alone on a fresh model of the same seed
    for kind in ORDER:
        alone = _model(tmp_path, kind, batch_size)
        assert _event(alone, kind) == first[kind], kind
        assert list(alone._monitors) == [kind]
