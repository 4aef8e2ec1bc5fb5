"""The statistical properties of the variance-guided filter's formulas (include/rtx.h
rtx_denoise_variance_params), checked on the float64 model of denoise_variance_model.py: no
GPU is needed.  The frame: 48 x 64, flat features, truth (1, 0.8, 0.6) times 1.3 from column 32 on, noise
of sd 0.005 in the even 16-column bands and 0.1 in the odd ones; the filter is given the true variance."""
import numpy as np
import pytest

import denoise_variance_model as VM
from rtxpy import abi

H, W = 48, 64
SIG = {"sigma_color": 2.0, "sigma_normal": 0.05, "sigma_albedo": 0.1, "sigma_plane": 0.02}


def flat_features(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    feat = np.zeros((h, w), abi.FEATURE_DTYPE)
    feat["z"] = 5.0
    feat["position"] = np.stack([(x - w / 2) * 0.01, (y - h / 2) * 0.01, np.full_like(x, 5.0)], -1)
    feat["normal"] = (0, 0, -1)
    feat["albedo"] = 0.5
    return feat


@pytest.fixture(scope="module")
def frame():
    x = np.arange(W)
    truth = np.empty((H, W, 3))
    truth[...] = (1.0, 0.8, 0.6)
    truth[:, x >= 32] *= 1.3
    sd = np.where((x // 16) % 2 == 0, 0.005, 0.1)[None, :, None] * np.ones((H, W, 3))
    noisy = truth + np.random.default_rng(7).normal(0.0, 1.0, (H, W, 3)) * sd
    return truth, noisy, sd ** 2, flat_features(H, W)


def run(noisy, V, feat, levels, **sig):
    c, v = noisy, V
    for k in range(levels):
        c, v = VM.level(c, v, feat, k, dict(SIG, **sig))
    return c, v


@pytest.fixture(scope="module")
def filtered(frame):
    _, noisy, V, feat = frame
    return run(noisy, V, feat, 3)


def mse(c, truth, cols):
    return float(((c[:, cols] - truth[:, cols]) ** 2).sum(-1).mean())


def test_quiet_band_interior_falls_tenfold(frame, filtered):
    truth = frame[0]
    m = mse(filtered[0], truth, slice(4, 12))
    print(f"band 0 interior: mse / (3 sd^2) = {m / (3 * 0.005 ** 2):.4f}")
    assert m <= 3 * 0.005 ** 2 / 10


def test_noisy_band_interior_falls_tenfold(frame, filtered):
    truth = frame[0]
    m = mse(filtered[0], truth, slice(20, 28))
    print(f"band 1 interior: mse / (3 sd^2) = {m / (3 * 0.1 ** 2):.4f}")
    assert m <= 3 * 0.1 ** 2 / 10


def test_the_quiet_side_of_the_step_stays_and_moves_without_the_colour_term(frame, filtered):
    truth, noisy, V, feat = frame
    # the column's mean absolute change from the filter's input, over rows and channels (its noise: sd 0.005)
    moved = np.abs(filtered[0][:, 32] - noisy[:, 32]).mean()
    off = np.abs(run(noisy, V, feat, 3, sigma_color=float("inf"))[0][:, 32] - noisy[:, 32]).mean()
    print(f"column 32: moved {moved:.4f}, colour term off {off:.4f}")
    assert moved < 0.01
    assert off > 0.1


def test_the_first_level_predicts_its_variance(frame):
    """with the colour term off the weights do not depend on the noise and the taps are independent, so
    V' = sum w^2 V / (sum w)^2 is the variance of the output: its mean over band 1's interior against the
    mean squared error there"""
    truth, noisy, V, feat = frame
    c, v = run(noisy, V, feat, 1, sigma_color=float("inf"))
    cols = slice(20, 28)
    ratio = float(v[:, cols].sum(-1).mean()) / mse(c, truth, cols)
    print(f"predicted / empirical = {ratio:.3f}")
    assert 0.8 <= ratio <= 1.4


def test_zero_variance_returns_the_input(frame):
    _, noisy, V, feat = frame
    c, v = run(noisy.astype(np.float32), np.zeros_like(V, dtype=np.float32), feat, 3)
    assert np.array_equal(c, noisy.astype(np.float32).astype(np.float64))
    assert not v.any()


def test_the_synthetic_frame_lets_every_term_decide():
    """the model's own power on the frame test_gpu_denoise_variance.py filters: at levels 0 and 1, leaving any
    one term out of e moves some pixel by more than 1e-2 M"""
    rgb, feat = VM.synthetic()
    V = VM.synthetic_variance(rgb)
    c, v = rgb, V
    for k in (0, 1):
        M, live = VM.finite_max(c), VM.live_mask(c, v, feat)
        assert live.sum() == 37 * 29 - 30 - 2 - 3
        full = VM.level(c, v, feat, k)
        for term in VM.TERMS:
            diff = np.abs(VM.level(c, v, feat, k, without=term)[0][live] - full[0][live]).max()
            print(f"level {k} without {term}: {diff / M:.3e} M")
            assert diff > 1e-2 * M, (k, term, diff / M)
        c, v = full
