"""`engine --denoise-variance` (host/main.c) on the GPU: with a multi-pass flag the saved rgb is
Renderer.denoise_variance of the library's mean, variance and features bit for bit and z is the render's;
without the flag, and with --denoise, the outputs are what the library gives without this filter."""
import os
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy

pytestmark = pytest.mark.gpu

FLAGS = ["-g", "path", "-n", "1", "--seed", "11"]
TARGET = "0.01"  # as test_gpu_adaptive_engine.py: some tiles meet it at once, edges do not


def engine(out, extra):
    cmd = [rtxpy.ENGINE, os.path.join("scenes", "scene1.json"), out, "64", "64"] + FLAGS + ["-f"] + extra
    p = subprocess.run(cmd, cwd=C.GOLDEN, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    r = rtxpy.Renderer(0)
    r.upload(scene)
    frame = scene.frame(64, 64)
    yield r, frame, rtxpy.params_from_args(FLAGS[:4], seed=11), r.features(frame)
    r.close()
    scene.close()


def library(r, frame, params, case):
    """(mean, z, variance) of the library for the engine's flags of `case`"""
    if case == "passes":
        return r.render_passes(frame, params, passes=4)
    if case == "aa":
        return r.render_passes(frame, params, passes=16, jitter=True)
    return r.render_adaptive(frame, params, 16, float(np.float32(float(TARGET))), jitter=True)[:3]


CASES = {"passes": ["--passes", "4"], "aa": ["--aa"], "adaptive": ["--adaptive", "--target-error", TARGET, "--aa"]}


@pytest.mark.parametrize("case", list(CASES))
def test_engine_denoise_variance_equals_the_library(lib, tmp_path, case):
    r, frame, params, feat = lib
    plain, den = str(tmp_path / "plain.tif"), str(tmp_path / "den.tif")
    assert "Denoising" not in engine(plain, CASES[case])
    log = engine(den, CASES[case] + ["--denoise-variance"])
    assert "Denoising with the variance." in log and "variance-guided filter levels" in log
    mean, z, var = library(r, frame, params, case)
    want, _ = r.denoise_variance(mean, var, feat)
    rgb0, z0 = rtxpy.read_tiff_raw(plain)
    rgb1, z1 = rtxpy.read_tiff_raw(den)
    assert np.array_equal(bits(rgb0), bits(mean)) and np.array_equal(bits(z0), bits(z))  # without the flag: as it was
    assert np.array_equal(bits(z1), bits(z))
    assert np.array_equal(bits(rgb1), bits(want))
    assert not np.array_equal(bits(rgb1), bits(rgb0))


def test_engine_denoise_alone_is_unchanged(lib, tmp_path):
    r, frame, params, feat = lib
    den = str(tmp_path / "den.tif")
    log = engine(den, ["--passes", "4", "--denoise"])
    assert "Denoising." in log and "variance" not in log
    mean, z, _ = library(r, frame, params, "passes")
    rgb1, z1 = rtxpy.read_tiff_raw(den)
    assert np.array_equal(bits(rgb1), bits(r.denoise(mean, feat))) and np.array_equal(bits(z1), bits(z))
